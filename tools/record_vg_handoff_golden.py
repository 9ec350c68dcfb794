#!/usr/bin/env python3
"""Record tests/golden/value_grad_handoff.npz: the gradient slabs and loss columns of the cases of
tests/test_value_grad_handoff_gpu.py (SHA-256 of the slabs, the small tensors in full), as the
build that runs this script computes them.  Run it on the build the test is to be compared with
-- the commit before a change that must stay bitwise -- with that build's package first on
PYTHONPATH (tools/build_vg_variants.py makes such package copies), on a GPU:

  PYTHONPATH=<package root of the reference build> python tools/record_vg_handoff_golden.py [OUT.npz]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(REPO)  # after PYTHONPATH: a reference build named there wins
sys.path.insert(1, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import test_value_grad_handoff_gpu as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    import relayrl_prototype_amd

    print("package:", os.path.dirname(relayrl_prototype_amd.__file__), flush=True)
    dev = torch.device("cuda", 0)
    arrays = {}
    for name in T.CASES:
        slab, loss = T.run_case(name, dev)
        slab2, loss2 = T.run_case(name, dev)
        assert torch.equal(slab.view(torch.int32), slab2.view(torch.int32)), name  # reproducible
        assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), name
        assert torch.isfinite(slab).all(), name
        for k, v in T.summarize(name, slab, loss).items():
            arrays[f"{name}/{k}"] = v
        print(name, tuple(slab.shape), bytes(arrays[f"{name}/sha"]).hex()[:16], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
