"""Every form of the TD-target launch (csrc/kernels/dqn.hip) through the public ``ops.dqn_targets``: uniform and
prioritised, one-step and 3-step, plain and dueling, with and without double Q, at H = 64 and 128, against the
bits recorded on the GPU before the four entry points became one (tests/golden/dqn_targets_forms.npz).  The
kernels are deterministic (Philox rows, fp32 MFMA, a bit-pattern atomicMax), so every array is compared exactly.

    PYTHONPATH=. python tests/test_dqn_targets_forms_gpu.py [OUT.npz]     # records the file from the same cases
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import MLPSpec, dqn_targets

from guarded import Guarded
from test_dqn_gpu import guarded_ring
from test_per_gpu import guarded_tree, random_leaves

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dqn_targets_forms.npz")
D, A, B = 4, 2, 70  # one full 64-row pass and a ragged second one
# Six of eight slots written, the last of them the newest: walks end at a done row, at the newest slot or at
# their full length, but none wraps at FILLED (a walk stops at slot 5 before it could); the wrap is covered by
# test_dqn_nstep_gpu.py, not here.
C, N, FILLED, NEWEST = 8, 4, 24, 5
SEED, UPDATE, GAMMA, BETA = (3 << 32) | 5, 2 ** 32 + 6, 0.97, 0.7
CASES = [(H, per, n, dueling, double_q) for H in (64, 128) for per in (False, True) for n in (1, 3)
         for dueling in (False, True) for double_q in (False, True)]


def case_id(case):
    H, per, n, dueling, double_q = case
    return f"H{H}-{'per' if per else 'uniform'}-n{n}-{'duel' if dueling else 'plain'}-{'double' if double_q else 'single'}"


@functools.lru_cache(maxsize=None)
def inputs():
    """The ring (all three done codes, random rewards) and the tree over its filled rows, built once."""
    gen = torch.Generator().manual_seed(17)
    u = torch.rand(C, N, generator=gen)
    done = torch.where(u < 0.15, 1.0, torch.where(u < 0.3, 2.0, 0.0))
    assert set(done.unique().tolist()) == {0.0, 1.0, 2.0}
    g, ring = guarded_ring(C, N, D)
    for dst, src in zip(ring, (torch.randn(C, N, D, generator=gen), torch.randn(C, N, D, generator=gen),
                               torch.randint(0, A, (C, N), generator=gen, dtype=torch.int32),
                               torch.randn(C, N, generator=gen), done)):
        dst.copy_(src)
    gt, _, pt = guarded_tree(random_leaves(C * N, FILLED, 23), 1.0)
    return g, ring, gt, pt.tree


def run_case(case):
    """-> the launch's arrays by name; Xb is compared with the ring here, not returned."""
    H, per, n, dueling, double_q = case
    g, ring, gt, tree = inputs()
    online, target = (MLPSpec(D, H, A + dueling).init(torch.Generator().manual_seed(k)).to(DEV) for k in (11, 12))
    names = ["Xb", "act_b", "y", "idx"] + (["w", "wmax"] if per else []) + ["last"]
    shapes = dict(Xb=((B, D), torch.float32), act_b=((B,), torch.int32), y=((B,), torch.float32),
                  idx=((B,), torch.int32), w=((B,), torch.float32), wmax=((1,), torch.float32), last=((B,), torch.int32))
    out = {k: Guarded(*shapes[k]) for k in names}
    kw = dict(tree=tree, beta=BETA) if per else {}
    dqn_targets(online, target, H, A, ring, FILLED, GAMMA, double_q, SEED, UPDATE, B,
                out=tuple(out[k].t for k in names), n_step=n, newest=NEWEST, dueling=dueling, **kw)
    torch.cuda.synchronize()
    assert all(o.guards_intact() for o in out.values()) and all(b.guards_intact() for b in g.values())
    assert gt.guards_intact()
    got = {k: out[k].t.cpu().numpy() for k in names}
    Xb = got.pop("Xb")
    want = ring.obs.reshape(-1, D)[torch.from_numpy(got["idx"]).long().to(DEV)].cpu().numpy()
    assert np.array_equal(Xb.view(np.uint32), want.view(np.uint32)), "Xb is not ring.obs at idx"
    return {k: (v.view(np.uint32) if v.dtype == np.float32 else v) for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_form_gives_the_recorded_bits(cuda, case):
    got = run_case(case)
    want = {k.split("/")[1]: v for k, v in golden().items() if k.split("/")[0] == case_id(case)}
    assert set(got) == set(want) and len(want) == (6 if case[1] else 4)
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (case_id(case), k)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    arrays = {f"{case_id(c)}/{k}": v for c in CASES for k, v in run_case(c).items()}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **arrays)
    print(f"{len(CASES)} cases, {len(arrays)} arrays -> {path} ({os.path.getsize(path)} bytes)")
