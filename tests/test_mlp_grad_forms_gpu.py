"""Every head of the fused gradient launch (csrc/kernels/mlp_grad.hip, value_grad.hip) through the public
``ops.mlp_grad`` -- and the quantile cases again through its alias ``ops.mlp_grad_qr`` -- at H = 64 and 128, plain,
weighted (row_w / w_norm / td_abs) and with the batch shape read from device memory, against the bits recorded on
the GPU before the three entry points and the twin bindings became one (tests/golden/mlp_grad_forms.npz).  The
kernels write per-block slabs and use no atomics, so every array is compared exactly; the gradient slab is held to
the SHA-256 of its bytes.

    PYTHONPATH=. python tests/test_mlp_grad_forms_gpu.py [OUT.npz]     # records the file from the same cases
"""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import GradHead, MLPSpec, grad_slabs, mlp_grad, mlp_grad_qr, set_value_grad_mode

from guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_grad_forms.npz")
B, D = 70, 4  # one full 64-row block and a ragged second one: two slabs
NVALID, INV_B_DEV = 37, 1.0 / 53
G = GradHead
# (name, head, A, quantiles, weighted, device-side batch shape, value_grad_mode or None)
FORMS = [("pg_cat-A3", G.PG_CAT, 3, 0, False, False, None),
         ("value-split", G.VALUE_MSE, 1, 0, False, False, 1),
         ("value-fp32", G.VALUE_MSE, 1, 0, False, False, 0),
         ("ppo_cat-A3", G.PPO_CAT, 3, 0, False, False, None),
         ("ppo_gauss-A1", G.PPO_GAUSS, 1, 0, False, False, None),
         ("pg_gauss-A1", G.PG_GAUSS, 1, 0, False, False, None)]
FORMS += [(f"q_td-A2-{'weighted' if w else 'plain'}", G.Q_TD, 2, 0, w, False, None) for w in (False, True)]
FORMS += [(f"q_duel-A{A}-{'weighted' if w else 'plain'}", G.Q_DUEL, A, 0, w, False, None)  # A = 1: VALU last layer
          for A in (1, 3) for w in (False, True)]
FORMS += [(f"q_qr-A{A}x{NQ}-{'weighted' if w else 'plain'}", G.Q_QR, A, NQ, w, False, None)
          for A, NQ in ((1, 1), (1, 2), (2, 8)) for w in (False, True)]
FORMS += [("q_td-A2-nvalid", G.Q_TD, 2, 0, True, True, None), ("q_qr-A2x8-nvalid", G.Q_QR, 2, 8, True, True, None)]
CASES = [(H,) + f for H in (64, 128) for f in FORMS]
QR_CASES = [c for c in CASES if c[2] == G.Q_QR]


def case_id(case):
    return f"H{case[0]}-{case[1]}"


def inputs(case):
    """Everything a head may read, from one seeded CPU generator per case."""
    H, name, head, A, NQ, weighted, dev_shape, _ = case
    gen = torch.Generator().manual_seed(1000 * H + 7 * CASES.index(case))
    gauss = head in (G.PPO_GAUSS, G.PG_GAUSS)
    outputs = 1 if head == G.VALUE_MSE else A + 1 if head == G.Q_DUEL else A * NQ if NQ else A
    kw = dict(params=MLPSpec(D, H, outputs, gauss).init(gen), X=torch.randn(B, D, generator=gen))
    kw["ret"] = torch.randn((B, NQ) if NQ else (B,), generator=gen)
    if gauss:
        kw["actc"] = torch.randn(B, A, generator=gen)
    elif head != G.VALUE_MSE:
        kw["act"] = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
    if head in (G.PG_CAT, G.PPO_CAT, G.PPO_GAUSS, G.PG_GAUSS):
        adv = torch.randn(B, generator=gen)
        kw.update(adv=adv, adv_stats=torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(B))]))
    if head in (G.PPO_CAT, G.PPO_GAUSS):
        kw["logp_old"] = -torch.rand(B, generator=gen) - 0.5
    if weighted:
        w = torch.rand(B, generator=gen) * 3.0 + 0.05
        kw.update(row_w=w, w_norm=w.max().reshape(1))
    if dev_shape:
        kw.update(nvalid=torch.tensor([NVALID], dtype=torch.int32), inv_B_dev=torch.tensor([INV_B_DEV]))
    return {k: v.to(DEV) for k, v in kw.items()}


def run_case(case, alias=False):
    """-> the launch's results by name: loss [ns, 6] and td_abs [B] as raw bits, the SHA-256 of the grad slab."""
    H, name, head, A, NQ, weighted, dev_shape, mode = case
    kw = inputs(case)
    params, X = kw.pop("params"), kw.pop("X")
    ns = grad_slabs(B, DEV)
    assert ns == 2
    gs, gl = Guarded((ns, params.numel())), Guarded((ns, 8))
    gtd = Guarded((B,)) if weighted else None
    kw.update(grad_slab=gs.t, loss_slab=gl.t, td_abs=gtd.t if weighted else None)
    clip = 0.75 if head in (G.Q_TD, G.Q_DUEL, G.Q_QR) else 0.2  # delta, kappa or the PPO clip
    prev = set_value_grad_mode(mode) if mode is not None else None
    try:
        if alias:
            slab, loss = mlp_grad_qr(params, X, A, NQ, H, kappa=clip, **kw)
        else:
            slab, loss = mlp_grad(head, params, X, A, H, clip_eps=clip, ent_coef=0.01, quantiles=NQ, **kw)
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            set_value_grad_mode(prev)
    assert slab.data_ptr() == gs.t.data_ptr() and loss.data_ptr() == gl.t.data_ptr()
    assert gs.guards_intact() and gl.guards_intact() and (gtd is None or gtd.guards_intact())
    assert bool(torch.isnan(gl.t[:, 6:]).all()), "the loss slab's last two columns are nobody's to write"
    got = {"loss": gl.t[:, :6].cpu().numpy().view(np.uint32),
           "grad_sha256": np.frombuffer(hashlib.sha256(gs.t.cpu().numpy().tobytes()).digest(), np.uint8)}
    if weighted:
        got["td_abs"] = gtd.t.cpu().numpy().view(np.uint32)
    return got


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def assert_recorded(case, got):
    want = {k.split("/")[1]: v for k, v in golden().items() if k.split("/")[0] == case_id(case)}
    assert set(got) == set(want) and len(want) == (3 if case[5] else 2)
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (case_id(case), k)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_head_gives_the_recorded_bits(cuda, case):
    assert_recorded(case, run_case(case))


@pytest.mark.parametrize("case", QR_CASES, ids=case_id)
def test_the_quantile_alias_gives_the_recorded_bits(cuda, case):
    assert_recorded(case, run_case(case, alias=True))


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    arrays = {f"{case_id(c)}/{k}": v for c in CASES for k, v in run_case(c).items()}
    for c in QR_CASES:  # the two routes agree before anything is recorded
        for k, v in run_case(c, alias=True).items():
            assert np.array_equal(arrays[f"{case_id(c)}/{k}"], v), (case_id(c), k)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **arrays)
    print(f"{len(CASES)} cases, {len(arrays)} arrays -> {path} ({os.path.getsize(path)} bytes)")
