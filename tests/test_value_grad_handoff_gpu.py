"""The head -> dh1 hand-off of the bf16x6 value-gradient kernel (value_grad.hip): b3 held as a
wave-uniform scalar, the relu'(h2) mask words and the first table fragments read ahead of the
dout chain, unsigned x-slab indices, and shorter relu'-bit / A-fragment-mask sequences.

None of it changes a floating-point operation or a summation order, so the gradient slabs and
the six loss columns must be bitwise what the kernel gave before the change.  Those are recorded
in tests/golden/value_grad_handoff.npz by tools/record_vg_handoff_golden.py (SHA-256 of each
case's gradient slabs; everything but the W2 block, and the loss columns, in full).
"""
import hashlib
import os

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import GradHead, MLPSpec, hip, mlp_grad, set_value_grad_mode

from test_value_grad_pipelined_gpu import _inputs

pytestmark = pytest.mark.gpu

H = 128
PIPE, V3 = 240, 176  # 128 | (V << 4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "value_grad_handoff.npz")

# hidden-2 units forced onto the relu kink (a zero W2 row leaves h2 = b2 exactly), in four
# different waves and lane groups, and the b2 each one gets
KINK_UNITS = (5, 42, 79, 127)
KINK_B2 = (0.0, -0.0, 1e-40, 1e-30)  # +0, -0, a positive denormal, a small normal

# name -> (kind, D, B, tune); every case runs on a grid sized for 2 CUs
CASES = {
    # ragged last slab; two and more slabs per workgroup; both image parities, all three x buffers;
    # the min(.., B - 1) clamp of the ret prefetch
    "v7_B65": ("value", 4, 65, PIPE),
    "v7_B129": ("value", 4, 129, PIPE),
    "v7_B385": ("value", 4, 385, PIPE),
    "v7_B657": ("value", 4, 657, PIPE),
    # the single-slab route
    "v3_B63": ("value", 4, 63, V3),
    "v3_B128": ("value", 4, 128, V3),
    # the DP = 8 value head and the 2-action categorical head (production variants)
    "d8_B385": ("value", 8, 385, 0),
    "pg2_B385": ("pg2", 4, 385, 0),
    "v7_kink_B129": ("kink", 4, 129, PIPE),
}


def _seed(name):
    return 9000 + sorted(CASES).index(name) * 1009 + CASES[name][2]


def case_inputs(name):
    """CPU inputs of a case.  _inputs perturbs every parameter, so b3 is non-zero."""
    kind, D, B, _ = CASES[name]
    if kind == "pg2":
        g = torch.Generator().manual_seed(_seed(name))
        pp = MLPSpec(D, H, 2, False).init(g)
        pp = pp + 0.05 * torch.randn(pp.shape, generator=g)
        X = torch.randn(B, D, generator=g) * 1.5
        adv = torch.randn(B, generator=g)
        act = torch.randint(0, 2, (B,), generator=g, dtype=torch.int32)
        return pp, X, adv, act
    pp, X, ret = _inputs(D, B, _seed(name))
    if kind == "kink":
        o = MLPSpec(D, H, 1, False).offsets()
        for u, b in zip(KINK_UNITS, KINK_B2):
            pp[o["w2"] + u * H:o["w2"] + (u + 1) * H] = 0.0
            pp[o["b2"] + u] = b
        assert pp[o["b2"] + KINK_UNITS[1]].view(torch.int32).item() == -(2 ** 31)  # -0.0 kept its sign
        assert 0.0 < pp[o["b2"] + KINK_UNITS[2]].item() < 1.1754944e-38  # a denormal
    return pp, X, ret


def run_case(name, dev):
    """(gradient slabs, the six loss columns) of a case, as CPU tensors."""
    kind, D, B, tune = CASES[name]
    inp = [t.to(dev) for t in case_inputs(name)]
    old_c = hip().set_cu_limit(2)
    old_m = set_value_grad_mode(1)
    old_t = hip().set_value_grad_tune(tune)
    try:
        if kind == "pg2":
            pp, X, adv, act = inp
            slab, loss = mlp_grad(GradHead.PG_CAT, pp, X, 2, H, act=act, adv=adv)
        else:
            pp, X, ret = inp
            slab, loss = mlp_grad(GradHead.VALUE_MSE, pp, X, 1, H, ret=ret)
        slab, loss = slab.clone(), loss[:, :6].clone()  # the kernel writes six of the eight columns
        torch.cuda.synchronize()
    finally:
        hip().set_value_grad_tune(old_t)
        set_value_grad_mode(old_m)
        hip().set_cu_limit(old_c)
    return slab.cpu(), loss.cpu()


def _spec(name):
    kind, D, _, _ = CASES[name]
    return MLPSpec(D, H, 2 if kind == "pg2" else 1, False)


def kink_index(name):
    """Flat indices of the kink units' W2 rows, b2 and w3 entries."""
    o = _spec(name).offsets()
    idx = []
    for u in KINK_UNITS:
        idx += list(range(o["w2"] + u * H, o["w2"] + (u + 1) * H)) + [o["b2"] + u, o["w3"] + u]
    return torch.tensor(idx)


def summarize(name, slab, loss):
    """What the golden file keeps of a case (numpy arrays of raw bits)."""
    o = _spec(name).offsets()
    P = slab.shape[1]
    rest = torch.cat([torch.arange(0, o["w2"]), torch.arange(o["b2"], P)])
    out = {
        "sha": np.frombuffer(hashlib.sha256(slab.contiguous().numpy().tobytes()).digest(), dtype=np.uint8),
        "rest": slab[:, rest].contiguous().numpy().view(np.uint32),
        "loss": loss.contiguous().numpy().view(np.uint32),
    }
    if CASES[name][0] == "kink":
        out["kink"] = slab[:, kink_index(name)].contiguous().numpy().view(np.uint32)
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][0] != "kink"])
def test_handoff_is_bitwise_the_recorded_kernel(cuda, golden, name):
    slab, loss = run_case(name, cuda)
    B = CASES[name][2]
    assert slab.shape[0] == min((B + 63) // 64, 2)
    assert torch.isfinite(slab).all()
    got = summarize(name, slab, loss)
    # the small tensors first: a mismatch there says where (b3 enters every one through dout)
    assert np.array_equal(got["loss"], golden[f"{name}/loss"])
    assert np.array_equal(got["rest"], golden[f"{name}/rest"])
    assert np.array_equal(got["sha"], golden[f"{name}/sha"])


def test_relu_kink_units_are_bitwise_the_recorded_kernel(cuda, golden):
    """h2 = +0, -0, a positive denormal and 1e-30 exactly: the relu' bit stays `h2 > 0.f`."""
    name = "v7_kink_B129"
    slab, loss = run_case(name, cuda)
    assert torch.isfinite(slab).all()
    got = summarize(name, slab, loss)
    assert np.array_equal(got["kink"], golden[f"{name}/kink"])
    assert np.array_equal(got["loss"], golden[f"{name}/loss"])
    assert np.array_equal(got["rest"], golden[f"{name}/rest"])
    assert np.array_equal(got["sha"], golden[f"{name}/sha"])
    # the units at +0 and -0 are off (no gradient through them), the one at 1e-30 is on
    o = _spec(name).offsets()
    g = slab.sum(0)
    for u in KINK_UNITS[:2]:
        assert g[o["b2"] + u].item() == 0.0 and not g[o["w2"] + u * H:o["w2"] + (u + 1) * H].any()
    assert g[o["b2"] + KINK_UNITS[3]].item() != 0.0
