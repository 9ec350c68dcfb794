"""The layer-1-pipelined variant of the bf16x6 value-gradient kernel (value_grad.hip, V = 7,
tune 240): layer 1 of a workgroup's next slab runs between the forward MFMAs of the current
one, into the second of two h1 images, and dW2's A fragments are built in registers.

Nothing in it reorders a sum, so its gradient and loss slabs must be bitwise those of V = 3
(tune 176), at every slab count per workgroup; it is also checked against float64 like the
other variants.
"""
import pytest
import torch

from relayrl_prototype_amd.ops import GradHead, MLPSpec, hip, mlp_grad, set_value_grad_mode

from test_value_grad_gpu import _away_from_relu_kinks, _grad64, _run

pytestmark = pytest.mark.gpu

H = 128
PIPE, V3 = 240, 176  # 128 | (V << 4)


def _inputs(D, B, seed):
    """Inputs as test_split_kernel_variants_match_float64 makes them (CPU tensors)."""
    g = torch.Generator().manual_seed(seed)
    pp = MLPSpec(D, H, 1, False).init(g)
    pp = pp + 0.05 * torch.randn(pp.shape, generator=g)
    X = torch.randn(B, D, generator=g) * 1.5
    ret = torch.randn(B, generator=g) * 20 + 5
    return pp, X, ret


def _slabs(tune, pp, X, ret, **kw):
    old_m = set_value_grad_mode(1)
    old_t = hip().set_value_grad_tune(tune)
    try:
        slab, loss = mlp_grad(GradHead.VALUE_MSE, pp, X, 1, H, ret=ret, **kw)
        slab, loss = slab.clone(), loss[:, :6].clone()  # the kernel writes six of the eight columns
        torch.cuda.synchronize()
    finally:
        hip().set_value_grad_tune(old_t)
        set_value_grad_mode(old_m)
    return slab, loss


@pytest.mark.parametrize("B", [1, 63, 64, 65, 128, 129, 383, 385, 657])
def test_pipelined_is_bitwise_v3_two_workgroups(cuda, B):
    """Grids sized for 2 CUs: one partial slab, exactly one and two slabs per workgroup, uneven
    slab counts, three and more slabs per workgroup (both image parities, all three x buffers)
    and a ragged last slab."""
    pp, X, ret = (t.to(cuda) for t in _inputs(4, B, 4000 + B))
    old = hip().set_cu_limit(2)
    try:
        s7, l7 = _slabs(PIPE, pp, X, ret)
        s3, l3 = _slabs(V3, pp, X, ret)
    finally:
        hip().set_cu_limit(old)
    assert s7.shape[0] == min((B + 63) // 64, 2)
    assert torch.isfinite(s7).all()
    assert torch.equal(s7, s3)
    assert torch.equal(l7, l3)


def test_pipelined_is_bitwise_v3_full_grid(cuda):
    pp, X, ret = (t.to(cuda) for t in _inputs(4, 70000, 74000))
    s7, l7 = _slabs(PIPE, pp, X, ret)
    s3, l3 = _slabs(V3, pp, X, ret)
    assert torch.equal(s7, s3)
    assert torch.equal(l7, l3)


def test_pipelined_device_row_count_matches_a_cut_batch(cuda):
    """A capacity of 657 rows with 385 valid ones (garbage behind them) is bitwise a cut batch of
    385 rows: the look-ahead of the slabs past nvalid contributes nothing."""
    cap, n = 657, 385
    pp, X, ret = (t.to(cuda) for t in _inputs(4, cap, 657385))
    X[n:] = float("nan")
    nv = torch.tensor([n], dtype=torch.int32, device=cuda)
    ibd = torch.tensor([1.0 / 7777.0], device=cuda)
    old = hip().set_cu_limit(2)
    try:
        s_dev, l_dev = _slabs(PIPE, pp, X, ret, inv_B=0.5, nvalid=nv, inv_B_dev=ibd)
        s_ref, l_ref = _slabs(PIPE, pp, X[:n].contiguous(), ret[:n].contiguous(), inv_B=1.0 / 7777.0)
    finally:
        hip().set_cu_limit(old)
    assert torch.isfinite(s_dev).all()
    assert torch.equal(s_dev, s_ref)
    assert torch.equal(l_dev, l_ref)
    assert int(l_dev.sum(0)[5].item()) == n


@pytest.mark.parametrize("D,B", [(4, 5000), (3, 777)])
def test_pipelined_matches_float64(cuda, D, B):
    """The body of test_split_kernel_variants_match_float64 for tune 240, with its bounds and its
    relu-kink filter."""
    pp, X, ret = _inputs(D, B, B + PIPE + D)
    keep = _away_from_relu_kinks(pp, X, D, H)
    X, ret = X[keep], ret[keep]
    B = X.shape[0]
    g64, loss64 = _grad64(pp, X, ret, D, H, 1.0 / B)
    old = hip().set_value_grad_tune(PIPE)
    try:
        gs, ls = _run(1, pp.to(cuda), X.to(cuda), ret.to(cuda), H)
        gs2, _ = _run(1, pp.to(cuda), X.to(cuda), ret.to(cuda), H)
    finally:
        hip().set_value_grad_tune(old)
    gf, _ = _run(0, pp.to(cuda), X.to(cuda), ret.to(cuda), H)
    scale = g64.abs().max().item()
    err_split = (gs - g64).abs().max().item() / scale
    err_fp32 = (gf - g64).abs().max().item() / scale
    assert err_split < 1e-5 and err_split <= 2.0 * err_fp32 + 2e-7, (err_split, err_fp32)
    assert abs(ls[0].item() - loss64) <= 1e-5 * abs(loss64) + 1e-6
    assert torch.equal(gs, gs2)


def test_pipelined_is_deterministic(cuda):
    pp, X, ret = (t.to(cuda) for t in _inputs(4, 32768, 32768))
    ref, lref = _slabs(PIPE, pp, X, ret)
    for _ in range(12):
        s, ls = _slabs(PIPE, pp, X, ret)
        assert torch.equal(s, ref)
        assert torch.equal(ls, lref)
