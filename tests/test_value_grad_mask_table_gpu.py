"""The relu'(h2) mask table of the factored value step (csrc/kernels/value_grad.hip): dh1's B
fragments are looked up per mask byte -- byte (row, g, c) = the relu'(h2) bits of features
32 c + 8 g + {0..7} -- in a 256-entry table, so every byte value has to be met.

B = 128, D = 4.  The low nibble of a byte comes from the sign of b2 (the same for every row); the
high nibble follows the row: x[row][d] is 0 or a value in [1, 1.22] by bit d of (row mod 16), the
first four h1 units are relu(x[d] - 0.5) (W1 = identity rows, b1 = -0.5: 0 or in [0.5, 0.72]), and
the byte's features 4..7 have b2 = -1 and a W2 entry of 4 on unit d, so they are on exactly where
bit d of the row is.  Slot s = 4 c + g of row r then holds byte 16 (r mod 16) + s: all 256 values
over rows 0..15, again in each further 16 rows with other magnitudes.  The other weights are
generic and small enough (|their part of a layer-2 pre-activation| < 0.5) to leave every sign
where it was put, at least 0.3 from the relu kink.

Gradients and loss are compared with the fp32-MFMA kernel and with the float64 autograd oracle
under the bounds of tests/test_value_grad_gpu.py.
"""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.models.mlp_spec import MLPSpec

from test_value_grad_gpu import _grad64

H, D, B = 128, 4, 128


def _inputs():
    g = torch.Generator().manual_seed(256)
    spec = MLPSpec(D, H, 1, False)
    pp = spec.init(g)
    o = 0
    W1 = pp[o:o + H * D].view(H, D); o += H * D
    b1 = pp[o:o + H]; o += H
    W2 = pp[o:o + H * H].view(H, H); o += H * H
    b2 = pp[o:o + H]; o += H
    b1 += 0.05 * torch.randn(H, generator=g)
    W1[:4] = torch.eye(4)
    b1[:4] = -0.5
    W2.mul_(0.25)  # generic part: |W2[k] . h1| stays well below 0.5 (checked below)
    W2[:, :4] = 0.0
    for k in range(H):
        c, gg, e = k // 32, (k % 32) // 8, k % 8
        s = 4 * c + gg
        if e < 4:
            b2[k] = 1.0 if (s >> e) & 1 else -1.0
        else:
            b2[k] = -1.0
            W2[k, e - 4] = 4.0
    rows = torch.arange(B)
    bits = torch.stack([(rows >> d) & 1 for d in range(D)], 1).float()
    X = bits * (1.0 + 0.22 * (rows // 16).float()[:, None] / 7.0)
    ret = torch.randn(B, generator=g) * 20 + 5
    return pp, X, ret


def _mask_bytes(pp, X):
    """[B, 16] mask bytes (slot 4 c + g) from float64 pre-activations, and the smallest |z2|."""
    p = pp.double()
    o = 0
    W1 = p[o:o + H * D].view(H, D); o += H * D
    b1 = p[o:o + H]; o += H
    W2 = p[o:o + H * H].view(H, H); o += H * H
    b2 = p[o:o + H]
    z1 = X.double() @ W1.T + b1
    z2 = torch.relu(z1) @ W2.T + b2
    on = (z2 > 0).numpy().astype(np.int64).reshape(B, 16, 8)
    return (on << np.arange(8)).sum(-1), z2.abs().min().item(), z1.abs().min().item()


def test_inputs_meet_every_mask_byte():
    pp, X, _ = _inputs()
    by, margin2, margin1 = _mask_bytes(pp, X)
    assert margin2 > 0.3, margin2  # far from the layer-2 kink: every kernel takes the same side
    assert margin1 > 1e-5, margin1  # (layer 1: test_value_grad_gpu's kink distance)
    assert np.array_equal(by[:16].reshape(-1), np.arange(256))
    for r in range(B):
        assert np.array_equal(by[r], 16 * (r % 16) + np.arange(16))


def _blocks():
    o, out = 0, {}
    for name, n in (("dW1", H * D), ("db1", H), ("dW2", H * H), ("db2", H), ("dW3", H), ("db3", 1)):
        out[name] = slice(o, o + n)
        o += n
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cu_limit", [1, 0])  # two slabs on one workgroup (look-ahead variant) / one slab each
def test_every_mask_byte_matches_fp32_kernel_and_float64(cuda, cu_limit):
    from relayrl_prototype_amd.ops import hip

    from test_value_grad_gpu import _run

    pp, X, ret = _inputs()
    g64, loss64 = _grad64(pp, X, ret, D, H, 1.0 / B)
    old = hip().set_cu_limit(cu_limit)
    try:
        gs, ls = _run(1, pp.to(cuda), X.to(cuda), ret.to(cuda), H)
        gf, lf = _run(0, pp.to(cuda), X.to(cuda), ret.to(cuda), H)
    finally:
        hip().set_cu_limit(old)
    scale = g64.abs().max().item()
    for name, sl in _blocks().items():
        err_split = (gs[sl] - g64[sl]).abs().max().item() / scale
        err_fp32 = (gf[sl] - g64[sl]).abs().max().item() / scale
        print(name, "err_split", err_split, "err_fp32", err_fp32)
        assert err_fp32 < 1e-5, (name, err_fp32)
        assert err_split < 1e-5, (name, err_split, err_fp32)
        assert err_split <= 2.0 * err_fp32 + 2e-7, (name, err_split, err_fp32)
    assert abs(lf[0].item() - loss64) <= 1e-5 * abs(loss64) + 1e-6
    assert abs(ls[0].item() - loss64) <= 1e-5 * abs(loss64) + 1e-6
    assert int(ls[5].item()) == B
