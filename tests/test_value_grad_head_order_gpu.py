"""The summation order of the head dot product of the bf16x6 kernels (csrc/kernels/value_grad.hip),
pinned independently of how the kernel reduces.

V of a row is sum_k w3[k] h2[k] + b3 in this order (docs/KERNELS.md): wave w owns features
16 w .. 16 w + 15; lane group g of the wave takes features 16 w + 4 g + r and chains r = 0..3
(multiply, then three fused multiply-adds); the four lane-group partials are added as
(g0 + g1) + (g2 + g3); the eight wave partials as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7));
b3 is added last.

The inputs make every product exact and the order visible: W2 = 0, so h2 = relu(b2) for every
row, and b2 / w3 are powers of two (2^24 .. 2^-3 products, mixed signs, some b2 < 0) drawn so that
the large terms cancel differently under different associations.  The order is emulated in numpy
float32 (every intermediate is a sum of a few dyadic numbers that float64 holds exactly, so a
float64 operation rounded to float32 is the fused fp32 operation), the emulation is checked to
tell the documented order from five others, and the kernels must match it bit for bit: the
value-forward output, and the grad kernel's loss with ret placed a dyadic distance from V (a loss
of exactly representable squares, the same in any summation order).
"""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.models.mlp_spec import MLPSpec

H, D = 128, 4
F32 = np.float32


def _fma(a, b, c):
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def _head(w3, h2, b3, lane="fwd", group="pair", wave="tree"):
    """The head output for one row under a given order (the documented one by default)."""
    wp = []
    for w in range(8):
        gp = []
        for g in range(4):
            k = 16 * w + 4 * g
            rs = range(4) if lane == "fwd" else range(3, -1, -1)
            acc = None
            for r in rs:
                acc = F32(w3[k + r] * h2[k + r]) if acc is None else _fma(w3[k + r], h2[k + r], acc)
            gp.append(acc)
        if group == "pair":
            s = F32(F32(gp[0] + gp[1]) + F32(gp[2] + gp[3]))
        elif group == "seq":
            s = F32(F32(F32(gp[0] + gp[1]) + gp[2]) + gp[3])
        elif group == "02_13":
            s = F32(F32(gp[0] + gp[2]) + F32(gp[1] + gp[3]))
        else:  # "03_12"
            s = F32(F32(gp[0] + gp[3]) + F32(gp[1] + gp[2]))
        wp.append(s)
    if wave == "tree":
        t = F32(F32(F32(wp[0] + wp[1]) + F32(wp[2] + wp[3])) + F32(F32(wp[4] + wp[5]) + F32(wp[6] + wp[7])))
    else:
        t = wp[0]
        for w in range(1, 8):
            t = F32(t + wp[w])
    return F32(t + b3)


ALTERNATIVES = [dict(group="seq"), dict(group="02_13"), dict(group="03_12"), dict(wave="seq"), dict(lane="rev")]


def _terms(rng):
    """128 products w3[k] h2[k]: pairs +m / -m of powers of two (so the exact sum is small), placed
    at random features, plus odd +-1 and +-1/8 terms; and their factors w3, b2."""
    mags = [2.0 ** 24, 2.0 ** 12, 1.0, 0.125]
    t = np.zeros(H)
    perm = rng.permutation(H)
    for i in range(0, 96, 2):
        m = mags[rng.integers(0, 3)]
        s = 1.0 if rng.integers(0, 2) else -1.0
        t[perm[i]], t[perm[i + 1]] = s * m, -s * m
    for i in range(96, 120):
        t[perm[i]] = (1.0 if rng.integers(0, 2) else -1.0) * mags[rng.integers(2, 4)]
    # perm[120:]: features with b2 < 0 (h2 = 0, product 0 whatever w3 is)
    e = rng.integers(-2, 3, size=H)  # h2 = 2^e where it is positive
    b2 = np.where(t != 0, 2.0 ** e, -(2.0 ** e))
    w3 = np.where(t != 0, t / 2.0 ** e, 2.0 ** 10)
    return w3.astype(F32), b2.astype(F32)


def _value_case(seed):
    rng = np.random.default_rng(seed)
    w3, b2 = _terms(rng)
    return w3, b2, F32(0.375)


def _params(w3_rows, b2, b3, A):
    """Flat parameters: W1 / b1 generic (they meet W2 = 0), W2 = 0, b2, W3 rows, b3."""
    spec = MLPSpec(D, H, A, False)
    g = torch.Generator().manual_seed(5)
    pp = spec.init(g)
    o = H * D + H
    pp[o:o + H * H] = 0.0
    o += H * H
    pp[o:o + H] = torch.from_numpy(b2)
    o += H
    for a in range(A):
        pp[o:o + H] = torch.from_numpy(w3_rows[a])
        o += H
    pp[o:o + A] = torch.from_numpy(np.asarray(b3, dtype=F32).reshape(A))
    assert o + A == spec.P
    return pp


VALUE_SEEDS = [7, 35]
CAT_SEED = 86


@pytest.mark.parametrize("seed", VALUE_SEEDS)
def test_emulation_tells_the_orders_apart(seed):
    """(CPU) The inputs do what they are for: each other association or order gives another V."""
    w3, b2, b3 = _value_case(seed)
    h2 = np.maximum(b2, F32(0))
    v = _head(w3, h2, b3)
    assert abs(float(v)) <= 64.0
    for alt in ALTERNATIVES:
        assert _head(w3, h2, b3, **alt) != v, alt


def test_lane_swap_network_keeps_the_association():
    """(CPU) The reduce-scatter over the lane groups: v_permlane16_swap exchanges the odd 16-lane
    rows of its first operand with the even rows of its second, v_permlane32_swap rows 2, 3 of the
    first with rows 0, 1 of the second (CDNA4 ISA).  Three swaps and three adds leave lane group
    g with (r0 + r1) + (r2 + r3) of value g, the one-value form's association."""
    def swap16(a, b):
        a, b = a.copy(), b.copy()
        for hi in (0, 2):
            a[hi + 1], b[hi] = b[hi].copy(), a[hi + 1].copy()
        return a, b

    def swap32(a, b):
        a, b = a.copy(), b.copy()
        a[2:], b[:2] = b[:2].copy(), a[2:].copy()
        return a, b

    rng = np.random.default_rng(0)
    pv = (rng.standard_normal((4, 4, 16)) * 10.0 ** rng.integers(-3, 4, size=(4, 4, 16))).astype(F32)  # [value][row][lane]
    a0, a1 = swap16(pv[0], pv[1])
    b0, b1 = swap16(pv[2], pv[3])
    c0, c1 = swap32(a0 + a1, b0 + b1)
    out = c0 + c1
    for g in range(4):
        want = (pv[g][0] + pv[g][1]) + (pv[g][2] + pv[g][3])
        assert np.array_equal(out[g], want)
    # the OR form: one permlane32_swap(x01, x23), one permlane16_swap of the result with itself
    x = rng.integers(0, 2 ** 32, size=(2, 4, 16), dtype=np.uint64).astype(np.uint32)
    p0, p1 = swap32(x[0], x[1])
    c = p0 | p1
    q0, q1 = swap16(c, c)
    o = q0 | q1
    for g in range(4):
        src = x[0] if g < 2 else x[1]
        assert np.array_equal(o[g], src[0] | src[1] | src[2] | src[3])


def _value_run(cuda, seed, B, cu_limit):
    from relayrl_prototype_amd.ops import FwdMode, GradHead, hip, mlp_forward, mlp_grad, set_value_grad_mode

    w3, b2, b3 = _value_case(seed)
    v = _head(w3, np.maximum(b2, F32(0)), b3)
    pp = _params([w3], b2, [b3], 1).to(cuda)
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(B, D, generator=g) * 1.5).to(cuda)
    # ret a dyadic distance from V: every (V - ret)^2 and their sum are exact in fp32
    d = np.array([0.5, 1.0, 2.0, -1.0, -0.25], dtype=F32)[np.arange(B) % 5]
    ret = (v - d).astype(F32)
    assert np.array_equal((v - ret).astype(F32), d)
    old_m = set_value_grad_mode(1)
    old_f = hip().set_value_fwd_mode(1)
    old_c = hip().set_cu_limit(cu_limit)
    try:
        vf = mlp_forward(FwdMode.VALUE, pp, X, 1, H)["v"].cpu().numpy()
        _, ls = mlp_grad(GradHead.VALUE_MSE, pp, X, 1, H, ret=torch.from_numpy(ret).to(cuda))
        ls = ls[:, :6].sum(0).cpu().numpy()
    finally:
        hip().set_cu_limit(old_c)
        hip().set_value_fwd_mode(old_f)
        set_value_grad_mode(old_m)
    return v, vf, ls, float(np.sum(d.astype(np.float64) ** 2))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", VALUE_SEEDS)
@pytest.mark.parametrize("B,cu_limit", [(128, 1), (64, 1), (128, 0)])
def test_value_head_order_is_the_documented_one(cuda, seed, B, cu_limit):
    """B = 128 on one workgroup: two slabs, the look-ahead variant; B = 64 (and B = 128 on two
    workgroups): one slab per workgroup, variant V = 3."""
    v, vf, ls, loss = _value_run(cuda, seed, B, cu_limit)
    print("emulated V", float(v), "forward V", set(vf.tolist()), "loss", float(ls[0]), "expected", loss)
    assert vf.dtype == np.float32 and np.array_equal(vf.view(np.uint32), np.full(B, v).view(np.uint32))
    assert float(ls[0]) == loss
    assert int(ls[5]) == B


def _cat_case():
    rng = np.random.default_rng(CAT_SEED)
    w30, b2 = _terms(rng)
    # the second action's row: the same |products| with another draw of signs at the same features
    flip = np.where(rng.integers(0, 2, size=H) > 0, F32(1), F32(-1))
    w31 = (w30 * flip).astype(F32)
    return np.stack([w30, w31]), b2, np.array([0.25, -0.5], dtype=F32)


def _cat_loss(l0, l1, B):
    """sum over B rows of -log p(action 0) and of the entropy, float64, from fp32 logits."""
    z = np.array([float(l0), float(l1)])
    lse = z.max() + np.log(np.exp(z - z.max()).sum())
    lp = z - lse
    return -B * lp[0], -B * float((np.exp(lp) * lp).sum())


def test_cat_emulation_tells_the_orders_apart():
    w3, b2, b3 = _cat_case()
    h2 = np.maximum(b2, F32(0))
    l = [_head(w3[a], h2, b3[a]) for a in range(2)]
    assert abs(float(l[0]) - float(l[1])) <= 8.0
    loss, _ = _cat_loss(l[0], l[1], 128)
    for alt in ALTERNATIVES:
        la = [_head(w3[a], h2, b3[a], **alt) for a in range(2)]
        assert abs(_cat_loss(la[0], la[1], 128)[0] - loss) > 1e-2 * max(1.0, abs(loss)), alt


@pytest.mark.gpu
def test_cat2_head_order_is_the_documented_one(cuda):
    """NA = 2 categorical head (the CartPole policy step), two slabs on one workgroup.  The kernel
    gives no logits out, so they are checked through the loss and the entropy they determine:
    -log softmax(l)[0] summed over the rows, against float64 from the emulated fp32 logits.  The
    bound is the device exp / log's (1e-5 relative is ~100 fp32 ulps); another order moves the loss
    by more than 1e-2 relative (test_cat_emulation_tells_the_orders_apart)."""
    from relayrl_prototype_amd.ops import GradHead, hip, mlp_grad, set_value_grad_mode

    B = 128
    w3, b2, b3 = _cat_case()
    h2 = np.maximum(b2, F32(0))
    l0, l1 = (_head(w3[a], h2, b3[a]) for a in range(2))
    loss, ent = _cat_loss(l0, l1, B)
    pp = _params(w3, b2, b3, 2).to(cuda)
    g = torch.Generator().manual_seed(1)
    X = (torch.randn(B, D, generator=g) * 1.5).to(cuda)
    act = torch.zeros(B, dtype=torch.int32, device=cuda)
    adv = torch.ones(B, device=cuda)
    old_m = set_value_grad_mode(1)
    old_c = hip().set_cu_limit(1)
    try:
        _, ls = mlp_grad(GradHead.PG_CAT, pp, X, 2, H, act=act, adv=adv)
        ls = ls[:, :6].sum(0).double().cpu().numpy()
    finally:
        hip().set_cu_limit(old_c)
        set_value_grad_mode(old_m)
    print("emulated logits", float(l0), float(l1), "loss", ls[0], "expected", loss, "entropy", ls[1], "expected", ent)
    assert abs(ls[0] - loss) <= 1e-5 * max(1.0, abs(loss))
    assert abs(ls[1] - ent) <= 1e-5 * max(1.0, abs(ent)) + 1e-5 * B
    assert int(ls[5]) == B
