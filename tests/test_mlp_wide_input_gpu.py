"""Observations of 33 .. 128 features on the GPU: the DT = 4 / 8 instances of the forward kernel and the wide-input
gradient kernel (csrc/kernels/mlp_forward.hip, mlp_grad_wide.hip) against the float64 oracles of ops/reference.py.
Every bound is BOUND_FACTOR times the fp32 oracle's own largest error against float64 at the same case; a scalar sum of
the loss slab also admits one fp32 rounding unit of the sum of its terms' magnitudes (docs/KERNELS.md, "Bounds of the
gradient tests").  Every output buffer of a launch that must write nothing is guarded."""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import FwdMode, GradHead, MLPSpec, grad_slabs, mlp_forward, mlp_grad, philox, reduce_slabs
from relayrl_prototype_amd.ops import reference as ref

import rollout_oracle as ro
from guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND_FACTOR = 4.0
# 33: one feature in the third tile, an empty fourth; 65: the first shape of 8 tiles; 100: a partial last tile; 128: full
SHAPES = [(33, 64), (65, 128), (100, 64), (128, 128)]
HEADS = [GradHead.PG_CAT, GradHead.PPO_CAT, GradHead.PG_GAUSS, GradHead.PPO_GAUSS, GradHead.VALUE_MSE]
GAUSS = (GradHead.PG_GAUSS, GradHead.PPO_GAUSS)
F64, F32 = torch.float64, torch.float32


def _grad_case(head, D, H, B, seed):
    """(A, params, X, the head's inputs), on the CPU.  Categorical heads: A = 3 and a mask that closes one action of
    some rows; Gaussian heads: A = 6."""
    gen = torch.Generator().manual_seed(seed)
    A = 6 if head in GAUSS else 3
    pp = MLPSpec(D, H, 1 if head == GradHead.VALUE_MSE else A, head in GAUSS).init(gen)
    X = torch.randn(B, D, generator=gen)
    if head == GradHead.VALUE_MSE:
        return A, pp, X, dict(ret=torch.randn(B, generator=gen) * 3)
    adv = torch.randn(B, generator=gen) * 2 + 0.3
    kw = dict(adv=adv, adv_stats=torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(B))]), ent_coef=0.01)
    if head in GAUSS:
        kw.update(actc=torch.randn(B, A, generator=gen) * 0.5, logp_old=-torch.rand(B, generator=gen) * 8)
    else:
        act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
        mask = torch.ones(B, A)
        mask[torch.arange(0, B, 5), (act[::5].long() + 1) % A] = 0.0  # never the action taken
        kw.update(act=act, mask=mask, logp_old=-torch.rand(B, generator=gen) * 2)
    if head in (GradHead.PG_CAT, GradHead.PG_GAUSS):
        del kw["logp_old"]
    return A, pp, X, kw


def _to_dev(kw):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}


def _assert_grad(tag, slab, loss, head, pp, X, A, H, kw, inv_B):
    """Gradient, the two scalar sums of the loss slab and the row count against the float64 oracle."""
    (g64, s64), (g32, s32) = (ref.mlp_grad_ref(int(head), pp, X, A, H, inv_B=inv_B, dtype=dt, **kw) for dt in (F64, F32))
    ls = loss.sum(0).cpu().double()
    second, col = ("v", 4) if head == GradHead.VALUE_MSE else ("entropy", 1)
    rows = "v_rows" if head == GradHead.VALUE_MSE else "ent_rows"
    checks = {"grad": (reduce_slabs(slab).cpu().double(), g64, g32.double(), 0.0),
              "loss": (ls[0], s64["loss"], s32["loss"], 2.0 ** -23 * float(s64["loss_rows"].abs().sum())),
              second: (ls[col], s64[second], s32[second], 2.0 ** -23 * float(s64[rows].abs().sum()))}
    for k, (got, w64, w32, unit) in checks.items():
        w64, w32 = torch.as_tensor(w64).double(), torch.as_tensor(w32).double()
        bound = BOUND_FACTOR * max(float((w32 - w64).abs().max()), unit)
        err = float((got - w64).abs().max())
        print(f"{tag} {k}: err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (k, err, bound)
    assert int(ls[5]) == len(X)


@pytest.mark.parametrize("device_rows", [False, True], ids=["B", "nvalid"])
@pytest.mark.parametrize("D,H", SHAPES)
@pytest.mark.parametrize("head", HEADS, ids=lambda h: h.name)
def test_wide_grad_matches_float64(cuda, head, D, H, device_rows):
    """B = 65 is a full slab plus one ragged row.  With nvalid = 49 the rows past it are poisoned and must stay inert."""
    B, nv = 65, 49
    A, pp, X, kw = _grad_case(head, D, H, B, 1000 * int(head) + D)
    n = nv if device_rows else B
    dkw, Xd = _to_dev(kw), X.to(DEV)
    if device_rows:
        Xd[nv:] = float("nan")
        for k in ("ret", "adv", "actc", "logp_old"):
            if k in dkw:
                dkw[k][nv:] = float("nan")
        if "act" in dkw:
            dkw["act"][nv:] = 99
        dkw["nvalid"] = torch.tensor([nv], dtype=torch.int32, device=DEV)
    slab, loss = mlp_grad(head, pp.to(DEV), Xd, A, H, inv_B=1.0 / B, **dkw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(slab).all())
    cut = {k: (v[:n] if torch.is_tensor(v) and k != "adv_stats" else v) for k, v in kw.items()}
    _assert_grad(f"{head.name} D = {D} H = {H} n = {n}", slab, loss, head, pp, X[:n], A, H, cut, 1.0 / B)


def test_wide_grad_restages_w1_for_every_slab(cuda):
    """One workgroup more than twice round the grid: workgroup 0 runs three slabs and stages W1 again for each, behind the
    barrier that frees the staging images.  Float64 bound, and a second launch gives the same bits."""
    D, H, head = 128, 128, GradHead.VALUE_MSE
    B = 2 * 64 * grad_slabs(1 << 22, DEV) + 65
    A, pp, X, kw = _grad_case(head, D, H, B, 7)
    out = [mlp_grad(head, pp.to(DEV), X.to(DEV), A, H, **_to_dev(kw)) for _ in range(2)]
    torch.cuda.synchronize()
    assert out[0][0].shape[0] == grad_slabs(1 << 22, DEV)
    _assert_grad(f"restage B = {B}", *out[0], head, pp, X, A, H, kw, 1.0 / B)
    # the kernels write six of a loss slab's eight columns
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1][:, :6], out[1][1][:, :6]), "two launches differ"


def _fwd_both(mode, pp, X, A, H, **kw):
    return tuple(ref.mlp_forward_ref(int(mode), pp, X, A, H, dtype=dt, **kw) for dt in (F64, F32))


@pytest.mark.parametrize("D,H", SHAPES)
def test_wide_forward_matches_float64(cuda, D, H):
    """B = 81: five full tiles and one of a single row, two workgroups.  The logits are compared unmasked (a closed
    action's logit is -1e8, whose fp32 spacing is 8); the mask is held through CAT_EVAL's log-prob and entropy."""
    B, A = 81, 5
    gen = torch.Generator().manual_seed(D)
    X = torch.randn(B, D, generator=gen)
    pv, pc, pg = (MLPSpec(D, H, a, g).init(gen) for a, g in ((1, False), (A, False), (A, True)))
    mask = (torch.rand(B, A, generator=gen) > 0.2).float()
    mask[:, 0] = 1.0
    act = torch.zeros(B, dtype=torch.int32)
    actc = torch.randn(B, A, generator=gen) * 0.5
    runs = [(FwdMode.VALUE, pv, {}, ("v",)), (FwdMode.LOGITS, pc, {}, ("logits",)),
            (FwdMode.CAT_EVAL, pc, dict(mask=mask, act_in=act), ("logp", "entropy")),
            (FwdMode.GAUSS_EVAL, pg, dict(actc_in=actc), ("logp", "entropy", "mean"))]
    for mode, pp, kw, keys in runs:
        r64, r32 = _fwd_both(mode, pp, X, A, H, **kw)
        got = mlp_forward(mode, pp.to(DEV), X.to(DEV), A, H, **_to_dev(kw))
        for k in keys:
            bound = BOUND_FACTOR * float((r32[k].double() - r64[k]).abs().max())
            err = float((got[k].cpu().double() - r64[k]).abs().max())
            print(f"D = {D} H = {H} {mode.name} {k}: err {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (mode.name, k, err, bound)


def test_wide_forward_samples_the_oracles_actions(cuda):
    """CAT_SAMPLE at (65, 128): the Philox draw of every row against the float64 cdf.  Rows whose uniform lies within the
    bound of a cdf step are left out; by the two oracles alone they are at most MAX_SKIP_SHARE of the rows."""
    D, H, A, B, seed, step, off = 65, 128, 6, 400, 1234567, 42, 100
    gen = torch.Generator().manual_seed(3)
    X, pp = torch.randn(B, D, generator=gen), MLPSpec(D, H, A).init(gen)
    r64, r32 = _fwd_both(FwdMode.CAT_SAMPLE, pp, X, A, H, seed=seed, step=step, row_offset=off)
    cdf64, cdf32 = (torch.cumsum(torch.softmax(r["logits"], -1), -1).double() for r in (r64, r32))
    bound = BOUND_FACTOR * float((cdf32 - cdf64).abs().max())
    u = torch.from_numpy(philox.uniforms(seed, step, np.arange(B, dtype=np.uint64) + np.uint64(off), 0)[0]).double()
    clear = (u.unsqueeze(-1) - cdf64).abs().min(-1).values > bound
    assert int((~clear).sum()) <= ro.MAX_SKIP_SHARE * B and bool((r32["act"] == r64["act"])[clear].all())
    got = mlp_forward(FwdMode.CAT_SAMPLE, pp.to(DEV), X.to(DEV), A, H, seed=seed, step=step, row_offset=off)
    assert len(torch.unique(r64["act"])) == A, "the weights must make every action occur"
    assert torch.equal(got["act"].cpu()[clear], r64["act"][clear])
    lbound = BOUND_FACTOR * float((r32["logp"].double() - r64["logp"])[clear].abs().max())
    assert float((got["logp"].cpu().double() - r64["logp"])[clear].abs().max()) <= lbound


def test_wide_refusals_write_nothing(cuda):
    """D = 129 is refused by name with nothing written; the Q heads still stop at D = 32."""
    H, A, B = 64, 3, 8
    X, pp = torch.zeros(B, 129, device=DEV), torch.zeros(MLPSpec(129, H, A).P, device=DEV)
    gs, gl, lo = Guarded((1, pp.numel())), Guarded((1, 8)), Guarded((B, A))
    z = torch.zeros(B, device=DEV)
    with pytest.raises(ValueError, match="128.*129"):
        mlp_grad(GradHead.PG_CAT, pp, X, A, H, act=z.int(), adv=z, grad_slab=gs.t, loss_slab=gl.t)
    with pytest.raises(ValueError, match="128.*129"):
        mlp_forward(FwdMode.LOGITS, pp, X, A, H, out=dict(logits=lo.t))
    q = torch.zeros(MLPSpec(33, H, A).P, device=DEV)
    gq = Guarded((1, q.numel()))
    with pytest.raises((ValueError, RuntimeError), match="32"):
        mlp_grad(GradHead.Q_TD, q, X[:, :33], A, H, act=z.int(), ret=z, grad_slab=gq.t, loss_slab=gl.t)
    torch.cuda.synchronize()
    for b in (gs, gl, lo, gq):
        assert b.guards_intact() and bool(torch.isnan(b.t).all())


def test_ppo_learner_on_wide_observations_matches_the_cpu_learner(cuda):
    """One PPO epoch (two policy steps, three value steps) at obs_dim 40: the HIP learner's parameters against the CPU
    learner's (fp32 autograd and a reference Adam step), to the tolerances of the trainer tests."""
    from relayrl_prototype_amd.algorithms.learner import PGLearner

    D, A, B = 40, 3, 200
    gen = torch.Generator().manual_seed(0)
    obs = torch.randn(B, D, generator=gen)
    act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
    adv, ret = torch.randn(B, generator=gen), torch.randn(B, generator=gen)
    logp_old = -torch.rand(B, generator=gen) - 0.6
    stats = torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(B))])
    out = []
    for dev in ("cpu", cuda):
        lr = PGLearner("ppo", obs_dim=D, act_dim=A, hidden=64, train_vf_iters=3, train_pi_iters=2, device=dev, seed=1)
        p0 = lr.pi.params.clone()
        lr.optimize(obs.to(dev), act=act.to(dev), adv=adv.to(dev), ret=ret.to(dev), adv_stats=stats.to(dev),
                    logp_old=logp_old.to(dev))
        assert not torch.equal(p0, lr.pi.params)
        out.append((lr.pi.params.cpu(), lr.vf.params.cpu()))
    for got, want in zip(out[1], out[0]):
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
