"""Categorical policies of 17 .. 64 actions on the GPU: the forward and gradient kernels of csrc/kernels/mlp_cat_wide.hip
(the wide MFMA output layer) against the float64 oracles of ops/reference.py.  Every bound is BOUND_FACTOR times the
fp32 oracle's own largest error against float64 at the same case; a scalar sum of the loss slab also admits one fp32
rounding unit of the sum of its terms' magnitudes (docs/KERNELS.md, "Bounds of the gradient tests").  Every output
buffer of a launch that must write nothing is guarded."""
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
# 17: one logit in the second tile; 33: the first 3-tile shape, one logit in the third; 48: a full third; 64: 4 tiles, full
ACTIONS = [17, 33, 48, 64]
# (4, 64): one input tile; (20, 128): two input tiles, the second partial, and the tightest LDS
TRUNKS = [(4, 64), (20, 128)]
HEADS = [GradHead.PG_CAT, GradHead.PPO_CAT]
F64, F32 = torch.float64, torch.float32


def _grad_case(head, D, H, A, B, seed):
    """(params, X, the head's inputs), on the CPU.  Every fifth row closes the last action of every 16-logit tile and
    takes none of them."""
    gen = torch.Generator().manual_seed(seed)
    pp, X = MLPSpec(D, H, A).init(gen), torch.randn(B, D, generator=gen)
    adv = torch.randn(B, generator=gen) * 2 + 0.3
    act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
    closed = torch.tensor(sorted({min(16 * t + 15, A - 1) for t in range((A + 15) // 16)}))
    act[::5] = torch.where(torch.isin(act[::5], closed), torch.zeros_like(act[::5]), act[::5])
    mask = torch.ones(B, A)
    mask[::5, closed] = 0.0
    kw = dict(adv=adv, adv_stats=torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(B))]), ent_coef=0.01,
              act=act, mask=mask)
    if head == GradHead.PPO_CAT:
        kw["logp_old"] = -torch.rand(B, generator=gen) * 2 - np.log(A) + 1
    return pp, X, kw


def _to_dev(kw):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}


def _assert_grad(tag, slab, loss, head, pp, X, A, H, kw, inv_B):
    """Gradient, the two scalar sums of the loss slab and the row count against the float64 oracle."""
    (g64, s64), (g32, s32) = (ref.mlp_grad_ref(int(head), pp, X, A, H, inv_B=inv_B, dtype=dt, **kw) for dt in (F64, F32))
    ls = loss.sum(0).cpu().double()
    checks = {"grad": (reduce_slabs(slab).cpu().double(), g64, g32.double(), 0.0),
              "loss": (ls[0], s64["loss"], s32["loss"], 2.0 ** -23 * float(s64["loss_rows"].abs().sum())),
              "entropy": (ls[1], s64["entropy"], s32["entropy"], 2.0 ** -23 * float(s64["ent_rows"].abs().sum()))}
    for k, (got, w64, w32, unit) in checks.items():
        w64, w32 = torch.as_tensor(w64).double(), torch.as_tensor(w32).double()
        bound = BOUND_FACTOR * max(float((w32 - w64).abs().max()), unit)
        err = float((got - w64).abs().max())
        print(f"{tag} {k}: err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (k, err, bound)
    assert int(ls[5]) == len(X)


@pytest.mark.parametrize("device_rows", [False, True], ids=["B", "nvalid"])
@pytest.mark.parametrize("D,H", TRUNKS)
@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("head", HEADS, ids=lambda h: h.name)
def test_wide_actions_grad_matches_float64(cuda, head, A, D, H, device_rows):
    """B = 65 is a full slab plus one ragged row.  With nvalid = 49 the rows past it are poisoned and must stay inert."""
    B, nv = 65, 49
    pp, X, kw = _grad_case(head, D, H, A, B, 1000 * int(head) + 10 * A + D)
    n = nv if device_rows else B
    dkw, Xd = _to_dev(kw), X.to(DEV)
    if device_rows:
        Xd[nv:] = float("nan")
        for k in ("adv", "logp_old"):
            if k in dkw:
                dkw[k][nv:] = float("nan")
        dkw["act"][nv:] = 99
        dkw["nvalid"] = torch.tensor([nv], dtype=torch.int32, device=DEV)
    slab, loss = mlp_grad(head, pp.to(DEV), Xd, A, H, inv_B=1.0 / B, **dkw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(slab).all())
    cut = {k: (v[:n] if torch.is_tensor(v) and k != "adv_stats" else v) for k, v in kw.items()}
    _assert_grad(f"{head.name} A = {A} D = {D} H = {H} n = {n}", slab, loss, head, pp, X[:n], A, H, cut, 1.0 / B)


def test_wide_actions_grad_restages_w3_for_every_slab(cuda):
    """One workgroup more than twice round the grid: workgroup 0 runs three slabs and stages the padded W3 again for the
    second and third.  Float64 bound, and a second launch gives the same bits."""
    D, H, A, head = 20, 128, 64, GradHead.PPO_CAT
    B = 2 * 64 * grad_slabs(1 << 22, DEV) + 65
    pp, X, kw = _grad_case(head, D, H, A, B, 7)
    out = [mlp_grad(head, pp.to(DEV), X.to(DEV), A, H, **_to_dev(kw)) for _ in range(2)]
    torch.cuda.synchronize()
    assert out[0][0].shape[0] == grad_slabs(1 << 22, DEV)
    _assert_grad(f"restage B = {B}", *out[0], head, pp, X, A, H, kw, 1.0 / B)
    # the kernels write six of a loss slab's eight columns
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1][:, :6], out[1][1][:, :6]), "two launches differ"


def _fwd_both(mode, pp, X, A, H, **kw):
    return tuple(ref.mlp_forward_ref(int(mode), pp, X, A, H, dtype=dt, **kw) for dt in (F64, F32))


@pytest.mark.parametrize("D,H", TRUNKS)
@pytest.mark.parametrize("A", ACTIONS)
def test_wide_actions_forward_matches_float64(cuda, A, D, H):
    """B = 81: five full tiles and one of a single row, two workgroups.  The logits are compared unmasked (a closed
    action's logit is -1e8, whose fp32 spacing is 8); the mask is held through CAT_EVAL's log-prob and entropy, with
    act_in = row % A over every tile and always open."""
    B = 81
    gen = torch.Generator().manual_seed(100 * A + D)
    X, pp = torch.randn(B, D, generator=gen), MLPSpec(D, H, A).init(gen)
    act = (torch.arange(B) % A).to(torch.int32)
    mask = (torch.rand(B, A, generator=gen) > 0.2).float()
    mask[:, 0] = 1.0
    mask[torch.arange(B), act.long()] = 1.0
    runs = [(FwdMode.LOGITS, {}, ("logits",)), (FwdMode.CAT_EVAL, dict(mask=mask, act_in=act), ("logp", "entropy"))]
    for mode, kw, keys in runs:
        r64, r32 = _fwd_both(mode, pp, X, A, H, **kw)
        got = mlp_forward(mode, pp.to(DEV), X.to(DEV), A, H, **_to_dev(kw))
        for k in keys:
            bound = BOUND_FACTOR * float((r32[k].double() - r64[k]).abs().max())
            err = float((got[k].cpu().double() - r64[k]).abs().max())
            print(f"A = {A} D = {D} H = {H} {mode.name} {k}: err {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (mode.name, k, err, bound)


@pytest.mark.parametrize("A", [64, 17])
def test_wide_actions_forward_samples_the_oracles_actions(cuda, A):
    """CAT_SAMPLE: the Philox draw of every row against the float64 cdf.  Rows whose uniform lies within the bound of a
    cdf step are left out; by the two oracles alone they are at most MAX_SKIP_SHARE of the rows, and the float64 draws
    reach every lane group's quarter of every 16-logit tile."""
    D, H, B, seed, step, off = 20, 128, 600, 1234567, 42, 100
    gen = torch.Generator().manual_seed(A)
    X, pp = torch.randn(B, D, generator=gen), MLPSpec(D, H, A).init(gen)
    r64, r32 = _fwd_both(FwdMode.CAT_SAMPLE, pp, X, A, H, seed=seed, step=step, row_offset=off)
    cdf64, cdf32 = (torch.cumsum(torch.softmax(r["logits"], -1), -1).double() for r in (r64, r32))
    bound = BOUND_FACTOR * float((cdf32 - cdf64).abs().max())
    u = torch.from_numpy(philox.uniforms(seed, step, np.arange(B, dtype=np.uint64) + np.uint64(off), 0)[0]).double()
    clear = (u.unsqueeze(-1) - cdf64).abs().min(-1).values > bound
    assert int((~clear).sum()) <= ro.MAX_SKIP_SHARE * B and bool((r32["act"] == r64["act"])[clear].all())
    assert set((r64["act"] // 4).tolist()) == {i // 4 for i in range(A)}, "the draws must reach every quarter tile"
    got = mlp_forward(FwdMode.CAT_SAMPLE, pp.to(DEV), X.to(DEV), A, H, seed=seed, step=step, row_offset=off)
    assert torch.equal(got["act"].cpu()[clear], r64["act"][clear])
    lbound = BOUND_FACTOR * float((r32["logp"].double() - r64["logp"])[clear].abs().max())
    assert float((got["logp"].cpu().double() - r64["logp"])[clear].abs().max()) <= lbound


def test_wide_actions_refusals_write_nothing(cuda):
    """65 actions, 17 actions with a head or mode that holds 16 outputs, and 17 actions at D = 33 are refused by range
    and value, with nothing written."""
    H, B = 64, 8
    z = torch.zeros(B, device=DEV)
    gl, guards = Guarded((1, 8)), []

    def grad(head, A, D, match, **kw):
        pp = torch.zeros(MLPSpec(D, H, A, "actc" in kw).P, device=DEV)
        gs = Guarded((1, pp.numel()))
        guards.append(gs)
        with pytest.raises(ValueError, match=match):
            mlp_grad(head, pp, torch.zeros(B, D, device=DEV), A, H, grad_slab=gs.t, loss_slab=gl.t, **kw)

    def fwd(mode, A, D, match, key, **kw):
        pp = torch.zeros(MLPSpec(D, H, A, "actc_in" in kw).P, device=DEV)
        out = {k: Guarded((B, A) if k in ("logits", "mean") else (B,)) for k in (key, "logp", "entropy")}
        guards.extend(out.values())
        with pytest.raises(ValueError, match=match):
            mlp_forward(mode, pp, torch.zeros(B, D, device=DEV), A, H, out={k: g.t for k, g in out.items()}, **kw)

    grad(GradHead.PG_CAT, 65, 4, r"\[1, 64\].*65", act=z.int(), adv=z)
    fwd(FwdMode.LOGITS, 65, 4, r"\[1, 64\].*65", "logits")
    grad(GradHead.PG_GAUSS, 17, 4, r"\[1, 16\].*17", actc=torch.zeros(B, 17, device=DEV), adv=z)
    grad(GradHead.Q_TD, 17, 4, r"\[1, 16\].*17", act=z.int(), ret=z)
    fwd(FwdMode.GAUSS_EVAL, 17, 4, r"\[1, 16\].*17", "mean", actc_in=torch.zeros(B, 17, device=DEV))
    grad(GradHead.PG_CAT, 17, 33, r"\[1, 32\].*33", act=z.int(), adv=z)
    fwd(FwdMode.LOGITS, 17, 33, r"\[1, 32\].*33", "logits")
    torch.cuda.synchronize()
    for b in [gl] + guards:
        assert b.guards_intact() and bool(torch.isnan(b.t).all())


def test_ppo_learner_on_18_actions_matches_the_cpu_learner(cuda):
    """One PPO epoch (two policy steps, three value steps) at act_dim 18, Atari's full action set: the HIP learner's
    parameters against the CPU learner's (fp32 autograd and a reference Adam step), to the trainer tests' tolerances."""
    from relayrl_prototype_amd.algorithms.learner import PGLearner

    D, A, B = 8, 18, 200
    gen = torch.Generator().manual_seed(0)
    obs = torch.randn(B, D, generator=gen)
    act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
    adv, ret = torch.randn(B, generator=gen), torch.randn(B, generator=gen)
    logp_old = -torch.rand(B, generator=gen) - 2.4
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
