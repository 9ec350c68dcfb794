"""The quantile-regression head (QR-DQN) on the GPU: the QR instances of the actor, the evaluator and the targets
kernel (csrc/kernels/dqn.hip, evaluate.hip), the HEAD_Q_QR gradient head (mlp_grad.hip) and the quantile
DQNTrainer, against the float64 host oracles (ops/reference.py, ops/dqn.py, tests/dqn_quantile_oracle.py).
Every output buffer of a kernel under test is guarded."""
import os

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import EvalTrace, GradHead, MLPSpec, dqn_nstep_walk_ref, dqn_rollout, dqn_rollout_grid
from relayrl_prototype_amd.ops import dqn_sample_rows_ref, dqn_targets, evaluate_policy_op, hip, mlp_grad, mlp_grad_qr
from relayrl_prototype_amd.ops import per_sample_rows_ref, reduce_slabs
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer

import dqn_oracle as do
import dqn_quantile_oracle as dq
import rollout_oracle as ro
from guarded import INT_SENTINEL, Guarded
from test_dqn_gpu import FWD_TOL, RING_SEED, TGT_C, TGT_N, TGT_T, TRAINER, _bits, cu_limit, guarded_ring, random_ring
from test_per_gpu import guarded_tree, random_leaves

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(2, 8), (4, 4), (3, 5), (2, 1), (1, 16)]  # (A, NQ)


def same_bits(a, b):
    return np.array_equal(_bits(a.t.cpu().numpy()), _bits(b.t.cpu().numpy()))


def qr_params(e, H, NQ):
    return MLPSpec(e.D, H, e.A * NQ).init(torch.Generator().manual_seed(3 + e.env_id))


def untouched(*bufs):
    for b in bufs:
        whole = b.big.cpu()
        assert bool(torch.isnan(whole).all()) if whole.dtype.is_floating_point else bool((whole == INT_SENTINEL).all())


# ------------------------------------------------------------------ 1. actor
ACT_T, ACT_STEP0 = 3, 5
ACTOR_CASES = [(name, NQ, H, N) for name, nqs in (("CartPole-v1", (1, 3, 8)), ("LunarLanderSynth-v0", (1, 4)))
               for NQ in nqs for H in (64, 128) for N in (17, 1400)]


def actor_launch(e, pdev, H, N, eps, NQ):
    g, ring = guarded_ring(ACT_T, N, e.D)
    persist = (Guarded((N, e.NS)), Guarded((N,), torch.int32), Guarded((N,)))
    stats = Guarded((dqn_rollout_grid(N), 8), fill=float(INT_SENTINEL))
    rc = dqn_rollout(e.env_id, pdev, H, ACT_T, 0, ring, persist[0].t, persist[1].t, persist[2].t, stats.t,
                     seed=RING_SEED, step0=ACT_STEP0, epsilon=eps, reset_all=True, max_steps=e.max_steps, quantiles=NQ)
    torch.cuda.synchronize()
    assert rc == 0
    bufs = dict(g, state=persist[0], ep_len=persist[1], ep_ret=persist[2], ep_stats=stats)
    for k, b in bufs.items():
        assert b.guards_intact(), f"{k}: the kernel wrote outside its buffer"
    return bufs


@pytest.mark.parametrize("name,NQ,H,N", ACTOR_CASES)
def test_quantile_actor_acts_on_the_sums(cuda, name, NQ, H, N):
    """T = 3 steps from the Philox reset into a ring of 3 slots; N = 17 is a ragged tile, N = 1400 is 88 tiles."""
    e = ro.env_of(name)
    params = qr_params(e, H, NQ)
    pdev = params.to(DEV)
    envs = np.arange(N)
    for eps in (0.0, 0.3, 1.0):
        bufs = actor_launch(e, pdev, H, N, eps, NQ)
        run = {k: bufs[k].t.cpu().numpy() for k in ("obs", "nobs", "act", "rew", "done")}
        obs, nobs, act, rew, done = (run[k] for k in ("obs", "nobs", "act", "rew", "done"))
        assert int(act.min()) >= 0 and int(act.max()) < e.A
        skipped = 0
        for t in range(ACT_T):
            explore, a_rand, _ = do.explore_draws(RING_SEED, ACT_STEP0 + t, envs, eps, e.A)
            assert explore.all() == (eps == 1.0) and (eps > 0.0 or not explore.any())
            a64, gap, tol = dq.sum_gap_tolerance(params, obs[t], e.A, NQ, H)
            np.testing.assert_array_equal(act[t][explore], a_rand[explore])
            clear = ~explore & (gap >= tol)
            np.testing.assert_array_equal(act[t][clear], a64[clear])
            skipped += int((~explore & (gap < tol)).sum())
        print(f"{name} NQ = {NQ} H = {H} N = {N} eps = {eps}: skipped {skipped} of {ACT_T * N}")
        assert skipped <= ro.MAX_SKIP_SHARE * ACT_T * N, (skipped, ACT_T * N)
        # the transitions do not depend on the net's shape: test_rollout_into_the_ring's checks
        rp = ro.replay(e, run, RING_SEED, ACT_STEP0, e.max_steps)
        ro._all(np.isin(done, (0, 1, 2)), "done codes")
        ro._all(np.abs(obs[0] - rp["obs0"]) <= 1e-6, "obs[0] vs the Philox reset")
        ro._all(ro.obs_close(e, nobs, rp["pred_obs"]), "nobs vs the oracle step, every row")
        ro._all(ro.rew_close(e, rew, rp["rew"]), "reward")
        sure = rp["margin"] > ro.EPS
        ro._all((done == rp["code"])[sure], "done code")
        assert int((~sure).sum()) <= ro.MAX_SKIP_SHARE * ACT_T * N
        live = done[:-1] == 0
        assert np.array_equal(_bits(obs[1:])[live], _bits(nobs[:-1])[live]), "obs[c+1] != nobs[c] on a running row"
        ro._all((np.abs(obs[1:] - rp["reset_obs"][:-1]) <= 1e-6)[~live], "obs[c+1] vs the Philox reset (done rows)")
        again = actor_launch(e, pdev, H, N, eps, NQ)
        for k in bufs:
            assert same_bits(bufs[k], again[k]), f"{k}: two launches differ"


def test_quantile_actor_refusals_write_nothing(cuda):
    e, H, N = ro.CartPole, 64, 17
    g, ring = guarded_ring(ACT_T, N, e.D)
    persist = (Guarded((N, e.NS)), Guarded((N,), torch.int32), Guarded((N,)))
    stats = Guarded((dqn_rollout_grid(N), 8), fill=float(INT_SENTINEL))
    plain = MLPSpec(e.D, H, e.A).init(torch.Generator().manual_seed(1)).to(DEV)
    q16 = MLPSpec(e.D, H, 16).init(torch.Generator().manual_seed(1)).to(DEV)
    args = (H, ACT_T, 0, ring, persist[0].t, persist[1].t, persist[2].t, stats.t)
    kw = dict(seed=1, step0=0, epsilon=0.1, reset_all=True, max_steps=10)
    with pytest.raises(ValueError, match=f"{plain.numel()} floats.*{q16.numel()}"):
        dqn_rollout(e.env_id, plain, *args, quantiles=8, **kw)
    with pytest.raises(ValueError, match="16"):
        dqn_rollout(e.env_id, q16, *args, quantiles=9, **kw)
    with pytest.raises(ValueError, match="dueling"):
        dqn_rollout(e.env_id, q16, *args, quantiles=8, dueling=True, **kw)
    with pytest.raises(ValueError, match="quantiles"):
        dqn_rollout(e.env_id, q16, *args, quantiles=-1, **kw)
    raw = (persist[0].t, persist[1].t, persist[2].t, ring.obs, ring.nobs, ring.act, ring.rew, ring.done, stats.t, 1, 0, 0.1,
           True, 10)
    for net, dueling, NQ in ((plain, False, 8), (q16, False, 9), (q16, True, 8), (q16, False, -1)):
        with pytest.raises(RuntimeError):  # the binding's own checks
            hip().dqn_rollout_qr(e.env_id, net, H, ACT_T, 0, *raw, dueling, NQ)
    torch.cuda.synchronize()
    untouched(g["obs"], g["nobs"], g["act"], g["rew"], g["done"], *persist)


# ------------------------------------------------------------------ 2. evaluator
@pytest.mark.parametrize("name,NQ,H", [(name, NQ, H) for name, nqs in (("CartPole-v1", (1, 3, 8)),
                                                                      ("LunarLanderSynth-v0", (1, 4)))
                                       for NQ in nqs for H in (64, 128)])
def test_quantile_evaluator_acts_on_the_sums(cuda, name, NQ, H):
    e = ro.env_of(name)
    N, E, Tc = 33, 1, 8
    params = qr_params(e, H, NQ)
    out = (Guarded((E, N)), Guarded((E, N), torch.int32), Guarded((E, N), torch.int32))
    tr = (Guarded((Tc, N, e.D)), Guarded((Tc, N), torch.int32), Guarded((Tc, N)), Guarded((Tc, N)))
    kw = dict(seed=RING_SEED, step0=7, out=tuple(o.t for o in out), trace=EvalTrace(*(t.t for t in tr)))
    evaluate_policy_op(e.env_id, params.to(DEV), H, E, N, greedy=True, quantiles=NQ, **kw)
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in out + tr)
    ep_ret, ep_len, ep_code = (o.t.cpu().numpy() for o in out)
    assert np.isin(ep_code, (1, 2)).all() and (ep_len >= 1).all() and np.isfinite(ep_ret).all()
    tr_obs, tr_act = tr[0].t.cpu().numpy(), tr[1].t.cpu().numpy()
    written = np.arange(Tc)[:, None] < ep_len[0][None, :]  # E = 1: an env steps until its episode ends
    assert np.array_equal(tr_act != INT_SENTINEL, written), "tr_act rows"
    a64, gap, tol = dq.sum_gap_tolerance(params, tr_obs[written], e.A, NQ, H)
    clear = gap >= tol
    assert np.array_equal(tr_act[written][clear], a64[clear]), "tr_act vs the float64 argmax of the sums"
    assert int((~clear).sum()) <= ro.MAX_SKIP_SHARE * Tc * N, int((~clear).sum())
    with pytest.raises(ValueError, match="greedily"):
        evaluate_policy_op(e.env_id, params.to(DEV), H, E, N, greedy=False, quantiles=NQ, **kw)
    with pytest.raises(RuntimeError):  # the binding refuses it too
        hip().evaluate_qr(e.env_id, params.to(DEV), H, out[0].t, out[1].t, out[2].t, *(t.t for t in tr), 1, 0, False,
                          e.max_steps, False, NQ)
    if NQ > 1:
        with pytest.raises(ValueError, match="floats"):  # a scalar net is not a quantile one
            evaluate_policy_op(e.env_id, ro.case_params(e, H, DEV), H, E, N, quantiles=NQ)


# ------------------------------------------------------------------ 3. targets
SEED, GAMMA, BETA = (3 << 32) | 5, 0.97, 0.7
TGT_CASES = [(H, A, NQ) for H in (64, 128) for A, NQ in SHAPES]


def _check_y(y, host, last, G, disc, online, target, D, H, A, NQ, double_q):
    """y [B, NQ] against float64: any action within FWD_TOL of the selecting net's top SUM may be a*, and all NQ
    values lie within FWD_TOL of that candidate's quantiles.  No row is skipped."""
    la = torch.from_numpy(np.asarray(last))
    nobs = host.nobs.reshape(-1, D)[la]
    out_t = dq.forward64(target, nobs, D, H, A * NQ)
    sel = dq.quantile_sums(dq.forward64(online, nobs, D, H, A * NQ) if double_q else out_t, A, NQ)
    top = sel.max(-1, keepdim=True).values
    cand = sel >= top - (FWD_TOL["atol"] + FWD_TOL["rtol"] * top.abs())                      # [B, A]
    boot = (host.done.reshape(-1)[la] != 1).double()
    ys = G.reshape(-1, 1, 1) + (disc * boot).reshape(-1, 1, 1) * out_t.reshape(-1, A, NQ)    # [B, A, NQ]
    close = (y.double().unsqueeze(1) - ys).abs() <= FWD_TOL["atol"] + FWD_TOL["rtol"] * ys.abs()
    ok = close.all(-1) & cand
    assert bool(ok.any(-1).all()), int((~ok.any(-1)).sum())


@pytest.mark.parametrize("double_q", [False, True])
@pytest.mark.parametrize("form", ["uniform", "prioritised", "nstep"])
@pytest.mark.parametrize("H,A,NQ", TGT_CASES)
def test_quantile_targets(cuda, H, A, NQ, form, double_q):
    D = min(2 * A, 16)
    L = TGT_C * TGT_N
    host, g, ring = random_ring(D, A, 100 * H + A)
    online = MLPSpec(D, H, A * NQ).init(torch.Generator().manual_seed(11))
    target = MLPSpec(D, H, A * NQ).init(torch.Generator().manual_seed(12))
    plain = tuple(MLPSpec(D, H, A).init(torch.Generator().manual_seed(s)).to(DEV) for s in (11, 12))
    don, dtg = online.to(DEV), target.to(DEV)
    per, nstep = form == "prioritised", form == "nstep"
    rew = host.rew.reshape(-1).double()

    def launch(nets, quantiles, B, filled, upd, tree):
        out = (Guarded((B, D)), Guarded((B,), torch.int32), Guarded((B, quantiles) if quantiles else (B,)),
               Guarded((B,), torch.int32))
        kw = dict(quantiles=quantiles) if quantiles else {}
        if per:
            out += (Guarded((B,)), Guarded((1,)))
            kw.update(tree=tree, beta=BETA)
        if nstep:
            out += (Guarded((B,), torch.int32),)
            kw.update(n_step=3, newest=filled // TGT_N - 1)
        dqn_targets(nets[0], nets[1], H, A, ring, filled, GAMMA, double_q, SEED, upd, B, out=tuple(o.t for o in out), **kw)
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in out) and all(b.guards_intact() for b in g.values())
        return out

    for B in (1, 63, 65, 1000):
        for filled in ((TGT_N * TGT_T, L) if nstep else (1, TGT_N * TGT_T, L)):  # the n-step form: whole slots
            upd = 2 ** 32 - 1 + B  # the update counter's high word matters
            tree = guarded_tree(random_leaves(L, filled, filled + B), 1.0)[2].tree if per else None
            out = launch((don, dtg), NQ, B, filled, upd, tree)
            base = launch(plain, 0, B, filled, upd, tree)
            for i in range(len(out)):  # sampling does not see the nets: everything but y is the scalar launch's
                if i != 2:
                    assert same_bits(out[i], base[i]), (i, B, filled)
            rows = per_sample_rows_ref(tree, SEED, upd, B, filled) if per else dqn_sample_rows_ref(SEED, upd, B, filled)
            np.testing.assert_array_equal(out[3].t.cpu().numpy(), rows)
            if nstep:
                last, G, disc, _ = dqn_nstep_walk_ref(rows, host, filled, filled // TGT_N - 1, 3, GAMMA, torch.float64)
                np.testing.assert_array_equal(out[-1].t.cpu().numpy(), last)
                G, disc = torch.from_numpy(G), torch.from_numpy(disc)
            else:
                last, G, disc = rows, rew[torch.from_numpy(rows)], torch.full((B,), GAMMA, dtype=torch.float64)
            _check_y(out[2].t.cpu(), host, last, G, disc, online, target, D, H, A, NQ, double_q)
            if B == 1000:  # two workgroups stride over the 16 slabs: the same bits
                with cu_limit(2):
                    again = launch((don, dtg), NQ, B, filled, upd, tree)
                assert all(same_bits(a, b) for a, b in zip(out, again))
    for k, b in g.items():  # the ring is an input: not one bit of it changed
        assert np.array_equal(_bits(b.t.cpu().numpy()), _bits(getattr(host, k).numpy())), k


def test_quantile_targets_refuse_bad_arguments(cuda):
    """24 outputs, negative quantiles, quantiles with dueling, a missing online net with double Q, a scalar net:
    refused in all four forms, and nothing is written."""
    D, H, B = 4, 64, 8
    _, _, ring = random_ring(D, 2, 1)
    L = TGT_C * TGT_N
    h = hip()
    q16 = MLPSpec(D, H, 16).init(torch.Generator().manual_seed(1)).to(DEV)
    q24 = MLPSpec(D, H, 24).init(torch.Generator().manual_seed(1)).to(DEV)
    plain = MLPSpec(D, H, 2).init(torch.Generator().manual_seed(1)).to(DEV)
    tree = guarded_tree(random_leaves(L, L, 1), 1.0)[2].tree
    out = (Guarded((B, D)), Guarded((B,), torch.int32), Guarded((B, 8)), Guarded((B,), torch.int32),
           Guarded((B,), torch.int32))
    w, wmax = Guarded((B,)), Guarded((1,))
    o = tuple(x.t for x in out)
    r = (ring.obs, ring.nobs, ring.act, ring.rew, ring.done)
    for net, A, online, extra in ((q24, 3, q24, dict(quantiles=8)), (q16, 2, q16, dict(quantiles=-1)),
                                  (q16, 2, q16, dict(quantiles=8, dueling=True)), (q16, 2, None, dict(quantiles=8)),
                                  (plain, 2, plain, dict(quantiles=8))):
        args = (online, net, H, A, *r, L, 0.9, True, 1, 0, *o[:4])
        per = dict(tree=tree, beta=0.5, w=w.t, wmax=wmax.t)
        with pytest.raises(RuntimeError):
            h.dqn_targets_qr(*args, **extra)
        with pytest.raises(RuntimeError):
            h.dqn_targets_qr(*args, n_step=3, newest=2, last=o[4], **extra)
        with pytest.raises(RuntimeError):
            h.dqn_targets_qr(*args, **per, **extra)
        with pytest.raises(RuntimeError):
            h.dqn_targets_qr(*args, **per, n_step=3, newest=2, last=o[4], **extra)
    with pytest.raises(ValueError, match="16"):
        dqn_targets(q24, q24, H, 3, ring, L, 0.9, True, 1, 0, B, out=o[:4], quantiles=8)
    with pytest.raises(ValueError, match="floats"):
        dqn_targets(plain, plain, H, 2, ring, L, 0.9, True, 1, 0, B, out=o[:4], quantiles=8)
    with pytest.raises(ValueError, match="dueling"):
        dqn_targets(q16, q16, H, 2, ring, L, 0.9, True, 1, 0, B, out=o[:4], quantiles=8, dueling=True)
    with pytest.raises(ValueError, match="targets"):  # y of the scalar shape
        dqn_targets(q16, q16, H, 2, ring, L, 0.9, True, 1, 0, B, out=(o[0], o[1], torch.zeros(B, device=DEV), o[3]),
                    quantiles=8)
    torch.cuda.synchronize()
    untouched(*out, w, wmax)
    dqn_targets(q16, q16, H, 2, ring, L, 0.9, True, 1, 0, B, out=o[:4], quantiles=8)  # the sound call
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[2].t).all()) and out[2].guards_intact()


# ------------------------------------------------------------------ 4. gradient head
def _q_qr_case(D, H, A, NQ, B, kappa, seed):
    gen = torch.Generator().manual_seed(seed)
    pp = MLPSpec(D, H, A * NQ).init(torch.Generator().manual_seed(6))
    X = torch.randn(B, D, generator=gen)
    act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
    out = ref.trunk(pp, X, D, H, A * NQ)[0].reshape(B, A, NQ)
    theta = out[torch.arange(B), act.long()]  # [B, NQ], the fp32 reference's values
    # targets inside the Huber zone and beyond +-kappa, both signs; rows 0 mod 7 land exactly on the quantiles
    # of the fp32 reference (u = 0 up to the kernel's own rounding of theta)
    off = torch.tensor([0.3, -0.3, 1.7, -1.7, 0.0])[(torch.arange(B).unsqueeze(1) + torch.arange(NQ)) % 5]
    T = theta.flip(-1) + off * kappa
    T[::7] = theta[::7]
    return pp, X, act, T.contiguous()


def _assert_q_qr(slab, loss, pp, X, act, T, A, NQ, H, kappa, inv_B, row_w=None, w_norm=None):
    """test_dqn_dueling_gpu._assert_q_duel for HEAD_Q_QR, its tolerances unchanged."""
    n = X.shape[0]
    g64, st = ref.mlp_grad_ref(int(GradHead.Q_QR), pp, X, A, H, act=act, ret=T, inv_B=inv_B, clip_eps=kappa,
                               dtype=torch.float64, row_w=row_w, w_norm=w_norm, quantiles=NQ)
    g = reduce_slabs(slab).cpu().double()
    scale = g64.abs().max().item() + 1e-12
    err = (g - g64).abs().max().item()
    assert err <= 2e-4 * scale + 1e-6, (err, scale)  # test_kernels_gpu.test_grad_matches_autograd
    ls = loss.sum(0).cpu()
    assert abs(ls[0].item() - st["loss"]) <= 1e-3 * (abs(st["loss"]) + 1)
    assert abs(ls[4].item() - st["v"]) <= 1e-3 * (abs(st["v"]) + 1)
    assert int(ls[5].item()) == n and (ls[1:4] == 0).all()
    return st


@pytest.mark.parametrize("H,A,NQ", TGT_CASES + [(H, 1, 1) for H in (64, 128)])
def test_q_qr_head_matches_float64_autograd(cuda, H, A, NQ):
    """(1, 1) has one output and (2, 1) two: the two VALU dW3 instances; the others take the MFMA tile path, and
    (2, 8), (4, 4) and (1, 16) fill its 16 rows; B = 65 and 4100 end in a partial slab.  Unweighted and weighted
    (row_w, w_norm, td_abs)."""
    kappa = 0.75
    for D in (2, 4, 8):
        for B in (1, 64, 65, 4100):
            pp, X, act, T = _q_qr_case(D, H, A, NQ, B, kappa, 1000 * D + B)
            args = (GradHead.Q_QR, pp.to(DEV), X.to(DEV), A, H)
            kw = dict(act=act.to(DEV), ret=T.to(DEV), clip_eps=kappa, quantiles=NQ)
            ns = int(hip().mlp_grad_slabs(B))
            gs, gl = Guarded((ns, pp.numel())), Guarded((ns, 8), fill=float(INT_SENTINEL))
            slab, loss = mlp_grad(*args, **kw, grad_slab=gs.t, loss_slab=gl.t)
            torch.cuda.synchronize()
            assert gs.guards_intact() and gl.guards_intact() and bool((gl.t[:, 6:] == INT_SENTINEL).all())
            _assert_q_qr(slab, loss[:, :6], pp, X, act, T, A, NQ, H, kappa, 1.0 / B)
            slab2, loss2 = mlp_grad(*args, **kw)
            assert torch.equal(slab, slab2) and torch.equal(loss[:, :6], loss2[:, :6]), "two launches differ"
            # the weighted instance
            w = torch.rand(B, generator=torch.Generator().manual_seed(B + D)) * 3.0 + 0.05
            wn = w.max().reshape(1)
            ws, wl, gtd = Guarded((ns, pp.numel())), Guarded((ns, 8), fill=float(INT_SENTINEL)), Guarded((B,))
            wkw = dict(kw, row_w=w.to(DEV), w_norm=wn.to(DEV))
            slab, loss = mlp_grad(*args, **wkw, grad_slab=ws.t, loss_slab=wl.t, td_abs=gtd.t)
            torch.cuda.synchronize()
            assert ws.guards_intact() and wl.guards_intact() and gtd.guards_intact()
            assert bool((wl.t[:, 6:] == INT_SENTINEL).all())
            st = _assert_q_qr(slab, loss[:, :6], pp, X, act, T, A, NQ, H, kappa, 1.0 / B, w, wn)
            torch.testing.assert_close(gtd.t.cpu().double(), st["td_abs"], **FWD_TOL)  # the unweighted row loss
            td2 = torch.zeros(B, device=DEV)
            slab2, loss2 = mlp_grad(*args, **wkw, td_abs=td2)
            assert torch.equal(slab, slab2) and torch.equal(loss[:, :6], loss2[:, :6]) and torch.equal(td2, gtd.t)


@pytest.mark.parametrize("H,A,NQ,D", [(128, 2, 1, 4), (64, 3, 5, 2), (128, 2, 8, 8), (64, 1, 16, 4)])
def test_q_qr_head_device_side_batch_shape_and_slab_loop(cuda, H, A, NQ, D):
    """nvalid < B with poisoned rows past it, inv_B from device memory, and (2 CUs) workgroups that walk
    several 64-row slabs; td_abs past nvalid is left alone."""
    kappa, B, nv = 1.0, 4100, 3001
    pp, X, act, T = _q_qr_case(D, H, A, NQ, B, kappa, 5)
    w = torch.rand(B, generator=torch.Generator().manual_seed(2)) + 0.5
    Xp, actp, Tp, wp = X.clone(), act.clone(), T.clone(), w.clone()
    Xp[nv:], Tp[nv:], actp[nv:], wp[nv:] = float("nan"), float("nan"), 99, float("nan")
    nvalid = torch.tensor([nv], dtype=torch.int32, device=DEV)
    inv_dev = torch.tensor([1.0 / 777], device=DEV)
    wn = w[:nv].max().reshape(1)
    for cus in (0, 2):
        with cu_limit(cus):
            slab, loss = mlp_grad(GradHead.Q_QR, pp.to(DEV), Xp.to(DEV), A, H, act=actp.to(DEV), ret=Tp.to(DEV),
                                  clip_eps=kappa, nvalid=nvalid, inv_B_dev=inv_dev, quantiles=NQ)
            assert slab.shape[0] == (2 if cus else min(65, hip().num_cus()))
            assert bool(torch.isfinite(slab).all())
            _assert_q_qr(slab, loss[:, :6], pp, X[:nv], act[:nv], T[:nv], A, NQ, H, kappa, 1.0 / 777)
            gtd = Guarded((B,))
            slab, loss = mlp_grad(GradHead.Q_QR, pp.to(DEV), Xp.to(DEV), A, H, act=actp.to(DEV), ret=Tp.to(DEV),
                                  clip_eps=kappa, nvalid=nvalid, inv_B_dev=inv_dev, row_w=wp.to(DEV), w_norm=wn.to(DEV),
                                  td_abs=gtd.t, quantiles=NQ)
            torch.cuda.synchronize()
            td = gtd.t.cpu()
            assert gtd.guards_intact() and bool(torch.isnan(td[nv:]).all()), "a row past nvalid wrote td_abs"
            st = _assert_q_qr(slab, loss[:, :6], pp, X[:nv], act[:nv], T[:nv], A, NQ, H, kappa, 1.0 / 777, w[:nv], wn)
            torch.testing.assert_close(td[:nv].double(), st["td_abs"], **FWD_TOL)


def test_q_qr_head_refusals_write_nothing(cuda):
    D, H, B = 4, 64, 8
    p16 = MLPSpec(D, H, 16).init(torch.Generator().manual_seed(1)).to(DEV)
    p24 = MLPSpec(D, H, 24).init(torch.Generator().manual_seed(1)).to(DEV)
    p2 = MLPSpec(D, H, 2).init(torch.Generator().manual_seed(1)).to(DEV)
    X, act = torch.zeros(B, D, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    T = torch.zeros(B, 8, device=DEV)
    gs, gl, gtd = Guarded((1, p24.numel())), Guarded((1, 8)), Guarded((B,))

    def raw(p, A, kappa, NQ):
        hip().mlp_grad_qr(p, X, A, NQ, H, act, T, 1.0 / B, kappa, gs.t, gl.t, td_abs=gtd.t)

    for p, A, kappa, NQ in ((p24, 3, 1.0, 8), (p16, 2, 1.0, 0), (p16, 2, 1.0, -1), (p16, 2, 0.0, 8), (p16, 2, -1.0, 8),
                            (p2, 2, 1.0, 8), (p24, 2, 1.0, 8)):
        with pytest.raises(RuntimeError):
            raw(p, A, kappa, NQ)
    with pytest.raises(RuntimeError):  # the scalar binding does not know the head
        hip().mlp_grad(int(GradHead.Q_QR), p16, X, 2, H, None, act, None, None, T, None, None, 1.0 / B, 1.0, 0.0, gs.t,
                       gl.t, None, None, None, None, gtd.t)
    with pytest.raises(ValueError, match="quantiles"):  # quantiles with another head
        mlp_grad(GradHead.Q_TD, p16, X, 16, H, act=act, ret=T[:, 0].contiguous(), quantiles=2)
    kw = dict(act=act, grad_slab=gs.t, loss_slab=gl.t)
    with pytest.raises(ValueError, match="16"):
        mlp_grad(GradHead.Q_QR, p24, X, 3, H, ret=T, quantiles=8, **kw)
    with pytest.raises(ValueError, match="threshold"):
        mlp_grad(GradHead.Q_QR, p16, X, 2, H, ret=T, quantiles=8, clip_eps=0.0, **kw)
    with pytest.raises(ValueError, match="floats"):
        mlp_grad(GradHead.Q_QR, p2, X, 2, H, ret=T, quantiles=8, **kw)
    with pytest.raises(ValueError, match="quantiles"):
        mlp_grad(GradHead.Q_QR, p16, X, 2, H, ret=T, **kw)
    torch.cuda.synchronize()
    untouched(gs, gl, gtd)
    slab, loss = mlp_grad_qr(p16, X, 2, 8, H, act=act, ret=T)  # the sound call, and the op it is an alias of
    ref_slab, ref_loss = mlp_grad(GradHead.Q_QR, p16, X, 2, H, act=act, ret=T, clip_eps=1.0, quantiles=8)
    assert torch.equal(slab, ref_slab) and torch.equal(loss[:, :6], ref_loss[:, :6]), "the op and its alias differ"


# ------------------------------------------------------------------ 5. trainer
def _state(tr):
    return [t.clone() for t in tr.snapshot_tensors()], dict(tr.counters())


@pytest.mark.parametrize("extra", [dict(quantiles=8), dict(quantiles=8, prioritized=True, n_step=3, per_beta_epochs=4),
                                   dict(quantiles=4, noisy=True)], ids=["uniform", "per-nstep", "noisy"])
def test_quantile_trainer_resume_is_bitwise_and_evaluate_touches_nothing(cuda, extra):
    kw = dict(TRAINER, **extra)
    NQ = extra["quantiles"]
    a = DQNTrainer(DQNConfig(**kw), device=cuda)
    assert a.q.P == MLPSpec(a.D, kw["hidden"], a.A * NQ).P and a.slab.shape[1] == a.q.P and a.y.shape == (64, NQ)
    assert a.target.numel() == a.q.P * (2 if extra.get("noisy") else 1)
    for _ in range(6):
        a.train_epoch()
    b = DQNTrainer(DQNConfig(**kw), device=cuda)
    for _ in range(3):
        b.train_epoch()
    before, counters = _state(b)
    res = b.evaluate(episodes=2, num_envs=33)
    assert res.stats()["episodes"] == 66
    after, counters2 = _state(b)
    assert counters == counters2 and all(torch.equal(x, y) for x, y in zip(before, after)), "evaluate() changed state"
    with pytest.raises(ValueError):
        b.evaluate(greedy=False)
    sd = b.state_dict()
    assert sd["cfg"]["quantiles"] == NQ and DQNConfig(**sd["cfg"]).quantiles == NQ
    c = DQNTrainer(DQNConfig(**kw), device=cuda)
    c.q.params.add_(1.0)  # other weights until the load
    c.target.zero_()
    c.load_state_dict(sd)
    for _ in range(3):
        c.train_epoch()
    torch.cuda.synchronize()
    assert a.counters() == c.counters() and a.updates == 12 and a.cursor == 0 and a.slots_written == 24
    for i, (x, y) in enumerate(zip(a.snapshot_tensors(), c.snapshot_tensors())):
        assert torch.equal(x, y), f"snapshot tensor {i} differs after the resume"
    assert int(a.q.step.item()) == 12 and not torch.equal(a.q.params, b.q.params)
    m = a.metrics()
    assert m["Quantiles"] == NQ and m["Dueling"] is False and m["Updates"] == 12
    assert np.isfinite(m["LossQ"]) and m["LossQ"] >= 0.0 and np.isfinite(m["QVals"])
    # a quantile checkpoint and a scalar trainer refuse each other by name, in both directions
    scalar = DQNTrainer(DQNConfig(**dict(kw, quantiles=0)), device=cuda)
    assert scalar.metrics()["Quantiles"] == 0 and scalar.state_dict()["cfg"]["quantiles"] == 0
    with pytest.raises(ValueError, match="quantiles"):
        scalar.load_state_dict(sd)
    with pytest.raises(ValueError, match="quantiles"):
        c.load_state_dict(scalar.state_dict())
    old = scalar.state_dict()
    del old["cfg"]["quantiles"]  # a checkpoint from before the quantile head: a scalar net
    scalar.load_state_dict(old)
    with pytest.raises(ValueError, match="quantiles"):
        c.load_state_dict(old)


def test_quantile_trainer_refuses_too_many_outputs(cuda):
    with pytest.raises(ValueError, match="16"):
        DQNTrainer(DQNConfig(**dict(TRAINER, quantiles=9)), device=cuda)  # CartPole: 18 outputs
    with pytest.raises(ValueError, match="16"):
        DQNTrainer(DQNConfig(**dict(TRAINER, env="LunarLanderSynth-v0", quantiles=5)), device=cuda)


def test_quantile_trainer_target_network_follows_its_schedule(cuda):
    tr = DQNTrainer(DQNConfig(**TRAINER, quantiles=8), device=cuda)
    tr.rollout()
    init = tr.target.clone()
    assert torch.equal(init, tr.q.params)
    prev = init
    for u in range(1, 8):
        tr.update()
        if u % 3 == 0:
            assert torch.equal(tr.target, tr.q.params) and not torch.equal(tr.target, prev)
            prev = tr.target.clone()
        else:
            assert torch.equal(tr.target, prev) and not torch.equal(tr.target, tr.q.params)


# ------------------------------------------------------------------ 6. CLI
def test_quantile_preset_trains_evaluates_and_checkpoints(cuda, tmp_path):
    from relayrl_prototype_amd.runtime.launcher import EVAL_COLUMNS, ckpt_dir, run_evaluate, run_preset

    small = {k: v for k, v in TRAINER.items() if k != "max_episode_steps"}
    rows = []
    last = run_preset("cartpole-dqn-quantile", 4, str(tmp_path), overrides=small, eval_every=2, checkpoint_every=4,
                      eval_episodes=1, eval_envs=32, on_metrics=rows.append)
    assert len(rows) == 4 and last["Epoch"] == 4 and last["Updates"] == 8
    assert last["Quantiles"] == 8 and last["NStep"] == 3 and 0.4 <= last["Beta"] <= 1.0 and last["Dueling"] is False
    for k in EVAL_COLUMNS:
        assert np.isfinite(rows[1][k]) and np.isfinite(last[k]), k
    ck = ckpt_dir(str(tmp_path), "cartpole-dqn-quantile", 0)
    assert os.path.exists(os.path.join(ck, "state.json"))
    out = run_evaluate(ck, episodes=64, num_envs=32)
    assert out["env"] == "CartPole-v1" and out["hidden"] == 64 and out["episodes"] == 64 and out["greedy"]
    assert out["checkpoint_epoch"] == 4 and 8.0 <= out["mean_return"] <= 500.0
    with pytest.raises(ValueError):
        run_evaluate(ck, episodes=4, num_envs=4, stochastic=True)


# ------------------------------------------------------------------ 7. learning
def test_quantile_trainer_learns_cartpole_like_the_cpu_oracle(cuda):
    """The CPU oracle loop with the quantile net (tests/dqn_quantile_oracle.py: the same algorithm and Philox
    draws, float64 networks) at the small shape plus quantiles = 8, 600 epochs = 1194 updates, scores a greedy mean
    return over 256 episodes of 138.80, 98.72, 116.81, 238.18 and 111.84 for seeds 1..5 (a random policy: about
    22).  The GPU trainer after the same number of updates must reach 80 % of the lowest."""
    tr = DQNTrainer(DQNConfig(**do.SMALL, seed=1, quantiles=8), device=cuda)
    for _ in range(dq.QR_EPOCHS):
        tr.train_epoch()
    assert tr.updates == dq.QR_UPDATES == 1194
    got = tr.evaluate(episodes=1, num_envs=do.EVAL_EPISODES).stats()["mean_return"]
    floor = 0.8 * min(dq.ORACLE_RETURNS_QR.values())
    print(f"GPU greedy mean return {got:.2f}, floor {floor:.2f}, oracle {dq.ORACLE_RETURNS_QR}")
    assert floor >= 44.0 and got >= floor, (got, floor)
