"""The categorical (C51) head on the GPU: the wide-output-layer instances of the actor, the evaluator, the targets
kernel and the HEAD_Q_C51 gradient kernel (csrc/kernels/wide.h, dqn.hip, evaluate.hip, mlp_grad.hip) against the float64
oracles of ops/reference.py, and the trainer built on them (resume, checkpoints, learning against the CPU oracle loop).  Every bound is
BOUND_FACTOR times the fp32 oracle's own error against float64 at the test's shapes (tests/dqn_c51_oracle.py).
Every output buffer of a kernel under test is guarded."""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import EvalTrace, MLPSpec, dqn_rollout, dqn_rollout_grid, dqn_targets, dqn_targets_ref
from relayrl_prototype_amd.ops import GradHead, evaluate_policy_op, hip, mlp_grad, reduce_slabs
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer

import dqn_c51_oracle as dc
import dqn_oracle as do
import rollout_oracle as ro
from guarded import INT_SENTINEL, Guarded
from test_dqn_gpu import RING_SEED, TGT_C, TGT_N, TRAINER, _bits, cu_limit, guarded_ring, random_ring
from test_dqn_quantile_gpu import same_bits, untouched
from test_per_gpu import guarded_tree, random_leaves

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (env, NA, H): 8 tiles with 4 per action; padding inside the second tile; no padding, 6 tiles; one mostly-padded tile
CASES = [("CartPole-v1", 51, 128), ("LunarLanderSynth-v0", 21, 64), ("Acrobot-v1", 32, 128), ("CartPole-v1", 3, 64)]
V_MIN, V_MAX = -10.0, 10.0


def c51_params(D, H, A, NA, seed, centre=None):
    """centre (an env's typical reset observation): layer 1 is scaled up and biased to be 0 there and the output bias
    is dropped, so that the greedy action depends on the small differences between the envs' observations."""
    spec = MLPSpec(D, H, A * NA)
    p = spec.init(torch.Generator().manual_seed(seed))
    if centre is not None:
        o = spec.offsets()
        p[o["w1"]:o["b1"]] *= 60.0
        p[o["b1"]:o["w2"]] = -p[o["w1"]:o["b1"]].reshape(H, D) @ torch.tensor(centre)
        p[o["w3"]:o["b3"]] *= 4.0
        p[o["b3"]:] = 0.0
    return p


# Acrobot observes the cosines of two small angles; CartPole starts around 0; the lander is left as it starts
CENTRE = {"Acrobot-v1": [1.0, 0.0, 1.0, 0.0, 0.0, 0.0], "CartPole-v1": [0.0] * 4, "LunarLanderSynth-v0": [0.0] * 8}


@pytest.mark.parametrize("name,NA,H", CASES)
def test_c51_actor_and_evaluator_act_on_the_expectations(cuda, name, NA, H):
    """N = 17 is a ragged tile.  The evaluator's greedy trace equals the float64 argmax of the expectations wherever the
    top-two gap exceeds the bound, and a greedy actor launch from the same reset fills its ring with that trace."""
    e = ro.env_of(name)
    N, E, Tc = 17, 1, 8
    params = c51_params(e.D, H, e.A, NA, 3 + e.env_id, CENTRE[name])
    pdev = params.to(DEV)
    out = (Guarded((E, N)), Guarded((E, N), torch.int32), Guarded((E, N), torch.int32))
    tr = (Guarded((Tc, N, e.D)), Guarded((Tc, N), torch.int32), Guarded((Tc, N)), Guarded((Tc, N)))
    sup = dict(atoms=NA, v_min=V_MIN, v_max=V_MAX)
    evaluate_policy_op(e.env_id, pdev, H, E, N, greedy=True, seed=RING_SEED, step0=7, out=tuple(o.t for o in out),
                       trace=EvalTrace(*(t.t for t in tr)), **sup)
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in out + tr)
    ep_len = out[1].t.cpu().numpy()
    tr_obs, tr_act = tr[0].t.cpu().numpy(), tr[1].t.cpu().numpy()
    written = np.arange(Tc)[:, None] < ep_len[0][None, :]
    assert np.array_equal(tr_act != INT_SENTINEL, written), "tr_act rows"
    q64, bound = dc.q_both(params, tr_obs[written], e.A, NA, H, V_MIN, V_MAX)
    a64, gap = ref.greedy_from_logits(q64)
    clear = (gap > bound).numpy()
    print(f"{name} NA = {NA} H = {H}: bound {bound:.3e}, {int((~clear).sum())} of {clear.size} cells within it")
    assert len(np.unique(a64.numpy()[clear])) >= 2, "the weights must make at least two actions occur"
    assert np.array_equal(tr_act[written][clear], a64.numpy()[clear])
    assert int((~clear).sum()) <= ro.MAX_SKIP_SHARE * Tc * N
    # the actor, greedy, from the same Philox reset
    g, ring = guarded_ring(Tc, N, e.D)
    persist = (Guarded((N, e.NS)), Guarded((N,), torch.int32), Guarded((N,)))
    stats = Guarded((dqn_rollout_grid(N), 8), fill=float(INT_SENTINEL))
    rc = dqn_rollout(e.env_id, pdev, H, Tc, 0, ring, persist[0].t, persist[1].t, persist[2].t, stats.t, seed=RING_SEED,
                     step0=7, epsilon=0.0, reset_all=True, max_steps=e.max_steps, **sup)
    torch.cuda.synchronize()
    assert rc == 0 and all(b.guards_intact() for b in (*g.values(), *persist, stats))
    assert np.array_equal(g["act"].t.cpu().numpy()[written], tr_act[written])
    assert np.array_equal(_bits(g["obs"].t.cpu().numpy())[written], _bits(tr_obs)[written])
    assert np.array_equal(_bits(g["rew"].t.cpu().numpy())[written], _bits(tr[2].t.cpu().numpy())[written])


def test_c51_refusals_write_nothing(cuda):
    e, H, N, T = ro.CartPole, 64, 17, 3
    g, ring = guarded_ring(T, N, e.D)
    persist = (Guarded((N, e.NS)), Guarded((N,), torch.int32), Guarded((N,)))
    stats = Guarded((dqn_rollout_grid(N), 8), fill=float(INT_SENTINEL))
    y = Guarded((8, 5))
    tout = (Guarded((8, e.D)), Guarded((8,), torch.int32), y, Guarded((8,), torch.int32))
    net = c51_params(e.D, H, e.A, 5, 1).to(DEV)
    n65 = c51_params(e.D, H, e.A, 65, 1).to(DEV)
    args = (H, T, 0, ring, persist[0].t, persist[1].t, persist[2].t, stats.t)
    kw = dict(seed=1, step0=0, epsilon=0.1, reset_all=True, max_steps=10)
    raw = (persist[0].t, persist[1].t, persist[2].t, ring.obs, ring.nobs, ring.act, ring.rew, ring.done, stats.t, 1, 0, 0.1,
           True, 10)
    r = (ring.obs, ring.nobs, ring.act, ring.rew, ring.done)
    X, m = torch.zeros(8, e.D, device=DEV), torch.full((8, 5), 0.2, device=DEV)
    gslab = (Guarded((1, net.numel())), Guarded((1, 8)))
    for p, bad, match in ((net, dict(atoms=5, v_min=0.0, v_max=1.0, quantiles=2), "atoms.*quantiles"),
                          (net, dict(atoms=5, v_min=0.0, v_max=1.0, dueling=True), "atoms.*dueling"),
                          (net, dict(atoms=1, v_min=0.0, v_max=1.0), "atoms"),
                          (net, dict(atoms=5, v_min=1.0, v_max=1.0), "v_min.*v_max"),
                          (n65, dict(atoms=65, v_min=0.0, v_max=1.0), "8 output tiles"),
                          (net, dict(atoms=6, v_min=0.0, v_max=1.0), "floats")):
        with pytest.raises(ValueError, match=match):
            dqn_rollout(e.env_id, p, *args, **kw, **bad)
        with pytest.raises(ValueError, match=match):
            evaluate_policy_op(e.env_id, p, H, 1, N, **bad)
        with pytest.raises(ValueError, match=match):
            dqn_targets(p, p, H, e.A, ring, T * N, 0.9, True, 1, 0, 8, out=tuple(o.t for o in tout), **bad)
        with pytest.raises(RuntimeError):  # the bindings' own checks
            hip().dqn_rollout(e.env_id, p, H, T, 0, *raw, **bad)
        with pytest.raises(RuntimeError):
            hip().dqn_targets(p, p, H, e.A, *r, T * N, 0.9, True, 1, 0, *(o.t for o in tout), **bad)
        if "dueling" not in bad:  # the gradient head takes no such keyword
            with pytest.raises(ValueError, match=match):
                mlp_grad(GradHead.Q_C51, p, X, e.A, H, act=tout[1].t, ret=m, grad_slab=gslab[0].t,
                         loss_slab=gslab[1].t, **bad)
            with pytest.raises(RuntimeError):
                hip().mlp_grad(int(GradHead.Q_C51), p, X, e.A, H, None, tout[1].t, None, None, m, None, None, 0.125, 1.0,
                               0.0, gslab[0].t, gslab[1].t, **bad)
    torch.cuda.synchronize()
    untouched(g["obs"], g["nobs"], g["act"], g["rew"], g["done"], *persist, *tout, *gslab)


SEED, GAMMA, BETA, B = (3 << 32) | 5, 0.97, 0.7, 65
TGT_CASES = [(2, 51, 128), (4, 21, 64), (3, 32, 128), (2, 3, 64)]  # (A, NA, H): the shapes of CASES
TV_MIN, TV_MAX = -1.0, 1.5  # the ring's rewards are N(0, 1): returns fall past both ends


@pytest.mark.parametrize("double_q", [False, True])
@pytest.mark.parametrize("form", ["uniform", "prioritised+3step"])
@pytest.mark.parametrize("A,NA,H", TGT_CASES)
def test_c51_targets(cuda, A, NA, H, form, double_q):
    """m [65, NA] against the float64 projection; row sums 1; everything but y bit-equal to the scalar launch."""
    D = min(2 * A, 16)
    L = TGT_C * TGT_N
    host, g, ring = random_ring(D, A, 100 * H + A)
    online, target = c51_params(D, H, A, NA, 11), c51_params(D, H, A, NA, 12)
    plain = tuple(MLPSpec(D, H, A).init(torch.Generator().manual_seed(s)).to(DEV) for s in (11, 12))
    per = form != "uniform"
    upd = 2 ** 32 - 1 + B
    kw = {}
    tree_host = None
    if per:
        leaves = random_leaves(L, L, L + B)
        tree_host = guarded_tree(leaves, 1.0)[2].tree
        kw.update(tree=tree_host, beta=BETA, n_step=3, newest=TGT_C - 1)

    def launch(nets, atoms):
        out = (Guarded((B, D)), Guarded((B,), torch.int32), Guarded((B, atoms) if atoms else (B,)),
               Guarded((B,), torch.int32))
        if per:
            out += (Guarded((B,)), Guarded((1,)), Guarded((B,), torch.int32))
        sup = dict(atoms=atoms, v_min=TV_MIN, v_max=TV_MAX) if atoms else {}
        dqn_targets(nets[0], nets[1], H, A, ring, L, GAMMA, double_q, SEED, upd, B, out=tuple(o.t for o in out), **kw, **sup)
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in out) and all(b.guards_intact() for b in g.values())
        return out

    out = launch((online.to(DEV), target.to(DEV)), NA)
    base = launch(plain, 0)
    for i in range(len(out)):
        if i != 2:
            assert same_bits(out[i], base[i]), i
    tree_cpu = tree_host.cpu() if per else None
    rkw = dict(kw, tree=tree_cpu) if per else {}
    refs = {dt: dqn_targets_ref(online, target, H, A, host, L, GAMMA, double_q, SEED, upd, B, dt, atoms=NA, v_min=TV_MIN,
                                v_max=TV_MAX, **rkw) for dt in (torch.float32, torch.float64)}
    m64, m32 = refs[torch.float64][2], refs[torch.float32][2].double()
    # by the reference alone: returns clamp at each end, and some rows put all their mass on one atom
    last = refs[torch.float64][-1] if per else refs[torch.float64][3]
    boot = (host.done.reshape(-1)[last] != 1)
    assert float(m64[:, 0].max()) > 0.5 and float(m64[:, -1].max()) > 0.5 and bool((~boot).any())
    assert bool((m64.max(-1).values > 1 - 1e-9).any())
    # rows whose a* the fp32 oracle itself cannot tell from float64's are not compared
    nobs = host.nobs.reshape(-1, D)[last]
    q64, qbound = dc.q_both(online if double_q else target, nobs, A, NA, H, TV_MIN, TV_MAX)
    clear = ref.greedy_from_logits(q64)[1] > qbound
    assert int((~clear).sum()) <= ro.MAX_SKIP_SHARE * B
    bound = dc.BOUND_FACTOR * float((m32 - m64)[clear].abs().max())
    sum_bound = dc.BOUND_FACTOR * float((m32.sum(-1) - 1).abs().max())
    m = out[2].t.cpu().double()
    err, serr = float((m - m64)[clear].abs().max()), float((m.sum(-1) - 1).abs().max())
    print(f"A = {A} NA = {NA} H = {H} {form} double_q = {double_q}: m err {err:.3e} (bound {bound:.3e}), "
          f"row sum err {serr:.3e} (bound {sum_bound:.3e})")
    assert err <= bound and serr <= sum_bound and float(m.min()) >= 0.0
    assert all(same_bits(a, b) for a, b in zip(out, launch((online.to(DEV), target.to(DEV)), NA))), "two launches differ"


# ------------------------------------------------------------------ the gradient head
GRAD_CASES = TGT_CASES + [(1, 5, 64)]  # and one action of one mostly-padded tile


def _grad_case(D, H, A, NA, B, seed):
    """Every 7th row of the target distributions m [B, NA] puts all its mass on one atom."""
    gen = torch.Generator().manual_seed(seed)
    pp = c51_params(D, H, A, NA, 6)
    X = torch.randn(B, D, generator=gen)
    act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
    m = torch.softmax(2.0 * torch.randn(B, NA, generator=gen), -1)
    m[::7] = torch.nn.functional.one_hot(torch.arange(len(m[::7])) % NA, NA).float()
    return pp, X, act, m.contiguous()


def _assert_c51_grad(slab, loss, td, pp, X, act, m, A, NA, H, inv_B, row_w=None, w_norm=None):
    """Gradient and row losses against float64 autograd, each within BOUND_FACTOR times the fp32 oracle's own largest
    error.  The two sums of the loss slab are single numbers, for which one oracle error is no measure: they are fp32
    sums of n >= 65 fp32 terms, so their bound is BOUND_FACTOR times the larger of the oracle's error (for Q(act), which
    cancels over a symmetric support, taken row by row and summed) and one fp32 rounding unit (2^-23) of the sum of the
    terms' magnitudes, which is below the first-order bound log2(n) * 2^-24 * sum |x| of a pairwise fp32 summation."""
    kw = dict(act=act, ret=m, inv_B=inv_B, row_w=row_w, w_norm=w_norm, atoms=NA, v_min=V_MIN, v_max=V_MAX)
    (g64, s64), (g32, s32) = (ref.mlp_grad_ref(int(GradHead.Q_C51), pp, X, A, H, dtype=dt, **kw)
                              for dt in (torch.float64, torch.float32))
    ls = loss.sum(0).cpu().double()
    got = {"grad": reduce_slabs(slab).cpu().double(), "loss": ls[0], "v": ls[4]}
    want = {"grad": (g64, g32), "loss": (s64["loss"], s32["loss"]), "v": (s64["v"], s32["v"])}
    wi = 1.0 if row_w is None else (row_w / w_norm).double()
    q_err = float((s32["q_act"].double() - s64["q_act"]).abs().sum())
    unit = {"loss": 2.0 ** -23 * float((wi * s64["td_abs"]).abs().sum()),
            "v": q_err + 2.0 ** -23 * float(s64["q_act"].abs().sum())}
    if td is not None:
        got["td_abs"], want["td_abs"] = td.cpu().double(), (s64["td_abs"], s32["td_abs"])
    for k, (w64, w32) in want.items():
        w64, w32 = torch.as_tensor(w64).double(), torch.as_tensor(w32).double()
        bound = dc.BOUND_FACTOR * max(float((w32 - w64).abs().max()), unit.get(k, 0.0))
        err = float((got[k] - w64).abs().max())
        print(f"A = {A} NA = {NA} H = {H} n = {len(X)} {k}: err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, k
    assert int(ls[5]) == len(X) and bool((ls[1:4] == 0).all())


@pytest.mark.parametrize("A,NA,H", GRAD_CASES)
def test_q_c51_head_matches_float64_autograd(cuda, A, NA, H):
    """B = 65 ends in a one-row slab.  Unweighted, then weighted with the row losses out."""
    D, B = min(2 * A, 16), 65
    pp, X, act, m = _grad_case(D, H, A, NA, B, 100 * H + NA)
    args = (GradHead.Q_C51, pp.to(DEV), X.to(DEV), A, H)
    kw = dict(act=act.to(DEV), ret=m.to(DEV), atoms=NA, v_min=V_MIN, v_max=V_MAX)
    ns = int(hip().mlp_grad_slabs(B))
    gs, gl = Guarded((ns, pp.numel())), Guarded((ns, 8))
    slab, loss = mlp_grad(*args, **kw, grad_slab=gs.t, loss_slab=gl.t)
    assert gs.guards_intact() and gl.guards_intact()
    _assert_c51_grad(slab, loss, None, pp, X, act, m, A, NA, H, 1.0 / B)
    w = torch.rand(B, generator=torch.Generator().manual_seed(B)) * 3.0 + 0.05
    wn = w.max().reshape(1)
    gtd = Guarded((B,))
    slab, loss = mlp_grad(*args, **kw, row_w=w.to(DEV), w_norm=wn.to(DEV), td_abs=gtd.t)
    torch.cuda.synchronize()
    assert gtd.guards_intact()
    _assert_c51_grad(slab, loss, gtd.t, pp, X, act, m, A, NA, H, 1.0 / B, w, wn)


@pytest.mark.parametrize("A,NA,H,cus", [(2, 51, 128, 1), (4, 21, 64, 0)])
def test_q_c51_head_device_side_batch_shape_and_slab_loop(cuda, A, NA, H, cus):
    """nvalid < B with poisoned rows past it, inv_B from device memory, row_w and td_abs; on one CU the workgroup walks
    three slabs and stages W3 again for each."""
    D, B, nv = 2 * A, 200, 131
    pp, X, act, m = _grad_case(D, H, A, NA, B, 5)
    w = torch.rand(B, generator=torch.Generator().manual_seed(2)) + 0.5
    Xp, actp, mp, wp = X.clone(), act.clone(), m.clone(), w.clone()
    Xp[nv:], mp[nv:], actp[nv:], wp[nv:] = float("nan"), float("nan"), 99, float("nan")
    wn = w[:nv].max().reshape(1)
    gtd = Guarded((B,))
    with cu_limit(cus):
        slab, loss = mlp_grad(GradHead.Q_C51, pp.to(DEV), Xp.to(DEV), A, H, act=actp.to(DEV), ret=mp.to(DEV),
                              nvalid=torch.tensor([nv], dtype=torch.int32, device=DEV),
                              inv_B_dev=torch.tensor([1.0 / 777], device=DEV), row_w=wp.to(DEV), w_norm=wn.to(DEV),
                              td_abs=gtd.t, atoms=NA, v_min=V_MIN, v_max=V_MAX)
        torch.cuda.synchronize()
    assert slab.shape[0] == (1 if cus else 4) and bool(torch.isfinite(slab).all())
    td = gtd.t.cpu()
    assert gtd.guards_intact() and bool(torch.isnan(td[nv:]).all()), "a row past nvalid wrote td_abs"
    _assert_c51_grad(slab, loss, td[:nv], pp, X[:nv], act[:nv], m[:nv], A, NA, H, 1.0 / 777, w[:nv], wn)


# ------------------------------------------------------------------ the trainer
@pytest.mark.parametrize("extra", [dict(), dict(prioritized=True, n_step=3, per_beta_epochs=4)],
                         ids=["uniform", "per-nstep"])
def test_c51_trainer_resume_is_bitwise_and_checkpoints_name_their_atoms(cuda, extra):
    kw = dict(TRAINER, atoms=51, v_min=0.0, v_max=10.0, **extra)
    a = DQNTrainer(DQNConfig(**kw), device=cuda)
    assert a.q.P == MLPSpec(a.D, kw["hidden"], a.A * 51).P and a.y.shape == (kw["batch_size"], 51)
    for _ in range(6):
        a.train_epoch()
    b = DQNTrainer(DQNConfig(**kw), device=cuda)
    for _ in range(3):
        b.train_epoch()
    assert b.evaluate(episodes=1, num_envs=33).stats()["episodes"] == 33
    sd = b.state_dict()
    assert sd["cfg"]["atoms"] == 51 and sd["cfg"]["v_max"] == 10.0
    c = DQNTrainer(DQNConfig(**kw), device=cuda)
    c.q.params.add_(1.0)  # other weights until the load
    c.load_state_dict(sd)
    for _ in range(3):
        c.train_epoch()
    torch.cuda.synchronize()
    assert a.counters() == c.counters() and a.updates > 0
    for i, (x, y) in enumerate(zip(a.snapshot_tensors(), c.snapshot_tensors())):
        assert torch.equal(x, y), f"snapshot tensor {i} differs after the resume"
    assert a.metrics()["Atoms"] == 51 and 0.0 <= a.metrics()["QVals"] <= 10.0
    other = DQNTrainer(DQNConfig(**dict(kw, atoms=21)), device=cuda)
    scalar = DQNTrainer(DQNConfig(**dict(kw, atoms=0)), device=cuda)
    for t in (other, scalar):
        with pytest.raises(ValueError, match="atoms"):
            t.load_state_dict(sd)
    with pytest.raises(ValueError, match="atoms"):
        c.load_state_dict(scalar.state_dict())


def test_c51_trainer_learns_cartpole_like_the_cpu_oracle(cuda):
    """The CPU oracle loop with the categorical net (tests/dqn_c51_oracle.py: the same algorithm and Philox draws,
    float64 networks) at the small shape plus 51 atoms on [0, 10], 600 epochs = 1194 updates, scores a greedy mean
    return over 256 episodes of 135.41, 414.51, 323.61, 203.82 and 278.71 for seeds 1..5 (a random policy: about 22).
    The GPU trainer after the same number of updates must reach 80 % of the lowest."""
    tr = DQNTrainer(DQNConfig(**do.SMALL, seed=1, **dc.C51_SMALL), device=cuda)
    for _ in range(do.SMALL_EPOCHS):
        tr.train_epoch()
    assert tr.updates == dc.C51_UPDATES
    got = tr.evaluate(episodes=1, num_envs=do.EVAL_EPISODES).stats()["mean_return"]
    floor = 0.8 * min(dc.ORACLE_RETURNS_C51.values())
    print(f"GPU greedy mean return {got:.2f}, floor {floor:.2f}, oracle {dc.ORACLE_RETURNS_C51}")
    assert got >= floor, (got, floor)
