"""V-trace off-policy correction (Espeholt et al. 2018) on the CPU: the float64 oracle against
GAE identities and a hand-computed case, the configuration checks, and the actor-learner engine
with ``correction="vtrace"`` on one rank and on two gloo ranks with lag 1."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.ops import vtrace_scan_tm

# Mean |log pi - log mu| per row, measured on this engine (CartPole-v1, 8 envs x 16 steps, hidden 64):
#   one rank, on-policy (the learner re-evaluates the actor's own weights):  5.6e-9 .. 8.4e-9  (fp32 rounding)
#   two ranks, max_lag = 1, pi_lr = 1e-2 (rank 1 acts on weights one update old), after 4 steps:  4.1e-2
#     (over both blocks of the shard; the colocated actor's half is on-policy)
# The bound between "on-policy" and "off-policy" is their geometric mean, 1.9e-5: the two sit 5e6 x apart.
_ON_POLICY = 8.4e-9
_LAGGED = 4.1e-2
ON_POLICY_BOUND = math.sqrt(_ON_POLICY * _LAGGED)


def _inputs(K, T, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    rew = torch.randn(K, T, N, generator=g, dtype=f64)
    val = torch.randn(K * T * N + K * N, generator=g, dtype=f64)
    tval = torch.randn(K, T, N, generator=g, dtype=f64)
    u = torch.rand(K, T, N, generator=g, dtype=f64)
    done = torch.where(u < 0.1, 1.0, torch.where(u < 0.2, 2.0, 0.0)).to(f64)
    done[0, T - 1, 0] = 1.0  # the bootstrap column is ignored behind a terminal ...
    done[K - 1, T - 1, 1] = 2.0  # ... and replaced by tval behind a truncation
    logp = -2.0 * torch.rand(K, T, N, generator=g, dtype=f64)
    return rew, done, val, tval, logp


@pytest.mark.parametrize("lam", [0.0, 0.5, 0.97, 1.0])
@pytest.mark.parametrize("bars", [(1.0, 1.0, 1.0), (2.0, 1.5, 3.0)])
def test_on_policy_is_gae(lam, bars):
    """logp_pi == logp_mu and thresholds >= 1: ret == V + GAE(lam), and adv == GAE(1) for lam == 1."""
    K, T, N = 3, 9, 5
    rew, done, val, tval, logp = _inputs(K, T, N)
    assert (done == 1).any() and (done == 2).any()
    for tv in (tval, None):
        adv, ret, stats, is_stats = vtrace_scan_tm(rew, done, val, logp, logp.clone(), 0.98, lam, *bars, tval=tv)
        g_adv, _, g_stats = ref.gae_scan_tm_ref(rew, done, val, 0.98, lam, tv)
        torch.testing.assert_close(ret, val[:K * T * N].reshape(K, T, N) + g_adv, rtol=1e-12, atol=1e-12)
        if lam == 1.0:
            torch.testing.assert_close(adv, g_adv, rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(stats, g_stats.to(stats.dtype), rtol=1e-12, atol=1e-12)
        assert stats[2].item() == K * T * N
        assert is_stats[0].item() == pytest.approx(K * T * N, abs=1e-9) and is_stats[1].item() == 0.0


def test_blocks_equal_separate_scans():
    """[K, T, N] with the flat val layout == K separate [T, N] scans."""
    K, T, N = 3, 6, 4
    rew, done, val, tval, mu = _inputs(K, T, N, seed=1)
    pi = mu + 0.5 * torch.randn(K, T, N, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    adv, ret, stats, is_stats = vtrace_scan_tm(rew, done, val, mu, pi, 0.98, 0.97, 1.5, 1.0, 2.0, tval=tval)
    s_sum = torch.zeros(3, dtype=torch.float64)
    i_sum = torch.zeros(2, dtype=torch.float64)
    for k in range(K):
        vk = torch.cat([val[k * T * N:(k + 1) * T * N], val[K * T * N + k * N:K * T * N + (k + 1) * N]])
        a, r, s, i = vtrace_scan_tm(rew[k], done[k], vk, mu[k], pi[k], 0.98, 0.97, 1.5, 1.0, 2.0, tval=tval[k])
        torch.testing.assert_close(adv[k], a, rtol=0, atol=0)
        torch.testing.assert_close(ret[k], r, rtol=0, atol=0)
        s_sum += s
        i_sum += i
    torch.testing.assert_close(stats, s_sum, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(is_stats, i_sum, rtol=1e-12, atol=1e-12)


def test_hand_case():
    """T = 3, N = 1, a terminal in the middle, ratios 1.2 / 0.5 / 3 against rho_bar = 1.5, c_bar = 1,
    pg_rho_bar = 2 (each threshold has a ratio above and one below it), gamma = 0.9, lam = 0.8:

      t = 2: v_next = V3 = 2; rho, c, rho_pg = 1.5, 0.8, 2;  delta = 3 + 0.9 * 2 + 0.5 = 5.3
             adv = 2 * 5.3 = 10.6;  acc = 1.5 * 5.3 = 7.95;  ret = -0.5 + 7.95 = 7.45
      t = 1: terminal, v_next = 0; rho, c, rho_pg = 0.5, 0.4, 0.5;  delta = 2 - 1 = 1
             adv = 0.5;  acc = 0.5 (the trace is cut);  ret = 1.5
      t = 0: v_next = V1 = 1; rho, c, rho_pg = 1.2, 0.8, 1.2
             adv = 1.2 * (1 + 0.9 * (1 + 0.5) - 0.5) = 2.22
             acc = 1.2 * (1 + 0.9 - 0.5) + 0.9 * 0.8 * 0.5 = 2.04;  ret = 2.54"""
    f64 = torch.float64
    rew = torch.tensor([[1.0], [2.0], [3.0]], dtype=f64)
    done = torch.tensor([[0.0], [1.0], [0.0]], dtype=f64)
    val = torch.tensor([0.5, 1.0, -0.5, 2.0], dtype=f64)
    ratio = torch.tensor([[1.2], [0.5], [3.0]], dtype=f64)
    mu = torch.full((3, 1), -1.0, dtype=f64)
    adv, ret, stats, is_stats = vtrace_scan_tm(rew, done, val, mu, mu + torch.log(ratio), 0.9, 0.8, 1.5, 1.0, 2.0)
    torch.testing.assert_close(adv.reshape(-1), torch.tensor([2.22, 0.5, 10.6], dtype=f64), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ret.reshape(-1), torch.tensor([2.54, 1.5, 7.45], dtype=f64), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(stats, torch.tensor([13.32, 117.5384, 3.0], dtype=f64), rtol=1e-12, atol=1e-12)
    expect = torch.tensor([3.2, math.log(1.2) + math.log(2.0) + math.log(3.0)], dtype=f64)
    torch.testing.assert_close(is_stats, expect, rtol=1e-12, atol=1e-12)
    # a truncation at t = 1 bootstraps with tval there and still cuts the trace from t = 2:
    #   t = 1: delta = 2 + 0.9 * 4 - 1 = 4.6;  adv = acc = 0.5 * 4.6 = 2.3;  ret = 3.3
    #   t = 0: adv = 1.2 * (1 + 0.9 * (1 + 2.3) - 0.5) = 4.164;  acc = 1.68 + 0.72 * 2.3 = 3.336;  ret = 3.836
    done[1, 0] = 2.0
    tval = torch.tensor([[9.0], [4.0], [9.0]], dtype=f64)
    adv, ret, _, _ = vtrace_scan_tm(rew, done, val, mu, mu + torch.log(ratio), 0.9, 0.8, 1.5, 1.0, 2.0, tval=tval)
    torch.testing.assert_close(adv.reshape(-1), torch.tensor([4.164, 2.3, 10.6], dtype=f64), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ret.reshape(-1), torch.tensor([3.836, 3.3, 7.45], dtype=f64), rtol=1e-12, atol=1e-12)


def test_wrapper_fills_preallocated_outputs():
    rew, done, val, tval, mu = _inputs(2, 4, 3, seed=3)
    adv, ret = torch.zeros(2, 4, 3), torch.zeros(2, 4, 3)
    stats, is_out = torch.zeros(3), torch.zeros(2)
    a, r, s, i = vtrace_scan_tm(rew, done, val, mu, mu - 0.1, 0.98, 0.97, adv=adv, ret=ret, stats_out=stats,
                                is_out=is_out, tval=tval)
    torch.testing.assert_close(adv, a.float())
    torch.testing.assert_close(ret, r.float())
    torch.testing.assert_close(stats, s.float())
    torch.testing.assert_close(is_out, i.float())
    with pytest.raises(ValueError, match="value function"):
        vtrace_scan_tm(rew, done, None, mu, mu, 0.98, 0.97)
    with pytest.raises(ValueError, match="positive"):
        vtrace_scan_tm(rew, done, val, mu, mu, 0.98, 0.97, rho_bar=0.0)


def test_config_validation():
    from relayrl_prototype_amd.algorithms.learner import PGLearner
    from relayrl_prototype_amd.runtime.actor_learner import ActorLearner, ActorLearnerConfig
    from relayrl_prototype_amd.runtime.rollout_learn import RolloutLearner

    def learner(algo="reinforce", baseline=True):
        return PGLearner(algo, 4, 2, 64, True, baseline, train_vf_iters=1, device="cpu")

    with pytest.raises(ValueError, match="ppo"):
        RolloutLearner(learner("ppo"), 4, 2, 0.99, 0.95, correction="vtrace")
    with pytest.raises(ValueError, match="value function"):
        RolloutLearner(learner(baseline=False), 4, 2, 0.99, 0.95, correction="vtrace")
    with pytest.raises(ValueError, match="agent rows"):
        RolloutLearner(learner(), 4, 2, 0.99, 0.95, correction="vtrace", agent_rows_enabled=True)
    rl = RolloutLearner(learner(), 4, 2, 0.99, 0.95, correction="vtrace")
    with pytest.raises(ValueError, match="agent rows"):  # the engine switches agent rows on after construction
        rl.agent_rows_enabled = True
    with pytest.raises(ValueError, match="correction="):
        RolloutLearner(learner(), 4, 2, 0.99, 0.95, correction="retrace")
    with pytest.raises(ValueError, match="positive"):
        RolloutLearner(learner(), 4, 2, 0.99, 0.95, correction="vtrace", c_bar=0.0)
    RolloutLearner(learner("ppo"), 4, 2, 0.99, 0.95).agent_rows_enabled = True  # untouched without the correction

    base = dict(env="CartPole-v1", num_envs=4, rollout_len=4, hidden=64, train_vf_iters=1, num_threads=1)
    for bad, why in ((dict(correction="retrace"), "correction="), (dict(correction="vtrace", algo="ppo"), "ppo"),
                     (dict(correction="vtrace", with_baseline=False), "value function"),
                     (dict(correction="vtrace", vtrace_rho_bar=-1.0), "positive")):
        with pytest.raises(ValueError, match=why):
            ActorLearner(ActorLearnerConfig(**base, **bad), device="cpu")


def test_config_reachable_from_engine_and_presets():
    """--set correction=vtrace / TrainingServer(engine="actor_learner", ...) hyperparameters reach the config
    by field name, like max_lag."""
    from relayrl_prototype_amd.runtime.actor_learner import ActorLearnerConfig
    from relayrl_prototype_amd.runtime.engine import _filter, resolve_engine
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    spec = resolve_engine("REINFORCE", 4, 2, {}, {}, {"correction": "vtrace", "vtrace_rho_bar": 2.0, "max_lag": 1},
                          engine="actor_learner")
    cfg = ActorLearnerConfig(**_filter(ActorLearnerConfig, spec.trainer))
    assert (cfg.correction, cfg.vtrace_rho_bar, cfg.vtrace_c_bar, cfg.max_lag) == ("vtrace", 2.0, 1.0, 1)
    kw = dict(PRESETS["lunarlander-reinforce-baseline"].overrides, correction="vtrace")
    assert ActorLearnerConfig(**_filter(ActorLearnerConfig, kw)).correction == "vtrace"
    assert ActorLearnerConfig().correction == "none"


def _run_world1(correction, steps):
    from relayrl_prototype_amd.runtime.actor_learner import ActorLearner, ActorLearnerConfig

    cfg = ActorLearnerConfig(env="CartPole-v1", num_envs=8, rollout_len=16, hidden=64, train_vf_iters=2, lam=1.0,
                             num_threads=1, seed=5, correction=correction)
    al = ActorLearner(cfg, device="cpu")
    ms = []
    for _ in range(steps):
        al.step()
        ms.append(al.metrics())
    al.finish()
    return al.learner.pi.params.clone(), al.learner.vf.params.clone(), ms


def test_actor_learner_world1_vtrace_equals_gae_at_lam1():
    """lam = 1 and on-policy data: the V-trace advantages and targets are the GAE ones, so one step
    leaves the same parameters (after one step both runs have sampled the same actions).

    Tolerance.  Two correction="none" runs agree exactly (measured 0.0).  The V-trace run differs by the
    fp32 rounding of ratio = exp(logp_pi - logp_mu) ~ 1 +- 1e-7 and of the regrouped recurrence; Adam's
    first steps move a parameter by ~lr * sign(g), so a 1e-7 relative change of a gradient moves the
    result by far less than one ulp and what remains is the last rounding of the parameter itself:
    at most 1 ulp per Adam step at |p| < 1, 2^-24 = 6.0e-8.  Measured: 7.5e-9 (policy, 1 step) and
    3.0e-8 (value net, 2 steps) with parameters up to 0.5.  Allowed: 10 x 2^-24."""
    tol = 10 * 2.0 ** -24
    p_none, v_none, _ = _run_world1("none", 1)
    p_vt, v_vt, ms = _run_world1("vtrace", 1)
    print("max |d pi|", (p_none - p_vt).abs().max().item(), "max |d vf|", (v_none - v_vt).abs().max().item())
    torch.testing.assert_close(p_vt, p_none, rtol=0, atol=tol)
    torch.testing.assert_close(v_vt, v_none, rtol=0, atol=tol)
    assert "MeanRho" in ms[0] and "MeanAbsLogRatio" in ms[0]


def test_actor_learner_world1_stays_on_policy():
    _, _, ms = _run_world1("vtrace", 3)
    _, _, ms_none = _run_world1("none", 1)
    assert "MeanRho" not in ms_none[0] and "MeanAbsLogRatio" not in ms_none[0]
    for m in ms:
        print("MeanRho", m["MeanRho"], "MeanAbsLogRatio", m["MeanAbsLogRatio"])
        assert 0.0 <= m["MeanAbsLogRatio"] < ON_POLICY_BOUND
        assert 1.0 - ON_POLICY_BOUND < m["MeanRho"] <= 1.0 + 1e-6  # min(1, ratio) <= 1, fp32 sum of B ones


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_lag1(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        from relayrl_prototype_amd.parallel.comm import init_distributed
        from relayrl_prototype_amd.runtime.actor_learner import ActorLearner, ActorLearnerConfig

        comm = init_distributed(backend="gloo")
        cfg = ActorLearnerConfig(env="CartPole-v1", num_envs=8, rollout_len=16, hidden=64, train_vf_iters=2,
                                 num_threads=1, seed=5, max_lag=1, learner_ranks=1, pi_lr=1e-2,
                                 correction="vtrace", verify_versions=True)
        al = ActorLearner(cfg, comm, device="cpu")
        for _ in range(4):
            al.step()
        al.finish()
        m = al.metrics()
        q.put((rank, bool(torch.isfinite(al.wbuf).all()), al.epoch, m.get("MeanRho"), m.get("MeanAbsLogRatio"),
               m.get("ActorVersions")))
        dist.destroy_process_group()
    except Exception:
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None, None))


def test_actor_learner_gloo_lag1_is_off_policy():
    """Two ranks, one learner: rank 1 rolls out on weights one update old, so the learner's batch is
    measurably off-policy (MeanAbsLogRatio far above the one-rank value) and training stays finite."""
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_lag1, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda r: r[0])
    for p in ps:
        p.join(timeout=60)
    for r in res:
        assert r[1] is True, (r[0], r[1])
        assert r[2] == 4
    rank, _, _, mean_rho, mean_abs, versions = res[0]
    print("MeanRho", mean_rho, "MeanAbsLogRatio", mean_abs, "versions", versions)
    assert versions == [3, 2]  # the colocated actor is current, the remote one lags by one update
    assert res[1][3] is None and res[1][4] is None  # the actor-only rank reports no learner columns
    assert mean_abs > ON_POLICY_BOUND
    assert 0.0 < mean_rho <= 1.0 + 1e-6
