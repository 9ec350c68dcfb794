"""V-trace on the GPU: vtrace_scan_tm_kernel against the float64 oracle, the K-block learner with
``correction="vtrace"`` against the CPU oracle, and the colocated actor-learner engine on cuda:0."""
import functools

import pytest
import torch

from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.ops import vtrace_scan_tm
from test_vtrace import ON_POLICY_BOUND

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.98, 0.97
SHAPES = [(1, 1, 1), (1, 7, 300), (3, 5, 33), (2, 64, 257)]
BARS = [(1.0, 1.0, 1.0), (2.0, 1.0, 1.0), (1.5, 1.0, 2.0)]


@functools.lru_cache(maxsize=None)
def _inputs(K, T, N):
    """fp32 inputs (what the kernel reads); the oracle gets the same values as float64."""
    g = torch.Generator().manual_seed(1000 * K + 10 * T + N)
    rew = torch.randn(K, T, N, generator=g)
    val = torch.randn(K * T * N + K * N, generator=g)
    tval = torch.randn(K, T, N, generator=g)
    u = torch.rand(K, T, N, generator=g)
    done = torch.where(u < 0.04, torch.ones_like(u), torch.where(u < 0.06, torch.full_like(u, 2.0),
                                                                  torch.zeros_like(u)))
    done[0, T - 1, 0] = 1.0            # one column ends in a terminal (bootstrap column ignored) ...
    done[K - 1, T - 1, N - 1] = 2.0    # ... and one in a truncation (for N = 1: this one)
    mu = -2.0 * torch.rand(K, T, N, generator=g)
    pi = mu + 0.5 * torch.randn(K, T, N, generator=g)
    return rew, done, val, tval, mu, pi


@functools.lru_cache(maxsize=None)
def _oracle(K, T, N, bars, with_tval=True):
    rew, done, val, tval, mu, pi = (x.double() for x in _inputs(K, T, N))
    return ref.vtrace_scan_tm_ref(rew, done, val, mu, pi, GAMMA, LAM, *bars, tval if with_tval else None)


def _check(cuda, K, T, N, bars, with_tval):
    rew, done, val, tval, mu, pi = (x.to(cuda) for x in _inputs(K, T, N))
    a_r, r_r, s_r, i_r = _oracle(K, T, N, bars, with_tval)
    a, r, s, i = vtrace_scan_tm(rew, done, val, mu, pi, GAMMA, LAM, *bars, tval=tval if with_tval else None)
    torch.testing.assert_close(a.cpu().double(), a_r, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(r.cpu().double(), r_r, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(s.cpu().double(), s_r, rtol=1e-3, atol=1e-2)
    torch.testing.assert_close(i.cpu().double(), i_r, rtol=1e-4, atol=0)


@pytest.mark.parametrize("bars", BARS)
@pytest.mark.parametrize("K,T,N", SHAPES)
def test_vtrace_scan_tm(cuda, K, T, N, bars):
    if T * N > 100:  # about half the ratios exceed 1 (and each threshold): both branches of every min
        ratio = torch.exp(_inputs(K, T, N)[5] - _inputs(K, T, N)[4])
        for b in set(bars):
            assert 0.05 < (ratio > b).float().mean().item() < 0.95
    _check(cuda, K, T, N, bars, True)


def test_vtrace_scan_tm_without_tval(cuda):
    _check(cuda, 3, 5, 33, (1.5, 1.0, 2.0), False)


def test_vtrace_scan_tm_preallocated_and_checked(cuda):
    """The preallocation arguments are written in place, and bad arguments raise before a launch."""
    from relayrl_prototype_amd.ops import hip

    K, T, N = 3, 5, 33
    rew, done, val, tval, mu, pi = (x.to(cuda) for x in _inputs(K, T, N))
    adv, ret = torch.zeros(K, T, N, device=cuda), torch.zeros(K, T, N, device=cuda)
    part = torch.zeros(hip().scan_tm_parts(K * N) * 5, device=cuda)
    stats, is_out = torch.zeros(3, device=cuda), torch.zeros(2, device=cuda)
    out = vtrace_scan_tm(rew, done, val, mu, pi, GAMMA, LAM, 1.5, 1.0, 2.0, adv=adv, ret=ret, stats_part=part,
                         stats_out=stats, is_out=is_out, tval=tval)
    assert all(o.data_ptr() == b.data_ptr() for o, b in zip(out, (adv, ret, stats, is_out)))
    a_r, r_r, s_r, i_r = _oracle(K, T, N, (1.5, 1.0, 2.0))
    torch.testing.assert_close(adv.cpu().double(), a_r, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(is_out.cpu().double(), i_r, rtol=1e-4, atol=0)
    h = hip()
    args = dict(rew=rew, done=done, val=val, tval=tval, logp_mu=mu, logp_pi=pi, adv=adv, ret=ret, stats_part=part,
                stats_out=stats, is_out=is_out, gamma=GAMMA, lam=LAM, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0)
    for bad in (dict(logp_pi=pi[:, :, :-1].contiguous()), dict(logp_mu=mu.double()), dict(val=val[:-1]),
                dict(stats_part=part[:-1]), dict(c_bar=0.0), dict(adv=adv[:, :-1].contiguous()),
                dict(logp_pi=pi.transpose(1, 2))):
        with pytest.raises(RuntimeError):
            h.vtrace_scan_tm(**dict(args, **bad))


@pytest.mark.parametrize("discrete", [True, False])
def test_rollout_learner_vtrace_matches_oracle(cuda, discrete):
    """K = 3 actor blocks through the HIP learner with correction="vtrace" == the same batch through the
    CPU oracle (the given logp = -U(0, 1) makes the batch off-policy by itself); the tolerances of
    test_rollout_learner_blocks_match_oracle."""
    from relayrl_prototype_amd.algorithms.learner import PGLearner
    from relayrl_prototype_amd.runtime.rollout_learn import RolloutLearner

    K, T, N = 3, 16, 64
    D, A = (4, 2) if discrete else (17, 6)
    g = torch.Generator().manual_seed(0)
    obs = torch.randn(K * T * N + K * N, D, generator=g)
    if discrete:
        act = torch.randint(0, A, (K, T, N), generator=g, dtype=torch.int32)
    else:
        act = torch.randn(K, T, N, A, generator=g)
    rew = torch.rand(K, T, N, generator=g)
    u = torch.rand(K, T, N, generator=g)
    done = torch.where(u < 0.05, torch.ones_like(u), torch.where(u < 0.07, torch.full_like(u, 2.0),
                                                                  torch.zeros_like(u)))
    logp = -torch.rand(K, T, N, generator=g)
    tobs = torch.randn(K, T, N, D, generator=g)
    out = []
    for dev in ("cpu", cuda):
        lr = PGLearner("reinforce", D, A, 128, discrete, True, 3e-4, 1e-3, 3, device=dev, seed=1, use_graphs=False)
        rl = RolloutLearner(lr, T, N, 0.98, 0.97, blocks=K, correction="vtrace", rho_bar=1.5, c_bar=1.0,
                            pg_rho_bar=2.0)
        rl.learn(obs.to(dev), act.to(dev), rew.to(dev), done.to(dev), logp.to(dev), tobs=tobs.to(dev))
        out.append((lr.pi.params.cpu(), lr.vf.params.cpu(), rl.ret.cpu(), rl.is_stats.cpu(), rl.adv.cpu()))
    print("max |d ret|", (out[1][2] - out[0][2]).abs().max().item(), "max |d adv|",
          (out[1][4] - out[0][4]).abs().max().item(), "max |d pi|", (out[1][0] - out[0][0]).abs().max().item(),
          "max |d vf|", (out[1][1] - out[0][1]).abs().max().item(), "is", out[0][3].tolist(), out[1][3].tolist())
    assert out[0][3][1].item() / (K * T * N) > 0.1  # off-policy indeed
    torch.testing.assert_close(out[1][2], out[0][2], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out[1][0], out[0][0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out[1][1], out[0][1], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out[1][3], out[0][3], rtol=1e-4, atol=0)


def _colocated(cuda, correction, steps=3):
    from relayrl_prototype_amd.runtime.actor_learner import ActorLearner, ActorLearnerConfig

    al = ActorLearner(ActorLearnerConfig(env="LunarLanderSynth-v0", num_envs=512, rollout_len=32, train_vf_iters=4,
                                         integrity="strict", correction=correction), device=cuda)
    assert al.actor.kind == "device" and al.topo.K == 1
    p0 = al.learner.pi.params.clone()
    for _ in range(steps):
        al.step()
    al.finish()
    return al, p0, al.metrics()


def test_actor_learner_vtrace_gpu(cuda):
    al, p0, m = _colocated(cuda, "vtrace")
    print("MeanRho", m["MeanRho"], "MeanAbsLogRatio", m["MeanAbsLogRatio"])
    assert m["EnvSteps"] == 3 * 32 * 512 and m["IntegrityMismatches"] == 0
    assert torch.isfinite(al.learner.pi.params).all() and torch.isfinite(al.learner.vf.params).all()
    assert not torch.equal(p0, al.learner.pi.params)
    assert torch.equal(al.actor.params, al.learner.pi.params)
    # the colocated actor rolls out on the newest weights: on-policy, within the bound of the CPU test
    assert 1.0 - ON_POLICY_BOUND <= m["MeanRho"] <= 1.0 + 1e-6
    # correction="none" is the parent's path: two runs from one seed end bit for bit equal
    a1, _, m1 = _colocated(cuda, "none")
    a2, _, _ = _colocated(cuda, "none")
    assert "MeanRho" not in m1
    assert torch.equal(a1.learner.pi.params, a2.learner.pi.params)
    assert torch.equal(a1.learner.vf.params, a2.learner.vf.params)
