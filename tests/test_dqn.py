"""DQN on the CPU: the replay sampler, the Q_TD gradient head and the TD-target oracles, the public
plumbing (preset, engine resolution, config loader) and the oracle training loop whose result is
the yardstick of the GPU learning test (tests/test_dqn_gpu.py)."""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import GradHead, MLPSpec, ReplayRing, dqn_sample_rows_ref, dqn_targets, dqn_targets_ref
from relayrl_prototype_amd.ops import mlp_grad, philox
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, dqn_seeds, epsilon_at

import dqn_oracle as do
import rollout_oracle as ro


# ------------------------------------------------------------------ sampling
def test_sample_rows_lie_in_range_and_depend_on_seed_and_update():
    for filled in (1, 2, 17, 1000, 2 ** 20 + 3, 2 ** 31 - 1):
        r = dqn_sample_rows_ref(1234, 7, 4096, filled)
        assert r.dtype == np.int64 and r.min() >= 0 and r.max() < filled
    a = dqn_sample_rows_ref(1234, 7, 4096, 1000)
    np.testing.assert_array_equal(a, dqn_sample_rows_ref(1234, 7, 4096, 1000))
    assert (a != dqn_sample_rows_ref(1234, 8, 4096, 1000)).mean() > 0.9
    assert (a != dqn_sample_rows_ref(1235, 7, 4096, 1000)).mean() > 0.9
    # the high word of the 64-bit update counter and of the key reach the draw
    assert (a != dqn_sample_rows_ref(1234, 7 + 2 ** 32, 4096, 1000)).mean() > 0.9
    assert (a != dqn_sample_rows_ref(1234 + 2 ** 32, 7, 4096, 1000)).mean() > 0.9
    assert (dqn_sample_rows_ref(5, 0, 100, 1) == 0).all()
    # roughly uniform: 16 equal bins of 65536 draws, chi-square with 15 degrees of freedom
    cnt = np.bincount(dqn_sample_rows_ref(9, 3, 65536, 16), minlength=16)
    assert (((cnt - 4096.0) ** 2) / 4096.0).sum() < 45.0, cnt
    with pytest.raises(ValueError):
        dqn_sample_rows_ref(1, 0, 4, 0)


def test_sample_formula_reaches_the_top_row():
    """row = (x * filled) >> 32: x = 2^32 - 1 gives filled - 1, x = 0 gives 0, for a filled that is
    no power of two and needs more than 20 bits."""
    filled = 2 ** 20 + 3
    assert (0xFFFFFFFF * filled) >> 32 == filled - 1
    assert (0 * filled) >> 32 == 0
    # and the implementation is that formula on Philox word x
    b = np.arange(64, dtype=np.uint32)
    x = philox.philox4x32(b, np.full(64, 11, np.uint32), np.zeros(64, np.uint32), np.zeros(64, np.uint32),
                          np.full(64, 77, np.uint32), np.zeros(64, np.uint32))[0]
    want = [(int(v) * filled) >> 32 for v in x]
    np.testing.assert_array_equal(dqn_sample_rows_ref(77, 11, 64, filled), want)


# ------------------------------------------------------------------ Q_TD head
def _huber_autograd(pp, X, act, y, A, H, delta):
    p = pp.double().clone().requires_grad_(True)
    q = ref.trunk(p, X.double(), X.shape[1], H, A)[0].gather(-1, act.long().unsqueeze(-1)).squeeze(-1)
    li = torch.nn.functional.huber_loss(q, y.double(), reduction="none", delta=delta)
    li.mean().backward()
    return p.grad, li.detach(), q.detach()


@pytest.mark.parametrize("D,H,A,B,delta", [(4, 64, 2, 65, 1.0), (8, 128, 4, 33, 0.5), (6, 64, 3, 1, 2.0)])
def test_q_td_reference_matches_float64_autograd(D, H, A, B, delta):
    torch.manual_seed(B)
    pp = MLPSpec(D, H, A).init(torch.Generator().manual_seed(6))
    X = torch.randn(B, D)
    act = torch.randint(0, A, (B,), dtype=torch.int32)
    q = ref.trunk(pp, X, D, H, A)[0].gather(-1, act.long().unsqueeze(-1)).squeeze(-1)
    # targets on both sides of the threshold, above and below Q
    off = torch.tensor([0.3, -0.3, 1.7, -1.7, 0.0])[torch.arange(B) % 5] * delta
    y = q + off
    g64, li, q64 = _huber_autograd(pp, X, act, y, A, H, delta)
    assert B < 5 or ((li < 0.5 * delta * delta).any() and (li > 0.5 * delta * delta).any())
    g, st = ref.mlp_grad_ref(int(GradHead.Q_TD), pp, X, A, H, act=act, ret=y, clip_eps=delta, dtype=torch.float64)
    torch.testing.assert_close(g, g64, rtol=1e-12, atol=1e-14)
    assert abs(st["loss"] - li.sum().item()) <= 1e-12 * (1 + li.sum().item())
    assert abs(st["v"] - q64.sum().item()) <= 1e-12 * (1 + abs(q64.sum().item())) and st["count"] == B
    # the fp32 path of the CPU op: same head through ops.mlp_grad
    g32, ls = mlp_grad(GradHead.Q_TD, pp, X, A, H, act=act, ret=y, clip_eps=delta)
    scale = g64.abs().max().item() + 1e-12
    assert (g32[0].double() - g64).abs().max().item() <= 2e-4 * scale + 1e-6
    assert abs(ls[0, 0].item() - li.sum().item()) <= 1e-3 * (li.sum().item() + 1) and int(ls[0, 5]) == B


# ------------------------------------------------------------------ TD targets
def _net_with_q(D, H, A, rows):
    """A network whose Q(x) depends on x[0] alone: Q_a(x) = rows[a][0] * relu(x0) + rows[a][1]."""
    spec = MLPSpec(D, H, A)
    p = torch.zeros(spec.P, dtype=torch.float64)
    W1, b1, W2, b2, W3, b3, _ = ref.unflatten(p, D, H, A)
    W1[0, 0] = 1.0
    W2[0, 0] = 1.0
    for a, (w, b) in enumerate(rows):
        W3[a, 0] = w
        b3[a] = b
    return p


def test_targets_reference_on_a_hand_built_case():
    D, H, A, gamma = 2, 64, 3, 0.5
    #            Q_0      Q_1       Q_2   at x0 = 2
    online = _net_with_q(D, H, A, [(1.0, 0.0), (2.0, 0.0), (0.0, 1.0)])   # 2, 4, 1 -> argmax 1
    target = _net_with_q(D, H, A, [(3.0, 0.0), (0.5, 0.0), (0.0, 5.0)])   # 6, 1, 5 -> argmax 0
    ring = ReplayRing.allocate(3, 1, D, "cpu")
    ring.nobs[:, 0, 0] = 2.0
    ring.obs[:, 0, 0] = torch.tensor([10.0, 11.0, 12.0])
    ring.act[:, 0] = torch.tensor([2, 0, 1], dtype=torch.int32)
    ring.rew[:, 0] = torch.tensor([1.0, -1.0, 0.25])
    ring.done[:, 0] = torch.tensor([0.0, 1.0, 2.0])  # running, terminal, truncated
    B, seed, upd = 64, 3, 0
    idx = dqn_sample_rows_ref(seed, upd, B, 3)
    assert set(idx) == {0, 1, 2}
    rew = np.array([1.0, -1.0, 0.25])[idx]
    for double_q, qsel in ((False, 6.0), (True, 1.0)):  # max of the target net / the target's value at the online argmax
        Xb, act_b, y, ix = dqn_targets_ref(online, target, H, A, ring, 3, gamma, double_q, seed, upd, B, torch.float64)
        np.testing.assert_array_equal(ix.numpy(), idx)
        np.testing.assert_array_equal(Xb[:, 0].numpy(), np.array([10.0, 11.0, 12.0])[idx])
        np.testing.assert_array_equal(act_b.numpy(), np.array([2, 0, 1])[idx])
        want = rew + gamma * np.where(idx == 1, 0.0, qsel)  # the terminal row drops the bootstrap, the truncated keeps it
        np.testing.assert_allclose(y.numpy(), want, rtol=0, atol=1e-12)
    # a tie takes the lowest index: the online net prefers actions 1 and 2 equally -> the target's Q_1
    tie = _net_with_q(D, H, A, [(0.0, 0.0), (0.0, 3.0), (0.0, 3.0)])
    _, _, y, _ = dqn_targets_ref(tie, target, H, A, ring, 3, gamma, True, seed, upd, B, torch.float64)
    np.testing.assert_allclose(y.numpy(), rew + gamma * np.where(idx == 1, 0.0, 1.0), rtol=0, atol=1e-12)
    # filled = 1 reads row 0 only; the CPU op is the reference
    out = dqn_targets(online.float(), target.float(), H, A, ring, 1, gamma, True, seed, upd, 5)
    assert (out[3] == 0).all() and torch.allclose(out[2], torch.full((5,), 1.0 + gamma * 1.0))


# ------------------------------------------------------------------ plumbing
def test_preset_engine_resolution_and_config_loader():
    from relayrl_prototype_amd.config import ConfigLoader
    from relayrl_prototype_amd.runtime import engine as eng
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    p = PRESETS["cartpole-dqn"]
    assert p.kind == "vec" and p.overrides["algo"] == "dqn" and p.overrides["env"] == "CartPole-v1"
    cfg = DQNConfig(**{k: v for k, v in p.overrides.items()})  # every override is a DQNConfig field
    assert cfg.buffer_slots % cfg.rollout_len == 0 and cfg.learning_starts <= cfg.buffer_slots * cfg.num_envs
    spec = eng.resolve_engine("DQN", 4, 2, {}, {}, {"epsilon": 0.9, "epsilon_min": 0.1, "q_lr": 1e-3, "batch_size": 64},
                              engine="vec")
    assert spec.algo == "dqn" and spec.kind == "vec" and spec.world_size == 1 and spec.env == "CartPole-v1"
    assert spec.trainer["algo"] == "dqn"
    assert (spec.trainer["eps_start"], spec.trainer["eps_end"], spec.trainer["q_lr"], spec.trainer["batch_size"]) == (
        0.9, 0.1, 1e-3, 64)
    with pytest.raises(ValueError):
        eng.resolve_engine("DQN", 4, 2, {}, {}, {}, engine="host")
    with pytest.raises(ValueError):
        eng.resolve_engine("DQN", 4, 2, {}, {}, {"world_size": 2}, engine="vec")
    with pytest.raises(ValueError):
        eng.resolve_engine("DQN", 4, 2, {}, {"world_size": 2}, {}, engine="vec")
    assert eng.resolve_engine("DQN", 4, 2, {}, {}, {}) is None  # no engine asked for
    assert eng.resolve_engine("REINFORCE", 4, 2, {}, {}, {}, engine="vec").algo == "reinforce"
    assert ConfigLoader("DQN").get_algorithm_params() is None  # reference parity: no fallback block


def test_trainer_refuses_what_it_does_not_support():
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNTrainer

    class Multi:
        multi = True

    with pytest.raises(ValueError):
        DQNTrainer(DQNConfig(), comm=Multi(), device="cpu")
    with pytest.raises(ValueError):
        DQNTrainer(DQNConfig(env="HalfCheetahSynth-v0"), device="cpu")
    with pytest.raises(ValueError):
        DQNTrainer(DQNConfig(buffer_slots=10, rollout_len=4), device="cpu")


def test_stochastic_evaluation_of_a_dqn_checkpoint_raises():
    from relayrl_prototype_amd.runtime.launcher import evaluate_checkpoint_state

    st = {"trainer": {"cfg": DQNConfig().to_dict(), "learner": {"pi": {"params": torch.zeros(8)}}, "epoch": 1}}
    with pytest.raises(ValueError, match="stochastic"):
        evaluate_checkpoint_state(st, stochastic=True)


def test_epsilon_schedule_and_seeds():
    cfg = DQNConfig(eps_start=1.0, eps_end=0.05, eps_decay_epochs=100)
    assert epsilon_at(cfg, 0) == 1.0 and epsilon_at(cfg, 100) == pytest.approx(0.05) and epsilon_at(cfg, 10 ** 6) == pytest.approx(0.05)
    assert epsilon_at(cfg, 50) == pytest.approx(0.525)
    assert len(set(dqn_seeds(1)) | set(dqn_seeds(2))) == 6


# ------------------------------------------------------------------ oracle training loop
def test_explore_draws_follow_epsilon():
    envs = np.arange(4096)
    ex0, _, _ = do.explore_draws(5, 9, envs, 0.0, 2)
    ex1, a1, _ = do.explore_draws(5, 9, envs, 1.0, 3)
    assert not ex0.any() and ex1.all()
    assert a1.min() == 0 and a1.max() == 2
    ex, _, _ = do.explore_draws(5, 9, envs, 0.25, 2)
    assert abs(ex.mean() - 0.25) < 0.03


@pytest.mark.parametrize("name", ["CartPole-v1", "Acrobot-v1", "LunarLanderSynth-v0"])
@pytest.mark.parametrize("H", [64, 128])
def test_case_weights_leave_few_greedy_cells_undecided(name, H):
    """The GPU rollout test leaves a greedy cell out when the float64 gap of its two largest Q-values is
    below 4x the fp32-vs-float64 Q error; with the case weights (rollout_oracle.case_params) on rollout
    observations that is at most MAX_SKIP_SHARE of the cells, by the float64 reference alone."""
    e = ro.env_of(name)
    params = ro.case_params(e, H)
    sim = ro.simulate(e, params, H, 80, 9, seed=(7 << 32) | 21, step0=2 ** 32 - 4, max_steps=6)
    obs = sim["obs"][:9].reshape(-1, e.D)
    _, gap, tol = do.q_gap_tolerance(params, obs, e.A, H)
    assert 0 < tol < 1e-4, tol
    assert (gap < tol).mean() <= ro.MAX_SKIP_SHARE, ((gap < tol).mean(), tol)


def test_oracle_loop_learns_cartpole_at_the_small_shape():
    """Seed 3, the lowest of the five recorded seeds (dqn_oracle.ORACLE_RETURNS), must be reproduced to
    within 20 % (BLAS builds may order float64 sums differently) and beat three times a random
    policy's 22 steps."""
    cfg = DQNConfig(**do.SMALL, seed=3)
    params, updates = do.oracle_dqn(cfg, do.SMALL_EPOCHS)
    first = -(-cfg.learning_starts // (cfg.num_envs * cfg.rollout_len))  # the epoch of the first update
    assert updates == (do.SMALL_EPOCHS - first + 1) * cfg.updates_per_epoch == 1194
    r = do.greedy_return(params, cfg.hidden, dqn_seeds(3)[2])
    print("oracle greedy return, seed 3:", r)
    untrained = do.greedy_return(MLPSpec(4, cfg.hidden, 2).init(torch.Generator().manual_seed(3)), cfg.hidden,
                                 dqn_seeds(3)[2])
    assert untrained < 40 and r >= 66.0
    assert r >= 0.8 * do.ORACLE_RETURNS[3]
