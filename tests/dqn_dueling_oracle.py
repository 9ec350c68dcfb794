"""Host oracles of the dueling head (tests/test_dqn_dueling.py, tests/test_dqn_dueling_gpu.py).

* ``fold``: the plain A-output net a dueling net of A + 1 outputs equals exactly (both streams are linear
  on the shared trunk).  It shares no code with ``reference.dueling_q``.
* ``adv_gap_tolerance``: ``dqn_oracle.q_gap_tolerance``'s rule for a net of A + 1 outputs, on the advantages.
* ``oracle_dqn_dueling``: the CPU oracle loop of tests/dqn_oracle.py with the dueling net,
  ``dqn_targets_ref(dueling=True)`` and ``HEAD_Q_DUEL``; its greedy returns are the yardstick of the GPU
  learning test.
"""
import numpy as np
import torch

from relayrl_prototype_amd.ops import MLPSpec, ReplayRing, dqn_targets_ref
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, dqn_seeds, epsilon_at

import dqn_oracle as do
import rollout_oracle as ro

# Greedy mean return over do.EVAL_EPISODES episodes at do.SMALL plus dueling=True, seeds 1..5, measured with
# oracle_dqn_dueling below (single-threaded torch, float64 networks) and greedy_return_dueling on the evaluation
# key dqn_seeds(seed)[2]; a random policy scores about 22.
#
# At do.SMALL_EPOCHS = 600 epochs (1194 updates) the five scored 167.91, 160.96, 240.57, 500.00 and 9.26: seed 5
# sat in a collapsed policy at that moment, and 80 % of 9.26 is below 44, twice a random policy, which is no
# bar at all.  So, once, both sides run twice as long: DUEL_EPOCHS = 1200 epochs (2394 updates), where the
# same five seeds score the values below.  No hyperparameter was changed.
DUEL_EPOCHS = 1200
DUEL_UPDATES = 2394
ORACLE_RETURNS_DUEL_600 = {1: 167.91, 2: 160.96, 3: 240.57, 4: 500.00, 5: 9.26}
ORACLE_RETURNS_DUEL = {1: 151.12, 2: 134.50, 3: 253.68, 4: 472.31, 5: 495.76}


def fold(params, D, H, A):
    """The plain ``MLPSpec(D, H, A)`` net of a dueling ``MLPSpec(D, H, A + 1)`` net:
    ``W3'[a] = W3[a] + W3[A] - mean_k W3[k]`` over the advantage rows k < A, and ``b3'`` alike."""
    W1, b1, W2, b2, W3, b3, _ = ref.unflatten(params, D, H, A + 1)
    W3f = W3[:A] + W3[A:A + 1] - W3[:A].mean(0, keepdim=True)
    b3f = b3[:A] + b3[A] - b3[:A].mean()
    return torch.cat([t.reshape(-1) for t in (W1, b1, W2, b2, W3f, b3f)])


def adv_gap_tolerance(params, obs, A, H):
    """(float64 argmax of the advantages, gap of the two largest float64 advantages, tol) at ``obs`` [n, D] for
    a dueling net of A + 1 outputs: tol is 4x the largest fp32-vs-float64 output difference of the CPU
    reference on these very inputs (dqn_oracle.q_gap_tolerance's rule)."""
    x = torch.from_numpy(np.ascontiguousarray(obs))
    o64 = ref.trunk(params.double(), x.double(), x.shape[1], H, A + 1)[0]
    o32 = ref.mlp_forward_ref(3, params, x, A + 1, H)["logits"]
    tol = 4.0 * float((o32.double() - o64).abs().max())
    act, gap = ref.greedy_from_logits(o64[:, :A])
    return act.numpy(), gap.numpy(), tol


def greedy_return_dueling(params, H, seed, episodes=do.EVAL_EPISODES, dtype=torch.float64):
    """``dqn_oracle.greedy_return`` for a dueling net: the action is the argmax of the advantages."""
    e = ro.CartPole
    envs = np.arange(episodes)
    s = e.reset(e.reset_uniforms(seed, 0, envs)).astype(np.float32)
    ret = np.zeros(episodes)
    alive = np.ones(episodes, bool)
    for t in range(e.max_steps):
        out, _ = ref.trunk(params.to(dtype), torch.from_numpy(e.obs(s)).to(dtype), e.D, H, e.A + 1)
        a = ref.greedy_from_logits(out[:, :e.A])[0].numpy()
        ns, r, term, _ = e.step(s, a, e.step_noise(seed, t, envs), np.float32)
        ret += np.where(alive, r, 0.0)
        alive &= ~term
        s = ns.astype(np.float32)
        if not alive.any():
            break
    return float(ret.mean())


def oracle_dqn_dueling(cfg: DQNConfig, epochs: int, dtype=torch.float64):
    """``dqn_oracle.oracle_dqn`` with the dueling net; returns (online parameters, number of updates)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _oracle_dqn_dueling(cfg, epochs, dtype)
    finally:
        torch.set_num_threads(threads)


def _oracle_dqn_dueling(cfg, epochs, dtype):
    e = ro.CartPole
    assert cfg.env == e.name and cfg.dueling and not cfg.prioritized and cfg.n_step == 1
    N, T, C, H, B = cfg.num_envs, cfg.rollout_len, cfg.buffer_slots, cfg.hidden, cfg.batch_size
    env_seed, sample_seed, _ = dqn_seeds(cfg.seed)
    online = MLPSpec(e.D, H, e.A + 1).init(torch.Generator().manual_seed(int(cfg.seed))).to(dtype)
    target = online.clone()
    m, v = torch.zeros_like(online), torch.zeros_like(online)
    ring = ReplayRing.allocate(C, N, e.D, "cpu")
    envs = np.arange(N)
    s = e.reset(e.reset_uniforms(env_seed, 0, envs)).astype(np.float32)
    ln = np.zeros(N, np.int64)
    cursor = written = updates = 0
    for epoch in range(epochs):
        eps = epsilon_at(cfg, epoch)
        for t in range(T):
            g = epoch * T + t
            obs = e.obs(s).astype(np.float32)
            out, _ = ref.trunk(online, torch.from_numpy(obs).to(dtype), e.D, H, e.A + 1)
            explore, a_rand, noise = do.explore_draws(env_seed, g, envs, eps, e.A)
            a = np.where(explore, a_rand, ref.greedy_from_logits(out[:, :e.A])[0].numpy())
            ns, r, term, _ = e.step(s, a, noise, np.float32)
            ns = ns.astype(np.float32)
            ln += 1
            done = np.where(term, 1, np.where(ln >= e.max_steps, 2, 0))
            k = cursor + t
            ring.obs[k], ring.nobs[k] = torch.from_numpy(obs), torch.from_numpy(e.obs(ns).astype(np.float32))
            ring.act[k], ring.rew[k] = torch.from_numpy(a.astype(np.int32)), torch.from_numpy(r.astype(np.float32))
            ring.done[k] = torch.from_numpy(done.astype(np.float32))
            rs = e.reset(e.done_reset_uniforms(env_seed, g, envs)).astype(np.float32)
            s = np.where((done > 0)[:, None], rs, ns)
            ln[done > 0] = 0
        cursor = (cursor + T) % C
        written += T
        if written * N < cfg.learning_starts:
            continue
        for _ in range(cfg.updates_per_epoch):
            Xb, act_b, y, _ = dqn_targets_ref(online, target, H, e.A, ring, min(written, C) * N, cfg.gamma, cfg.double_q,
                                              sample_seed, updates, B, dtype, dueling=True)
            grad, _ = ref.mlp_grad_ref(ref.HEAD_Q_DUEL, online, Xb, e.A, H, act=act_b, ret=y, clip_eps=cfg.huber_delta,
                                       dtype=dtype)
            updates += 1
            ref.adam_ref(online, m, v, grad, updates, cfg.q_lr)
            if updates % cfg.target_update_every == 0:
                target.copy_(online)
    return online, updates
