"""CPU oracle of the DQN trainer (relayrl_prototype_amd/runtime/dqn_trainer.py): the same algorithm
in pure torch (float64 networks, autograd, Adam) on the float32 CartPole oracle of rollout_oracle.py.

It draws what the device draws: Philox resets and env noise, the explore flag and the random action
of every (env, global step), the replay rows of every (batch row, update), and it starts from the
trainer's seeded weights.  Only the arithmetic differs (float64 networks against fp32 MFMA), so its
greedy return after K updates is the yardstick of the GPU learning test.
"""
import numpy as np
import torch

from relayrl_prototype_amd.ops import MLPSpec, ReplayRing, dqn_targets_ref, philox
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, dqn_seeds, epsilon_at

import rollout_oracle as ro

# The small shape of the learning tests: 64 envs x 4 steps per epoch, a ring of 8192 transitions.
SMALL = dict(env="CartPole-v1", num_envs=64, rollout_len=4, hidden=64, buffer_slots=128, batch_size=128,
             updates_per_epoch=2, gamma=0.9, q_lr=1e-3, eps_start=1.0, eps_end=0.05, eps_decay_epochs=200,
             learning_starts=1024, target_update_every=50, double_q=True, huber_delta=1.0)
SMALL_EPOCHS = 600
EVAL_EPISODES = 256
# Greedy mean return over EVAL_EPISODES episodes after SMALL_EPOCHS epochs (1194 updates), seeds 1..5,
# measured with oracle_dqn below (single-threaded torch, float64); a random policy scores about 22.
ORACLE_RETURNS = {1: 146.29, 2: 110.66, 3: 96.61, 4: 135.32, 5: 159.39}


def explore_draws(env_seed, gstep, envs, epsilon, A):
    """(explore flag, random action, env noise) of global step ``gstep``, as dqn.hip computes them."""
    u = philox.uniforms(env_seed, gstep, envs, 0)
    explore = u[2] < np.float32(epsilon)
    a_rand = np.minimum(A - 1, np.floor(u[3] * np.float32(A)).astype(np.int64))
    return explore, a_rand, u[1]


def q_gap_tolerance(params, obs, A, H):
    """(float64 greedy action, gap of the two largest float64 Q-values, tol) at ``obs`` [n, D]: tol is 4x the
    largest fp32-vs-float64 Q difference of the CPU reference on these very inputs."""
    x = torch.from_numpy(np.ascontiguousarray(obs))
    q64 = ref.trunk(params.double(), x.double(), x.shape[1], H, A)[0]
    q32 = ref.mlp_forward_ref(3, params, x, A, H)["logits"]
    tol = 4.0 * float((q32.double() - q64).abs().max())
    act, gap = ref.greedy_from_logits(q64)
    return act.numpy(), gap.numpy(), tol


def greedy_return(params, H, seed, episodes=EVAL_EPISODES, dtype=torch.float64):
    """Mean return of ``episodes`` greedy CartPole episodes (one per env, fresh Philox resets)."""
    e = ro.CartPole
    envs = np.arange(episodes)
    s = e.reset(e.reset_uniforms(seed, 0, envs)).astype(np.float32)
    ret = np.zeros(episodes)
    alive = np.ones(episodes, bool)
    for t in range(e.max_steps):
        q, _ = ref.trunk(params.to(dtype), torch.from_numpy(e.obs(s)).to(dtype), e.D, H, e.A)
        a = ref.greedy_from_logits(q)[0].numpy()
        ns, r, term, _ = e.step(s, a, e.step_noise(seed, t, envs), np.float32)
        ret += np.where(alive, r, 0.0)
        alive &= ~term
        s = ns.astype(np.float32)
        if not alive.any():
            break
    return float(ret.mean())


def oracle_dqn(cfg: DQNConfig, epochs: int, dtype=torch.float64):
    """Train for ``epochs`` epochs; returns (online parameters, number of updates).  Runs torch
    single-threaded: the matrices are tiny, and more threads only slow them down."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _oracle_dqn(cfg, epochs, dtype)
    finally:
        torch.set_num_threads(threads)


def _oracle_dqn(cfg, epochs, dtype):
    e = ro.CartPole
    assert cfg.env == e.name
    N, T, C, H, B = cfg.num_envs, cfg.rollout_len, cfg.buffer_slots, cfg.hidden, cfg.batch_size
    env_seed, sample_seed, _ = dqn_seeds(cfg.seed)
    online = MLPSpec(e.D, H, e.A).init(torch.Generator().manual_seed(int(cfg.seed))).to(dtype)
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
            q, _ = ref.trunk(online, torch.from_numpy(obs).to(dtype), e.D, H, e.A)
            explore, a_rand, noise = explore_draws(env_seed, g, envs, eps, e.A)
            a = np.where(explore, a_rand, ref.greedy_from_logits(q)[0].numpy())
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
                                              sample_seed, updates, B, dtype)
            grad, _ = ref.mlp_grad_ref(ref.HEAD_Q_TD, online, Xb, e.A, H, act=act_b, ret=y, clip_eps=cfg.huber_delta,
                                       dtype=dtype)
            updates += 1
            ref.adam_ref(online, m, v, grad, updates, cfg.q_lr)
            if updates % cfg.target_update_every == 0:
                target.copy_(online)
    return online, updates
