"""CPU oracle of the DQN trainer with n-step returns: the loop of tests/dqn_oracle.py (float64 networks,
autograd, Adam, the device's Philox draws on the float32 CartPole oracle) with ``n_step`` and ``newest``, the
slot the rollout wrote last, passed to ``dqn_targets_ref``.  With ``n_step = 1`` it is that loop bit for bit
(tests/test_dqn_nstep.py holds it to that).
"""
import numpy as np
import torch

from relayrl_prototype_amd.ops import MLPSpec, ReplayRing, dqn_targets_ref
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, dqn_seeds, epsilon_at

import dqn_oracle as do
import rollout_oracle as ro

# Greedy mean return over dqn_oracle.EVAL_EPISODES episodes after dqn_oracle.SMALL_EPOCHS epochs (1194 updates)
# at dqn_oracle.SMALL with n_step = 3, seeds 1..5, measured with oracle_dqn_nstep below (single-threaded torch,
# float64); a random policy scores about 22.  Seed 1 has not left that level after 1194 updates: at this shape
# the return of a single seed swings widely (see tests/per_oracle.py), with three-step returns as without.
ORACLE_RETURNS_N3 = {1: 26.09, 2: 187.66, 3: 128.86, 4: 81.32, 5: 260.52}


def oracle_dqn_nstep(cfg: DQNConfig, epochs: int, dtype=torch.float64):
    """Train for ``epochs`` epochs; returns (online parameters, number of updates)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _oracle_dqn_nstep(cfg, epochs, dtype)
    finally:
        torch.set_num_threads(threads)


def _oracle_dqn_nstep(cfg, epochs, dtype):
    e = ro.CartPole
    assert cfg.env == e.name and not cfg.prioritized
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
            explore, a_rand, noise = do.explore_draws(env_seed, g, envs, eps, e.A)
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
            Xb, act_b, y = dqn_targets_ref(online, target, H, e.A, ring, min(written, C) * N, cfg.gamma, cfg.double_q,
                                           sample_seed, updates, B, dtype, n_step=cfg.n_step,
                                           newest=(cursor - 1) % C)[:3]
            grad, _ = ref.mlp_grad_ref(ref.HEAD_Q_TD, online, Xb, e.A, H, act=act_b, ret=y, clip_eps=cfg.huber_delta,
                                       dtype=dtype)
            updates += 1
            ref.adam_ref(online, m, v, grad, updates, cfg.q_lr)
            if updates % cfg.target_update_every == 0:
                target.copy_(online)
    return online, updates
