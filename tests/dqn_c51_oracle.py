"""Host oracles of the categorical (C51) head's tests: the textbook l / u projection of Bellemare et al. 2017 and the
bounds the GPU tests hold the kernels to, which come from the fp32 oracle's own error against float64."""
import numpy as np
import torch

from relayrl_prototype_amd.ops import MLPSpec, ReplayRing, dqn_targets_ref
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, dqn_seeds, epsilon_at

import dqn_oracle as do
import rollout_oracle as ro

BOUND_FACTOR = 4.0  # the project's multiple of the fp32 oracle's maximum error (tests/test_dqn_gpu.py: the greedy gap)


def project_textbook(p, G, c, v_min, v_max):
    """Algorithm 1 of the paper in float64 numpy: b_j = (clip(G + c z_j) - v_min) / dz, l = floor b_j, u = ceil b_j,
    m_l += p_j (u - b_j), m_u += p_j (b_j - l).  Where b_j is an integer (l == u) both weights are 0 and the mass is
    DROPPED: the reason the kernels use the gather form."""
    p = np.asarray(p, np.float64)
    B, NA = p.shape
    dz = (v_max - v_min) / (NA - 1)
    z = v_min + dz * np.arange(NA)
    b = (np.clip(np.asarray(G)[:, None] + np.asarray(c)[:, None] * z[None, :], v_min, v_max) - v_min) / dz
    lo, up = np.floor(b).astype(int), np.ceil(b).astype(int)
    m = np.zeros_like(p)
    for j in range(NA):
        np.add.at(m, (np.arange(B), lo[:, j]), p[:, j] * (up[:, j] - b[:, j]))
        np.add.at(m, (np.arange(B), up[:, j]), p[:, j] * (b[:, j] - lo[:, j]))
    return m, b


def q_both(params, obs, A, NA, H, v_min, v_max):
    """(Q float64 [n, A], bound): the expectations at ``obs`` and BOUND_FACTOR times the fp32 oracle's largest error."""
    D = obs.shape[-1]
    x = torch.as_tensor(obs).reshape(-1, D)
    q64 = ref.c51_q(ref.trunk(params.double(), x.double(), D, H, A * NA)[0], A, NA, v_min, v_max)[0]
    q32 = ref.c51_q(ref.trunk(params.float(), x.float(), D, H, A * NA)[0], A, NA, v_min, v_max)[0]
    return q64, BOUND_FACTOR * float((q32.double() - q64).abs().max())


# ---------------------------------------------------------------- the CPU oracle loop of the learning test
# dqn_oracle.SMALL plus 51 atoms on [0, 10]: rewards of 1 at gamma 0.9, so returns lie in [0, 10).
C51_SMALL = dict(atoms=51, v_min=0.0, v_max=10.0)
# Greedy mean return over do.EVAL_EPISODES episodes after do.SMALL_EPOCHS = 600 epochs (1194 updates), seeds 1..5,
# measured with oracle_dqn_c51 below (single-threaded torch, float64 networks) and greedy_return_c51 on the evaluation
# key dqn_seeds(seed)[2]; a random policy scores about 22.
C51_UPDATES = 1194
ORACLE_RETURNS_C51 = {1: 135.41, 2: 414.51, 3: 323.61, 4: 203.82, 5: 278.71}


def forward64(params, X, D, H, outputs):
    """The MLP in float64, written out on the unflattened net."""
    W1, b1, W2, b2, W3, b3, _ = ref.unflatten(params.double(), D, H, outputs)
    return torch.relu(torch.relu(X.double() @ W1.t() + b1) @ W2.t() + b2) @ W3.t() + b3


def expectations(out, A, NA, v_min, v_max):
    """[n, A * NA] logits -> Q [n, A] = sum_i z_i softmax(block a)_i, in plain float64 tensor algebra."""
    z = v_min + (v_max - v_min) / (NA - 1) * torch.arange(NA, dtype=torch.float64)
    return (torch.softmax(out.double().reshape(-1, A, NA), -1) * z).sum(-1)


def greedy_return_c51(params, H, NA, v_min, v_max, seed, episodes=do.EVAL_EPISODES):
    """``dqn_oracle.greedy_return`` for a categorical net: the action is the argmax of the expectations."""
    e = ro.CartPole
    envs = np.arange(episodes)
    s = e.reset(e.reset_uniforms(seed, 0, envs)).astype(np.float32)
    ret, alive = np.zeros(episodes), np.ones(episodes, bool)
    for t in range(e.max_steps):
        q = expectations(forward64(params, torch.from_numpy(e.obs(s)), e.D, H, e.A * NA), e.A, NA, v_min, v_max)
        ns, r, term, _ = e.step(s, ref.greedy_from_logits(q)[0].numpy(), e.step_noise(seed, t, envs), np.float32)
        ret += np.where(alive, r, 0.0)
        alive &= ~term
        s = ns.astype(np.float32)
        if not alive.any():
            break
    return float(ret.mean())


def oracle_dqn_c51(cfg: DQNConfig, epochs: int, dtype=torch.float64):
    """``dqn_oracle.oracle_dqn`` with the categorical net (the same algorithm and Philox draws as the GPU trainer,
    uniform one-step replay); returns (online parameters, number of updates)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _oracle_dqn_c51(cfg, epochs, dtype)
    finally:
        torch.set_num_threads(threads)


def _oracle_dqn_c51(cfg, epochs, dtype):
    e = ro.CartPole
    NA, sup = int(cfg.atoms), dict(atoms=int(cfg.atoms), v_min=cfg.v_min, v_max=cfg.v_max)
    assert cfg.env == e.name and NA >= 2 and not cfg.prioritized and cfg.n_step == 1
    N, T, C, H, B = cfg.num_envs, cfg.rollout_len, cfg.buffer_slots, cfg.hidden, cfg.batch_size
    env_seed, sample_seed, _ = dqn_seeds(cfg.seed)
    online = MLPSpec(e.D, H, e.A * NA).init(torch.Generator().manual_seed(int(cfg.seed))).to(dtype)
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
            out, _ = ref.trunk(online, torch.from_numpy(obs).to(dtype), e.D, H, e.A * NA)
            explore, a_rand, noise = do.explore_draws(env_seed, g, envs, eps, e.A)
            q = ref.c51_q(out, e.A, NA, cfg.v_min, cfg.v_max)[0]
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
                                              sample_seed, updates, B, dtype, **sup)
            grad, _ = ref.mlp_grad_ref(ref.HEAD_Q_C51, online, Xb, e.A, H, act=act_b, ret=y, dtype=dtype, **sup)
            updates += 1
            ref.adam_ref(online, m, v, grad, updates, cfg.q_lr)
            if updates % cfg.target_update_every == 0:
                target.copy_(online)
    return online, updates
