"""Host oracles of the quantile-regression head (tests/test_dqn_quantile.py, tests/test_dqn_quantile_gpu.py), in
float64 and written out in loops and plain tensor algebra: they share no code with ``reference.quantile_q``,
``mlp_grad_ref(HEAD_Q_QR)`` or ``dqn_targets_ref(quantiles=)``, which they check.

* ``quantile_sums``: the per-action sums of a net of A * NQ outputs (action-major).
* ``qr_loss_rows``: the quantile-Huber loss of every row, differentiable, written as the double sum it is.
* ``qr_targets_loop``: the [B, NQ] targets, one batch row at a time.
* ``sum_gap_tolerance``: ``dqn_oracle.q_gap_tolerance``'s rule on the SUMS.
* ``oracle_dqn_quantile``: the CPU oracle loop of tests/dqn_oracle.py with the quantile net; its greedy returns
  are the yardstick of the GPU learning test.
"""
import numpy as np
import torch

from relayrl_prototype_amd.ops import MLPSpec, ReplayRing, dqn_targets_ref
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, dqn_seeds, epsilon_at

import dqn_oracle as do
import rollout_oracle as ro

# Greedy mean return over do.EVAL_EPISODES episodes at do.SMALL plus quantiles=8, seeds 1..5, after
# do.SMALL_EPOCHS = 600 epochs (1194 updates), measured with oracle_dqn_quantile below (single-threaded torch,
# float64 networks) and greedy_return_quantile on the evaluation key dqn_seeds(seed)[2]; a random policy scores
# about 22.
QR_EPOCHS = do.SMALL_EPOCHS
QR_UPDATES = 1194
ORACLE_RETURNS_QR = {1: 138.80, 2: 98.72, 3: 116.81, 4: 238.18, 5: 111.84}


def forward64(params, X, D, H, outputs):
    """The MLP in float64, written out on the unflattened net."""
    W1, b1, W2, b2, W3, b3, _ = ref.unflatten(params.double(), D, H, outputs)
    h2 = torch.relu(torch.relu(X.double() @ W1.t() + b1) @ W2.t() + b2)
    return h2 @ W3.t() + b3


def quantile_sums(out, A, NQ):
    """[n, A * NQ] -> [n, A]: column a is the sum of outputs a * NQ .. a * NQ + NQ - 1."""
    s = torch.zeros(out.shape[0], A, dtype=out.dtype)
    for a in range(A):
        for i in range(NQ):
            s[:, a] = s[:, a] + out[:, a * NQ + i]
    return s


def qr_loss_rows(out, act, T, A, NQ, kappa):
    """rho [B] of the issue: (1 / NQ) sum_i sum_j |tau_i - [u_ij < 0]| H(u_ij) / kappa, u_ij = T_j - theta_i."""
    B = out.shape[0]
    rho = []
    for b in range(B):
        a = int(act[b])
        tot = out.new_zeros(())
        for i in range(NQ):
            tau = (2 * i + 1) / (2 * NQ)
            theta = out[b, a * NQ + i]
            for j in range(NQ):
                u = T[b, j] - theta
                uv = float(u.detach())
                hub = 0.5 * u * u if abs(uv) <= kappa else kappa * (u.abs() - 0.5 * kappa)
                tot = tot + abs(tau - (1.0 if uv < 0 else 0.0)) * hub / kappa
        rho.append(tot / NQ)
    return torch.stack(rho)


def qr_targets_loop(online, target, H, A, NQ, ring, last, G, disc, double_q):
    """y [B, NQ] in float64, row by row, from the walk's results (last, G, disc as float64 arrays)."""
    D = ring.obs.shape[-1]
    nobs = ring.nobs.reshape(-1, D).double()
    done = ring.done.reshape(-1)
    y = torch.zeros(len(last), NQ, dtype=torch.float64)
    for b, r in enumerate(last):
        x = nobs[int(r)].reshape(1, D)
        out_t = forward64(target, x, D, H, A * NQ)[0]
        sel = forward64(online, x, D, H, A * NQ)[0] if double_q else out_t
        sums = [float(sum(sel[a * NQ + i] for i in range(NQ))) for a in range(A)]
        astar = max(range(A), key=lambda a: (sums[a], -a))
        boot = 0.0 if float(done[int(r)]) == 1.0 else 1.0
        for j in range(NQ):
            y[b, j] = float(G[b]) + float(disc[b]) * boot * float(out_t[astar * NQ + j])
    return y


def sum_gap_tolerance(params, obs, A, NQ, H):
    """(float64 argmax of the quantile sums, gap of the two largest float64 sums, tol) at ``obs`` [n, D]: tol is
    4x the largest fp32-vs-float64 difference of the SUMS of the CPU reference on these very inputs
    (dqn_oracle.q_gap_tolerance's rule)."""
    x = torch.from_numpy(np.ascontiguousarray(obs))
    s64 = quantile_sums(forward64(params, x, x.shape[1], H, A * NQ), A, NQ)
    o32 = ref.mlp_forward_ref(3, params, x, A * NQ, H)["logits"]
    s32 = ref.quantile_q(o32, A, NQ)
    tol = 4.0 * float((s32.double() - s64).abs().max())
    act, gap = ref.greedy_from_logits(s64)
    return act.numpy(), gap.numpy(), tol


def greedy_return_quantile(params, H, NQ, seed, episodes=do.EVAL_EPISODES):
    """``dqn_oracle.greedy_return`` for a quantile net: the action is the argmax of the quantile sums."""
    e = ro.CartPole
    envs = np.arange(episodes)
    s = e.reset(e.reset_uniforms(seed, 0, envs)).astype(np.float32)
    ret = np.zeros(episodes)
    alive = np.ones(episodes, bool)
    for t in range(e.max_steps):
        out = forward64(params, torch.from_numpy(e.obs(s)), e.D, H, e.A * NQ)
        a = ref.greedy_from_logits(quantile_sums(out, e.A, NQ))[0].numpy()
        ns, r, term, _ = e.step(s, a, e.step_noise(seed, t, envs), np.float32)
        ret += np.where(alive, r, 0.0)
        alive &= ~term
        s = ns.astype(np.float32)
        if not alive.any():
            break
    return float(ret.mean())


def oracle_dqn_quantile(cfg: DQNConfig, epochs: int, dtype=torch.float64):
    """``dqn_oracle.oracle_dqn`` with the quantile net; returns (online parameters, number of updates)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _oracle_dqn_quantile(cfg, epochs, dtype)
    finally:
        torch.set_num_threads(threads)


def _oracle_dqn_quantile(cfg, epochs, dtype):
    e = ro.CartPole
    NQ = int(cfg.quantiles)
    assert cfg.env == e.name and NQ >= 1 and not cfg.dueling and not cfg.prioritized and cfg.n_step == 1
    N, T, C, H, B = cfg.num_envs, cfg.rollout_len, cfg.buffer_slots, cfg.hidden, cfg.batch_size
    env_seed, sample_seed, _ = dqn_seeds(cfg.seed)
    online = MLPSpec(e.D, H, e.A * NQ).init(torch.Generator().manual_seed(int(cfg.seed))).to(dtype)
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
            out, _ = ref.trunk(online, torch.from_numpy(obs).to(dtype), e.D, H, e.A * NQ)
            explore, a_rand, noise = do.explore_draws(env_seed, g, envs, eps, e.A)
            a = np.where(explore, a_rand, ref.greedy_from_logits(ref.quantile_q(out, e.A, NQ))[0].numpy())
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
                                              sample_seed, updates, B, dtype, quantiles=NQ)
            grad, _ = ref.mlp_grad_ref(ref.HEAD_Q_QR, online, Xb, e.A, H, act=act_b, ret=y, clip_eps=cfg.huber_delta,
                                       dtype=dtype, quantiles=NQ)
            updates += 1
            ref.adam_ref(online, m, v, grad, updates, cfg.q_lr)
            if updates % cfg.target_update_every == 0:
                target.copy_(online)
    return online, updates
