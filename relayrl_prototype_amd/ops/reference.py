"""Pure-PyTorch fp32 oracles of every HIP kernel.

These are the numerics ground truth for the kernel tests (tests/test_kernels_gpu.py)
and the execution path for CPU tensors.  They implement the reference's math
(REINFORCE.py:141-160, kernel.py:23-37, replay_buffer.py:48-111,
BaseReplayBuffer.py:12-53) with the documented fixes: true log_softmax log-probs,
true entropy, and an epsilon in the advantage normalisation.
"""
from __future__ import annotations

import numpy as np
import torch

from . import philox

MODE_VALUE, MODE_CAT_SAMPLE, MODE_CAT_EVAL, MODE_LOGITS, MODE_GAUSS_SAMPLE, MODE_GAUSS_EVAL = range(6)
HEAD_PG_CAT, HEAD_VALUE_MSE, HEAD_PPO_CAT, HEAD_PPO_GAUSS, HEAD_PG_GAUSS, HEAD_Q_TD, HEAD_Q_DUEL, HEAD_Q_QR = range(8)
HALF_LOG_2PI = 0.91893853320467274


def unflatten(params: torch.Tensor, D: int, H: int, A: int, gaussian: bool = False):
    o = 0

    def take(n, shape):
        nonlocal o
        t = params[o : o + n].view(*shape)
        o += n
        return t

    W1 = take(H * D, (H, D))
    b1 = take(H, (H,))
    W2 = take(H * H, (H, H))
    b2 = take(H, (H,))
    W3 = take(A * H, (A, H))
    b3 = take(A, (A,))
    log_std = take(A, (A,)) if gaussian else None
    return W1, b1, W2, b2, W3, b3, log_std


def trunk(params, X, D, H, A, gaussian=False):
    W1, b1, W2, b2, W3, b3, log_std = unflatten(params, D, H, A, gaussian)
    h1 = torch.relu(X @ W1.t() + b1)
    h2 = torch.relu(h1 @ W2.t() + b2)
    out = h2 @ W3.t() + b3
    return out, log_std


def masked_logits(logits, mask):
    if mask is None:
        return logits
    return logits + (mask - 1.0) * 1e8


def cat_sample_from_u(logits: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """Inverse-CDF draw matching rrl::cat_sample (first a with u < cdf[a] and p > 0)."""
    lse = torch.logsumexp(logits, dim=-1, keepdim=True)
    p = torch.exp(logits - lse)
    cdf = torch.cumsum(p, dim=-1)
    ok = (u.unsqueeze(-1) < cdf) & (p > 0)
    A = logits.shape[-1]
    idx = torch.arange(A, device=logits.device).expand_as(p)
    big = torch.full_like(idx, A)
    first = torch.where(ok, idx, big).min(dim=-1).values
    last_pos = torch.where(p > 0, idx, torch.full_like(idx, -1)).max(dim=-1).values
    return torch.where(first < A, first, last_pos.clamp(min=0))


@torch.no_grad()
def mlp_forward_ref(mode, params, X, A, H, mask=None, act_in=None, actc_in=None, seed=0, step=0, row_offset=0):
    B, D = X.shape
    gaussian = mode in (MODE_GAUSS_SAMPLE, MODE_GAUSS_EVAL)
    Aeff = 1 if mode == MODE_VALUE else A
    out, log_std = trunk(params.float(), X.float(), D, H, Aeff, gaussian)
    res = {}
    if mode == MODE_VALUE:
        res["v"] = out[:, 0]
        return res
    if not gaussian:
        logits = masked_logits(out, mask)
        logp_all = torch.log_softmax(logits, dim=-1)
        p = torch.exp(logp_all)
        ent = -(p * torch.where(p > 0, logp_all, torch.zeros_like(logp_all))).sum(-1)
        res["logits"] = logits
        res["entropy"] = ent
        if mode == MODE_CAT_SAMPLE:
            rows = np.arange(B, dtype=np.uint64) + np.uint64(row_offset)
            u = torch.from_numpy(philox.uniforms(seed, step, rows, 0)[0]).to(X.device)
            a = cat_sample_from_u(logits, u)
            res["act"] = a.to(torch.int32)
            res["logp"] = logp_all.gather(-1, a.long().unsqueeze(-1)).squeeze(-1)
        elif mode == MODE_CAT_EVAL:
            res["logp"] = logp_all.gather(-1, act_in.long().unsqueeze(-1)).squeeze(-1)
        return res
    mu = out
    std = torch.exp(log_std)
    if mode == MODE_GAUSS_SAMPLE:
        rows = np.arange(B, dtype=np.uint64) + np.uint64(row_offset)
        zs = []
        for a in range(A):
            u = philox.uniforms(seed, step, rows, 16 + (a & ~1))
            u1 = np.maximum(u[2] if a & 1 else u[0], np.float32(1e-7))
            u2 = u[3] if a & 1 else u[1]
            zs.append(np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2))
        z = torch.from_numpy(np.stack(zs, -1).astype(np.float32)).to(X.device)
        x = mu + std * z
        res["act"] = x
    else:
        x = actc_in
    zz = (x - mu) / std
    res["logp"] = (-0.5 * zz * zz - log_std - HALF_LOG_2PI).sum(-1)
    res["entropy"] = (0.5 + HALF_LOG_2PI + log_std).sum(-1).expand(B)
    res["mean"] = mu
    return res


def greedy_from_logits(logits: torch.Tensor):
    """(argmax action, gap between the two largest logits).  A tie takes the lowest index, like
    rrl::argmax_first, and has gap 0; one action alone has an infinite gap."""
    top = logits.max(dim=-1, keepdim=True).values
    A = logits.shape[-1]
    idx = torch.arange(A, device=logits.device).expand_as(logits)
    act = torch.where(logits == top, idx, torch.full_like(idx, A)).min(dim=-1).values
    if A == 1:
        return act, torch.full(logits.shape[:-1], float("inf"), dtype=logits.dtype, device=logits.device)
    two = torch.topk(logits, 2, dim=-1).values
    return act, two[..., 0] - two[..., 1]


def dueling_q(out: torch.Tensor, A: int) -> torch.Tensor:
    """The dueling combine of ``out`` [..., A + 1] (columns 0 .. A-1 the advantages, column A the state
    value) -> Q [..., A], in the kernels' operation order (rrl::dueling_q), in ``out``'s dtype:

        s = out[0]; s += out[k] for k = 1 .. A-1 (ascending, one add each);  m = s / A
        Q(a) = (out[A] - m) + out[a]

    The greedy action of a dueling net is the argmax of the ADVANTAGES ``out[..., :A]``, not of Q."""
    A = int(A)
    if out.shape[-1] != A + 1:
        raise ValueError(f"a dueling net over {A} actions has {A + 1} outputs, got {out.shape[-1]}")
    s = out[..., 0]
    for k in range(1, A):
        s = s + out[..., k]
    m = s / torch.tensor(float(A), dtype=out.dtype, device=out.device)
    return (out[..., A] - m).unsqueeze(-1) + out[..., :A]


def quantile_q(out: torch.Tensor, A: int, NQ: int) -> torch.Tensor:
    """The per-action quantile sums of ``out`` [..., A * NQ] (column ``a * NQ + i`` is quantile ``i`` of action
    ``a``) -> s [..., A], in the kernels' operation order (rrl::quantile_argmax), in ``out``'s dtype:

        s_a = out[a * NQ]; s_a += out[a * NQ + i] for i = 1 .. NQ-1 (ascending, one add each)

    There is no division: the greedy action of a quantile net is the argmax of these sums, and the Q-value the
    metrics report is ``s_a / NQ``."""
    A, NQ = int(A), int(NQ)
    if NQ < 1 or out.shape[-1] != A * NQ:
        raise ValueError(f"a quantile net over {A} actions with {NQ} quantiles has {A * NQ} outputs, "
                         f"got {out.shape[-1]}")
    th = out.reshape(*out.shape[:-1], A, NQ)
    s = th[..., 0]
    for i in range(1, NQ):
        s = s + th[..., i]
    return s


@torch.no_grad()
def greedy_actions_ref(params, obs, A, H, dtype=torch.float64):
    """The greedy action of the categorical policy at ``obs`` [..., D] and the gap between its two
    largest logits, computed in ``dtype``: what evaluate.hip's ``greedy = 1`` is held to wherever the
    gap exceeds the kernel's logit error."""
    D = obs.shape[-1]
    logits, _ = trunk(params.to(dtype), obs.reshape(-1, D).to(dtype), D, H, A)
    act, gap = greedy_from_logits(logits)
    return act.reshape(obs.shape[:-1]), gap.reshape(obs.shape[:-1])


def normalize_adv(adv, adv_stats):
    if adv_stats is None:
        return adv
    n = torch.clamp(adv_stats[2], min=1.0)
    mean = adv_stats[0] / n
    var = torch.clamp(adv_stats[1] / n - mean * mean, min=0.0)
    return (adv - mean) / (torch.sqrt(var) + 1e-8)


def mlp_grad_ref(head, params, X, A, H, mask=None, act=None, actc=None, adv=None, ret=None, logp_old=None,
                 adv_stats=None, inv_B=None, clip_eps=0.2, ent_coef=0.0, dtype=torch.float32, row_w=None,
                 w_norm=None, quantiles=0):
    """Returns (flat gradient, stats dict) of sum_i loss_i * inv_B (+ entropy bonus);
    ``dtype=torch.float64`` gives the float64 oracle (tools/grad_fuzz_probe.py).
    ``HEAD_Q_TD``: loss_i = huber(Q(x_i)[act_i] - ret_i, delta) with delta = ``clip_eps``, times
    ``row_w[i] / w_norm`` where the weights of prioritised replay are given; ``stats["td_abs"]`` is
    |Q - ret| per row.  ``HEAD_Q_DUEL`` is the same loss on a dueling net: ``A`` stays the number of
    actions, ``params`` has ``A + 1`` outputs and Q is ``dueling_q`` of them.
    ``HEAD_Q_QR`` (``quantiles`` = NQ >= 1): ``params`` has ``A * NQ`` outputs, ``ret`` is [B, NQ] and with
    theta_i = out[act * NQ + i], tau_i = (2 i + 1) / (2 NQ), u_ij = ret_j - theta_i, kappa = ``clip_eps`` > 0
    loss_i = rho = (1 / NQ) sum_i sum_j |tau_i - [u_ij < 0]| huber_kappa(u_ij) / kappa, times the weight;
    ``stats["td_abs"]`` is the UNWEIGHTED rho per row and ``stats["v"]`` sums ``quantile_q(out)[act] / NQ``."""
    B, D = X.shape
    gaussian = head in (HEAD_PPO_GAUSS, HEAD_PG_GAUSS)
    NQ = int(quantiles)
    if (head == HEAD_Q_QR) != (NQ > 0) or NQ < 0:
        raise ValueError(f"quantiles ({NQ}) goes with HEAD_Q_QR, where it is >= 1")
    if head == HEAD_Q_QR and not 1 <= int(A) * NQ <= 16:
        raise ValueError(f"a quantile net has A * quantiles <= 16 outputs, got {A} * {NQ}")
    if head == HEAD_Q_QR and not clip_eps > 0:
        raise ValueError(f"the quantile head needs a Huber threshold (clip_eps / huber_delta) > 0, got {clip_eps}")
    Aeff = 1 if head == HEAD_VALUE_MSE else A + 1 if head == HEAD_Q_DUEL else A * NQ if head == HEAD_Q_QR else A
    if inv_B is None:
        inv_B = 1.0 / max(B, 1)
    p = params.detach().to(dtype).clone().requires_grad_(True)
    out, log_std = trunk(p, X.to(dtype), D, H, Aeff, gaussian)
    stats = {}
    if head == HEAD_VALUE_MSE:
        v = out[:, 0]
        li = (v - ret) ** 2
        loss = li.sum() * inv_B
        stats.update(loss=li.sum().item(), v=v.sum().item(), count=B)
    elif head == HEAD_Q_QR:
        idx = act.long().reshape(B, 1, 1).expand(B, 1, NQ)
        theta = out.reshape(B, A, NQ).gather(1, idx).squeeze(1)            # [B, NQ]
        u = ret.to(dtype).reshape(B, 1, NQ) - theta.unsqueeze(-1)          # [B, i, j]
        tau = ((2 * torch.arange(NQ, dtype=dtype, device=out.device) + 1) / (2 * NQ)).reshape(1, NQ, 1)
        au = u.abs()
        hub = torch.where(au <= clip_eps, 0.5 * u * u, clip_eps * (au - 0.5 * clip_eps))
        rho = ((tau - (u.detach() < 0).to(dtype)).abs() * hub / clip_eps).sum((1, 2)) / NQ
        li = rho
        if row_w is not None:
            li = (row_w.to(dtype) / torch.as_tensor(w_norm).to(dtype).reshape(-1)[0]) * rho
        loss = li.sum() * inv_B
        s_act = quantile_q(out, A, NQ).gather(-1, act.long().unsqueeze(-1)).squeeze(-1)
        stats.update(loss=li.sum().item(), v=(s_act / NQ).sum().item(), count=B, td_abs=rho.detach())
    elif head in (HEAD_Q_TD, HEAD_Q_DUEL):
        qs = dueling_q(out, A) if head == HEAD_Q_DUEL else out
        q = qs.gather(-1, act.long().unsqueeze(-1)).squeeze(-1)
        diff = q - ret.to(dtype)
        ad = diff.abs()
        li = torch.where(ad <= clip_eps, 0.5 * diff * diff, clip_eps * (ad - 0.5 * clip_eps))
        if row_w is not None:
            li = (row_w.to(dtype) / torch.as_tensor(w_norm).to(dtype).reshape(-1)[0]) * li
        loss = li.sum() * inv_B
        stats.update(loss=li.sum().item(), v=q.sum().item(), count=B, td_abs=ad.detach())
    else:
        advn = normalize_adv(adv.to(dtype), None if adv_stats is None else adv_stats.to(dtype))
        if not gaussian:
            logits = masked_logits(out, mask)
            logp_all = torch.log_softmax(logits, dim=-1)
            logp = logp_all.gather(-1, act.long().unsqueeze(-1)).squeeze(-1)
            pr = torch.exp(logp_all)
            ent = -(pr * torch.where(pr > 0, logp_all, torch.zeros_like(logp_all))).sum(-1)
        else:
            std = torch.exp(log_std)
            zz = (actc - out) / std
            logp = (-0.5 * zz * zz - log_std - HALF_LOG_2PI).sum(-1)
            ent = (0.5 + HALF_LOG_2PI + log_std).sum(-1).expand(B)
        if head in (HEAD_PG_CAT, HEAD_PG_GAUSS):
            li = -logp * advn
        else:
            ratio = torch.exp(logp - logp_old)
            s1 = ratio * advn
            s2 = torch.clamp(ratio, 1 - clip_eps, 1 + clip_eps) * advn
            li = -torch.minimum(s1, s2)
            stats["clipfrac"] = ((ratio - 1).abs() > clip_eps).float().sum().item()
        loss = li.sum() * inv_B - ent_coef * ent.sum() * inv_B
        stats.update(loss=li.sum().item(), entropy=ent.sum().item(), count=B)
        if logp_old is not None:
            stats["kl"] = (logp_old - logp).sum().item()
    loss.backward()
    return p.grad.detach(), stats


def discount_cumsum(x: np.ndarray, discount: float) -> np.ndarray:
    """scipy-free equivalent of BaseReplayBuffer.discount_cumsum (lfilter reversed)."""
    out = np.zeros_like(x, dtype=np.float64)
    run = 0.0
    for t in range(len(x) - 1, -1, -1):
        run = x[t] + discount * run
        out[t] = run
    return out


@torch.no_grad()
def gae_scan_tm_ref(rew, done, val, gamma, lam, tval=None):
    """done codes: 0 running, 1 terminal, 2 time-limit truncation (bootstrap tval[t]).

    [K, T, N] inputs (K actor blocks) with flat ``val`` [K*T*N + K*N] are scanned as one
    [T, K*N] problem (column k*N + n)."""
    if rew.dim() == 3:
        K, T, N = rew.shape
        tm = lambda x: x.reshape(K, T, N).permute(1, 0, 2).reshape(T, K * N)  # noqa: E731
        v = None
        if val is not None:
            vf = val.reshape(-1)
            v = torch.cat([tm(vf[:K * T * N]), vf[K * T * N:K * T * N + K * N].reshape(1, K * N)])
        a, r, s = gae_scan_tm_ref(tm(rew), tm(done), v, gamma, lam, None if tval is None else tm(tval))
        back = lambda x: x.reshape(T, K, N).permute(1, 0, 2).contiguous()  # noqa: E731
        return back(a), back(r), s
    T, N = rew.shape
    if val is not None:
        val = val.reshape(T + 1, N)
    adv = torch.zeros_like(rew)
    ret = torch.zeros_like(rew)
    if val is not None:
        v_next = val[T].clone()
        adv_next = torch.zeros(N, dtype=rew.dtype, device=rew.device)
        ret_next = v_next.clone()
        for t in range(T - 1, -1, -1):
            nd = (done[t] == 0).to(rew.dtype)
            vb = torch.where(done[t] > 1.5, tval[t], torch.zeros_like(rew[t])) if tval is not None \
                else torch.zeros_like(rew[t])
            delta = rew[t] + gamma * (v_next * nd + vb) - val[t]
            adv[t] = delta + gamma * lam * nd * adv_next
            ret[t] = rew[t] + gamma * (nd * ret_next + vb)
            adv_next, ret_next, v_next = adv[t], ret[t], val[t]
    else:
        adv_next = torch.zeros(N, dtype=rew.dtype, device=rew.device)
        ret_next = torch.zeros(N, dtype=rew.dtype, device=rew.device)
        for t in range(T - 1, -1, -1):
            nd = (done[t] == 0).to(rew.dtype)
            adv[t] = rew[t] + gamma * lam * nd * adv_next
            ret[t] = rew[t] + gamma * nd * ret_next
            adv_next, ret_next = adv[t], ret[t]
    stats = torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(T * N), device=rew.device)])
    return adv, ret, stats


@torch.no_grad()
def vtrace_scan_tm_ref(rew, done, val, logp_mu, logp_pi, gamma, lam, rho_bar, c_bar, pg_rho_bar, tval=None):
    """V-trace (Espeholt et al. 2018) on the layout and done codes of ``gae_scan_tm_ref`` ->
    (adv, ret, stats[3], is_stats[2]), computed in the dtype of the inputs.

    ``ret`` is the V-trace target v_t, ``adv`` the policy-gradient advantage
    min(pg_rho_bar, ratio) * (r_t + gamma * v_{t+1} - V_t); ``is_stats`` = (sum min(rho_bar, ratio),
    sum |logp_pi - logp_mu|).  On-policy with thresholds >= 1, ``ret`` = V + GAE(lam)."""
    if rew.dim() == 3:
        K, T, N = rew.shape
        tm = lambda x: x.reshape(K, T, N).permute(1, 0, 2).reshape(T, K * N)  # noqa: E731
        vf = val.reshape(-1)
        v = torch.cat([tm(vf[:K * T * N]), vf[K * T * N:K * T * N + K * N].reshape(1, K * N)])
        a, r, s, i = vtrace_scan_tm_ref(tm(rew), tm(done), v, tm(logp_mu), tm(logp_pi), gamma, lam, rho_bar, c_bar,
                                        pg_rho_bar, None if tval is None else tm(tval))
        back = lambda x: x.reshape(T, K, N).permute(1, 0, 2).contiguous()  # noqa: E731
        return back(a), back(r), s, i
    T, N = rew.shape
    val = val.reshape(T + 1, N)
    adv = torch.zeros_like(rew)
    ret = torch.zeros_like(rew)
    zero = torch.zeros(N, dtype=rew.dtype, device=rew.device)
    acc = zero.clone()
    v_prev = val[T].clone()
    log_ratio = logp_pi - logp_mu
    ratio = torch.exp(log_ratio)
    rho = torch.clamp(ratio, max=rho_bar)
    c = lam * torch.clamp(ratio, max=c_bar)
    rho_pg = torch.clamp(ratio, max=pg_rho_bar)
    for t in range(T - 1, -1, -1):
        nd = (done[t] == 0).to(rew.dtype)
        vb = torch.where(done[t] > 1.5, tval[t], zero) if tval is not None else zero
        v_next = nd * v_prev + vb
        adv[t] = rho_pg[t] * (rew[t] + gamma * (v_next + nd * acc) - val[t])
        acc = rho[t] * (rew[t] + gamma * v_next - val[t]) + gamma * c[t] * nd * acc
        ret[t] = val[t] + acc
        v_prev = val[t]
    stats = torch.stack([adv.sum(), (adv * adv).sum(), torch.tensor(float(T * N), dtype=rew.dtype, device=rew.device)])
    is_stats = torch.stack([rho.sum(), log_ratio.abs().sum()])
    return adv, ret, stats, is_stats


@torch.no_grad()
def scan_flat_ref(rew, done, val, boot, gamma, lam):
    """Per-path finish_path semantics over a flat buffer (replay_buffer.py:48-79)."""
    r = rew.detach().cpu().double().numpy()
    d = done.detach().cpu().numpy() > 0
    v = None if val is None else val.detach().cpu().double().numpy()
    b = None if boot is None else boot.detach().cpu().double().numpy()
    L = len(r)
    adv = np.zeros(L)
    ret = np.zeros(L)
    start = 0
    for t in range(L):
        if d[t] or t == L - 1:
            sl = slice(start, t + 1)
            last = float(b[t]) if (b is not None and d[t]) else 0.0
            if v is not None:
                rr = np.append(r[sl], last)
                vv = np.append(v[sl], last)
                deltas = rr[:-1] + gamma * vv[1:] - vv[:-1]
                adv[sl] = discount_cumsum(deltas, gamma * lam)
                ret[sl] = discount_cumsum(rr, gamma)[:-1]
            else:
                adv[sl] = discount_cumsum(r[sl], gamma * lam)
                ret[sl] = discount_cumsum(r[sl], gamma)
            start = t + 1
    a = torch.from_numpy(adv.astype(np.float32)).to(rew.device)
    rt = torch.from_numpy(ret.astype(np.float32)).to(rew.device)
    stats = torch.tensor([adv.sum(), (adv * adv).sum(), float(L)], dtype=torch.float32, device=rew.device)
    return a, rt, stats


@torch.no_grad()
def adam_ref(param, m, v, grad, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """In-place torch.optim.Adam math on flat tensors; `step` is the new step count."""
    g = grad
    if weight_decay:
        g = g + weight_decay * param
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1**step
    bc2 = 1 - beta2**step
    denom = (v.sqrt() / (bc2**0.5)).add_(eps)
    param.addcdiv_(m, denom, value=-lr / bc1)


# ---------------------------------------------------------------------- rollout integrity
STATUS_CHECKSUM, STATUS_SEQ, STATUS_VERSION = 1, 2, 4


def _words(t) -> np.ndarray:
    """The 32-bit words of a tensor's storage order (element size a multiple of 4 bytes)."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(t)
    if a.dtype.itemsize % 4:
        raise ValueError(f"payload_checksum: dtype {a.dtype} is not a multiple of 4 bytes wide")
    return a.reshape(-1).view(np.uint32)


def payload_checksum_ref(segments) -> torch.Tensor:
    """int64[2] holding the bits of (s1, s2) mod 2^64 over the concatenated 32-bit words
    w_0 .. w_{n-1} of ``segments``: s1 = sum w_i, s2 = sum (i + 1) w_i (checksum.hip).
    numpy uint64 arithmetic wraps modulo 2^64 by definition."""
    s1 = np.uint64(0)
    s2 = np.uint64(0)
    base = 0
    with np.errstate(over="ignore"):
        for seg in segments:
            w = _words(seg).astype(np.uint64)
            idx = np.arange(base + 1, base + 1 + w.size, dtype=np.uint64)
            s1 = s1 + w.sum(dtype=np.uint64)
            s2 = s2 + (idx * w).sum(dtype=np.uint64)
            base += w.size
    return torch.from_numpy(np.array([s1, s2], dtype=np.uint64).view(np.int64).copy())


def payload_verify_ref(sums, hdr, ck_col, expected_seq, lo, hi) -> torch.Tensor:
    """int32[K] status: bit 0 sums != header columns ck_col, ck_col + 1 (raw 64-bit integers),
    bit 1 header seq (column 0) != expected_seq, bit 2 header version (column 7) outside [lo, hi]."""
    h = hdr.detach().cpu().contiguous().numpy()
    s = sums.detach().cpu().contiguous().numpy().reshape(-1, 2).view(np.uint64)
    got = np.ascontiguousarray(h[:, ck_col:ck_col + 2]).view(np.uint64)
    st = np.zeros(h.shape[0], dtype=np.int32)
    st |= np.where((got != s).any(axis=1), STATUS_CHECKSUM, 0).astype(np.int32)
    st |= np.where(h[:, 0] == float(expected_seq), 0, STATUS_SEQ).astype(np.int32)
    st |= np.where((h[:, 7] >= float(lo)) & (h[:, 7] <= float(hi)), 0, STATUS_VERSION).astype(np.int32)
    return torch.from_numpy(st)
