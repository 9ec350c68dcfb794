"""DQN device ops (csrc/kernels/dqn.hip) and their host oracles.

* ``dqn_rollout``: the epsilon-greedy fused actor; T steps of N device envs into T slots of a replay
  ring.  Like ``evaluate_policy_op`` it has no PyTorch path: it needs the HIP extension and GPU tensors.
* ``dqn_targets``: sample ring rows, gather the batch and build the TD targets from the target (and,
  for double Q-learning, the online) network.  CPU tensors take ``dqn_targets_ref``.
* ``dqn_sample_rows_ref`` / ``dqn_nstep_walk_ref`` / ``dqn_targets_ref``: the oracles the kernel is held to.

``n_step > 1`` forms the n-step return at sample time: the sampled row walks forward through the ring
(same env, next slot) before the bootstrap, see ``dqn_nstep_walk_ref``.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import philox
from . import reference as ref


class ReplayRing(NamedTuple):
    """Time-major SoA replay ring of C slots x N envs; a ring row is ``slot * N + env``."""
    obs: torch.Tensor   # [C, N, D] the observation the action was computed from
    nobs: torch.Tensor  # [C, N, D] the post-step, pre-reset observation
    act: torch.Tensor   # [C, N] int32
    rew: torch.Tensor   # [C, N]
    done: torch.Tensor  # [C, N] 0 running, 1 terminal, 2 time-limit truncation

    @staticmethod
    def allocate(C: int, N: int, D: int, device) -> "ReplayRing":
        return ReplayRing(torch.zeros(C, N, D, device=device), torch.zeros(C, N, D, device=device),
                          torch.zeros(C, N, dtype=torch.int32, device=device), torch.zeros(C, N, device=device),
                          torch.zeros(C, N, device=device))


def dqn_rollout_grid(num_envs: int) -> int:
    """Rows of the ``ep_stats`` tensor ``dqn_rollout`` fills for ``num_envs`` envs."""
    from . import hip

    return int(hip().dqn_rollout_grid(int(num_envs)))


def check_quantiles(A: int, quantiles, dueling: bool = False) -> int:
    """``quantiles`` as the kernels take it -> NQ: 0 is the scalar net; NQ >= 1 a quantile net of ``A * NQ <= 16``
    outputs, which the dueling head is not built for."""
    NQ = int(quantiles)
    if NQ < 0:
        raise ValueError(f"quantiles must be >= 0, got {quantiles}")
    if NQ > 0 and dueling:
        raise ValueError("quantiles > 0 with dueling=True is not built: the two heads share 16 outputs and the "
                         "combination needs its own design; set quantiles=0 or dueling=False")
    if NQ > 0 and int(A) * NQ > 16:
        raise ValueError(f"a quantile net has A * quantiles <= 16 outputs, got A = {A} and quantiles = {NQ}")
    return NQ


def check_q_params(params, D: int, H: int, A: int, dueling: bool, name: str = "params", quantiles: int = 0):
    """A Q-network over ``A`` actions is ``MLPSpec(D, H, A)``, a dueling one ``MLPSpec(D, H, A + 1)`` (at most
    16 outputs, so ``A <= 15``), a quantile one ``MLPSpec(D, H, A * quantiles)`` (``A * quantiles <= 16``):
    ``params`` must have exactly that many floats."""
    from .mlp import MLPSpec

    NQ = check_quantiles(A, quantiles, dueling) if quantiles else 0
    if dueling and not 1 <= int(A) <= 15:
        raise ValueError(f"a dueling net has A + 1 <= 16 outputs: A must be in [1, 15], got {A}")
    if NQ > 0:
        want = MLPSpec(int(D), int(H), int(A) * NQ).P
        if params is not None and params.numel() != want:
            raise ValueError(f"{name} has {params.numel()} floats; a quantile Q-network of D = {D}, H = {H}, A = {A}, "
                             f"quantiles = {NQ} has {want}")
        return
    want = MLPSpec(int(D), int(H), int(A) + (1 if dueling else 0)).P
    if params is not None and params.numel() != want:
        raise ValueError(f"{name} has {params.numel()} floats; a {'dueling' if dueling else 'plain'} Q-network of "
                         f"D = {D}, H = {H}, A = {A} has {want} (dueling = {bool(dueling)})")


def dqn_rollout(env_id: int, params: torch.Tensor, hidden: int, rollout_len: int, slot0: int, ring: ReplayRing,
                state, ep_len, ep_ret, ep_stats, *, seed: int, step0: int, epsilon: float, reset_all: bool,
                max_steps: int, dueling: bool = False, quantiles: int = 0) -> int:
    """T = ``rollout_len`` epsilon-greedy steps of every env into ring slots ``slot0 .. slot0 + T - 1``.
    Returns 0, or the kernel's negative code (nothing written) for a launch that would wrap: unless
    ``C % T == 0``, ``slot0 % T == 0`` and ``slot0 + T <= C``.  Asynchronous on the current stream.

    ``dueling``: ``params`` is a dueling net of ``A + 1`` outputs (``reference.dueling_q``); a greedy step
    takes the lowest-index argmax of its ``A`` advantage outputs.  The draws and the ring do not change.

    ``quantiles`` = NQ >= 1: ``params`` is a quantile net of ``A * NQ`` outputs (``reference.quantile_q``); a greedy
    step takes the lowest-index argmax of the per-action quantile sums.  Again the draws and the ring do not change."""
    from . import hip

    h = hip()  # raises NativeExtensionMissing: there is no fallback
    if not params.is_cuda:
        raise ValueError("dqn_rollout runs the HIP kernel only: params must be a GPU tensor")
    if dueling or quantiles:
        D, A, _, _ = h.env_dims(int(env_id))
        check_q_params(params, D, hidden, A, bool(dueling), quantiles=quantiles)
    if quantiles:  # the quantile nets have a binding of their own: the scalar one parses what it always parsed
        return int(h.dqn_rollout_qr(int(env_id), params, int(hidden), int(rollout_len), int(slot0), state, ep_len,
                                    ep_ret, ring.obs, ring.nobs, ring.act, ring.rew, ring.done, ep_stats, int(seed),
                                    int(step0), float(epsilon), bool(reset_all), int(max_steps), bool(dueling),
                                    int(quantiles)))
    return int(h.dqn_rollout(int(env_id), params, int(hidden), int(rollout_len), int(slot0), state, ep_len, ep_ret,
                             ring.obs, ring.nobs, ring.act, ring.rew, ring.done, ep_stats, int(seed), int(step0),
                             float(epsilon), bool(reset_all), int(max_steps), bool(dueling)))


def dqn_sample_rows_ref(seed: int, update: int, B: int, filled: int) -> np.ndarray:
    """int64 [B]: the ring rows batch rows 0 .. B - 1 of update ``update`` read,
    ``(philox((b, update_lo, update_hi, 0), seed).x * filled) >> 32``."""
    if filled < 1 or filled >= 2 ** 31:
        raise ValueError(f"filled must be in [1, 2^31), got {filled}")
    b = np.arange(B, dtype=np.uint32)
    n = b.shape
    x = philox.philox4x32(b, np.full(n, update & 0xFFFFFFFF, np.uint32), np.full(n, (update >> 32) & 0xFFFFFFFF, np.uint32),
                          np.zeros(n, np.uint32), np.full(n, seed & 0xFFFFFFFF, np.uint32),
                          np.full(n, (seed >> 32) & 0xFFFFFFFF, np.uint32))[0]
    return ((x.astype(np.uint64) * np.uint64(filled)) >> np.uint64(32)).astype(np.int64)


def check_nstep(n_step, newest, num_envs: int, filled: int):
    """The arguments of an n-step walk, as the kernel's entry point checks them -> ``(n_step, newest)``."""
    n_step = int(n_step)
    if n_step < 1:
        raise ValueError(f"n_step must be >= 1, got {n_step}")
    if newest is None:
        raise ValueError("n_step > 1 needs newest, the ring slot written last")
    if num_envs < 1 or filled < 1 or filled % num_envs:
        raise ValueError(f"an n-step walk needs whole slots: filled ({filled}) must be a multiple of num_envs ({num_envs})")
    if not 0 <= int(newest) < filled // num_envs:
        raise ValueError(f"newest must be in [0, {filled // num_envs}), got {newest}")
    return n_step, int(newest)


def dqn_nstep_walk_ref(rows, ring: ReplayRing, filled: int, newest: int, n_step: int, gamma: float,
                       dtype=torch.float32):
    """The n-step walk of ring rows ``rows`` [B] -> ``(last int64 [B], G [B], disc [B], m int64 [B])``:

        last = r0; G = rew[r0]; disc = gamma; m = 1
        while m < n_step and done[last] == 0 and slot(last) != newest:
            last += N; if last >= filled: last -= filled      # same env, next slot, ring wrap
            G += disc * rew[last]; disc *= gamma; m += 1

    in ``dtype``, ``G`` and ``disc`` updated in that order one step at a time.  A terminal (1) or a truncation
    (2) ends the walk, and so does the newest slot: the row then has an m-step return with m < n_step."""
    N = int(ring.act.shape[1])
    n_step, newest = check_nstep(n_step, newest, N, int(filled))
    np_dtype = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    rew = ring.rew.reshape(-1).cpu().numpy().astype(np_dtype)
    done = ring.done.reshape(-1).cpu().numpy()
    last = np.asarray(rows, np.int64).copy()
    g = np_dtype(gamma)
    G, disc, m = rew[last].copy(), np.full(last.shape, g, np_dtype), np.ones(last.shape, np.int64)
    for _ in range(n_step - 1):
        go = (m < n_step) & (done[last] == 0) & (last // N != newest)
        if not go.any():
            break
        nxt = last + N
        nxt = np.where(nxt >= filled, nxt - filled, nxt)
        last = np.where(go, nxt, last)
        G = np.where(go, (G + disc * rew[last]).astype(np_dtype), G)
        disc = np.where(go, (disc * g).astype(np_dtype), disc)
        m = m + go
    return last, G, disc, m


@torch.no_grad()
def dqn_targets_ref(online, target, H: int, A: int, ring: ReplayRing, filled: int, gamma: float, double_q: bool,
                    seed: int, update: int, B: int, dtype=torch.float32, tree=None, beta: Optional[float] = None,
                    n_step: int = 1, newest: Optional[int] = None, dueling: bool = False, quantiles: int = 0):
    """-> ``(Xb [B, D], act_b [B] int32, y [B], idx [B] int64)`` in ``dtype``;
    ``y = rew + gamma * (done == 1 ? 0 : 1) * Q_target(nobs, a*)`` with ``a*`` the lowest-index argmax of the
    target (``double_q`` false) or online net.  With ``tree`` (the priority sum tree of ops/per.py) the rows
    are ``per_sample_rows_ref``'s and two more results follow: ``w [B] = (filled * leaf / total)^-beta`` and
    ``wmax [1]``, its maximum.

    ``n_step > 1`` (with ``newest``, the ring slot written last) walks every sampled row forward
    (``dqn_nstep_walk_ref``) and ``y = G + disc * (done[last] == 1 ? 0 : 1) * Q_target(nobs[last], a*)``, ``a*``
    chosen at ``nobs[last]``; everything else still refers to the sampled row, and one more result follows at
    the end: ``last [B]`` int64, the row the target bootstrapped from.

    ``dueling``: both nets are dueling nets of ``A + 1`` outputs; ``a*`` is the lowest-index argmax of the
    selecting net's advantages and ``Q_target`` is ``reference.dueling_q`` of the target net.

    ``quantiles`` = NQ >= 1: both nets are quantile nets of ``A * NQ`` outputs, ``a*`` is the lowest-index argmax of
    the selecting net's quantile sums (``reference.quantile_q``), ``y`` is [B, NQ] and
    ``y[b, j] = G + disc * boot * theta_target[a* * NQ + j]``.  Everything but ``y`` is that of the scalar call."""
    D = ring.obs.shape[-1]
    dev = ring.obs.device
    NQ = check_quantiles(A, quantiles, dueling)
    _check_q_nets(online if double_q else None, target, D, H, A, dueling, NQ)
    n_step = int(n_step)
    if n_step != 1:
        check_nstep(n_step, newest, int(ring.act.shape[1]), int(filled))
    if tree is None:
        rows = dqn_sample_rows_ref(seed, update, B, filled)
    else:
        from .per import per_sample_rows_ref, per_weights_ref

        rows = per_sample_rows_ref(tree, seed, update, B, filled)
        w = per_weights_ref(tree, rows, filled, beta, dtype).to(dev)
    idx = torch.from_numpy(rows).to(dev)
    if n_step == 1:  # the walk of length one
        last, G, disc = idx, ring.rew.reshape(-1)[idx].to(dtype), gamma
    else:
        last, G, disc = (torch.from_numpy(x).to(dev)
                         for x in dqn_nstep_walk_ref(rows, ring, filled, newest, n_step, gamma, dtype)[:3])
    nobs = ring.nobs.reshape(-1, D)[last].to(dtype)
    boot = (ring.done.reshape(-1)[last] != 1).to(dtype)
    if NQ > 0:
        out_t = ref.trunk(target.to(dtype), nobs, D, H, A * NQ)[0]
        sel = ref.trunk(online.to(dtype), nobs, D, H, A * NQ)[0] if double_q else out_t
        astar, _ = ref.greedy_from_logits(ref.quantile_q(sel, A, NQ))
        theta = out_t.reshape(-1, A, NQ).gather(1, astar.reshape(-1, 1, 1).expand(-1, 1, NQ)).squeeze(1)
        col = (lambda t: t.unsqueeze(-1)) if torch.is_tensor(disc) else (lambda t: t)
        y = G.unsqueeze(-1) + col(disc) * boot.unsqueeze(-1) * theta
    else:
        q_t, astar = _q_and_astar(online, target, nobs, D, H, A, double_q, dueling, dtype)
        y = G + disc * boot * q_t.gather(-1, astar.unsqueeze(-1)).squeeze(-1)
    res = (ring.obs.reshape(-1, D)[idx], ring.act.reshape(-1)[idx].to(torch.int32), y, idx)
    if tree is not None:
        res += (w, w.max().reshape(1))
    return res if n_step == 1 else res + (last,)


def _check_q_nets(online, target, D, H, A, dueling, quantiles=0):
    """The sizes of the nets a targets call reads.  A hidden size the kernels do not have is the launch's to
    refuse (a GPU call), so it is not judged here."""
    if target.is_cuda and int(H) not in (64, 128):
        return
    check_q_params(target, D, H, A, dueling, "target", quantiles)
    check_q_params(online, D, H, A, dueling, "online", quantiles)


def _q_and_astar(online, target, nobs, D, H, A, double_q, dueling, dtype):
    """(Q_target [B, A], a* [B]) at ``nobs``: the selecting net is the online one with ``double_q``, else the
    target; a dueling net selects on its advantage outputs and evaluates ``reference.dueling_q``."""
    AO = A + 1 if dueling else A
    out_t = ref.trunk(target.to(dtype), nobs, D, H, AO)[0]
    sel = ref.trunk(online.to(dtype), nobs, D, H, AO)[0] if double_q else out_t
    astar, _ = ref.greedy_from_logits(sel[..., :A])
    return (ref.dueling_q(out_t, A) if dueling else out_t), astar


def dqn_targets(online: Optional[torch.Tensor], target: torch.Tensor, H: int, A: int, ring: ReplayRing, filled: int,
                gamma: float, double_q: bool, seed: int, update: int, B: int, out=None, dtype=torch.float32,
                tree=None, beta: Optional[float] = None, n_step: int = 1, newest: Optional[int] = None,
                dueling: bool = False, quantiles: int = 0):
    """Sample, gather and TD target in one launch -> ``(Xb, act_b, y, idx)``; ``out`` = the four tensors to
    write into (``idx`` int32 on the GPU, or None to skip it).  CPU tensors take the torch reference in
    ``dtype``; a GPU tensor without the extension raises.

    ``tree`` (the ``[2 * P2]`` priority sum tree of ops/per.py) selects the prioritised form: the rows come
    from the tree, and the result (and ``out``) is ``(Xb, act_b, y, idx, w, wmax)`` with the importance
    weights ``w [B] = (filled * leaf / total)^-beta`` and ``wmax [1]`` their maximum; ``idx`` is mandatory.

    ``n_step > 1`` selects the n-step instance of the kernel (``dqn_targets_ref`` has the semantics): it needs
    ``newest``, the ring slot written last, and takes the envs per slot from the ring.  The result then ends in
    ``last [B]`` (int32 on the GPU), the row each target bootstrapped from; an ``out`` may carry it as one more
    trailing tensor, or leave it out (or None) to skip it.  ``n_step == 1`` is the one-step launch as it was.

    ``dueling`` selects the dueling instances: ``A`` stays the action count, ``online`` / ``target`` are
    ``MLPSpec(D, H, A + 1)`` nets (``dqn_targets_ref`` has the semantics).  The sampled rows and every result
    but ``y`` are those of the plain launch on the same ring.

    ``quantiles`` = NQ >= 1 selects the quantile instances: ``online`` / ``target`` are ``MLPSpec(D, H, A * NQ)``
    nets and ``y`` is [B, NQ] (``dqn_targets_ref`` has the semantics); again only ``y`` differs from the scalar
    launch.  It is refused together with ``dueling``."""
    from . import use_hip, hip

    per = tree is not None
    dueling = bool(dueling)
    NQ = check_quantiles(A, quantiles, dueling) if quantiles else 0
    _check_q_nets(online if double_q else None, target, ring.obs.shape[-1], H, A, dueling, NQ)
    if per and not (beta is not None and 0.0 < beta <= 1.0):
        raise ValueError(f"the prioritised form needs beta in (0, 1], got {beta}")
    n_step = int(n_step)
    base = 6 if per else 4
    if n_step != 1:
        n_step, newest = check_nstep(n_step, newest, int(ring.act.shape[1]), int(filled))
    else:
        newest = None  # the one-step launch has no walk to check
    if out is not None and len(out) not in (base, base + 1):
        raise ValueError(f"out must hold {base} tensors, or {base + 1} with a trailing last; got {len(out)}")
    if n_step == 1 and out is not None and len(out) > base and out[base] is not None and out[3] is None:
        raise ValueError("at n_step = 1 last is idx: it cannot be written without idx")
    if not use_hip(target):
        res = dqn_targets_ref(online, target, H, A, ring, filled, gamma, double_q, seed, update, B, dtype, tree, beta,
                              n_step, newest, dueling, NQ)
        if out is None:
            return res
        if n_step == 1:
            res += (res[3],)  # a one-step target bootstraps from its own row
        for dst, src in zip(out, res):
            if dst is not None:
                dst.copy_(src)
        return out
    dev = target.device
    if out is None:
        out = (torch.empty(B, ring.obs.shape[-1], device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty((B, NQ) if NQ else (B,), device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        if per:
            out += (torch.empty(B, device=dev), torch.empty(1, device=dev))
        if n_step != 1:
            out += (torch.empty(B, dtype=torch.int32, device=dev),)
    if out[2].numel() != (B * NQ if NQ else B):
        raise ValueError(f"y must hold {B * NQ if NQ else B} targets, got {out[2].numel()}")
    if per and out[3] is None:
        raise ValueError("the prioritised form writes idx: it cannot be skipped")
    w, wmax = out[4:6] if per else (None, None)
    # the binding's optionals (tree, beta, w, wmax, n_step, newest, last, dueling) in its order: a positional call
    # parses faster than a keyword one, and this is the one place that makes it
    if NQ:  # the quantile nets have a binding of their own: the scalar one parses what it always parsed
        hip().dqn_targets_qr(online if double_q else None, target, int(H), int(A), ring.obs, ring.nobs, ring.act,
                             ring.rew, ring.done, int(filled), float(gamma), bool(double_q), int(seed), int(update),
                             *out[:4], tree, float(beta) if per else None, w, wmax, n_step, newest,
                             out[base] if len(out) > base else None, dueling, NQ)
        return out
    hip().dqn_targets(online if double_q else None, target, int(H), int(A), ring.obs, ring.nobs, ring.act, ring.rew,
                      ring.done, int(filled), float(gamma), bool(double_q), int(seed), int(update), *out[:4], tree,
                      float(beta) if per else None, w, wmax, n_step, newest,
                      out[base] if len(out) > base else None, dueling)
    return out
