"""Policy evaluation: fixed weights, whole episodes, the greedy action.

``evaluate_policy`` runs ``episodes`` complete episodes in each of ``num_envs`` device envs through
the fused evaluation kernel (csrc/kernels/evaluate.hip) and returns an ``EvalResult``: the three
``[episodes, num_envs]`` tensors of the launch and their statistics.  The returns the trainers
report (``AverageEpRet``) come from sampled training rollouts cut at epoch boundaries; this is the
score of the policy itself.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops import evaluate_policy_op

STAT_FIELDS = ("episodes", "mean_return", "std_return", "min_return", "max_return", "mean_length",
               "truncated_share")


class EvalResult:
    """``ep_ret`` (float32), ``ep_len`` and ``ep_code`` (int32; 1 terminal, 2 time limit), each
    ``[E, N]``.  The statistics are float64 torch reductions on the tensors' device, computed on
    first use behind ONE synchronising read; ``std_return`` is the population deviation like the
    trainers' ``StdEpRet``."""

    def __init__(self, ep_ret: torch.Tensor, ep_len: torch.Tensor, ep_code: torch.Tensor, greedy: bool = True,
                 seed: int = 0, step0: int = 0):
        self.ep_ret, self.ep_len, self.ep_code = ep_ret, ep_len, ep_code
        self.greedy, self.seed, self.step0 = bool(greedy), int(seed), int(step0)
        self._stats = None

    def stats(self) -> dict:
        if self._stats is None:
            r = self.ep_ret.double().reshape(-1)
            ln = self.ep_len.double().reshape(-1)
            mean = r.mean()
            packed = torch.stack([mean, (r - mean).square().mean().sqrt(), r.min(), r.max(), ln.mean(),
                                  (self.ep_code == 2).double().mean()])
            v = packed.tolist()  # the one device -> host read
            self._stats = dict(zip(STAT_FIELDS, [int(r.numel())] + v))
        return self._stats

    def __getattr__(self, name):
        if name in STAT_FIELDS:
            return self.stats()[name]
        raise AttributeError(name)

    def to_dict(self) -> dict:
        d = dict(self.stats())
        d.update(greedy=self.greedy, seed=self.seed, step0=self.step0)
        return d

    def __repr__(self):
        return f"EvalResult({self.to_dict()})"


def evaluate_policy(env: str, params: torch.Tensor, hidden: int, episodes: int, num_envs: int, greedy: bool = True,
                    seed: int = 0, step0: int = 0, max_episode_steps: Optional[int] = None, device=None,
                    dueling: bool = False, quantiles: int = 0) -> EvalResult:
    """Score the flat policy weights ``params`` on the device env ``env``: ``num_envs`` envs x
    ``episodes`` complete episodes each, greedy (argmax / mean action) or sampled like training.
    Env resets and env noise come from the Philox stream ``(seed, step0 + t)``.

    ``dueling``: ``params`` is a dueling Q-network (``A + 1`` outputs) of a discrete env, scored greedily on
    its advantage outputs; ``greedy=False`` raises.

    ``quantiles`` = NQ >= 1: ``params`` is a quantile Q-network (``A * NQ`` outputs) of a discrete env, scored
    greedily on the per-action quantile sums; ``greedy=False`` and ``dueling`` raise."""
    from .vec_trainer import CONTINUOUS_DEVICE_ENVS, DEVICE_ENVS

    if env not in DEVICE_ENVS:
        raise ValueError(f"no device implementation of env {env!r}; have {list(DEVICE_ENVS)}")
    if dueling and env in CONTINUOUS_DEVICE_ENVS:
        raise ValueError(f"a dueling Q-network needs a discrete action space; {env!r} is continuous")
    if dueling and not greedy:
        raise ValueError("a dueling Q-network is evaluated greedily: softmax-of-Q is not this algorithm's policy")
    quantiles = int(quantiles)
    if quantiles < 0:
        raise ValueError(f"quantiles must be >= 0, got {quantiles}")
    if quantiles and dueling:
        raise ValueError("quantiles > 0 with dueling=True is not built")
    if quantiles and env in CONTINUOUS_DEVICE_ENVS:
        raise ValueError(f"a quantile Q-network needs a discrete action space; {env!r} is continuous")
    if quantiles and not greedy:
        raise ValueError("a quantile Q-network is evaluated greedily: softmax-of-Q is not this algorithm's policy")
    if device is None:
        device = params.device if params.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    p = params.detach().to(device=device, dtype=torch.float32).contiguous()
    consts = None
    if env in CONTINUOUS_DEVICE_ENVS:
        from .. import _native

        consts = torch.tensor(_native.env_constants(env), dtype=torch.float32, device=device)
    ep_ret, ep_len, ep_code, _ = evaluate_policy_op(DEVICE_ENVS[env], p, hidden, episodes, num_envs, greedy=greedy,
                                                    seed=seed, step0=step0, max_steps=max_episode_steps,
                                                    env_consts=consts, dueling=bool(dueling),
                                                    **(dict(quantiles=quantiles) if quantiles else {}))
    return EvalResult(ep_ret, ep_len, ep_code, greedy, seed, step0)


# Steps between two reads of the device counter ``remaining`` in evaluate_pixel_policy (one 4-byte
# synchronising read each).  At 2,048 envs a whole evaluation took 39.18 / 38.71 / 38.46 / 38.37 ms
# with 8 / 32 / 128 / 512 (docs/PERF_NOTES.md): 32 is within 0.9 % of never polling and overshoots
# the last episode by at most 31 steps.
PIXEL_POLL_EVERY = 32


class PixelEvalTrace:
    """Per-step trace buffers of ``evaluate_pixel_policy`` (tests): ``act`` [S, N] int32, ``logits``
    [S, N, A], ``rew`` / ``done`` [S, N] for up to ``S`` steps, row t written for the envs that
    stepped at step t.  The caller may hand in its own (e.g. guarded, prefilled) tensors."""

    def __init__(self, steps: int, num_envs: int, act_dim: int, device, act=None, logits=None, rew=None, done=None):
        S, N = int(steps), int(num_envs)
        self.steps = S
        self.act = torch.zeros(S, N, dtype=torch.int32, device=device) if act is None else act
        self.logits = torch.zeros(S, N, act_dim, device=device) if logits is None else logits
        self.rew = torch.zeros(S, N, device=device) if rew is None else rew
        self.done = torch.zeros(S, N, device=device) if done is None else done

    def rows(self, t: int):
        return self.act[t], self.logits[t], self.rew[t], self.done[t]


def evaluate_pixel_policy(model, episodes: int, num_envs: int, greedy: bool = True, seed: int = 0, step0: int = 0,
                          max_episode_steps: int = 6750, row0: int = 0, poll_every: Optional[int] = None,
                          trace: Optional[PixelEvalTrace] = None) -> EvalResult:
    """Score the weights of ``model`` (a ``DeviceNatureCNN``) on PongSynth-v0: ``num_envs`` fresh envs
    play ``episodes`` whole episodes each, greedy (the lowest index among the maximal logits) or
    sampled like a training rollout.

    Everything but the model's weights and its scratch rows ``row0 .. row0 + num_envs`` is owned
    here: a fresh ``DevicePong`` reset at counter ``step0``, a 5-slot frame ring (16-wave conv
    stack) or an s2d observation buffer, the episode slots, ``ep_cnt`` and the device counter
    ``remaining``.  Step t launches, eagerly on the current stream, the conv stack (no a1 / a2
    stores), the fc split-K GEMM and the fused head + env step + render kernel
    (``DevicePong.eval_step``) with the host counters ``step0 + 1 + t``: the same ``(seed, step0)``
    replays the same evaluation.  The result also carries ``steps`` (the steps launched), ``ep_cnt``,
    ``remaining`` and the ``env``.

    Every ``poll_every`` steps ``remaining`` is read (4 bytes, one synchronisation) and the loop
    ends at 0, and in any case after ``episodes * max_episode_steps`` steps.  An env that has
    finished its episodes is frozen inside the step kernel but still passes through the conv stack
    and the fc GEMM, so the tail of an evaluation -- a few envs still playing -- costs full steps
    (no compaction of frozen envs)."""
    from ..envs.pong import DevicePong, FrameRing
    from ..models.nature_cnn import HIDDEN, FC_IN, OBS_S2D

    E, N = int(episodes), int(num_envs)
    if E < 1 or N < 1:
        raise ValueError("evaluate_pixel_policy: episodes and num_envs must be >= 1")
    max_steps = int(max_episode_steps)
    if max_steps < 1 or E * max_steps >= 2 ** 31:
        raise ValueError("evaluate_pixel_policy: need max_episode_steps >= 1 and episodes * max_episode_steps < 2^31")
    if row0 < 0 or row0 + N > model.max_batch:
        raise ValueError(f"evaluate_pixel_policy: rows {row0} .. {row0 + N} exceed the model's {model.max_batch}")
    if not model.fc_nt or model.A > 8:
        raise RuntimeError("evaluate_pixel_policy needs the split-K fc (RRL_FC_NT=1) and at most 8 actions")
    poll = PIXEL_POLL_EVERY if poll_every is None else int(poll_every)
    if poll < 1:
        raise ValueError("evaluate_pixel_policy: poll_every >= 1")
    dev = model.device
    env = DevicePong(N, dev, seed, max_steps)
    env.step_count = int(step0)
    ring = None
    if model.fused_convs and model.fwd_layout in (0, 64):  # the 16-wave conv stack reads frame rows
        ring = FrameRing(N, 5, dev)  # a step reads the frames of steps t - 3 .. t and writes t + 1
        obs = torch.zeros(N, 4, dtype=torch.int32, device=dev)
        env.reset(ring=(ring, obs))
    else:
        obs = torch.zeros((N,) + tuple(OBS_S2D), dtype=torch.uint8, device=dev)
        env.reset(obs)
    ep_cnt = torch.zeros(N, dtype=torch.int32, device=dev)
    ep_ret = torch.zeros(E, N, device=dev)
    ep_len = torch.zeros(E, N, dtype=torch.int32, device=dev)
    ep_code = torch.zeros(E, N, dtype=torch.int32, device=dev)
    remaining = torch.full((1,), N, dtype=torch.int32, device=dev)
    fc_b, hp = model.head_params()
    splits = model.fc_splits(N)
    assert splits * N * HIDDEN <= model._fc_part.numel(), "fc split-K partials exceed the preallocated buffer"
    a3 = model._rows(model.a3, row0, N, FC_IN)
    wfc = model.shadow[model.o["wfc"]:model.o["bfc"]]
    steps, limit = 0, E * max_steps
    while steps < limit:
        x = obs if ring is None else ring.obs(obs)
        model.forward(x, row0, fc=False, store_acts=False)
        used = int(model.h.fc_nt_part(a3, wfc, model._fc_part, N, HIDDEN, FC_IN, splits))
        env.eval_step(model._fc_part, used, fc_b, hp, model.A, seed, step0 + 1 + steps, step0 + 1 + steps, obs, E,
                      ep_cnt, ep_ret, ep_len, ep_code, remaining, greedy=greedy, ring=ring,
                      trace=None if trace is None or steps >= trace.steps else trace.rows(steps))
        steps += 1
        if steps % poll == 0 and int(remaining.item()) == 0:
            break
    res = EvalResult(ep_ret, ep_len, ep_code, greedy, seed, step0)
    res.steps, res.ep_cnt, res.remaining, res.env = steps, ep_cnt, remaining, env
    return res


def not_supported(what: str):
    """The evaluate() of a trainer without a device-env evaluation path."""
    raise NotImplementedError(f"evaluate() is not implemented for {what}: policy evaluation runs the fused "
                              "device-env kernel of the in-process vec engine (VecTrainer.evaluate)")
