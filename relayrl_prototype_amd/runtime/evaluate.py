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
                    seed: int = 0, step0: int = 0, max_episode_steps: Optional[int] = None, device=None) -> EvalResult:
    """Score the flat policy weights ``params`` on the device env ``env``: ``num_envs`` envs x
    ``episodes`` complete episodes each, greedy (argmax / mean action) or sampled like training.
    Env resets and env noise come from the Philox stream ``(seed, step0 + t)``."""
    from .vec_trainer import CONTINUOUS_DEVICE_ENVS, DEVICE_ENVS

    if env not in DEVICE_ENVS:
        raise ValueError(f"no device implementation of env {env!r}; have {list(DEVICE_ENVS)}")
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
                                                    env_consts=consts)
    return EvalResult(ep_ret, ep_len, ep_code, greedy, seed, step0)


def not_supported(what: str):
    """The evaluate() of a trainer without a device-env evaluation path."""
    raise NotImplementedError(f"evaluate() is not implemented for {what}: policy evaluation runs the fused "
                              "device-env kernel of the in-process vec engine (VecTrainer.evaluate)")
