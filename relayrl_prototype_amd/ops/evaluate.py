"""Fused policy evaluation (csrc/kernels/evaluate.hip): every one of N device envs runs E complete
episodes under fixed weights, in one launch.

There is no PyTorch path: the op needs the HIP extension and GPU tensors and raises otherwise.
The float64 env oracles of the tests (tests/rollout_oracle.py) and ``reference.greedy_actions_ref``
are what the kernel is held to.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch


class EvalTrace(NamedTuple):
    """The first Tc steps in the rollout buffers' layout.  Row t of an env is written only while
    that env is still running one of its E episodes; other cells keep what they held."""
    obs: torch.Tensor   # [Tc, N, D] the observation the action of step t was computed from
    act: torch.Tensor   # [Tc, N] int32, or [Tc, N, A] float for a continuous env
    rew: torch.Tensor   # [Tc, N]
    done: torch.Tensor  # [Tc, N] 0 running, 1 episode end of either kind


def evaluate_policy_op(env_id: int, params: torch.Tensor, hidden: int, episodes: int, num_envs: int, *,
                       greedy: bool = True, seed: int = 0, step0: int = 0, max_steps: Optional[int] = None,
                       env_consts: Optional[torch.Tensor] = None, trace_steps: int = 0, out=None,
                       trace: Optional[EvalTrace] = None, dueling: bool = False, quantiles: int = 0):
    """-> ``(ep_ret, ep_len, ep_code, trace-or-None)``: float32 / int32 / int32 ``[episodes, num_envs]``
    (code 1 terminal, 2 time limit).  ``out`` = the three tensors to write into; ``trace`` = an
    ``EvalTrace`` to write into, or ``trace_steps`` > 0 to have one allocated (zero-filled).
    ``env_consts`` is required for the continuous env (``_native.env_constants(name)``).
    Asynchronous on the current stream, like the other ops.

    ``dueling`` (discrete envs, ``greedy`` only): ``params`` is a dueling Q-network of ``A + 1`` outputs and
    the action is the lowest-index argmax of its ``A`` advantage outputs.

    ``quantiles`` = NQ >= 1 (discrete envs, ``greedy`` only): ``params`` is a quantile Q-network of ``A * NQ``
    outputs and the action is the lowest-index argmax of the per-action quantile sums."""
    from . import hip

    h = hip()  # raises NativeExtensionMissing: there is no fallback
    if not params.is_cuda:
        raise ValueError("evaluate_policy_op runs the HIP kernel only: params must be a GPU tensor")
    D, A, _, env_max = h.env_dims(int(env_id))
    continuous = int(env_id) == h.ENV_IDS["ENV_HALFCHEETAH"]
    if continuous and env_consts is None:
        raise ValueError("the continuous device env needs env_consts")
    if dueling:
        from .dqn import check_q_params

        if continuous:
            raise ValueError("a dueling Q-network needs a discrete action space")
        if not greedy:
            raise ValueError("a dueling Q-network is evaluated greedily: softmax-of-Q is not this algorithm's policy")
        check_q_params(params, D, hidden, A, True, quantiles=quantiles)
    elif quantiles:
        from .dqn import check_q_params

        if continuous:
            raise ValueError("a quantile Q-network needs a discrete action space")
        if not greedy:
            raise ValueError("a quantile Q-network is evaluated greedily: softmax-of-Q is not this algorithm's policy")
        check_q_params(params, D, hidden, A, False, quantiles=quantiles)
    E, N = int(episodes), int(num_envs)
    if E < 1 or N < 1:
        raise ValueError(f"episodes and num_envs must be >= 1, got {E} and {N}")
    max_steps = int(max_steps or env_max)
    dev = params.device
    if out is None:
        out = (torch.empty(E, N, device=dev), torch.empty(E, N, dtype=torch.int32, device=dev),
               torch.empty(E, N, dtype=torch.int32, device=dev))
    ep_ret, ep_len, ep_code = out
    if tuple(ep_ret.shape) != (E, N):
        raise ValueError(f"ep_ret must be [{E}, {N}], got {tuple(ep_ret.shape)}")
    if trace is None and trace_steps > 0:
        Tc = int(trace_steps)
        act = torch.zeros(Tc, N, A, device=dev) if continuous else torch.zeros(Tc, N, dtype=torch.int32, device=dev)
        trace = EvalTrace(torch.zeros(Tc, N, D, device=dev), act, torch.zeros(Tc, N, device=dev),
                          torch.zeros(Tc, N, device=dev))
    tr = tuple(trace) if trace is not None else (None, None, None, None)
    args = (int(hidden), ep_ret, ep_len, ep_code, *tr, int(seed), int(step0), bool(greedy), max_steps)
    if continuous:
        h.evaluate_cont(int(env_id), params, env_consts, *args)
    elif quantiles:  # the quantile nets have a binding of their own
        h.evaluate_qr(int(env_id), params, *args, bool(dueling), int(quantiles))
    elif dueling:
        h.evaluate(int(env_id), params, *args, True)
    else:
        h.evaluate(int(env_id), params, *args)
    return ep_ret, ep_len, ep_code, trace
