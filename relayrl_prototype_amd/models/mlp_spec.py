"""Flat-parameter MLP layout (``MLPSpec``), importable without torch: CPU agents (api/agent.py,
models/cpu_policy.py) split the learner's flat weight vector with it; the device learner and
the kernels use the same offsets (ops/mlp.py re-exports it).  ``q_outputs`` is the one copy of the rule
for how many outputs a Q-network has."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional


def q_outputs(A: int, dueling: bool = False, quantiles: int = 0) -> int:
    """Outputs of a Q-network over ``A`` actions, as the kernels hold them (16 at most): ``A`` for the plain net,
    ``A + 1`` (the state value) for the dueling one, ``A * quantiles`` for the quantile one (``quantiles`` = 0 is a
    scalar net), and never both.  Raises ``ValueError`` for a combination that is not built."""
    A, NQ = int(A), int(quantiles)
    if NQ < 0:
        raise ValueError(f"quantiles must be >= 0, got {quantiles}")
    if NQ > 0 and dueling:
        raise ValueError("quantiles > 0 with dueling=True is not built: the two heads share 16 outputs and the "
                         "combination needs its own design; set quantiles=0 or dueling=False")
    if NQ > 0 and A * NQ > 16:
        raise ValueError(f"a quantile net has A * quantiles <= 16 outputs, got A = {A} and quantiles = {NQ}")
    if dueling and not 1 <= A <= 15:
        raise ValueError(f"a dueling net has A + 1 <= 16 outputs: A must be in [1, 15], got {A}")
    return A * NQ if NQ else A + 1 if dueling else A


def c51_outputs(A: int, atoms: int, v_min: float, v_max: float, dueling: bool = False, quantiles: int = 0) -> int:
    """Outputs of a categorical (C51) Q-network over ``A`` actions, ``A * atoms``, as the wide output layer holds them:
    every action's atoms are rounded up to whole tiles of 16 outputs and 8 tiles are the limit, so CartPole takes up
    to 64 atoms and the envs of 3 or 4 actions up to 32.  Raises ``ValueError`` for what is not built: ``atoms`` with
    ``quantiles`` or with ``dueling``, ``atoms < 2``, ``v_max <= v_min``, or a head past the tile limit."""
    A, NA = int(A), int(atoms)
    if int(quantiles):
        raise ValueError(f"atoms = {NA} with quantiles = {quantiles} is not built: set one of the two")
    if dueling:
        raise ValueError(f"atoms = {NA} with dueling = True is not built: set one of the two")
    if NA < 2:
        raise ValueError(f"atoms must be 0 or >= 2, got {atoms}")
    if not float(v_max) > float(v_min):
        raise ValueError(f"atoms needs v_min < v_max, got v_min = {v_min} and v_max = {v_max}")
    if A < 1 or NA > 64 or A * ((NA + 15) // 16) > 8:
        raise ValueError(f"a categorical net has A * ceil(atoms / 16) <= 8 output tiles, got A = {A} and atoms = {NA}")
    return A * NA


def munchausen_on(munchausen: float, m_tau: float, m_clip: float, double_q: bool = False, dueling: bool = False,
                  atoms: int = 0) -> bool:
    """Whether the Munchausen targets are on (``munchausen`` = alpha > 0), and whether the kernels have the
    combination: alpha in [0, 1]; alpha > 0 needs ``m_tau`` > 0 and ``m_clip`` < 0, has no argmax for ``double_q`` to
    select and is built for the plain and the quantile net.  Raises ``ValueError`` naming the fields otherwise."""
    alpha = float(munchausen)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"munchausen must be in [0, 1], got {munchausen}")
    if alpha == 0.0:
        return False
    if not float(m_tau) > 0.0:
        raise ValueError(f"munchausen = {alpha} needs m_tau > 0, got {m_tau}")
    if not float(m_clip) < 0.0:
        raise ValueError(f"munchausen = {alpha} needs m_clip < 0, got {m_clip}")
    if double_q:
        raise ValueError(f"munchausen = {alpha} with double_q = True is not built: the soft target has no argmax to "
                         "select; set double_q=False")
    if dueling:
        raise ValueError(f"munchausen = {alpha} with dueling = True is not built: set one of the two")
    if int(atoms):
        raise ValueError(f"munchausen = {alpha} with atoms = {atoms} is not built: set one of the two")
    return True


def lambda_on(q_lambda: float, n_step: int = 1, quantiles: int = 0, atoms: int = 0, munchausen: float = 0.0) -> bool:
    """Whether the lambda-return targets are on (``q_lambda`` < 1), and whether the kernels have the combination:
    ``q_lambda`` in [0, 1]; below 1 it mixes the 1 .. n-step targets of a walk of ``n_step`` in [2, 8] steps on the scalar
    hard-max target.  A mixture of return distributions is not the mean of their quantiles or atoms and the soft target
    has no argmax to mix, so those are refused.  Raises ``ValueError`` naming the fields otherwise."""
    lam = float(q_lambda)
    if not 0.0 <= lam <= 1.0:  # a NaN fails it too
        raise ValueError(f"q_lambda must be in [0, 1], got {q_lambda}")
    if lam == 1.0:
        return False
    if not 2 <= int(n_step) <= 8:
        raise ValueError(f"q_lambda = {lam} needs n_step in [2, 8], got {n_step}")
    if int(quantiles):
        raise ValueError(f"q_lambda = {lam} with quantiles = {quantiles} is not built: a mixture of return "
                         "distributions is not the mean of their quantiles")
    if int(atoms):
        raise ValueError(f"q_lambda = {lam} with atoms = {atoms} is not built: a mixture of return distributions is "
                         "not the mean of their atoms")
    if float(munchausen) > 0.0:
        raise ValueError(f"q_lambda = {lam} with munchausen = {munchausen} is not built: set one of the two")
    return True


@dataclass(frozen=True)
class MLPSpec:
    """Linear(D,H)-ReLU-Linear(H,H)-ReLU-Linear(H,A) [+ log_std(A)]."""

    D: int
    H: int
    A: int
    gaussian: bool = False

    @property
    def P(self) -> int:
        D, H, A = self.D, self.H, self.A
        return H * D + H + H * H + H + A * H + A + (A if self.gaussian else 0)

    def offsets(self):
        D, H, A = self.D, self.H, self.A
        o = {}
        o["w1"] = 0
        o["b1"] = H * D
        o["w2"] = o["b1"] + H
        o["b2"] = o["w2"] + H * H
        o["w3"] = o["b2"] + H
        o["b3"] = o["w3"] + A * H
        o["log_std"] = o["b3"] + A
        return o

    def init(self, generator=None, device="cpu", log_std_init: float = -0.5, out_gain: Optional[float] = None):
        """nn.Linear default init (kaiming_uniform(a=sqrt(5)) == U(+-1/sqrt(fan_in)))."""
        import torch

        D, H, A = self.D, self.H, self.A
        parts = []
        for fan_in, fan_out in ((D, H), (H, H), (H, A)):
            bound = 1.0 / math.sqrt(fan_in)
            w = (torch.rand(fan_out * fan_in, generator=generator) * 2 - 1) * bound
            b = (torch.rand(fan_out, generator=generator) * 2 - 1) * bound
            if out_gain is not None and fan_out == A:
                w = w * out_gain
                b = b * 0
            parts += [w, b]
        if self.gaussian:
            parts.append(torch.full((A,), float(log_std_init)))
        return torch.cat(parts).float().to(device)

    def unflatten(self, params):
        from ..ops import reference as ref

        return ref.unflatten(params, self.D, self.H, self.A, self.gaussian)
