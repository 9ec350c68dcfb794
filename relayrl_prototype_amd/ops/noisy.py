"""NoisyNet exploration (Fortunato et al. 2018, factorised Gaussian noise) for the DQN path: the two
kernels of csrc/kernels/noisy.hip and their host oracles.

All three linear layers of the ``MLPSpec(D, H, A_out)`` net are noisy.  A noisy net keeps ``theta = [mu (P);
sigma (P)]`` and every launch that reads weights gets the flat effective parameters ``mu + sigma * eps`` of
one (role, draw) instead, so the big kernels stay as they are.

The contract (docs/KERNELS.md has the full text):

* unit ``i`` of (role ``r``, layer ``l`` = 1..3, side ``s`` = 0 in / 1 out) at the 64-bit draw ``d`` takes the
  Philox4x32-10 word at counter ``(i, lo32(d), hi32(d), 16 + 8 r + 2 (l - 1) + s)`` under the run's noise
  key; ``u0 = u01(word.x)``, ``u1 = u01(word.y)``, ``n = sqrtf(-2 logf(1 - u0)) * cosf(6.283185307179586f * u1)``;
* unit factor ``f = copysignf(sqrtf(fabsf(n)), n)``;
* ``eps_W[j][i] = f_out[j] * f_in[i]`` (one fp32 multiply), ``eps_b[j] = f_out[j]``;
* ``W_eff = mu + sigma * eps``: one fp32 multiply, then one fp32 add, never fused.

The unit vector of one (role, draw) has ``U = D + 4 H + A_out`` entries laid out
``[in1 (D), out1 (H), in2 (H), out2 (H), in3 (H), out3 (A_out)]``.

Roles: 0 the actor (draw = epoch), 1 the online net in the loss, 2 the target net, 3 the online net that
selects ``a*`` under double Q (draws = the update index).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import philox
from .mlp import MLPSpec

ROLE_ACTOR, ROLE_ONLINE, ROLE_TARGET, ROLE_SELECT = 0, 1, 2, 3
MAX_JOBS = 3
TWO_PI_F32 = np.float32(6.283185307179586)


def noisy_num_units(spec: MLPSpec) -> int:
    return spec.D + 4 * spec.H + spec.A


def _unit_blocks(spec: MLPSpec):
    """(tag offset 2 (l - 1) + s, count) of the six blocks of the unit vector, in its order."""
    D, H, A = spec.D, spec.H, spec.A
    return [(0, D), (1, H), (2, H), (3, H), (4, H), (5, A)]


def _check_spec(spec: MLPSpec):
    if spec.gaussian:
        raise ValueError("a noisy net is a Q-network: no log_std")
    if not (1 <= spec.D <= 16 and 1 <= spec.A <= 16):
        raise ValueError(f"D and A_out must be in [1, 16], got D = {spec.D}, A_out = {spec.A}")


def noisy_words(key: int, role: int, draw: int, spec: MLPSpec):
    """(x, y) uint32 [U]: the two Philox words every unit of (role, draw) is made of."""
    if not 0 <= int(role) <= 3:
        raise ValueError(f"role must be in [0, 3], got {role}")
    xs, ys = [], []
    for off, n in _unit_blocks(spec):
        i = np.arange(n, dtype=np.uint32)
        full = lambda v: np.full(i.shape, v, np.uint32)  # noqa: E731
        w = philox.philox4x32(i, full(draw & 0xFFFFFFFF), full((draw >> 32) & 0xFFFFFFFF),
                              full(16 + 8 * int(role) + off), full(key & 0xFFFFFFFF), full((key >> 32) & 0xFFFFFFFF))
        xs.append(w[0])
        ys.append(w[1])
    return np.concatenate(xs), np.concatenate(ys)


def noisy_units_ref(key: int, role: int, draw: int, spec: MLPSpec, dtype=np.float64):
    """``(n [U], f [U])``: the unit normals and the unit factors of (role, draw).  ``dtype=np.float64`` is the
    oracle (the same Philox words, exact ``u0`` / ``u1``, double-precision Box-Muller); ``dtype=np.float32``
    emulates the kernel's arithmetic step by step in numpy float32."""
    x, y = noisy_words(key, role, draw, spec)
    u0, u1 = philox.u01(x), philox.u01(y)  # fp32, exact 24-bit fractions
    if dtype == np.float32:
        one = np.float32(1.0)
        r = np.sqrt(np.float32(-2.0) * np.log(one - u0, dtype=np.float32), dtype=np.float32)
        n = (r * np.cos(TWO_PI_F32 * u1, dtype=np.float32)).astype(np.float32)
        f = np.copysign(np.sqrt(np.abs(n), dtype=np.float32), n).astype(np.float32)
        return n, f
    if dtype != np.float64:
        raise ValueError("dtype must be np.float64 or np.float32")
    u0, u1 = u0.astype(np.float64), u1.astype(np.float64)
    n = np.sqrt(-2.0 * np.log(1.0 - u0)) * np.cos(2.0 * math.pi * u1)
    return n, np.copysign(np.sqrt(np.abs(n)), n)


def noisy_eps_ref(units, spec: MLPSpec) -> torch.Tensor:
    """The flat noise ``eps [P]`` of the unit factors ``units [U]`` in the dtype of ``units`` (fp32: one multiply
    per weight, as the kernel): per layer ``outer(f_out, f_in)`` then ``f_out``."""
    f = torch.as_tensor(units).reshape(-1)
    if f.numel() != noisy_num_units(spec):
        raise ValueError(f"units has {f.numel()} entries, the net has {noisy_num_units(spec)}")
    blocks, at = [], 0
    for _, n in _unit_blocks(spec):
        blocks.append(f[at:at + n])
        at += n
    parts = []
    for l in range(3):
        f_in, f_out = blocks[2 * l], blocks[2 * l + 1]
        parts += [torch.outer(f_out, f_in).reshape(-1), f_out]
    return torch.cat(parts)


def noisy_compose_ref(theta: torch.Tensor, units, spec: MLPSpec) -> torch.Tensor:
    """``mu + sigma * eps`` in the dtype of ``theta``: a multiply, then an add."""
    P = spec.P
    theta = theta.reshape(-1)
    if theta.numel() != 2 * P:
        raise ValueError(f"theta must be [mu ({P}); sigma ({P})], got {theta.numel()} floats")
    eps = noisy_eps_ref(torch.as_tensor(units).to(theta.dtype), spec).to(theta.device)
    prod = theta[P:] * eps
    return theta[:P] + prod


def noisy_grad_ref(slab: torch.Tensor, eps: torch.Tensor) -> torch.Tensor:
    """``[g; g * eps]`` with ``g`` the sum of the slabs in ascending order, one add at a time."""
    slab = slab.reshape(-1, eps.numel())
    g = slab[0].clone()
    for s in range(1, slab.shape[0]):
        g = g + slab[s]
    return torch.cat([g, g * eps.to(g.dtype)])


def noisy_sigma_init(spec: MLPSpec, sigma0: float) -> torch.Tensor:
    """fp32 ``[P]``: ``sigma0 / sqrt(fan_in)`` for every weight and bias of each layer."""
    _check_spec(spec)
    if not float(sigma0) >= 0.0:
        raise ValueError(f"noisy_sigma0 must be >= 0, got {sigma0}")
    D, H, A = spec.D, spec.H, spec.A
    parts = [torch.full((fan_out * fan_in + fan_out,), float(sigma0) / math.sqrt(fan_in))
             for fan_in, fan_out in ((D, H), (H, H), (H, A))]
    return torch.cat(parts).float()


def _as_list(x, n):
    return list(x) if isinstance(x, (list, tuple)) else [x] * n


def noisy_compose(theta, roles: Sequence[int], draws: Sequence[int], spec: MLPSpec, key: int,
                  out: Optional[torch.Tensor] = None, units_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Effective parameters of up to three (role, draw) jobs in ONE launch -> ``out [njobs, P]``.  ``theta`` is
    one ``[2 P]`` tensor or one per job (the target net has its own); ``units_out [njobs, U]`` (optional)
    receives the unit factors.  CPU tensors take the fp32 numpy emulation."""
    from . import use_hip, hip

    _check_spec(spec)
    roles = [int(r) for r in roles]
    njobs = len(roles)
    draws = [int(d) for d in _as_list(draws, njobs)]
    thetas = _as_list(theta, njobs)
    if not 1 <= njobs <= MAX_JOBS or len(draws) != njobs or len(thetas) != njobs:
        raise ValueError(f"noisy_compose takes 1 to {MAX_JOBS} jobs with one role, draw and theta each")
    if any(not 0 <= r <= 3 for r in roles):
        raise ValueError(f"roles must be in [0, 3], got {roles}")
    P, U = spec.P, noisy_num_units(spec)
    for t in thetas:
        if t.numel() != 2 * P:
            raise ValueError(f"theta must be [mu ({P}); sigma ({P})], got {t.numel()} floats")
    if out is None:
        out = torch.empty(njobs, P, device=thetas[0].device)
    if out.numel() != njobs * P:
        raise ValueError(f"out must hold {njobs} x {P} floats, got {out.numel()}")
    if units_out is not None and units_out.numel() != njobs * U:
        raise ValueError(f"units_out must hold {njobs} x {U} floats, got {units_out.numel()}")
    if not use_hip(thetas[0]):
        for k in range(njobs):
            f = torch.from_numpy(noisy_units_ref(key, roles[k], draws[k], spec, np.float32)[1])
            out.view(njobs, P)[k].copy_(noisy_compose_ref(thetas[k].float(), f, spec))
            if units_out is not None:
                units_out.view(njobs, U)[k].copy_(f)
        return out
    rc = int(hip().noisy_compose(thetas, roles, draws, int(spec.D), int(spec.H), int(spec.A), int(key), out, units_out))
    if rc != 0:  # a missing kernel or a refused launch is an error, never a fallback
        raise RuntimeError(f"noisy_compose refused the launch (code {rc})")
    return out


def noisy_grad(slab: torch.Tensor, role: int, draw: int, spec: MLPSpec, key: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient slabs ``[nslab, P]`` of the effective parameters of (role, draw) -> ``out [2 P]``, the gradient
    of ``[mu; sigma]``: the slabs summed in ascending order, and that sum times ``eps``."""
    from . import use_hip, hip

    _check_spec(spec)
    if not 0 <= int(role) <= 3:
        raise ValueError(f"role must be in [0, 3], got {role}")
    P = spec.P
    if slab.dim() != 2 or slab.shape[1] != P or slab.shape[0] < 1:
        raise ValueError(f"slab must be [nslab >= 1, {P}], got {tuple(slab.shape)}")
    if out is None:
        out = torch.empty(2 * P, device=slab.device)
    if out.numel() != 2 * P:
        raise ValueError(f"out must hold 2 x {P} floats, got {out.numel()}")
    if not use_hip(slab):
        f = torch.from_numpy(noisy_units_ref(key, int(role), int(draw), spec, np.float32)[1])
        out.copy_(noisy_grad_ref(slab.float(), noisy_eps_ref(f, spec)))
        return out
    if not slab.is_contiguous():
        raise ValueError("slab must be contiguous")
    rc = int(hip().noisy_grad(slab, int(role), int(draw), int(spec.D), int(spec.H), int(spec.A), int(key), out,
                              int(slab.shape[0])))
    if rc != 0:
        raise RuntimeError(f"noisy_grad refused the launch (code {rc})")
    return out
