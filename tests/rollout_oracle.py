"""Host oracle of the fused rollout kernels (csrc/kernels/rollout.hip): env physics, episode
bookkeeping and the ``ep_stats`` rows, in numpy, with no GPU.

* Env oracles for the five device envs, written from the gymnasium equations (CartPole-v1,
  MountainCar-v0, Acrobot-v1 "book" dynamics under one RK4 step) and from the env descriptions in
  ``csrc/kernels/envs.h`` (LunarLanderSynth, HalfCheetahSynth).  Each has ``reset(u)``,
  ``obs(state)``, ``state_from_obs(obs)`` and ``step(state, act, noise, dtype)`` which returns the
  next state, the reward, ``terminated`` and a *margin*: the distance of the decisive quantity from
  the nearest threshold the step compares against.  A cell whose margin is below ``EPS`` may
  legitimately fall on either side in fp32, so the done-code check leaves it out.
* ``dtype=np.float64`` is the reference.  ``np.float32`` runs the same formulas in the device's
  precision and is used only to size tolerances (``measure_f32_vs_f64``).  Decimal constants are
  the device's fp32 literals in both, so the two differ by rounding alone.
* ``replay`` is a one-step replay of a finished device rollout: at every t the state is re-synced
  from the device's ``obs[t]`` and stepped with the device's recorded action, so nothing drifts.
* ``episode_stats`` recomputes the six ``ep_stats`` quantities and the persistent ``ep_len`` /
  ``ep_ret`` from the device's own ``rew`` and ``done`` buffers.
* ``INJECTED`` is the table of hand-built boundary states that ``reset_all = 0`` feeds the kernels
  (decision branches a random policy never reaches); ``test_rollout_oracle.py`` proves on the CPU
  that each gives its intended outcome for every action.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from relayrl_prototype_amd.ops import philox

EPS = 1e-4            # margin below which a done code is not compared
MAX_SKIP_SHARE = 0.005  # at most 0.5 % of the cells of a case may be skipped that way
F32_ULP = 2.0 ** -23


def _consts(dtype):
    """c(v): the fp32 literal v, held in ``dtype``."""
    return lambda v: dtype(np.float32(v))


def _u(seed, step, envs, tag):
    return np.stack(philox.uniforms(seed, step, envs, tag), 1)  # [n, 4] float32


class _Env:
    continuous = False
    terminates = True

    @classmethod
    def reset_uniforms(cls, seed, step, envs):
        """The draws of the reset at counter ``(env, step, tag 1)``."""
        return _u(seed, step, envs, 1)

    @classmethod
    def done_reset_uniforms(cls, seed, gstep, envs):
        """The draws of the reset that follows a done at global step ``gstep``."""
        return cls.reset_uniforms(seed, gstep, envs)

    @classmethod
    def step_noise(cls, seed, gstep, envs):
        """The env noise of global step ``gstep``: the second word of the action draw (tag 0)."""
        return philox.uniforms(seed, gstep, envs, 0)[1]

    @classmethod
    def obs(cls, state):
        return np.asarray(state)

    @classmethod
    def state_from_obs(cls, obs):
        return np.asarray(obs, np.float64)


class CartPole(_Env):
    env_id, name, D, A, NS, max_steps = 0, "CartPole-v1", 4, 2, 4, 500
    obs_tol = dict(rtol=1e-4, atol=1e-5)
    rew_tol = dict(rtol=0, atol=0)

    @classmethod
    def reset(cls, u):
        c = _consts(np.float64)
        return c(-0.05) + c(0.1) * np.asarray(u, np.float64)

    @classmethod
    def step(cls, state, act, noise=None, dtype=np.float64):
        c = _consts(dtype)
        x, xd, th, thd = np.asarray(state, dtype).T
        gravity, masspole, total_mass, length, tau = c(9.8), c(0.1), c(1.1), c(0.5), c(0.02)
        pml = masspole * length
        force = np.where(np.asarray(act) == 1, c(10), c(-10))
        ct, st = np.cos(th), np.sin(th)
        temp = (force + pml * thd * thd * st) / total_mass
        thacc = (gravity * st - ct * temp) / (length * (c(4.0 / 3.0) - masspole * ct * ct / total_mass))
        xacc = temp - pml * thacc * ct / total_mass
        ns = np.stack([x + tau * xd, xd + tau * xacc, th + tau * thd, thd + tau * thacc], 1)
        lim = np.float64(np.float32(12 * 2) * np.float32(np.pi) / np.float32(360))
        dx = np.abs(ns[:, 0].astype(np.float64)) - np.float64(np.float32(2.4))
        dth = np.abs(ns[:, 2].astype(np.float64)) - lim
        term = (dx > 0) | (dth > 0)
        margin = np.minimum(np.abs(dx), np.abs(dth))
        return ns, np.ones(len(ns), dtype), term, margin


class MountainCar(_Env):
    env_id, name, D, A, NS, max_steps = 1, "MountainCar-v0", 2, 3, 2, 200
    bounds = np.array([1.2, 0.07])  # |pos|, |vel|

    @classmethod
    def reset(cls, u):
        c = _consts(np.float64)
        u = np.asarray(u, np.float64)
        return np.stack([c(-0.6) + c(0.2) * u[:, 0], np.zeros(len(u))], 1)

    @classmethod
    def step(cls, state, act, noise=None, dtype=np.float64):
        c = _consts(dtype)
        pos, vel = np.asarray(state, dtype).T
        vel = vel + (np.asarray(act) - 1).astype(dtype) * c(0.001) + np.cos(c(3) * pos) * c(-0.0025)
        vel = np.clip(vel, c(-0.07), c(0.07))
        pos = np.clip(pos + vel, c(-1.2), c(0.6))
        vel = np.where((pos == c(-1.2)) & (vel < 0), dtype(0), vel)  # inelastic left wall
        term = pos >= c(0.5)
        margin = np.abs(pos.astype(np.float64) - 0.5)
        return np.stack([pos, vel], 1), np.full(len(pos), -1, dtype), term, margin


class Acrobot(_Env):
    env_id, name, D, A, NS, max_steps = 2, "Acrobot-v1", 6, 3, 4, 500
    bounds = np.array([1, 1, 1, 1, 4 * np.pi, 9 * np.pi])  # cos, sin, cos, sin, dtheta1, dtheta2

    @classmethod
    def reset(cls, u):
        c = _consts(np.float64)
        return c(-0.1) + c(0.2) * np.asarray(u, np.float64)

    @classmethod
    def obs(cls, state):
        s = np.asarray(state)
        return np.stack([np.cos(s[:, 0]), np.sin(s[:, 0]), np.cos(s[:, 1]), np.sin(s[:, 1]), s[:, 2], s[:, 3]], 1)

    @classmethod
    def state_from_obs(cls, obs):
        o = np.asarray(obs, np.float64)
        return np.stack([np.arctan2(o[:, 1], o[:, 0]), np.arctan2(o[:, 3], o[:, 2]), o[:, 4], o[:, 5]], 1)

    @staticmethod
    def _dsdt(th1, th2, d1_, d2_, torque, c):
        # gymnasium AcrobotEnv._dsdt, book_or_nips = "book", all masses, lengths and inertias 1,
        # centres of mass at 0.5
        m1 = m2 = l1 = i1 = i2 = c(1)
        lc1 = lc2 = c(0.5)
        g, half_pi = c(9.8), c(np.pi / 2)
        d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + c(2) * l1 * lc2 * np.cos(th2)) + i1 + i2
        d2 = m2 * (lc2 * lc2 + l1 * lc2 * np.cos(th2)) + i2
        phi2 = m2 * lc2 * g * np.cos(th1 + th2 - half_pi)
        phi1 = (-m2 * l1 * lc2 * d2_ * d2_ * np.sin(th2) - c(2) * m2 * l1 * lc2 * d2_ * d1_ * np.sin(th2)
                + (m1 * lc1 + m2 * l1) * g * np.cos(th1 - half_pi) + phi2)
        dd2 = (torque + d2 / d1 * phi1 - m2 * l1 * lc2 * d1_ * d1_ * np.sin(th2) - phi2) / (
            m2 * lc2 * lc2 + i2 - d2 * d2 / d1)
        dd1 = -(d2 * dd2 + phi1) / d1
        return np.stack([d1_, d2_, dd1, dd2], 1)

    @classmethod
    def step_unbounded(cls, state, act, dtype=np.float64):
        """One RK4 step of 0.2 s, before the angle wrap and the velocity clamps."""
        c = _consts(dtype)
        y0 = np.asarray(state, dtype)
        torque = (np.asarray(act) - 1).astype(dtype)
        f = lambda y: cls._dsdt(y[:, 0], y[:, 1], y[:, 2], y[:, 3], torque, c)  # noqa: E731
        dt = c(0.2)
        k1 = f(y0)
        k2 = f(y0 + c(0.5) * dt * k1)
        k3 = f(y0 + c(0.5) * dt * k2)
        k4 = f(y0 + dt * k3)
        return y0 + dt / c(6) * (k1 + c(2) * k2 + c(2) * k3 + k4)

    @classmethod
    def step(cls, state, act, noise=None, dtype=np.float64):
        c = _consts(dtype)
        ns = cls.step_unbounded(state, act, dtype)
        pi = c(np.pi)
        for k in (0, 1):
            a = ns[:, k]
            for _ in range(3):  # |dtheta| dt < 2 pi: one turn at the most; three for injected states
                a = np.where(a > pi, a - c(2) * pi, a)
                a = np.where(a < -pi, a + c(2) * pi, a)
            ns[:, k] = a
        v1, v2 = dtype(np.float32(4) * np.float32(np.pi)), dtype(np.float32(9) * np.float32(np.pi))
        ns[:, 2] = np.clip(ns[:, 2], -v1, v1)
        ns[:, 3] = np.clip(ns[:, 3], -v2, v2)
        height = -np.cos(ns[:, 0]) - np.cos(ns[:, 1] + ns[:, 0])
        term = height > c(1)
        margin = np.abs(height.astype(np.float64) - 1.0)
        return ns, np.where(term, dtype(0), dtype(-1)), term, margin


class LunarLanderSynth(_Env):
    """Point-mass lander: gravity 10/6 per 1/50 s step scaled by 6, main engine 13/6 along the body
    axis, side engines 0.6/6 laterally and 1.5 of angular acceleration, lateral noise
    U(-0.05, 0.05); gymnasium's potential shaping with a +20 leg term below y = 0.05; +-100 on
    touchdown (soft inside four bounds) and -100 out of bounds."""
    env_id, name, D, A, NS, max_steps = 3, "LunarLanderSynth-v0", 8, 4, 7, 1000
    obs_tol = dict(rtol=1e-4, atol=1e-4)
    rew_tol = dict(rtol=1e-3, atol=1e-3)

    @staticmethod
    def _shaping(x, y, vx, vy, ang, c):
        legs = np.where(y < c(0.05), c(20), c(0))
        return c(-100) * np.sqrt(x * x + y * y) - c(100) * np.sqrt(vx * vx + vy * vy) - c(100) * np.abs(ang) + legs

    @classmethod
    def reset(cls, u):
        c = _consts(np.float64)
        u = np.asarray(u, np.float64)
        s = np.zeros((len(u), 7))
        s[:, 0] = c(-0.3) + c(0.6) * u[:, 0]
        s[:, 1] = c(1.4)
        s[:, 2] = c(-0.5) + u[:, 1]
        s[:, 3] = c(-0.3) + c(0.3) * u[:, 2]
        s[:, 4] = c(-0.1) + c(0.2) * u[:, 3]
        s[:, 6] = cls._shaping(s[:, 0], s[:, 1], s[:, 2], s[:, 3], s[:, 4], c)
        return s

    @classmethod
    def obs(cls, state):
        s = np.asarray(state)
        leg = (s[:, 1] < np.float32(0.05)).astype(s.dtype)
        return np.concatenate([s[:, :6], leg[:, None], leg[:, None]], 1)

    @classmethod
    def state_from_obs(cls, obs):
        o = np.asarray(obs, np.float64)
        sh = cls._shaping(o[:, 0], o[:, 1], o[:, 2], o[:, 3], o[:, 4], _consts(np.float64))
        return np.concatenate([o[:, :6], sh[:, None]], 1)

    @classmethod
    def step(cls, state, act, noise, dtype=np.float64):
        c = _consts(dtype)
        x, y, vx, vy, ang, angv, prev = np.asarray(state, dtype).T
        act = np.asarray(act)
        main, side = act == 2, (act == 1) | (act == 3)
        direction = np.where(act == 1, c(-1), c(1))
        dt = c(1) / c(50)
        ax = np.where(main, -np.sin(ang) * c(13) / c(6), np.where(side, direction * np.cos(ang) * c(0.6) / c(6), c(0)))
        ay = c(-10) / c(6) + np.where(main, np.cos(ang) * c(13) / c(6), c(0))
        aa = np.where(side, -direction * c(1.5), c(0))
        fuel = np.where(main, c(0.3), np.where(side, c(0.03), c(0)))
        ax = ax + (c(-0.05) + c(0.1) * np.asarray(noise).astype(dtype))
        vx = vx + ax * dt * c(6)
        vy = vy + ay * dt * c(6)
        angv = angv + aa * dt
        x = x + vx * dt
        y = y + vy * dt
        ang = ang + angv * dt
        sh = cls._shaping(x, y, vx, vy, ang, c)
        rew = sh - prev - fuel
        ground = y <= 0
        oob = np.abs(x) >= 1
        soft = (np.abs(vy) < c(0.5)) & (np.abs(vx) < c(0.5)) & (np.abs(ang) < c(0.3)) & (np.abs(x) < c(0.5))
        rew = rew + np.where(ground, np.where(soft, c(100), c(-100)), np.where(oob, c(-100), c(0)))
        d = lambda v: np.abs(v.astype(np.float64))  # noqa: E731
        margin = np.minimum.reduce([d(y), np.abs(d(x) - 1.0), np.abs(y.astype(np.float64) - 0.05)])
        landing = np.minimum.reduce([np.abs(d(vy) - 0.5), np.abs(d(vx) - 0.5), np.abs(d(ang) - 0.3),
                                     np.abs(d(x) - 0.5)])
        margin = np.where(ground, np.minimum(margin, landing), margin)
        y = np.where(ground, dtype(0), y)
        return np.stack([x, y, vx, vy, ang, angv, sh], 1), rew, ground | oob, margin


class HalfCheetahSynth(_Env):
    """s' = tanh(A s + B clip(u, -1, 1)) + U(-0.01, 0.01), reward s'[8] - 0.1 |clip(u)|^2; the env
    only truncates.  Noise: 17 of the 20 uniforms of tags 8..12; resets: tags 16..20, and after a
    truncation at counter gstep + 2**32."""
    env_id, name, D, A, NS, max_steps = 4, "HalfCheetahSynth-v0", 17, 6, 17, 1000
    continuous, terminates = True, False
    obs_tol = dict(rtol=1e-4, atol=1e-4)
    rew_tol = dict(rtol=1e-4, atol=1e-4)
    _mats = None

    @classmethod
    def constants(cls):
        from relayrl_prototype_amd import _native

        return np.asarray(_native.env_constants(cls.name), np.float32)

    @classmethod
    def matrices(cls):
        if cls._mats is None:
            k = cls.constants()
            cls._mats = (k[:289].reshape(17, 17), k[289:].reshape(17, 6))
        return cls._mats

    @classmethod
    def reset_uniforms(cls, seed, step, envs):
        return np.concatenate([_u(seed, step, envs, 16 + q) for q in range(5)], 1)[:, :17]

    @classmethod
    def done_reset_uniforms(cls, seed, gstep, envs):
        return cls.reset_uniforms(seed, gstep + 2 ** 32, envs)

    @classmethod
    def step_noise(cls, seed, gstep, envs):
        return np.concatenate([_u(seed, gstep, envs, 8 + q) for q in range(5)], 1)[:, :17]

    @classmethod
    def reset(cls, u):
        c = _consts(np.float64)
        return c(-0.1) + c(0.2) * np.asarray(u, np.float64)

    @classmethod
    def step(cls, state, act, noise, dtype=np.float64):
        c = _consts(dtype)
        am, bm = (m.astype(dtype) for m in cls.matrices())
        s = np.asarray(state, dtype)
        u = np.clip(np.asarray(act).astype(dtype), c(-1), c(1))
        ns = np.tanh(s @ am.T + u @ bm.T) + (c(-0.01) + c(0.02) * np.asarray(noise).astype(dtype))
        rew = ns[:, 8] - c(0.1) * (u * u).sum(1)
        return ns, rew, np.zeros(len(ns), bool), np.full(len(ns), np.inf)


ENVS = {e.env_id: e for e in (CartPole, MountainCar, Acrobot, LunarLanderSynth, HalfCheetahSynth)}
ENVS.update({e.name: e for e in list(ENVS.values())})


def env_of(env):
    return env if isinstance(env, type) else ENVS[env]


# ------------------------------------------------------------------ MountainCar / Acrobot tolerances
# Nobody had measured these two envs, so their tolerances come from the oracle itself: the largest
# difference between its float32 and its float64 one-step prediction (measure_f32_vs_f64), over the
# inputs of the full-rollout cases and of the injected states, per observation component.  The
# tolerance is 8 x that difference -- the device rounds sinf / cosf differently and contracts
# multiply-adds, over the ~40 dependent operations of an RK4 step -- and never less than 4 ulp of
# the component's bound (1 for cos / sin, 4 pi and 9 pi for the Acrobot velocities, 1.2 and 0.07
# for MountainCar).  The rewards of both envs are the constants -1 / 0: float32 and float64 agree
# exactly, and the comparison is exact.
#
# Measured (517 envs x 24 steps at max_steps 9, plus both steps of the injected launches under
# every pair of actions):
#   MountainCar  pos 4.59e-08   vel 3.50e-09   (reward 0)
#   Acrobot      cos1 2.73e-07  sin1 4.46e-07  cos2 6.05e-07  sin2 1.13e-06  dth1 5.94e-05  dth2 4.29e-05
#                (reward 0; the velocity figures come from the step after the injected 9 pi state,
#                where the accelerations reach 1e3 rad/s^2; the rollout cases alone give 4e-06)
# 4 ulp of the bounds: 5.72e-07 (1.2), 3.34e-08 (0.07), 4.77e-07 (1), 5.99e-06 (4 pi), 1.35e-05 (9 pi)
# Resulting absolute tolerances (derived_atol):
#   MountainCar  pos 5.72e-07   vel 3.34e-08
#   Acrobot      cos1 2.18e-06  sin1 3.57e-06  cos2 4.84e-06  sin2 9.04e-06  dth1 4.75e-04  dth2 3.43e-04
MEASURED_F32_VS_F64 = {
    "MountainCar-v0": np.array([4.59e-08, 3.50e-09]),
    "Acrobot-v1": np.array([2.73e-07, 4.46e-07, 6.05e-07, 1.13e-06, 5.94e-05, 4.29e-05]),
}


def derived_atol(env):
    """Per-component absolute tolerance of MountainCar / Acrobot observations."""
    e = env_of(env)
    return np.maximum(8.0 * MEASURED_F32_VS_F64[e.name], 4.0 * F32_ULP * e.bounds)


def obs_close(env, got, want):
    """Elementwise: does the device observation ``got`` match the oracle's ``want``?"""
    e = env_of(env)
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if hasattr(e, "obs_tol"):
        return np.abs(got - want) <= e.obs_tol["atol"] + e.obs_tol["rtol"] * np.abs(want)
    return np.abs(got - want) <= derived_atol(e)


def rew_close(env, got, want):
    e = env_of(env)
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = getattr(e, "rew_tol", dict(rtol=0, atol=0))
    return np.abs(got - want) <= tol["atol"] + tol["rtol"] * np.abs(want)


def measure_f32_vs_f64(env, obs, act, noise=None):
    """Largest |float32 - float64| one-step prediction of the oracle, per observation component
    and for the reward, from the same inputs (the reference against itself)."""
    e = env_of(env)
    s = e.state_from_obs(obs)
    n64, r64, _, _ = e.step(s, act, noise, np.float64)
    n32, r32, _, _ = e.step(s.astype(np.float32), act, noise, np.float32)
    d = np.abs(e.obs(n32).astype(np.float64) - e.obs(n64))
    return d.max(0), float(np.abs(r32.astype(np.float64) - r64).max())


# ------------------------------------------------------------------ replay of a device rollout
def replay(env, bufs, seed, step0, max_steps, state_in=None, len_in=None, ret_in=None, has_tobs=True):
    """One-step replay of a finished device rollout.  ``bufs`` holds the device's ``obs``
    [T+1, N, D], ``act``, ``rew`` and ``done`` [T, N] as numpy arrays; ``state_in`` / ``len_in`` /
    ``ret_in`` are the persistent inputs of a ``reset_all = 0`` launch (None: ``reset_all = 1``).

    Per (t, env): ``pred_obs`` the oracle's next observation from the device's ``obs[t]`` and
    action, ``rew``, ``term``, ``margin``, the expected done ``code``, ``reset_obs`` the
    observation of the Philox reset a done at t is followed by, and ``len`` / ``ret`` of the
    running episode after step t.  The bookkeeping follows the *device's* done buffer, so a
    disputed termination affects one cell and not the rest of its column.  ``obs0`` is the expected
    first observation, ``state_out`` / ``len_out`` / ``ret_out`` the expected persistent outputs.
    """
    e = env_of(env)
    obs, act, rew, done = (np.asarray(bufs[k]) for k in ("obs", "act", "rew", "done"))
    T, N = done.shape
    envs = np.arange(N)
    if state_in is None:
        s0 = e.reset(e.reset_uniforms(seed, step0, envs))
        ln, rt = np.zeros(N, np.int64), np.zeros(N)
    else:
        s0 = np.asarray(state_in, np.float64)
        ln, rt = np.asarray(len_in, np.int64).copy(), np.asarray(ret_in, np.float64).copy()
    out = dict(obs0=e.obs(s0), pred_obs=np.zeros((T, N, e.D)), rew=np.zeros((T, N)), term=np.zeros((T, N), bool),
               margin=np.zeros((T, N)), code=np.zeros((T, N), np.int64), reset_obs=np.zeros((T, N, e.D)),
               len=np.zeros((T, N), np.int64), ret=np.zeros((T, N)))
    state = s0
    for t in range(T):
        g = step0 + t
        ns, r, term, margin = e.step(e.state_from_obs(obs[t]), act[t], e.step_noise(seed, g, envs), np.float64)
        ln = ln + 1
        rt = rt + rew[t].astype(np.float64)
        trunc = ln >= max_steps
        rs = e.reset(e.done_reset_uniforms(seed, g, envs))
        out["pred_obs"][t], out["rew"][t], out["term"][t], out["margin"][t] = e.obs(ns), r, term, margin
        out["code"][t] = np.where(term, 1, np.where(trunc, 2 if has_tobs else 1, 0))
        out["reset_obs"][t] = e.obs(rs)
        out["len"][t], out["ret"][t] = ln, rt
        d = done[t] > 0
        state = np.where(d[:, None], rs, ns)
        ln = np.where(d, 0, ln)
        rt = np.where(d, 0.0, rt)
    out.update(state_out=state, len_out=ln, ret_out=rt)
    return out


def _all(mask, what):
    mask = np.asarray(mask)
    if not mask.all():
        bad = np.argwhere(~mask)
        raise AssertionError(f"{what}: {len(bad)} of {mask.size} cells differ, first at {tuple(bad[0])}")


def assert_replay(env, bufs, rp):
    """Hold a device rollout (``bufs`` as for ``replay``, plus ``tobs`` [T, N, D] pre-filled with
    NaN, or None) to its replay ``rp``; returns the share of cells whose done code was not
    compared (margin <= EPS), which must not exceed MAX_SKIP_SHARE."""
    e = env_of(env)
    obs, rew, done = (np.asarray(bufs[k]) for k in ("obs", "rew", "done"))
    tobs = bufs.get("tobs")
    _all(np.isin(done, (0, 1, 2)), "done codes")
    _all(np.abs(obs[0] - rp["obs0"]) <= 1e-6, "obs[0] vs the initial state")
    live = done == 0
    _all(obs_close(e, obs[1:], rp["pred_obs"])[live], "obs[t+1] vs the oracle step (running rows)")
    _all((np.abs(obs[1:] - rp["reset_obs"]) <= 1e-6)[~live], "obs[t+1] vs the Philox reset (done rows)")
    _all(rew_close(e, rew, rp["rew"]), "reward, terminal rows included")
    sure = rp["margin"] > EPS
    _all((done == rp["code"])[sure], "done code")
    share = float((~sure).mean())
    assert share <= MAX_SKIP_SHARE, f"{share:.4%} of the cells lie within {EPS} of a threshold: pick another seed"
    if tobs is None:
        _all(done != 2, "code 2 without tobs")
    else:
        boot = done == 2
        _all(np.isnan(np.asarray(tobs)[~boot]), "tobs written where done != 2")
        _all(obs_close(e, tobs, rp["pred_obs"])[boot], "tobs vs the pre-reset observation")
    return share


def episode_stats(rew, done, len_in=None, ret_in=None):
    """The episodes a rollout finished, from the device's ``rew`` and ``done`` [T, N]: ``env``,
    ``t``, ``len`` and ``ret`` of each, where ``ret`` is the running fp32 sum the kernel keeps
    (``ret += r`` per step, from ``ret_in``), which float32 addition reproduces bit for bit.  The
    six ``ep_stats`` quantities are float64 reductions of those values; ``ep_len`` / ``ep_ret``
    are the expected persistent outputs."""
    rew, done = np.asarray(rew, np.float32), np.asarray(done)
    T, N = rew.shape
    ln = np.zeros(N, np.int64) if len_in is None else np.asarray(len_in, np.int64).copy()
    rt = np.zeros(N, np.float32) if ret_in is None else np.asarray(ret_in, np.float32).copy()
    ep = dict(env=[], t=[], len=[], ret=[])
    for t in range(T):
        ln = ln + 1
        rt = (rt + rew[t]).astype(np.float32)
        d = np.nonzero(done[t] > 0)[0]
        ep["env"].append(d)
        ep["t"].append(np.full(len(d), t))
        ep["len"].append(ln[d])
        ep["ret"].append(rt[d])
        ln[d] = 0
        rt[d] = 0
    ep = {k: np.concatenate(v) for k, v in ep.items()}
    r64 = ep["ret"].astype(np.float64)
    n = len(r64)
    return dict(episodes=ep, n_done=n, sum_ret=r64.sum(), sumsq_ret=(r64 * r64).sum(),
                max_ret=r64.max() if n else -np.inf, min_ret=r64.min() if n else np.inf,
                sum_len=int(ep["len"].sum()), ep_len=ln, ep_ret=rt)


def stats_rows(ep, row_of_env, lane_of_env, grid):
    """Expected ``ep_stats`` [grid, 6] (float64) when env i reports into row ``row_of_env[i]``, and
    the largest number of episodes any one lane (``lane_of_env``) accumulated."""
    rows = np.zeros((grid, 6))
    rows[:, 3], rows[:, 4] = -np.inf, np.inf
    r64 = ep["ret"].astype(np.float64)
    for k in range(len(r64)):
        b = row_of_env[ep["env"][k]]
        rows[b, 0] += 1
        rows[b, 1] += r64[k]
        rows[b, 2] += r64[k] * r64[k]
        rows[b, 3] = max(rows[b, 3], r64[k])
        rows[b, 4] = min(rows[b, 4], r64[k])
        rows[b, 5] += ep["len"][k]
    per_lane = np.bincount(np.asarray(lane_of_env)[ep["env"]]) if len(r64) else np.zeros(1, np.int64)
    return rows, int(per_lane.max())


# ------------------------------------------------------------------ CPU stand-in for a device rollout
def simulate(env, params, H, N, T, seed, step0, max_steps, has_tobs=True, state_in=None, len_in=None, ret_in=None):
    """The rollout the device would produce, from the oracle in float32 and the fp32 policy
    oracle (``ops.reference.mlp_forward_ref``): same Philox resets, action draws and noise.  Not a
    reference (an action can differ where a logit rounds differently, and Gaussian actions use
    numpy's normals); it provides, without a GPU, the inputs of the full-rollout cases for the
    tolerance measurement and the margin statistics, and buffers of the device's shapes and
    dtypes to try the GPU tests' assertions on."""
    import torch

    from relayrl_prototype_amd.ops import reference as ref

    e = env_of(env)
    envs = np.arange(N)
    f32 = np.float32
    if state_in is None:
        s = e.reset(e.reset_uniforms(seed, step0, envs)).astype(f32)
        ln = np.zeros(N, np.int64)
    else:
        s, ln = np.asarray(state_in, f32), np.asarray(len_in, np.int64).copy()
    obs = np.zeros((T + 1, N, e.D), f32)
    tobs = np.full((T, N, e.D), np.nan, f32)
    act = np.zeros((T, N, e.A), f32) if e.continuous else np.zeros((T, N), np.int32)
    rew, done, logp = np.zeros((T, N), f32), np.zeros((T, N), f32), np.zeros((T, N), f32)
    for t in range(T):
        g = step0 + t
        obs[t] = e.obs(s)
        x = torch.from_numpy(obs[t])
        if e.continuous:
            mu = ref.mlp_forward_ref(3, params, x, e.A, H)["logits"].numpy()
            act[t] = mu + np.random.default_rng(g).standard_normal(mu.shape).astype(f32)
        else:
            r = ref.mlp_forward_ref(1, params, x, e.A, H, seed=seed, step=g)
            act[t], logp[t] = r["act"].numpy(), r["logp"].numpy()
        ns, r, term, _ = e.step(s, act[t], e.step_noise(seed, g, envs), f32)
        ln += 1
        trunc = ln >= max_steps
        rew[t] = r
        done[t] = np.where(term, 1, np.where(trunc, 2 if has_tobs else 1, 0))
        d = done[t] > 0
        tobs[t][done[t] == 2] = e.obs(ns.astype(f32))[done[t] == 2]
        rs = e.reset(e.done_reset_uniforms(seed, g, envs)).astype(f32)
        s = np.where(d[:, None], rs, ns.astype(f32))
        ln[d] = 0
    obs[T] = e.obs(s)
    st = episode_stats(rew, done, len_in, ret_in)
    return dict(obs=obs, act=act, logp=logp, rew=rew, done=done, tobs=tobs, state=s, ep_len=st["ep_len"].astype(np.int32),
                ep_ret=st["ep_ret"])


# The full-rollout cases: short time limits so that every env ends episodes inside T steps (the
# Lander lands by itself around step 26).  CartPole's counter crosses 2**32 inside the rollout and
# Acrobot's seed has high bits, for the 64-bit halves of the Philox counter and key.
CASES = {
    "CartPole-v1": dict(max_steps=12, T=48, seed=777, step0=2 ** 32 - 7),
    "MountainCar-v0": dict(max_steps=9, T=24, seed=31, step0=0),
    "Acrobot-v1": dict(max_steps=9, T=24, seed=(5 << 32) | 19, step0=640),
    "LunarLanderSynth-v0": dict(max_steps=1000, T=40, seed=5, step0=0),
    "HalfCheetahSynth-v0": dict(max_steps=4, T=10, seed=11, step0=3),
}


def case_params(env, H, device=None):
    """The policy weights of a case (seeded init), as the flat fp32 tensor the kernels take."""
    import torch

    from relayrl_prototype_amd.ops import MLPSpec

    e = env_of(env)
    p = MLPSpec(e.D, H, e.A, gaussian=e.continuous).init(torch.Generator().manual_seed(3 + e.env_id))
    return p if device is None else p.to(device)


# ------------------------------------------------------------------ injected boundary states
@dataclass
class Scenario:
    """A hand-built state for a ``reset_all = 0`` launch whose first step has one outcome for
    every action.  ``state`` holds the physical state (Lander: without prev_shaping, which
    ``injected_inputs`` fills in).  ``at_limit`` puts the episode one step short of the time limit.
    ``check(next_state, reward)`` states the intended effect on the oracle's output."""
    name: str
    state: tuple
    term: bool
    at_limit: bool = False
    ep_ret: float = 0.0
    check: Optional[Callable] = None
    two_steps: bool = False  # the effect shows in the persistent state after a second, uneventful step

    def code(self, has_tobs=True):
        return 1 if self.term else ((2 if has_tobs else 1) if self.at_limit else 0)


_PI32 = float(np.float32(np.pi))
_TH_LIM = 12 * 2 * np.pi / 360

MID = {
    "CartPole-v1": (0.01, -0.02, 0.015, 0.01),
    "MountainCar-v0": (-0.5, 0.005),
    "Acrobot-v1": (0.05, -0.04, 0.02, 0.03),
    "LunarLanderSynth-v0": (0.05, 1.0, 0.1, -0.1, 0.02, 0.0),
    "HalfCheetahSynth-v0": tuple(0.05 * ((-1) ** k) * (1 + k % 3) / 3 for k in range(17)),
}

_soft = (0.1, 0.002, 0.05, -0.25, 0.02, 0.0)


def _lander(**kw):
    s = dict(zip(("x", "y", "vx", "vy", "ang", "angv"), _soft))
    s.update(kw)
    return tuple(s.values())


INJECTED = {
    "CartPole-v1": [
        Scenario("x_out", (2.399, 1.0, 0.0, 0.0), True, ep_ret=7.0, check=lambda s, r: s[0] > 2.4),
        Scenario("theta_out", (0.0, 0.0, 0.2090, 0.5), True, ep_ret=3.0, check=lambda s, r: s[2] > _TH_LIM),
        Scenario("x_out_neg", (-2.399, -1.0, 0.0, 0.0), True, check=lambda s, r: s[0] < -2.4),
        Scenario("theta_out_neg", (0.0, 0.0, -0.2090, -0.5), True, check=lambda s, r: s[2] < -_TH_LIM),
        Scenario("time_limit", MID["CartPole-v1"], False, at_limit=True, ep_ret=41.0),
        Scenario("term_at_limit", (2.399, 1.0, 0.0, 0.0), True, at_limit=True, ep_ret=41.0),
    ],
    "MountainCar-v0": [
        Scenario("flag", (0.495, 0.06), True, ep_ret=-150.0, check=lambda s, r: s[0] >= 0.5),
        Scenario("left_wall", (-1.195, -0.06), False,
                 check=lambda s, r: s[0] == float(np.float32(-1.2)) and s[1] == 0.0),
        Scenario("vel_clamp_hi", (-1.047, 0.0695), False, check=lambda s, r: s[1] == float(np.float32(0.07))),
        Scenario("vel_clamp_lo", (0.0, -0.0695), False, check=lambda s, r: s[1] == float(np.float32(-0.07))),
        Scenario("time_limit", MID["MountainCar-v0"], False, at_limit=True, ep_ret=-48.0),
        Scenario("term_at_limit", (0.495, 0.06), True, at_limit=True, ep_ret=-48.0),
    ],
    "Acrobot-v1": [
        # the tip is below the bar height (-cos th1 - cos(th1 + th2) = 0.65) and swinging up
        Scenario("swing_up", (1.9, 0.0, 3.0, 0.0), True, ep_ret=-30.0, check=lambda s, r: r == 0.0),
        # second link folded back, so the tip stays low while the first angle passes +-pi
        Scenario("wrap_pos", (3.1, 3.0, 2.0, -2.0), False, two_steps=True, check=lambda s, r: s[0] < 0),
        Scenario("wrap_neg", (-3.1, -3.0, -2.0, 2.0), False, two_steps=True, check=lambda s, r: s[0] > 0),
        # gravity (dth1) resp. the coupling (dth2) accelerates past the bound under every torque
        Scenario("clamp_dth1", (-2.6, 0.0, 4 * _PI32 - 0.01, 0.0), False,
                 check=lambda s, r: s[2] == float(np.float32(4) * np.float32(np.pi))),
        Scenario("clamp_dth2", (0.25, -0.3, 0.0, 9 * _PI32 - 0.01), False,
                 check=lambda s, r: s[3] == float(np.float32(9) * np.float32(np.pi))),
        Scenario("clamp_dth1_neg", (2.6, 0.0, -(4 * _PI32 - 0.01), 0.0), False,
                 check=lambda s, r: s[2] == -float(np.float32(4) * np.float32(np.pi))),
        Scenario("clamp_dth2_neg", (-0.25, 0.3, 0.0, -(9 * _PI32 - 0.01)), False,
                 check=lambda s, r: s[3] == -float(np.float32(9) * np.float32(np.pi))),
        Scenario("time_limit", MID["Acrobot-v1"], False, at_limit=True, ep_ret=-48.0),
        Scenario("term_at_limit", (1.9, 0.0, 3.0, 0.0), True, at_limit=True, ep_ret=-48.0),
    ],
    "LunarLanderSynth-v0": [
        # y = 0.002 and vy = -0.25 keep every action's touchdown inside the bounds: the free-fall
        # step adds -0.2 to vy (|vy| < 0.5 needs vy > -0.3) and the main engine lifts y by 0.0038
        Scenario("soft", _soft, True, ep_ret=12.5, check=lambda s, r: s[1] == 0.0 and r > 50),
        Scenario("hard", _lander(vy=-0.9), True, ep_ret=-3.0, check=lambda s, r: s[1] == 0.0 and r < -50),
        Scenario("tilted", _lander(ang=0.4), True, check=lambda s, r: s[1] == 0.0 and r < -50),
        Scenario("tilted_neg", _lander(ang=-0.4), True, check=lambda s, r: s[1] == 0.0 and r < -50),
        Scenario("out_of_bounds", (0.999, 1.0, 0.6, -0.1, 0.0, 0.0), True,
                 check=lambda s, r: s[0] >= 1.0 and s[1] > 0 and r < -50),
        # the leg flag sets and the shaping gains +20 (without it the reward would be below -15)
        Scenario("legs", (0.05, 0.052, 0.0, -0.3, 0.0, 0.0), False,
                 check=lambda s, r: 0 < s[1] < 0.05 and r > -5),
        Scenario("time_limit", MID["LunarLanderSynth-v0"], False, at_limit=True, ep_ret=-20.0),
        Scenario("term_at_limit", _soft, True, at_limit=True, ep_ret=-20.0),
    ],
    "HalfCheetahSynth-v0": [
        Scenario("time_limit", MID["HalfCheetahSynth-v0"], False, at_limit=True, ep_ret=1.75),
    ],
}


def injected_inputs(env, N, max_steps, tail=True):
    """(state [N, NS], ep_len [N], ep_ret [N], rows) of an injected launch: scenario k sits in row
    ``rows[k]`` (the last rows when ``tail``, so that a ragged last tile holds some), every other
    row holds the env's mid-range state three steps into an episode."""
    e = env_of(env)
    sc = INJECTED[e.name]
    phys = np.tile(np.asarray(MID[e.name], np.float64), (N, 1))
    ln = np.full(N, 3, np.int64)
    rt = np.full(N, -2.5)
    rows = [N - 1 - k for k in range(len(sc))] if tail else list(range(len(sc)))
    for k, s in zip(rows, sc):
        phys[k] = s.state
        ln[k] = max_steps - 1 if s.at_limit else 3
        rt[k] = s.ep_ret
    phys = phys.astype(np.float32).astype(np.float64)  # what the device will read
    state = e.state_from_obs(e.obs(phys)) if e is LunarLanderSynth else phys
    return state, ln, rt, rows
