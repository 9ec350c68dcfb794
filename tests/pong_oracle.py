"""Host oracle of the PongSynth step kernels (csrc/kernels/pong.hip): one env step, the episode
bookkeeping, the Philox serves and resets, and the two renders, in numpy, with no GPU.

Written from the rules of the env (``envs/pong.py`` docstring, the comments of ``pong.hip``), not
from ``PongRef``; ``tests/test_pong_oracle.py`` holds ``PongRef`` to it.

* The field is 84 x 84 with walls at y = 2 and y = 82; the ball is 2 x 2; the paddles (half-height
  5, width 2) stand at x = 76 (agent) and x = 6 (opponent) and stay inside [7, 77].  One step is 4
  sub-steps that stop at the first point.  Per sub-step: the agent moves 2.5 by its action, the
  opponent moves at most 1.6 towards ``by + 1`` while the ball approaches it and towards 42
  otherwise, the ball moves and bounces off the walls, then the contact gates, then the point test.
* ``step(state, act, seed, abs_step, max_steps, dtype)`` is vectorised over rows; ``abs_step`` and
  ``max_steps`` may differ per row, so a whole recorded run is one call.  ``dtype=np.float64`` is
  the reference; ``np.float32`` runs the same formulas in the device's precision and is used to
  size ``ATOL`` (``measure_f32_vs_f64``), to stand in for the device on the CPU (``simulate``) and
  for the hand-built ties that are exact only in float32.  Decimal constants are the device's
  fp32 literals in both, so the two differ by rounding alone.
* The *margin* of a row is the smallest distance, over the sub-steps it simulated, of a compared
  quantity from its threshold, computed in float64 from the float32 inputs (0 when a quantity sits
  on its threshold and no other is within ``EPS`` of its own).  A cell with
  ``0 < margin < EPS`` may fall on either side in fp32 and is not compared.  A margin of exactly 0
  IS compared: a tie of exactly representable inputs is a tie in both precisions, and the first
  approach after every serve (41 +- 1.5 * 22 = 74 or 8) sits on one, so these are the cells that
  tell ``>=`` from ``>``.
* ``replay`` is teacher-forced: every step is predicted from the device's own pre-step state,
  widened to float64, so a disagreement shows at the step where it happens and cannot compound.
  It is sound because the first state is held to the oracle's reset and every later state to a
  prediction from an already-checked one.
* ``render`` / ``frame`` are the observation ([N, 21, 21, 64] space-to-depth of the 4-frame stack)
  and the 7056-byte frame of the frame ring.  They hold float32 comparisons of single sums, no
  products, so FMA contraction cannot change them: the device must match byte for byte.
* ``SCENARIOS`` are the hand-built boundary states a ``reset_all = 0`` launch is fed.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable, Optional

import numpy as np

from relayrl_prototype_amd.ops import philox

from rollout_oracle import EPS, MAX_SKIP_SHARE  # noqa: F401  (the same skip rule and cap)

STATE = 32
BX, BY, VX, VY, PA, PO, SA, SO, T, RET, VALID = range(11)
HIST = 16
INT_SLOTS = [SA, SO, T, RET, VALID, 11, 12, 13, 14, 15]  # integer valued: compared exactly
CONT_SLOTS = [BX, BY, VX, VY, PA, PO] + list(range(HIST, HIST + 16))  # compared within ATOL
TAG_SERVE, TAG_RESET = 0x51, 0x52
FRAME_BYTES = 7056

# ATOL: the largest |float32 - float64| one-step prediction of this oracle (measure_f32_vs_f64)
# over the states of the two replay cases below (300 envs x 450 steps each, float32 stand-in runs)
# and of the injected launch is
#     2.06e-05   (a position after four sub-steps beyond 64, where half an ulp is 3.8e-6, moved by
#                 a velocity that itself carries a rounding)
# The device may also contract ``vy + 0.35 * (...)`` and ``30 + 24 * u`` into FMAs, which changes at
# most one rounding per expression -- the same order as float32 against float64 -- so the
# tolerance is 4 x the measurement.  tests/test_pong_oracle.py asserts measured <= ATOL / 4.
MEASURED_F32_VS_F64 = 2.07e-5
ATOL = 8.3e-5

f32 = np.float32
_M32 = 0xFFFFFFFF


def _consts(dtype):
    """c(v): the fp32 literal v, held in ``dtype``."""
    return lambda v: dtype(np.float32(v))


# ------------------------------------------------------------------ Philox draws
def words(seed, abs_step, envs, tag):
    """The 4 uint32 words of counter (env, step_lo, step_hi, tag) under key (seed_lo, seed_hi)."""
    envs = np.asarray(envs, np.uint64)
    st = np.broadcast_to(np.asarray(abs_step, dtype=np.uint64), envs.shape)
    full = lambda v: np.full(envs.shape, v, np.uint32)  # noqa: E731
    return philox.philox4x32((envs & np.uint64(_M32)).astype(np.uint32), (st & np.uint64(_M32)).astype(np.uint32),
                             (st >> np.uint64(32)).astype(np.uint32), full(tag), full(seed & _M32),
                             full((seed >> 32) & _M32))


def _serve(w, dtype):
    """(bx, by, vx, vy) of a serve from the words ``w``."""
    c = _consts(dtype)
    u0, u2 = philox.u01(w[0]).astype(dtype), philox.u01(w[2]).astype(dtype)
    by = c(30) + c(24) * u0
    vx = np.where((w[1] & np.uint32(1)) != 0, c(1.5), c(-1.5))
    vy = (u2 - c(0.5)) * c(3)
    return np.full(by.shape, c(41)), by, vx, vy


def _reset_rows(w, dtype):
    """The state a reset leaves: everything 0, paddles at 42, a serve, 4 copies of the frame."""
    bx, by, vx, vy = _serve(w, dtype)
    s = np.zeros((len(by), STATE), dtype)
    s[:, BX], s[:, BY], s[:, VX], s[:, VY] = bx, by, vx, vy
    s[:, PA] = s[:, PO] = 42
    for k in range(4):
        s[:, HIST + 4 * k:HIST + 4 * k + 4] = s[:, [BX, BY, PA, PO]]
    s[:, VALID] = 1
    return s


def reset_state(seed, abs_step, envs, tag=TAG_SERVE, dtype=np.float64):
    """``reset_all = 1`` draws tag 0x51; the reset that ends an episode draws tag 0x52."""
    return _reset_rows(words(seed, abs_step, envs, tag), dtype)


# ------------------------------------------------------------------ one step
OVER_AGENT, OVER_OPP, OVER_TIME = 1, 2, 4  # bits of rec.over


def _run(state, act, w_serve, w_reset, max_steps, dtype):
    c = _consts(dtype)
    s = np.array(state, dtype)
    n = len(s)
    bx, by, vx, vy, pa, po = (s[:, k].copy() for k in range(6))
    a = np.asarray(act).reshape(n)
    move = np.where((a == 2) | (a == 4), c(-1), np.where((a == 3) | (a == 5), c(1), c(0)))  # RIGHT = up
    pad_lo, pad_hi = c(2) + c(5), c(82) - c(5)
    reward = np.zeros(n, dtype)
    point_sub = np.full(n, -1)
    scorer = np.zeros(n, np.int64)  # +1 agent, -1 opponent
    hit = np.zeros((n, 4), np.int8)   # per sub-step: 1 agent paddle, 2 opponent paddle
    wall = np.zeros((n, 4), np.int8)  # per sub-step: bit 0 top, bit 1 bottom
    near, tie = np.full(n, np.inf), np.zeros(n, bool)  # the smallest non-zero distance; any exact tie
    d64 = lambda x, thr: np.abs(np.asarray(x, np.float64) - thr)  # noqa: E731
    for sub in range(4):
        live = point_sub < 0
        n_pa = np.clip(pa + move * c(2.5), pad_lo, pad_hi)
        target = np.where(vx < 0, by + c(1), c(42))
        n_po = np.clip(po + np.clip(target - po, -c(1.6), c(1.6)), pad_lo, pad_hi)
        n_bx, n_by, n_vy = bx + vx, by + vy, vy
        top = n_by < c(2)
        m = [d64(vx, 0.0), d64(n_by, 2.0)]
        n_by, n_vy = np.where(top, c(4) - n_by, n_by), np.where(top, -n_vy, n_vy)
        bot = n_by + c(2) > c(82)
        m.append(d64(n_by + c(2), 82.0))
        n_by, n_vy = np.where(bot, c(160) - n_by, n_by), np.where(bot, -n_vy, n_vy)
        cy = n_by + c(1)
        da, do = np.abs(cy - n_pa), np.abs(cy - n_po)
        hit_a = (vx > 0) & (n_bx + c(2) >= c(76)) & (bx + c(2) <= c(78)) & (da <= c(6))
        hit_o = ~hit_a & (vx < 0) & (n_bx <= c(8)) & (bx >= c(6)) & (do <= c(6))
        gates_a = np.minimum.reduce([d64(n_bx + c(2), 76.0), d64(bx + c(2), 78.0), d64(da, 6.0)])
        gates_o = np.minimum.reduce([d64(n_bx, 8.0), d64(bx, 6.0), d64(do, 6.0)])
        m.append(np.where(vx > 0, gates_a, gates_o))
        speed = np.minimum(np.abs(vx) * c(1.05), c(3))
        n_vx = np.where(hit_a, -speed, np.where(hit_o, speed, vx))
        n_vy = np.where(hit_a, np.clip(n_vy + c(0.35) * (cy - n_pa), -c(3), c(3)),
                        np.where(hit_o, np.clip(n_vy + c(0.35) * (cy - n_po), -c(3), c(3)), n_vy))
        n_bx = np.where(hit_a, c(74), np.where(hit_o, c(8), n_bx))
        opp = live & (n_bx > c(84))
        agent = live & ~opp & (n_bx + c(2) < c(0))
        m += [d64(n_bx, 84.0), d64(n_bx + c(2), 0.0)]
        m = np.stack(m)
        near = np.where(live, np.minimum(near, np.where(m > 0, m, np.inf).min(0)), near)
        tie |= live & (m == 0).any(0)
        pa, po = np.where(live, n_pa, pa), np.where(live, n_po, po)
        bx, by = np.where(live, n_bx, bx), np.where(live, n_by, by)
        vx, vy = np.where(live, n_vx, vx), np.where(live, n_vy, vy)
        hit[:, sub] = np.where(live, hit_a * 1 + hit_o * 2, 0)
        wall[:, sub] = np.where(live, top * 1 + bot * 2, 0)
        reward = reward + agent.astype(dtype) - opp.astype(dtype)
        scorer = scorer + agent - opp
        point_sub = np.where(opp | agent, sub, point_sub)
    # a tie counts as margin 0 only when nothing else in the step is within EPS of its threshold
    margin = np.where(near < EPS, near, np.where(tie, 0.0, near))
    point = point_sub >= 0
    sv = _serve(w_serve, dtype)
    bx, by, vx, vy = (np.where(point, x, y) for x, y in zip(sv, (bx, by, vx, vy)))
    s[:, BX], s[:, BY], s[:, VX], s[:, VY], s[:, PA], s[:, PO] = bx, by, vx, vy, pa, po
    s[:, SA] += scorer > 0
    s[:, SO] += scorer < 0
    s[:, T] += 1
    s[:, RET] += reward
    s[:, HIST:HIST + 12] = s[:, HIST + 4:HIST + 16].copy()
    s[:, HIST + 12:HIST + 16] = s[:, [BX, BY, PA, PO]]
    s[:, VALID] = np.minimum(s[:, VALID] + 1, 4)
    ms = np.broadcast_to(np.asarray(max_steps), (n,))
    why = OVER_AGENT * (s[:, SA] >= 21) + OVER_OPP * (s[:, SO] >= 21) + OVER_TIME * ((ms > 0) & (s[:, T] >= ms))
    over = why > 0
    ret, ln = s[:, RET].copy(), s[:, T].copy()
    acc = over[:, None] * np.stack([np.ones(n), ret, ln, ret * ret], 1).astype(np.float64)
    s = np.where(over[:, None], _reset_rows(w_reset, dtype), s)
    rec = SimpleNamespace(point_sub=point_sub, scorer=scorer, hit=hit, wall=wall, over=why)
    return SimpleNamespace(state=s, rew=reward, done=over.astype(dtype), fin_ret=np.where(over, ret, 0),
                           fin_len=np.where(over, ln, 0), acc=acc, margin=margin, rec=rec)


def step(state, act, seed, abs_step, max_steps, dtype=np.float64, envs=None):
    """One step of every row of ``state`` [n, 32] (float32 values) under ``act``: ``.state``,
    ``.rew``, ``.done``, ``.fin_ret``, ``.fin_len``, ``.acc`` (the ``ep_acc`` increment [n, 4],
    float64), ``.margin`` (always of the float64 run) and ``.rec``, the branch record: the point's
    sub-step (-1: none) and scorer, the paddle hit and the walls per sub-step, the reasons of
    ``over``.  Row i is env ``envs[i]`` (default i) at step counter ``abs_step`` (scalar or [n])."""
    state = np.asarray(state)
    envs = np.arange(len(state)) if envs is None else np.asarray(envs)
    w1, w2 = words(seed, abs_step, envs, TAG_SERVE), words(seed, abs_step, envs, TAG_RESET)
    out = _run(state, act, w1, w2, max_steps, np.float64)
    if dtype is not np.float64:
        margin = out.margin
        out = _run(state, act, w1, w2, max_steps, dtype)
        out.margin = margin
    return out


# ------------------------------------------------------------------ renders
def _image(h4):
    """[n, 84, 84] uint8 image of frames ``h4`` [n, 4] = (bx, by, pa, po): pixel (y, x) is tested
    at its centre (y + 0.5, x + 0.5), in float32."""
    h4 = np.asarray(h4, f32)
    bx, by, pa, po = (h4[:, k, None] for k in range(4))
    p = np.arange(84, dtype=f32) + f32(0.5)
    ball_rows, ball_cols = (p >= by) & (p < by + f32(2)), (p >= bx) & (p < bx + f32(2))
    pa_rows, po_rows = np.abs(p - pa) < f32(5), np.abs(p - po) < f32(5)
    pa_cols, po_cols = (p >= f32(76)) & (p < f32(78)), (p >= f32(6)) & (p < f32(8))
    lit = (ball_rows[:, :, None] & ball_cols[:, None, :]) | (pa_rows[:, :, None] & pa_cols[None, None, :]) | \
        (po_rows[:, :, None] & po_cols[None, None, :])
    walls = np.where((p < f32(2)) | (p >= f32(82)), np.uint8(100), np.uint8(0))
    return np.where(lit, np.uint8(255), walls[None, :, None]).astype(np.uint8)


def render(hist):
    """uint8 [N, 21, 21, 64]: obs[a][b][dy * 16 + dx * 4 + f] = frame f (oldest first) of the
    history rows ``hist`` [N, 16] at pixel (4a + dy, 4b + dx)."""
    hist = np.asarray(hist, f32).reshape(-1, 4, 4)
    n = len(hist)
    img = np.stack([_image(hist[:, f]) for f in range(4)], -1)  # [n, y, x, f]
    return np.ascontiguousarray(img.reshape(n, 21, 4, 21, 4, 4).transpose(0, 1, 3, 2, 4, 5)).reshape(n, 21, 21, 64)


def frame(hist_row):
    """The frame-ring frame of the newest history entry: uint8 [7056] = [a][b][dy][dx] (or
    [n, 7056] for rows [n, 16])."""
    h = np.asarray(hist_row, f32).reshape(-1, 16)
    img = _image(h[:, 12:16])
    out = np.ascontiguousarray(img.reshape(len(h), 21, 4, 21, 4).transpose(0, 1, 3, 2, 4)).reshape(len(h), FRAME_BYTES)
    return out[0] if np.ndim(hist_row) == 1 else out


def ring_rows(valid, abs_step, slots, num_envs):
    """fidx [N, 4] after the step of counter ``abs_step``: frame f of the observation is the one
    of step ``abs_step - (3 - f)``, clamped to the env's last reset (``valid`` distinct frames), in
    store row ``slot * N + env`` with ``slot = step mod slots``."""
    valid = np.asarray(valid).astype(np.int64)
    age = np.minimum(3 - np.arange(4)[None, :], np.maximum(valid, 1)[:, None] - 1)
    return (((int(abs_step) - age) % slots) * num_envs + np.arange(num_envs)[:, None]).astype(np.int32)


# ------------------------------------------------------------------ replay of a recorded run
def replay(states, acts, seed, abs_steps, max_steps, reset_step=None):
    """One-step predictions of a recorded run.  ``states`` [S + 1, N, 32] float32 are the device's
    states before step 0 .. after step S - 1, ``acts`` [S, N] its actions, ``abs_steps`` [S] the
    step counters.  ``reset_step``: the counter of the ``reset_all = 1`` launch that made
    ``states[0]`` (None: ``states[0]`` is an input, not checked).  Returns ``step``'s fields
    shaped [S, N, ...] plus ``reset`` (the expected ``states[0]`` or None)."""
    states = np.asarray(states)
    S, N = np.asarray(acts).shape
    envs = np.tile(np.arange(N), S)
    st = np.repeat(np.asarray([int(x) for x in abs_steps], dtype=np.uint64), N)
    ms = np.broadcast_to(np.asarray(max_steps), (S, N)).reshape(S * N)  # a scalar, or per cell
    o = step(states[:-1].reshape(S * N, STATE), np.asarray(acts).reshape(S * N), seed, st, ms, np.float64, envs)
    sh = lambda x: x.reshape((S, N) + x.shape[1:])  # noqa: E731
    rec = SimpleNamespace(**{k: sh(v) for k, v in vars(o.rec).items()})
    return SimpleNamespace(state=sh(o.state), rew=sh(o.rew), done=sh(o.done), fin_ret=sh(o.fin_ret),
                           fin_len=sh(o.fin_len), acc=sh(o.acc), margin=sh(o.margin), rec=rec,
                           reset=None if reset_step is None else reset_state(seed, reset_step, np.arange(N)))


def _all(mask, what):
    mask = np.asarray(mask)
    if not mask.all():
        bad = np.argwhere(~mask)
        raise AssertionError(f"{what}: {len(bad)} of {mask.size} cells differ, first at {tuple(bad[0])}")


def compared(margin):
    """The cells that are compared: all but those with 0 < margin < EPS."""
    return ~((margin > 0) & (margin < EPS))


def assert_state(got, want, what, cells=None):
    """Integer-valued slots exactly, continuous ones within ATOL (``cells``: a mask of rows)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    cells = np.ones(got.shape[:-1], bool) if cells is None else cells
    _all((got[..., INT_SLOTS] == want[..., INT_SLOTS])[cells], f"{what}: integer-valued state slots")
    _all((np.abs(got[..., CONT_SLOTS] - want[..., CONT_SLOTS]) <= ATOL)[cells], f"{what}: continuous state slots")


def assert_replay(states, outputs, rp):
    """Hold a recorded run (``states`` as for ``replay``, ``outputs`` the device's ``rew``,
    ``done``, ``fin_ret``, ``fin_len`` [S, N]) to its replay; returns the share of skipped cells."""
    states = np.asarray(states)
    if rp.reset is not None:
        assert_state(states[0], rp.reset, "state after reset_all")
    cells = compared(rp.margin)
    assert_state(states[1:], rp.state, "state after the step", cells)
    for k in ("rew", "done", "fin_ret", "fin_len"):
        _all((np.asarray(outputs[k], np.float64) == getattr(rp, k))[cells], k)
    return float((~cells).mean())


def expected_ep_acc(prefill, outputs, rp):
    """``ep_acc`` [N, 4] after the run, in float64: ``prefill`` plus (1, RET, T, RET^2) of every
    finished episode -- the oracle's, and in a skipped cell what the device reported."""
    done, fr, fl = (np.asarray(outputs[k], np.float64) for k in ("done", "fin_ret", "fin_len"))
    dev = (done > 0)[..., None] * np.stack([np.ones_like(fr), fr, fl, fr * fr], -1)
    inc = np.where(compared(rp.margin)[..., None], rp.acc, dev)
    return np.asarray(prefill, np.float64) + inc.sum(0)


def measure_f32_vs_f64(states, acts, seed, abs_steps, max_steps):
    """Largest |float32 - float64| one-step prediction of the oracle itself over the continuous
    slots, from the same float32 inputs ([S, N, 32] pre-step states), on the compared cells."""
    states, acts = np.asarray(states, f32), np.asarray(acts)
    S, N = acts.shape
    envs = np.tile(np.arange(N), S)
    st = np.repeat(np.asarray([int(x) for x in abs_steps], dtype=np.uint64), N)
    ms = np.broadcast_to(np.asarray(max_steps), (S, N)).reshape(S * N)
    a = (states.reshape(S * N, STATE), acts.reshape(S * N), seed, st, ms)
    o64, o32 = step(*a, np.float64, envs), step(*a, f32, envs)
    cells = compared(o64.margin)
    d = np.abs(o32.state.astype(np.float64) - o64.state)[:, CONT_SLOTS]
    return float(d[cells].max())


# ------------------------------------------------------------------ the replay cases
# The seed has both 32-bit halves non-zero and bit 62 set (DevicePong keeps 63 bits).  Actions are
# uniform over the 6; under them every natural ending is an opponent win.
SEED = (0x4D2B7A91 << 32) | 0x9E3779B1
STEP0 = 5          # counter of the reset launch; step t of the run is counter STEP0 + 1 + t
N_ENVS, STEPS = 300, 450
CASES = {"natural": dict(max_steps=0, act_seed=101), "truncated": dict(max_steps=37, act_seed=202)}
# the step-counter forms: the carry into step_hi happens at the 3rd step, the time limit ends
# every episode after it, so serves and resets are drawn with the high counter word set
CARRY_BASE, CARRY_MAX_STEPS, CARRY_ACT_SEED = 2 ** 32 - 3, 5, 303


def actions(steps, n, act_seed):
    return np.random.default_rng(act_seed).integers(0, 6, (steps, n)).astype(np.int32)


def simulate(n, acts, seed, step0, max_steps, prefill=(0.0, 0.0, 0.0, 0.0), dtype=f32):
    """The buffers a device run would leave, from the oracle in ``dtype`` (float32: a stand-in for
    the device on the CPU): reset at counter ``step0``, then ``acts`` [S, n] at ``step0 + 1 ..``."""
    S = len(acts)
    states = np.zeros((S + 1, n, STATE), dtype)
    out = {k: np.zeros((S, n), dtype) for k in ("rew", "done", "fin_ret", "fin_len")}
    states[0] = reset_state(seed, step0, np.arange(n), TAG_SERVE, dtype)
    acc = np.tile(np.asarray(prefill, dtype), (n, 1))
    for t in range(S):
        o = step(states[t], acts[t], seed, step0 + 1 + t, max_steps, dtype)
        states[t + 1] = o.state
        for k in out:
            out[k][t] = getattr(o, k)
        acc = (acc + o.acc.astype(dtype)).astype(dtype)
    out.update(states=states, acts=np.asarray(acts), ep_acc=acc, abs_steps=[step0 + 1 + t for t in range(S)])
    return out


# ------------------------------------------------------------------ injected boundary states
@dataclass
class Scenario:
    """A hand-built state for a ``reset_all = 0`` launch.  ``state`` overrides slots of ``MID``
    (``hist``: the 16 history floats), ``expect(rec)`` names the branch on the oracle's record of
    the row, ``check(s, out)`` states the outcome on the next state ``s`` [32] and the row's
    outputs ``out`` (rew, done, fin_ret, fin_len).  ``near``: the decisive quantity is within one
    ulp of its threshold, or a tie that is exact only in float32 (the opponent's paddle moves by
    the inexact 1.6): the float64 comparison skips the cell, ``expect`` is held on the float32
    record, and ``check`` -- exact in float32, every input being exactly representable -- decides."""
    name: str
    state: dict
    act: int = 0
    max_steps: int = 50
    expect: Optional[Callable] = None
    check: Optional[Callable] = None
    near: bool = False
    hist: tuple = field(default_factory=tuple)


MID = {BX: 40.0, BY: 40.0, VX: 1.5, VY: 0.5, PA: 42.0, PO: 42.0, SA: 3.0, SO: 5.0, T: 10.0, RET: -2.0, VALID: 4.0}
MID_HIST = (34.0, 38.0, 42.0, 42.0, 35.5, 38.5, 42.0, 42.0, 37.0, 39.0, 42.0, 42.0, 38.5, 39.5, 42.0, 42.0)
INJ_MAX_STEPS = 50
INJ_SEED, INJ_STEP = (0x2B << 32) | 7, 2 ** 32 + 9


def _up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


def _dn(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


def _opp_edge():
    """Opponent window tie in float32: the paddle moves 40 -> fl(40 + 1.6f), the ball's centre
    arrives exactly 6 below it (cy = BY + VY + 1 with VY = 2, so that it leaves the window again)."""
    po = f32(40) + f32(1.6)
    return float(po + f32(6) - f32(1) - f32(2))


_no_hit = lambda r: (r.hit == 0).all() and r.point_sub == -1  # noqa: E731
_fresh = lambda s: s[SA] == 0 and s[SO] == 0 and s[T] == 0 and s[RET] == 0 and s[VALID] == 1  # noqa: E731
_agent_lane = {BX: 73.0, VX: 1.5}   # arrives at bx = 74.5 inside both gates
_opp_lane = {BX: 9.0, VX: -1.5}     # arrives at bx = 7.5 inside both gates

SCENARIOS = [
    # ---- game end
    Scenario("agent_win", {BX: -0.5, VX: -2.0, VY: 0.0, SA: 20.0, SO: 7.0, RET: 12.0, T: 30.0},
             expect=lambda r: r.point_sub == 0 and r.scorer == 1 and r.over == OVER_AGENT,
             check=lambda s, o: o == (1, 1, 13, 31) and _fresh(s)),
    Scenario("opponent_win", {BX: 83.0, VX: 2.0, SO: 20.0, SA: 2.0, RET: -15.0, T: 30.0},
             expect=lambda r: r.point_sub == 0 and r.scorer == -1 and r.over == OVER_OPP,
             check=lambda s, o: o == (-1, 1, -16, 31) and _fresh(s)),
    # ---- truncation
    Scenario("time_limit", {T: 49.0}, expect=lambda r: r.point_sub == -1 and r.over == OVER_TIME,
             check=lambda s, o: o == (0, 1, -2, 50) and _fresh(s)),
    Scenario("time_limit_with_point", {BX: 83.0, VX: 2.0, T: 49.0, RET: -4.0},
             expect=lambda r: r.point_sub == 0 and r.over == OVER_TIME,
             check=lambda s, o: o == (-1, 1, -5, 50) and _fresh(s)),
    Scenario("no_time_limit", {T: 100000.0}, max_steps=0, expect=lambda r: r.over == 0,
             check=lambda s, o: o == (0, 0, 0, 0) and s[T] == 100001),
    # ---- point timing: the paddles stop with the point
    Scenario("point_sub_step_1", {BX: 83.0, VX: 2.0, PO: 50.0}, act=2,
             expect=lambda r: r.point_sub == 0 and r.scorer == -1,
             check=lambda s, o: s[PA] == 39.5 and abs(s[PO] - 48.4) < 1e-4 and s[SO] == 6 and s[RET] == -3),
    Scenario("point_sub_step_4", {BX: 77.5, VX: 2.0, PO: 50.0}, act=3,
             expect=lambda r: r.point_sub == 3 and (r.hit == 0).all(),
             check=lambda s, o: s[PA] == 52.0 and abs(s[PO] - 43.6) < 1e-4 and o[0] == -1),
    # ---- agent paddle: window |cy - pa| <= 6, gates bx + 2 >= 76 and BX + 2 <= 78
    Scenario("agent_window_top_edge", {**_agent_lane, BY: 35.5, VY: -0.5}, expect=lambda r: r.hit[0] == 1,
             check=lambda s, o: s[VX] < 0),
    Scenario("agent_window_above", {**_agent_lane, BY: _dn(35.5), VY: -0.5}, near=True, expect=_no_hit,
             check=lambda s, o: s[VX] == 1.5),
    Scenario("agent_window_bottom_edge", {**_agent_lane, BY: 46.5, VY: 0.5}, expect=lambda r: r.hit[0] == 1,
             check=lambda s, o: s[VX] < 0),
    Scenario("agent_window_below", {**_agent_lane, BY: _up(46.5), VY: 0.5}, near=True, expect=_no_hit,
             check=lambda s, o: s[VX] == 1.5),
    Scenario("agent_front_gate_tie", {BX: 72.5, VX: 1.5}, expect=lambda r: r.hit[0] == 1,
             check=lambda s, o: s[VX] < 0),
    Scenario("agent_front_gate_short", {BX: _dn(72.5), VX: 1.5}, near=True,
             expect=lambda r: r.hit[0] == 0 and r.hit[1] == 1, check=lambda s, o: s[VX] < 0),
    Scenario("agent_back_gate_tie", {BX: 76.0, VX: 1.5}, expect=lambda r: r.hit[0] == 1,
             check=lambda s, o: s[VX] < 0),
    Scenario("agent_back_gate_behind", {BX: _up(76.0), VX: 1.5}, near=True, expect=_no_hit,
             check=lambda s, o: s[VX] == 1.5 and s[BX] > 78),
    # ---- opponent paddle: window |cy - po| <= 6, gates bx <= 8 and BX >= 6
    Scenario("opponent_window_edge", {**_opp_lane, BY: _opp_edge(), VY: 2.0, PO: 40.0}, near=True,
             expect=lambda r: r.hit[0] == 2, check=lambda s, o: s[VX] > 0),
    Scenario("opponent_window_beyond", {**_opp_lane, BY: _up(_opp_edge()), VY: 2.0, PO: 40.0}, near=True,
             expect=_no_hit, check=lambda s, o: s[VX] == -1.5),
    Scenario("opponent_front_gate_tie", {BX: 9.5, VX: -1.5, VY: 0.0, PO: 41.0}, expect=lambda r: r.hit[0] == 2,
             check=lambda s, o: s[VX] > 0),
    Scenario("opponent_front_gate_short", {BX: _up(9.5), VX: -1.5, VY: 0.0, PO: 41.0}, near=True,
             expect=lambda r: r.hit[0] == 0 and r.hit[1] == 2, check=lambda s, o: s[VX] > 0),
    Scenario("opponent_back_gate_tie", {BX: 6.0, VX: -1.5, VY: 0.0, PO: 41.0}, expect=lambda r: r.hit[0] == 2,
             check=lambda s, o: s[VX] > 0),
    Scenario("opponent_back_gate_behind", {BX: _dn(6.0), VX: -1.5, VY: 0.0, PO: 41.0}, near=True, expect=_no_hit,
             check=lambda s, o: s[VX] == -1.5 and s[BX] < 6),
    # ---- contact: the speed cap and the vy clamps
    Scenario("vx_cap", {BX: 72.0, VX: 2.9}, expect=lambda r: r.hit[0] == 1, check=lambda s, o: s[VX] == -3.0),
    Scenario("vy_clamp_high", {**_agent_lane, BY: 43.5, VY: 2.5}, expect=lambda r: r.hit[0] == 1,
             check=lambda s, o: s[VY] == 3.0),
    Scenario("vy_clamp_low", {**_opp_lane, BY: 40.0, VY: -2.5, PO: 45.0}, expect=lambda r: r.hit[0] == 2,
             check=lambda s, o: s[VY] == -3.0 and s[VX] > 0),
    # ---- walls: by = 2 and by + 2 = 82 exactly do not bounce
    Scenario("top_wall_tie", {BY: 4.5, VY: -2.5}, expect=lambda r: list(r.wall) == [0, 1, 0, 0],
             check=lambda s, o: s[VY] == 2.5),
    Scenario("top_wall_below", {BY: _dn(4.5), VY: -2.5}, near=True, expect=lambda r: list(r.wall) == [1, 0, 0, 0],
             check=lambda s, o: s[VY] == 2.5),
    Scenario("bottom_wall_tie", {BY: 77.5, VY: 2.5}, expect=lambda r: list(r.wall) == [0, 2, 0, 0],
             check=lambda s, o: s[VY] == -2.5),
    Scenario("bottom_wall_beyond", {BY: _up(77.5), VY: 2.5}, near=True, expect=lambda r: list(r.wall) == [2, 0, 0, 0],
             check=lambda s, o: s[VY] == -2.5),
    # ---- paddles
    Scenario("agent_clamp_7", {PA: 8.0}, act=2, check=lambda s, o: s[PA] == 7.0),
    Scenario("agent_clamp_77", {PA: 76.0}, act=3, check=lambda s, o: s[PA] == 77.0),
    Scenario("action_1_is_noop", {}, act=1, check=lambda s, o: s[PA] == 42.0),
    Scenario("action_4_is_up", {}, act=4, check=lambda s, o: s[PA] == 32.0),
    Scenario("action_5_is_down", {}, act=5, check=lambda s, o: s[PA] == 52.0),
    Scenario("opponent_tracks_the_ball", {VX: -1.5, PO: 20.0}, check=lambda s, o: abs(s[PO] - 26.4) < 1e-4),
    Scenario("opponent_tracks_exactly", {VX: -1.5, VY: 0.25, PO: 40.5}, check=lambda s, o: s[PO] == 41.75),
    Scenario("opponent_drifts_to_centre", {PO: 50.0}, check=lambda s, o: abs(s[PO] - 43.6) < 1e-4),
    Scenario("opponent_rests_at_centre", {PO: 43.0}, check=lambda s, o: s[PO] == 42.0),
    Scenario("opponent_clamp_7", {VX: -1.5, BY: 3.0, VY: 0.25, PO: 8.0}, check=lambda s, o: s[PO] == 7.0),
    Scenario("opponent_clamp_77", {VX: -1.5, BY: 79.0, VY: -0.25, PO: 76.0}, check=lambda s, o: s[PO] == 77.0),
    # ---- the distinct-frame count
    Scenario("valid_1", {VALID: 1.0}, check=lambda s, o: s[VALID] == 2),
    Scenario("valid_2", {VALID: 2.0}, check=lambda s, o: s[VALID] == 3),
    Scenario("valid_3", {VALID: 3.0}, check=lambda s, o: s[VALID] == 4),
    Scenario("valid_4", {VALID: 4.0}, check=lambda s, o: s[VALID] == 4),
    # ---- the ball partly off screen, in the new frame and in the older ones
    Scenario("ball_off_right", {BX: 77.5, VX: 1.5}, hist=(82.5, 30.0, 42.0, 42.0, 83.25, 31.0, 42.0, 42.0,
                                                          84.0, 32.0, 42.0, 42.0, 82.0, 33.0, 42.0, 42.0),
             expect=_no_hit, check=lambda s, o: s[BX] == 83.5),
    Scenario("ball_off_left", {BX: 5.0, VX: -1.5}, hist=(-1.5, 30.0, 42.0, 42.0, -0.5, 31.0, 42.0, 42.0,
                                                         -2.0, 32.0, 42.0, 42.0, -1.0, 33.0, 42.0, 42.0),
             expect=_no_hit, check=lambda s, o: s[BX] == -1.0),
]


def scenario_inputs(n, scenarios=None):
    """(state [n, 32] float32, act [n], max_steps [n], rows): scenario k fills rows k, k + K, ..."""
    sc = SCENARIOS if scenarios is None else scenarios
    rows = np.arange(n) % len(sc)
    state = np.zeros((n, STATE), f32)
    act, ms = np.zeros(n, np.int32), np.zeros(n, np.int64)
    for i, k in enumerate(rows):
        s = sc[k]
        for slot, v in {**MID, **s.state}.items():
            state[i, slot] = v
        state[i, HIST:] = s.hist if s.hist else MID_HIST
        act[i], ms[i] = s.act, s.max_steps
    return state, act, ms, rows


def assert_scenarios(states, outputs, act, rows, scenarios=None, seed=INJ_SEED, abs_step=INJ_STEP):
    """Hold one injected step (``states`` [2, n, 32], ``outputs`` [1, n], the scenarios' own
    actions) to the oracle and to every scenario's ``check``; the skipped cells must be exactly
    the ``near`` scenarios."""
    sc = SCENARIOS if scenarios is None else scenarios
    ms = np.array([sc[k].max_steps for k in rows])
    rp = replay(states, act[None], seed, [abs_step], ms[None])
    assert_replay(states, outputs, rp)
    skipped = ~compared(rp.margin)[0]
    for i, k in enumerate(rows):
        s = sc[k]
        assert skipped[i] == s.near, f"{s.name}: margin {rp.margin[0, i]}"
        if s.check is not None:
            o = tuple(float(outputs[q][0, i]) for q in ("rew", "done", "fin_ret", "fin_len"))
            assert s.check(np.asarray(states[1][i], np.float64), o), f"{s.name}: {states[1][i][:11]}, {o}"
    return rp
