"""The PongSynth oracle (tests/pong_oracle.py) against independent code, with no GPU: ``PongRef``
(the CPU trainer's env) step by step and through the injected boundary states, the oracle's own
float32 run (the tolerance and the skipped share of the cases tests/test_pong_episodes_gpu.py
replays), and the branch every injected scenario is meant to reach."""
from functools import lru_cache

import numpy as np
import pytest

from relayrl_prototype_amd.envs.pong import PongRef

import pong_oracle as po


def _ref_run(max_steps, n=64, steps=400, seed=po.SEED, act_seed=7):
    """A free-running PongRef under random actions: its states before / after every step, its
    outputs and its renders at every 8th step."""
    ref = PongRef(n, seed, max_steps)
    ref.step_count = po.STEP0
    obs0 = ref.reset()
    acts = po.actions(steps, n, act_seed)
    states = np.zeros((steps + 1, n, po.STATE), np.float32)
    out = {k: np.zeros((steps, n), np.float32) for k in ("rew", "done", "fin_ret", "fin_len")}
    states[0] = ref.s
    drawn = {-1: obs0}
    for t in range(steps):
        out["rew"][t], out["done"][t], out["fin_ret"][t], out["fin_len"][t] = ref.step(acts[t])
        states[t + 1] = ref.s
        if t % 8 == 0 or out["done"][t].any():
            drawn[t] = ref.render()
    return states, acts, out, drawn


@pytest.mark.parametrize("max_steps", [0, 37])
def test_pongref_matches_the_oracle_step_by_step(max_steps):
    states, acts, out, drawn = _ref_run(max_steps)
    steps = len(acts)
    rp = po.replay(states, acts, po.SEED, [po.STEP0 + 1 + t for t in range(steps)], max_steps, reset_step=po.STEP0)
    share = po.assert_replay(states, out, rp)
    assert share <= po.MAX_SKIP_SHARE
    ends = rp.rec.over[out["done"] > 0]
    if max_steps:
        assert (ends == po.OVER_TIME).all() and len(ends) == 64 * (steps // max_steps)
    else:  # random play loses: natural endings are 21 points of the opponent
        assert len(ends) > 10 and (ends == po.OVER_OPP).all()
    assert (rp.margin == 0).mean() > 0.01  # the ties that tell >= from > are in the run
    for t, obs in drawn.items():
        assert np.array_equal(obs, po.render(states[t + 1][:, po.HIST:])), f"render after step {t}"


def test_pongref_matches_the_oracle_on_the_injected_states():
    n = 2 * len(po.SCENARIOS) + 3
    state, act, ms, rows = po.scenario_inputs(n)
    states = np.stack([state, state])
    out = {k: np.zeros((1, n), np.float32) for k in ("rew", "done", "fin_ret", "fin_len")}
    for limit in np.unique(ms):  # PongRef has one time limit per batch
        ref = PongRef(n, po.INJ_SEED, int(limit))
        ref.s, ref.step_count = state.copy(), po.INJ_STEP
        res = ref.step(act)
        pick = ms == limit
        states[1][pick] = ref.s[pick]
        for k, v in zip(("rew", "done", "fin_ret", "fin_len"), res):
            out[k][0][pick] = v[pick]
        assert np.array_equal(ref.render()[pick], po.render(ref.s[pick][:, po.HIST:]))
    po.assert_scenarios(states, out, act, rows)


@lru_cache(maxsize=None)
def _stand_in(case):
    """The float32 oracle's own run of a replay case of the GPU file."""
    c = po.CASES[case]
    return po.simulate(po.N_ENVS, po.actions(po.STEPS, po.N_ENVS, c["act_seed"]), po.SEED, po.STEP0, c["max_steps"])


@pytest.mark.parametrize("case", list(po.CASES))
def test_skipped_share_of_the_replay_cases(case):
    """The cap holds for the reference alone, with the seeds the GPU file uses; and the float32
    stand-in passes the assertions the device run will face."""
    run, c = _stand_in(case), po.CASES[case]
    rp = po.replay(run["states"], run["acts"], po.SEED, run["abs_steps"], c["max_steps"], reset_step=po.STEP0)
    share = po.assert_replay(run["states"], run, rp)
    print(f"{case}: {share:.4%} of {rp.margin.size} cells within {po.EPS} of a threshold, "
          f"{(rp.margin == 0).mean():.2%} exactly on one, {int((run['done'] > 0).sum())} episodes")
    assert share <= po.MAX_SKIP_SHARE / 5  # nowhere near the cap
    assert np.array_equal(po.expected_ep_acc(np.zeros(4), run, rp), run["ep_acc"].astype(np.float64))
    ends = rp.rec.over[run["done"] > 0]
    if c["max_steps"]:
        assert (ends == po.OVER_TIME).all() and len(ends) == po.N_ENVS * (po.STEPS // c["max_steps"])
    else:
        assert (ends == po.OVER_OPP).all() and len(ends) > 200


def test_step_counter_case_share():
    acts = po.actions(8, po.N_ENVS, po.CARRY_ACT_SEED)
    run = po.simulate(po.N_ENVS, acts, po.SEED, po.CARRY_BASE, po.CARRY_MAX_STEPS)
    rp = po.replay(run["states"], acts, po.SEED, run["abs_steps"], po.CARRY_MAX_STEPS, reset_step=po.CARRY_BASE)
    assert po.assert_replay(run["states"], run, rp) <= po.MAX_SKIP_SHARE
    lo = po.words(po.SEED, 2 ** 32 + 1, [0, 1], po.TAG_SERVE)
    assert not np.array_equal(lo, po.words(po.SEED, 1, [0, 1], po.TAG_SERVE))  # the high counter word is used
    assert not np.array_equal(lo, po.words(po.SEED & 0xFFFFFFFF, 2 ** 32 + 1, [0, 1], po.TAG_SERVE))  # and the key's


def test_atol_is_four_times_the_measured_float32_error():
    worst = 0.0
    for case, c in po.CASES.items():
        run = _stand_in(case)
        worst = max(worst, po.measure_f32_vs_f64(run["states"][:-1], run["acts"], po.SEED, run["abs_steps"], c["max_steps"]))
    state, act, ms, _ = po.scenario_inputs(96)
    worst = max(worst, po.measure_f32_vs_f64(state[None], act[None], po.INJ_SEED, [po.INJ_STEP], ms[None]))
    print(f"largest |float32 - float64| one-step prediction: {worst:.3e} (recorded {po.MEASURED_F32_VS_F64:.3e})")
    assert worst <= po.MEASURED_F32_VS_F64 <= po.ATOL / 4
    assert po.ATOL < po.EPS


def test_every_scenario_reaches_its_branch():
    n = len(po.SCENARIOS)
    assert len({s.name for s in po.SCENARIOS}) == n
    state, act, ms, rows = po.scenario_inputs(n)
    assert np.array_equal(state.astype(np.float64).astype(np.float32), state)
    o64 = po.step(state, act, po.INJ_SEED, po.INJ_STEP, ms, np.float64)
    o32 = po.step(state, act, po.INJ_SEED, po.INJ_STEP, ms, np.float32)
    row = lambda rec, i: type(rec)(**{k: v[i] for k, v in vars(rec).items()})  # noqa: E731
    for i, s in enumerate(po.SCENARIOS):
        assert (0 < o64.margin[i] < po.EPS) == s.near, (s.name, o64.margin[i])
        if not s.near and s.name.endswith(("_tie", "_edge")):
            assert o64.margin[i] == 0, s.name
        for o in (o32,) if s.near else (o32, o64):
            if s.expect is not None:
                assert s.expect(row(o.rec, i)), (s.name, vars(row(o.rec, i)))
            out = tuple(float(getattr(o, k)[i]) for k in ("rew", "done", "fin_ret", "fin_len"))
            assert s.check is None or s.check(o.state[i].astype(np.float64), out), (s.name, o.state[i][:11], out)
        if s.name in ("agent_win", "opponent_win"):  # the state afterwards is the tag-0x52 reset, not the serve
            want = po.reset_state(po.INJ_SEED, po.INJ_STEP, [i], po.TAG_RESET)[0]
            other = po.reset_state(po.INJ_SEED, po.INJ_STEP, [i], po.TAG_SERVE)[0]
            assert np.array_equal(o64.state[i], want) and not np.array_equal(want, other)
    # the float32 stand-in passes the assertions the device launch will face
    n = 96
    state, act, ms, rows = po.scenario_inputs(n)
    o = po.step(state, act, po.INJ_SEED, po.INJ_STEP, ms, np.float32)
    outs = {k: getattr(o, k)[None] for k in ("rew", "done", "fin_ret", "fin_len")}
    po.assert_scenarios(np.stack([state, o.state]), outs, act, rows)


def test_renders_agree_with_each_other_and_clip_the_ball():
    """``frame`` is the newest frame's bytes of ``render``; a ball partly off screen lights only
    its on-screen pixels; one that left it lights none."""
    hist = np.array([[82.5, 30.0, 42.0, 20.0, -1.25, 31.0, 7.0, 77.0, 84.0, 0.5, 42.0, 42.0, 83.25, 81.0, 42.0, 42.0]],
                    np.float32)
    obs = po.render(hist).reshape(21, 21, 4, 4, 4)  # a, b, dy, dx, f
    fr = po.frame(hist[0]).reshape(21, 21, 4, 4)
    assert np.array_equal(obs[..., 3], fr)
    img = obs.transpose(4, 0, 2, 1, 3).reshape(4, 84, 84)  # f, y, x
    lit = lambda f, y0, y1, x0, x1: int((img[f, y0:y1, x0:x1] == 255).sum())  # noqa: E731
    assert lit(0, 30, 32, 78, 84) == 4   # bx = 82.5: columns 82 and 83 (centres 82.5, 83.5), rows 30 and 31
    assert lit(1, 31, 33, 0, 6) == 2     # bx = -1.25: column 0 only (0.5 < 0.75)
    assert lit(2, 0, 84, 78, 84) == 0    # bx = 84: gone
    assert lit(3, 78, 84, 78, 84) == 2   # by = 81: rows 81, 82 x column 83; the wall rows keep 100 elsewhere
    assert img[3, 83, 40] == 100 and img[3, 1, 40] == 100 and img[3, 2, 40] == 0
