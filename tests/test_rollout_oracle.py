"""The rollout oracle (tests/rollout_oracle.py) against independent code, with no GPU: the host
C++ envs of ``_native.VecEnv``, its own float32 run, and the intended outcomes of the injected
boundary states that tests/test_rollout_episodes_gpu.py feeds the kernels."""
import itertools

import numpy as np
import pytest

import rollout_oracle as ro


def _ptr(a):
    return a.ctypes.data


def _host_run(name, n=64, steps=300, seed=4):
    """(prev obs, act, next obs, done, episode length after the step) per step of a host VecEnv
    under uniformly random actions; after a done, ``next obs`` is the host's reset observation."""
    from relayrl_prototype_amd import _native

    env = _native.VecEnv(name, n, seed, 1)
    e = ro.env_of(name)
    assert (env.obs_dim, env.act_dim, env.max_steps) == (e.D, e.A, e.max_steps)
    obs = np.zeros((n, e.D), np.float32)
    rew, done = np.zeros(n, np.float32), np.zeros(n, np.float32)
    env.reset_ptr(_ptr(obs))
    rng = np.random.default_rng(seed)
    ln = np.zeros(n, np.int64)
    for _ in range(steps):
        prev = obs.copy()
        act = rng.integers(0, e.A, n).astype(np.int32)
        env.step_ptr(_ptr(act), _ptr(obs), _ptr(rew), _ptr(done))
        ln += 1
        yield prev, act, obs.copy(), rew.copy(), done.copy(), ln.copy()
        ln[done > 0] = 0


@pytest.mark.parametrize("name", ["CartPole-v1", "MountainCar-v0", "Acrobot-v1"])
def test_oracle_matches_host_env(name):
    e = ro.env_of(name)
    live_rows = dones = 0
    for prev, act, nxt, rew, done, ln in _host_run(name):
        ns, r, term, margin = e.step(e.state_from_obs(prev), act, None, np.float64)
        live = done == 0
        assert ro.obs_close(e, nxt, e.obs(ns))[live].all()
        assert ro.rew_close(e, rew, r).all()
        sure = (margin > ro.EPS) & (ln < e.max_steps)  # at the time limit the host's done is a truncation
        assert ((done > 0) == term)[sure].all()
        assert (done[ln >= e.max_steps] > 0).all()
        live_rows += live.sum()
        dones += (done > 0).sum()
    # (a random Acrobot rarely swings up in 300 steps: its terminations come from injected states)
    assert live_rows > 64 * 250 and (dones > 0 or name == "Acrobot-v1")


def test_lander_oracle_matches_host_env_noise_free_components():
    """The host Lander draws its lateral noise from the host RNG, so only what that noise does not
    reach is compared: y, vy, angle, angular velocity and the leg flags."""
    e = ro.LunarLanderSynth
    cols = [1, 3, 4, 5, 6, 7]
    live_rows = dones = 0
    for prev, act, nxt, rew, done, ln in _host_run(e.name):
        ns, r, term, margin = e.step(e.state_from_obs(prev), act, np.full(len(act), 0.5, np.float32), np.float64)
        live = done == 0
        assert ro.obs_close(e, nxt, e.obs(ns))[live][:, cols].all()
        # one step of noise moves x by at most 0.006 * 0.02, so |x| - 1 is decided beyond that
        sure = margin > ro.EPS + 2e-4
        assert ((done > 0) == term)[sure].all()
        live_rows += live.sum()
        dones += (done > 0).sum()
    assert live_rows > 64 * 250 and dones > 64


def _actions(e, rng):
    if not e.continuous:
        return [np.array([a]) for a in range(e.A)]
    return [rng.uniform(-2, 2, (1, e.A)) for _ in range(4)] + [np.full((1, e.A), v) for v in (-3.0, 0.0, 3.0)]


@pytest.mark.parametrize("name", list(ro.INJECTED))
def test_injected_states_have_one_outcome_for_every_action(name):
    """Every scenario of the injected-state table ends its first step as intended whatever the
    policy samples (and whatever the env noise), with the decisive quantity well clear of its
    threshold; the padding rows and the two-step scenarios stay uneventful for two steps."""
    e = ro.env_of(name)
    rng = np.random.default_rng(0)
    max_steps = 50
    state, ln, rt, rows = ro.injected_inputs(e, 17, max_steps)
    noises = [np.full((1, 17) if e.continuous else 1, u, np.float32) for u in (0.0, 0.5, 1 - 2.0 ** -24)]
    names = set()
    for sc, row in zip(ro.INJECTED[name], rows):
        names.add(sc.name)
        assert ln[row] == (max_steps - 1 if sc.at_limit else 3) and rt[row] == sc.ep_ret
        for act, noise in itertools.product(_actions(e, rng), noises):
            ns, r, term, margin = e.step(state[row:row + 1], act, noise, np.float64)
            assert bool(term[0]) == sc.term, (sc.name, act)
            assert margin[0] > 10 * ro.EPS, (sc.name, act, margin)
            assert sc.check is None or sc.check(ns[0], float(r[0])), (sc.name, act, ns, r)
            if sc.two_steps:
                for act2 in _actions(e, rng):
                    _, _, term2, margin2 = e.step(ns, act2, noise, np.float64)
                    assert not term2[0] and margin2[0] > 10 * ro.EPS, (sc.name, act, act2)
        assert sc.code(True) == (1 if sc.term else 2 if sc.at_limit else 0)
        assert sc.code(False) == (1 if sc.term or sc.at_limit else 0)
    assert "time_limit" in names and (not e.terminates or "term_at_limit" in names)
    mid = state[:1]
    assert 0 not in rows
    for act, act2, noise in itertools.product(_actions(e, rng), _actions(e, rng), noises):
        ns, _, term, margin = e.step(mid, act, noise, np.float64)
        _, _, term2, margin2 = e.step(ns, act2, noise, np.float64)
        assert not term[0] and not term2[0] and min(margin[0], margin2[0]) > 10 * ro.EPS


def _case_sim(name, N=517, H=128):
    c = ro.CASES[name]
    return ro.simulate(name, ro.case_params(name, H), H, N, c["T"], c["seed"], c["step0"], c["max_steps"])


@pytest.fixture(scope="module")
def sims():
    return {name: _case_sim(name) for name in ro.CASES}


@pytest.mark.parametrize("name", list(ro.CASES))
def test_replay_holds_the_float32_oracle_rollout(sims, name):
    """The assertions the GPU tests make of a device rollout, made of the oracle's own float32
    rollout: the replay, the done codes, the resets, ``tobs`` and the episode statistics agree,
    the case ends episodes with the codes it is meant to show, and few cells are near a threshold."""
    e, c, bufs = ro.env_of(name), ro.CASES[name], dict(sims[name])
    T, N = bufs["done"].shape
    rp = ro.replay(e, bufs, c["seed"], c["step0"], c["max_steps"])
    share = ro.assert_replay(e, bufs, rp)
    print(f"{name}: {share:.4%} of {T * N} cells within {ro.EPS} of a threshold")
    codes = set(np.unique(bufs["done"]).astype(int))
    assert codes == ({0, 1} if name == "LunarLanderSynth-v0" else {0, 1, 2} if name == "CartPole-v1" else {0, 2})
    st = ro.episode_stats(bufs["rew"], bufs["done"])
    assert st["n_done"] == (bufs["done"] > 0).sum() > 0
    assert st["sum_len"] + st["ep_len"].sum() == T * N
    np.testing.assert_array_equal(st["ep_len"], rp["len_out"])
    np.testing.assert_allclose(st["ep_ret"], rp["ret_out"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(st["sum_ret"] + st["ep_ret"].sum(dtype=np.float64), bufs["rew"].sum(dtype=np.float64),
                               rtol=1e-5)
    # a continuation from the persistent outputs of the first half counts every episode once
    h = T // 2
    a = ro.episode_stats(bufs["rew"][:h], bufs["done"][:h])
    b = ro.episode_stats(bufs["rew"][h:], bufs["done"][h:], a["ep_len"], a["ep_ret"])
    assert a["n_done"] + b["n_done"] == st["n_done"] and a["sum_len"] + b["sum_len"] == st["sum_len"]
    assert max(a["max_ret"], b["max_ret"]) == st["max_ret"] and min(a["min_ret"], b["min_ret"]) == st["min_ret"]
    np.testing.assert_array_equal(b["ep_ret"], st["ep_ret"])


def test_replay_notices_wrong_bookkeeping(sims):
    """The replay is not vacuous: a reward, a done code, a reset and a tobs row that are off by
    what a bookkeeping slip would cause each fail it."""
    name = "CartPole-v1"
    e, c = ro.env_of(name), ro.CASES[name]

    def run(mutate):
        bufs = {k: v.copy() for k, v in sims[name].items()}
        mutate(bufs)
        ro.assert_replay(e, bufs, ro.replay(e, bufs, c["seed"], c["step0"], c["max_steps"]))

    run(lambda b: None)
    t1, n1 = np.argwhere(sims[name]["done"] == 1)[0]
    t2, n2 = np.argwhere(sims[name]["done"] == 2)[0]

    def set_(key, idx, val):
        def f(b):
            b[key][idx] = val
        return f

    for mutate in (set_("done", (t1, n1), 2.0), set_("done", (t2, n2), 1.0), set_("done", (t2, n2), 0.0),
                   set_("rew", (t1, n1), 0.0), set_("tobs", (t1, n1, 0), 0.5), set_("tobs", (t2, n2, 1), np.nan),
                   set_("obs", (t2 + 1, n2, 0), 0.049), set_("obs", (0, 3, 2), 0.2)):
        with pytest.raises(AssertionError):
            run(mutate)


def test_derived_tolerances_follow_the_recorded_measurement(sims):
    """MountainCar / Acrobot tolerances are 8 x the recorded float32-vs-float64 difference of the
    oracle, floored at 4 ulp of each component's bound; the difference measured now, over the
    case inputs and the injected states under every action, is what was recorded (to within 2 x,
    for another libm)."""
    for name in ro.MEASURED_F32_VS_F64:
        e, c, bufs = ro.env_of(name), ro.CASES[name], sims[name]
        d_obs, d_rew = np.zeros(e.D), 0.0
        for t in range(c["T"]):
            do, dr = ro.measure_f32_vs_f64(e, bufs["obs"][t], bufs["act"][t])
            d_obs, d_rew = np.maximum(d_obs, do), max(d_rew, dr)
        state, _, _, _ = ro.injected_inputs(e, 17, 50)
        for a, a2 in itertools.product(range(e.A), range(e.A)):  # both steps of the injected launches
            o1 = e.obs(state.astype(np.float32))
            o2 = e.obs(e.step(state.astype(np.float32), np.full(17, a), None, np.float32)[0])
            for o, b in ((o1, a), (o2, a2)):
                do, dr = ro.measure_f32_vs_f64(e, o, np.full(17, b))
                d_obs, d_rew = np.maximum(d_obs, do), max(d_rew, dr)
        print(name, "float32 vs float64:", " ".join(f"{v:.3g}" for v in d_obs), "reward", d_rew)
        assert d_rew == 0.0
        assert (d_obs <= 2 * ro.MEASURED_F32_VS_F64[name]).all(), d_obs
        tol = ro.derived_atol(e)
        np.testing.assert_array_equal(tol, np.maximum(8 * ro.MEASURED_F32_VS_F64[name], 4 * 2.0 ** -23 * e.bounds))
        assert (tol < 1e-3).all()
