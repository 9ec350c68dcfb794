"""Episode bookkeeping of the fused rollout kernels (csrc/kernels/rollout.hip) against the host
oracle of tests/rollout_oracle.py, through both discrete kernels (the one-workgroup-per-tile
``rollout_wide_kernel`` and the tile-stride ``rollout_kernel``) and the continuous one:

a. full rollouts replayed step by step: physics, terminal rewards, done codes, Philox resets, tobs;
b. ``ep_stats`` row by row, and the persistent ``state`` / ``ep_len`` / ``ep_ret``;
c. injected boundary states through ``reset_all = 0`` (branches a random policy never reaches);
d. one launch of T1 + T2 steps against two launches that continue each other, bit for bit.

Every output buffer is the middle of a larger sentinel-filled tensor whose guards must survive.
"""
import math
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import MLPSpec, hip
from relayrl_prototype_amd.ops import reference as ref

import rollout_oracle as ro
from guarded import INT_SENTINEL, Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@contextmanager
def kernel(kind, N):
    """Size the grids so that N envs run through the wanted kernel; yields the ep_stats rows.
    ``wide``: all CUs, one workgroup per tile.  ``tile``: grids for 2 CUs, so 4 workgroups of 4
    waves stride over the tiles."""
    h = hip()
    old = h.set_cu_limit(2) if kind == "tile" else None
    try:
        grid, tiles = h.rollout_grid(N), (N + 15) // 16
        assert grid == tiles if kind == "wide" else grid < tiles, (kind, N, grid, tiles)
        yield grid
    finally:
        if old is not None:
            h.set_cu_limit(old)


def launch(env, kind, N, T, H, seed, step0, max_steps, state_in=None, len_in=None, ret_in=None, has_tobs=True,
           persist=None):
    """One rollout launch into guarded buffers.  ``state_in`` (with ``len_in``, ``ret_in``) or
    ``persist`` (the guarded state / ep_len / ep_ret of an earlier launch) make it a
    ``reset_all = 0`` continuation.  Returns the buffers as numpy arrays plus ``persist``."""
    e = ro.env_of(env)
    h = hip()
    params = ro.case_params(e, H, DEV)
    reset_all = state_in is None and persist is None
    if persist is None:
        persist = (Guarded((N, e.NS), fill=state_in), Guarded((N,), torch.int32, fill=len_in),
                   Guarded((N,), fill=ret_in))
    state, ep_len, ep_ret = persist
    g = dict(obs=Guarded((T + 1, N, e.D)),
             act=Guarded((T, N, e.A)) if e.continuous else Guarded((T, N), torch.int32),
             logp=Guarded((T, N)), rew=Guarded((T, N)), done=Guarded((T, N)), tobs=Guarded((T, N, e.D)))
    with kernel(kind, N) as grid:
        g["ep_stats"] = Guarded((grid, 8), fill=float(INT_SENTINEL))
        tobs = g["tobs"].t if has_tobs else None
        args = (H, state.t, ep_len.t, ep_ret.t, g["obs"].t, g["act"].t, g["logp"].t, g["rew"].t, g["done"].t, tobs,
                g["ep_stats"].t, seed, step0, reset_all, max_steps)
        if e.continuous:
            h.rollout_cont(e.env_id, params, torch.from_numpy(e.constants()).to(DEV), *args)
        else:
            h.rollout(e.env_id, params, *args)
        torch.cuda.synchronize()
    g.update(state=state, ep_len=ep_len, ep_ret=ep_ret)
    for k, b in g.items():
        assert b.guards_intact(), f"{k}: the kernel wrote outside its buffer"
    out = {k: b.t.cpu().numpy() for k, b in g.items()}
    if not has_tobs:
        assert np.isnan(out.pop("tobs")).all()
    out.update(persist=persist, grid=grid, params=params.cpu(), env=e, kind=kind, N=N, T=T, H=H, seed=seed,
               step0=step0, max_steps=max_steps)
    return out


def reduction_map(run):
    """(ep_stats row, accumulating lane) of every env.  Wide kernel: workgroup b owns tile b.
    Otherwise wave w of ``4 * grid`` owns tiles w, w + 4 * grid, ...; a workgroup is 4 waves."""
    env = np.arange(run["N"])
    tile = env // 16
    if run["kind"] == "wide" and not run["env"].continuous:
        return tile, env
    wave = tile % (4 * run["grid"])
    return wave // 4, wave * 16 + env % 16


def check_policy(run):
    """act / logp against the fp32 policy oracle at the stored observations."""
    e, T, N = run["env"], run["T"], run["N"]
    pc = run["params"]
    obs, act, logp = (torch.from_numpy(run[k]) for k in ("obs", "act", "logp"))
    if e.continuous:
        o = MLPSpec(e.D, run["H"], e.A, gaussian=True).offsets()["log_std"]
        ls = pc[o:o + e.A]
        assert torch.isfinite(act).all()
        for t in range(T):
            mu = ref.mlp_forward_ref(3, pc, obs[t], e.A, run["H"])["logits"]
            z = (act[t] - mu) / torch.exp(ls)
            torch.testing.assert_close(logp[t], (-0.5 * z * z - ls - 0.9189385332046727).sum(-1), rtol=1e-3, atol=2e-3)
        return
    assert int(act.min()) >= 0 and int(act.max()) < e.A
    differ = 0
    for t in range(T):
        r = ref.mlp_forward_ref(2, pc, obs[t], e.A, run["H"], act_in=act[t])
        torch.testing.assert_close(logp[t], r["logp"], rtol=1e-4, atol=1e-4)
        rs = ref.mlp_forward_ref(1, pc, obs[t], e.A, run["H"], seed=run["seed"], step=run["step0"] + t)
        differ += int((rs["act"] != act[t]).sum())
    assert differ <= max(1, 0.02 * T * N), differ  # a draw within rounding of a cdf step may go either way


def check_stats(run, stats_list, len_in=None, ret_in=None):
    """``ep_stats`` (summed over ``stats_list``, the launches that together cover ``run``'s rew /
    done) and the persistent outputs against episode_stats of the device's own buffers."""
    st = ro.episode_stats(run["rew"], run["done"], len_in, ret_in)
    ep = st["episodes"]
    row_of, lane_of = reduction_map(run)
    want, per_lane = ro.stats_rows(ep, row_of, lane_of, run["grid"])
    # fp32 accumulation chain: a lane's episodes, the 6 levels of the 64-lane butterfly and the
    # 2 levels over a workgroup's 4 waves
    chain = per_lane + int(math.log2(64)) + int(math.log2(4))
    amax = float(np.abs(ep["ret"]).max()) if st["n_done"] else 0.0
    if len(stats_list) == 1:  # row by row
        dev = stats_list[0].astype(np.float64)
        assert (dev[:, 6:] == INT_SENTINEL).all()
        for q in (0, 3, 4, 5):
            np.testing.assert_array_equal(dev[:, q], want[:, q], err_msg=f"ep_stats column {q}")
        idle = want[:, 0] == 0
        assert (dev[idle, 1] == 0).all() and (dev[idle, 2] == 0).all()
        tol = want[:, 0] * 2.0 ** -23 * chain
        assert (np.abs(dev[:, 1] - want[:, 1]) <= tol * amax).all()
        assert (np.abs(dev[:, 2] - want[:, 2]) <= tol * amax * amax).all()
    tot = np.stack([s.astype(np.float64) for s in stats_list])
    n, s1, s2, sl = (tot[:, :, q].sum() for q in (0, 1, 2, 5))
    assert n == st["n_done"] and sl == st["sum_len"]
    assert tot[:, :, 3].max() == st["max_ret"] and tot[:, :, 4].min() == st["min_ret"]
    tol = st["n_done"] * 2.0 ** -23 * chain
    assert abs(s1 - st["sum_ret"]) <= tol * amax, (s1, st["sum_ret"], tol * amax)
    assert abs(s2 - st["sumsq_ret"]) <= tol * amax * amax, (s2, st["sumsq_ret"], tol * amax * amax)
    np.testing.assert_array_equal(run["ep_len"], st["ep_len"])
    np.testing.assert_array_equal(run["ep_ret"], st["ep_ret"])  # the same fp32 additions, bit for bit
    return st


def check_state(run, rp):
    """The persistent state against the oracle's, and against the last observation row."""
    e, state = run["env"], run["state"]
    ro._all(ro.obs_close(e, e.obs(state), e.obs(rp["state_out"])), "state vs the oracle's final state")
    if e is ro.Acrobot:
        assert (np.abs(state[:, :2]) <= np.float32(np.pi) + 1e-6).all(), "angles are kept in [-pi, pi]"
        ro._all(ro.obs_close(e, run["obs"][-1], e.obs(state.astype(np.float64))), "obs[T] vs state")
    else:
        np.testing.assert_array_equal(run["obs"][-1], e.obs(state))
    if e is ro.LunarLanderSynth:
        ro._all(ro.rew_close(e, state[:, 6], rp["state_out"][:, 6]), "prev_shaping")
    np.testing.assert_allclose(run["ep_ret"], rp["ret_out"], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(run["ep_len"], rp["len_out"])


# ------------------------------------------------------------------ a, b: full rollouts
SHAPES = [("wide", 37, 128), ("wide", 16, 128), ("wide", 1, 128), ("wide", 37, 64), ("tile", 517, 128),
          ("tile", 517, 64)]
FULL = [(name, kind, N, H) for name in ro.CASES for kind, N, H in SHAPES]


@lru_cache(maxsize=None)
def full_run(name, kind, N, H):
    c = ro.CASES[name]
    run = launch(name, kind, N, c["T"], H, c["seed"], c["step0"], c["max_steps"])
    run["rp"] = ro.replay(name, run, c["seed"], c["step0"], c["max_steps"])
    return run


@pytest.mark.parametrize("name,kind,N,H", FULL)
def test_full_rollout_replay(cuda, name, kind, N, H):
    run = full_run(name, kind, N, H)
    share = ro.assert_replay(name, run, run["rp"])
    print(f"{name} {kind} N={N} H={H}: {share:.4%} of {run['T'] * N} cells within {ro.EPS} of a threshold")
    check_policy(run)
    codes = set(np.unique(run["done"]).astype(int))
    if name == "LunarLanderSynth-v0":
        assert codes == {0, 1}  # every lander comes down inside 40 steps, none reaches step 1000
    elif name == "CartPole-v1" and N >= 16:
        assert codes == {0, 1, 2}  # poles that fall before step 12, and the time limit
    else:  # MountainCar / Acrobot / HalfCheetah end only by the time limit; so may 4 episodes of one pole
        assert 2 in codes and codes <= ({0, 1, 2} if name == "CartPole-v1" else {0, 2})


@pytest.mark.parametrize("name,kind,N,H", FULL)
def test_full_rollout_episode_stats_and_persistent_outputs(cuda, name, kind, N, H):
    run = full_run(name, kind, N, H)
    st = check_stats(run, [run["ep_stats"]])
    assert st["n_done"] > 0
    check_state(run, run["rp"])


def test_trainer_metrics_match_the_buffers_across_an_epoch_boundary(cuda):
    """VecTrainer's episode_sums() / metrics() of the second epoch, recomputed from its rew / done
    and the ep_len / ep_ret the first epoch left: an episode that spans the boundary counts once,
    with its full return.  (CartPole returns are small integers: every fp32 sum is exact.)"""
    from relayrl_prototype_amd.runtime.vec_trainer import VecTrainer, VecTrainerConfig

    tr = VecTrainer(VecTrainerConfig(num_envs=64, rollout_len=20, max_episode_steps=12, use_graphs=False, seed=2),
                    device=cuda)
    tr.rollout()
    torch.cuda.synchronize()
    len1, ret1 = tr.ep_len.cpu().numpy(), tr.ep_ret.cpu().numpy()
    assert (len1 > 0).any() and (ret1 == len1).all()
    tr.epoch += 1
    tr.rollout()
    torch.cuda.synchronize()
    st = ro.episode_stats(tr.rew.cpu().numpy(), tr.done.cpu().numpy(), len1, ret1)
    ep = st["episodes"]
    spans = ep["len"] > ep["t"] + 1  # longer than its steps in this epoch: it began in the first
    assert spans.any() and (ep["ret"][spans] == ep["len"][spans]).all()
    n, s = tr.episode_sums()
    assert (n, s) == (st["n_done"], st["sum_ret"])
    m = tr.metrics()
    assert m["Episodes"] == st["n_done"]
    assert m["AverageEpRet"] == st["sum_ret"] / st["n_done"]
    assert m["EpLen"] == st["sum_len"] / st["n_done"]
    assert (m["MaxEpRet"], m["MinEpRet"]) == (st["max_ret"], st["min_ret"])
    assert tr.average_ep_return() == st["sum_ret"] / st["n_done"]
    np.testing.assert_array_equal(tr.ep_len.cpu().numpy(), st["ep_len"])
    np.testing.assert_array_equal(tr.ep_ret.cpu().numpy(), st["ep_ret"])


# ------------------------------------------------------------------ c: injected boundary states
INJ_MAX_STEPS, INJ_SEED, INJ_STEP0 = 50, 9, 77


@pytest.mark.parametrize("kind,N", [("wide", 17), ("tile", 81)])
@pytest.mark.parametrize("name", list(ro.INJECTED))
def test_injected_boundary_states(cuda, name, kind, N):
    e = ro.env_of(name)
    state, ln, rt, rows = ro.injected_inputs(e, N, INJ_MAX_STEPS)
    kw = dict(state_in=state, len_in=ln, ret_in=rt)
    run = launch(name, kind, N, 2, 128, INJ_SEED, INJ_STEP0, INJ_MAX_STEPS, **kw)
    rp = ro.replay(e, run, INJ_SEED, INJ_STEP0, INJ_MAX_STEPS, **kw)
    ro.assert_replay(e, run, rp)
    st = check_stats(run, [run["ep_stats"]], ln, rt)
    check_state(run, rp)
    no_tobs = launch(name, kind, N, 2, 128, INJ_SEED, INJ_STEP0, INJ_MAX_STEPS, has_tobs=False, **kw)
    ro.assert_replay(e, no_tobs, ro.replay(e, no_tobs, INJ_SEED, INJ_STEP0, INJ_MAX_STEPS, has_tobs=False, **kw))
    check_stats(no_tobs, [no_tobs["ep_stats"]], ln, rt)
    ns, _, _, _ = e.step(state, run["act"][0], e.step_noise(INJ_SEED, INJ_STEP0, np.arange(N)), np.float64)
    seen = e.state_from_obs(run["obs"][1])
    ep = st["episodes"]
    for sc, row in zip(ro.INJECTED[name], rows):
        assert rp["margin"][0, row] > ro.EPS, sc.name
        code = sc.code(True)
        assert run["done"][0, row] == code, sc.name
        assert no_tobs["done"][0, row] == sc.code(False), sc.name
        assert np.isnan(run["tobs"][0, row]).all() == (code != 2), sc.name
        if sc.check is not None:  # the device's own next state where it shows, else its reward
            assert sc.check(seen[row] if code == 0 and not sc.two_steps else ns[row], float(run["rew"][0, row])), sc.name
        if sc.two_steps:
            assert (run["done"][:, row] == 0).all() and sc.check(run["state"][row], 0.0), sc.name
        if code:
            k = np.nonzero((ep["env"] == row) & (ep["t"] == 0))[0]
            assert len(k) == 1 and ep["len"][k[0]] == ln[row] + 1
            assert ep["ret"][k[0]] == np.float32(np.float32(rt[row]) + run["rew"][0, row])  # ep_ret input counted
            if run["done"][1, row] == 0:
                assert run["ep_len"][row] == 1  # the new episode counts from 0
    assert (run["done"][0, np.setdiff1d(np.arange(N), rows)] == 0).all()


# ------------------------------------------------------------------ d: continuation is bitwise
SPLITS = {"CartPole-v1": (7, 9), "MountainCar-v0": (5, 8), "Acrobot-v1": (5, 8), "LunarLanderSynth-v0": (24, 16),
          "HalfCheetahSynth-v0": (6, 5)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("kind,N", [("wide", 37), ("tile", 517)])
@pytest.mark.parametrize("name", list(ro.CASES))
def test_continuation_is_bitwise(cuda, name, kind, N):
    """Both ways do the same arithmetic on the same persisted fp32 state: any difference is a bug."""
    c, (T1, T2) = ro.CASES[name], SPLITS[name]
    a = (c["seed"], c["step0"], c["max_steps"])
    one = launch(name, kind, N, T1 + T2, 128, *a)
    first = launch(name, kind, N, T1, 128, *a)
    assert (first["ep_len"] > 0).any(), "no episode straddles the split"
    second = launch(name, kind, N, T2, 128, a[0], a[1] + T1, a[2], persist=first["persist"])
    for k in ("act", "logp", "rew", "done", "tobs"):
        assert np.array_equal(_bits(one[k]), _bits(np.concatenate([first[k], second[k]]))), k
    assert np.array_equal(_bits(one["obs"]), _bits(np.concatenate([first["obs"][:-1], second["obs"]]))), "obs"
    assert np.array_equal(_bits(first["obs"][-1]), _bits(second["obs"][0])), "obs at the split"
    for k in ("state", "ep_len", "ep_ret"):
        assert np.array_equal(_bits(one[k]), _bits(second[k])), k
    st = check_stats(one, [one["ep_stats"]])
    assert st["n_done"] > 0
    check_stats(one, [first["ep_stats"], second["ep_stats"]])
