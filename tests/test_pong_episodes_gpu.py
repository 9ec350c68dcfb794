"""The PongSynth step kernels (csrc/kernels/pong.hip) against the host oracle of
tests/pong_oracle.py, through the thread-per-env form (``hist=``), the step + render form
(``obs=``), the frame-ring form (``frames=``, the training default) and the head-fused form:

a. full runs replayed step by step: physics, points, serves, 21-point endings and truncations,
   Philox resets, ``fin_ret`` / ``fin_len``, ``ep_acc``, and the renders byte for byte;
b. the two forms of the step counter across the carry into its high word;
c. injected boundary states through ``reset_all = 0`` (ties and branches random play never meets);
d. the pixel trainer's metrics across epoch boundaries, rebuilt from its ``rew`` / ``done``.

Every output buffer is the middle of a larger sentinel-filled tensor whose guards must survive.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import hip

import pong_oracle as po
from guarded import BYTE_SENTINEL, DEV, Guarded

pytestmark = pytest.mark.gpu

R = 5                                # ring slots
PREFILL = (3.0, -7.0, 100.0, 60.0)   # ep_acc starts non-zero: the kernel must add, not store
EARLY = 20                           # ep_acc is also read after this many steps
OUTS = ("rew", "done", "fin_ret", "fin_len")
N, S = po.N_ENVS, po.STEPS


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _outs(shape):
    return {k: Guarded(shape) for k in OUTS}


def _check_guards(g):
    for k, b in g.items():
        assert b.guards_intact(), f"{k}: the kernel wrote outside its buffer"


def _download(g):
    return {k: b.t.cpu().numpy() for k, b in g.items()}


# ------------------------------------------------------------------ a: full replay
@lru_cache(maxsize=None)
def full_run(case, form):
    """S steps of N envs through ``DevicePong`` (device step counter), everything kept on the
    device and downloaded once."""
    from relayrl_prototype_amd.envs.pong import DevicePong, FrameRing

    c = po.CASES[case]
    acts = po.actions(S, N, c["act_seed"])
    acts_d = torch.from_numpy(acts).to(DEV)
    env = DevicePong(N, DEV, po.SEED, c["max_steps"])
    assert env.seed == po.SEED
    g = dict(state=Guarded((N * po.STATE,)), states=Guarded((S + 1, N, po.STATE)), ep_acc=Guarded((N, 4), fill=PREFILL),
             **{k + "0": Guarded((N,)) for k in OUTS}, **_outs((S, N)))
    env.state, env.ep_acc = g["state"].t, g["ep_acc"].t
    env.rew, env.done, env.fin_ret, env.fin_len = (g[k + "0"].t for k in OUTS)  # what the reset launch is handed
    env.step_count = po.STEP0
    ring = None
    if form == "hist":
        g["hist"] = Guarded((S + 1, N, 16))
        env.reset(hist_out=g["hist"].t[0])
    else:
        ring = FrameRing(N, R, DEV)
        g["frames"] = Guarded((R * N * po.FRAME_BYTES,), torch.uint8)
        g["fidx"] = Guarded((S + 1, N, 4), torch.int32)
        ring.frames = g["frames"].t
        env.reset(ring=(ring, g["fidx"].t[0]))
    g["states"].t[0].copy_(env.state.view(N, po.STATE))
    early = None
    for t in range(S):
        env.fin_ret, env.fin_len = g["fin_ret"].t[t], g["fin_len"].t[t]
        if ring is None:
            env.step(acts_d[t], None, g["rew"].t[t], g["done"].t[t], hist_out=g["hist"].t[t + 1])
        else:
            env.step(acts_d[t], g["fidx"].t[t + 1], g["rew"].t[t], g["done"].t[t], ring=ring)
        g["states"].t[t + 1].copy_(env.state.view(N, po.STATE))
        if t + 1 == EARLY:
            early = env.ep_acc.clone()
    stats = env.episode_stats().cpu().numpy()
    assert env.step_count == po.STEP0 + 1 + S
    torch.cuda.synchronize()
    _check_guards(g)
    run = _download(g)
    run.update(acts=acts, acc_early=early.cpu().numpy(), stats=stats, max_steps=c["max_steps"], form=form,
               abs_steps=[po.STEP0 + 1 + t for t in range(S)])
    return run


def check_full(run):
    """The host side of the full replay (numpy only)."""
    states, ms = run["states"], run["max_steps"]
    rp = po.replay(states, run["acts"], po.SEED, run["abs_steps"], ms, reset_step=po.STEP0)
    share = po.assert_replay(states, run, rp)
    print(f"max_steps={ms} {run['form']}: {share:.4%} of {rp.margin.size} cells within {po.EPS} of a threshold, "
          f"{(rp.margin == 0).mean():.2%} exactly on one, {int((run['done'] > 0).sum())} episodes")
    assert share <= po.MAX_SKIP_SHARE
    assert np.array_equal(run["state"].reshape(N, po.STATE), states[-1])
    for k in OUTS:  # the reset launch leaves them alone
        assert np.isnan(run[k + "0"]).all(), f"reset_all wrote {k}"
    ends = rp.rec.over[run["done"] > 0]
    if ms:
        assert (ends == po.OVER_TIME).all() and len(ends) == N * (S // ms)
    else:
        assert (ends == po.OVER_OPP).all() and len(ends) > 200  # 21-point endings, all lost by random play
    # ep_acc: the float64 accumulation from the prefill, exactly (small integers: every fp32 sum is exact)
    want = po.expected_ep_acc(PREFILL, run, rp)
    assert np.array_equal(run["ep_acc"].astype(np.float64), want)
    assert (want[:, 0] > PREFILL[0]).any()
    idle = ~(run["done"][:EARLY] > 0).any(0)
    assert idle.any()
    pre = np.tile(np.asarray(PREFILL, np.float32), (N, 1))
    assert np.array_equal(_bits(run["acc_early"][idle]), _bits(pre[idle])), "ep_acc touched where no episode ended"
    assert np.array_equal(run["acc_early"].astype(np.float64),
                          po.expected_ep_acc(PREFILL, {k: run[k][:EARLY] for k in OUTS},
                                             po.replay(states[:EARLY + 1], run["acts"][:EARLY], po.SEED,
                                                       run["abs_steps"][:EARLY], ms)))
    assert np.array_equal(run["stats"], run["ep_acc"].astype(np.float64).sum(0))  # DevicePong.episode_stats()
    return rp


def render_steps(run):
    """6 steps spread over the run: the first, the one with the most episode ends (its
    observation is the reset's), the one after it, and three more."""
    busiest = int((run["done"] > 0).sum(1).argmax())
    assert (run["done"][busiest] > 0).any()
    return sorted({0, busiest, min(busiest + 1, S - 1), S // 3, (2 * S) // 3 + 1, S - 1})


def relaunch(run, t, form):
    """Step t of a recorded run again, from its recorded state, in one launch of ``form``."""
    g = dict(state=Guarded((N * po.STATE,), fill=run["states"][t].reshape(-1)), ep_acc=Guarded((N, 4), fill=PREFILL),
             **_outs((N,)))
    kw = {}
    if form == "obs":
        g["obs"] = Guarded((N, 21, 21, 64), torch.uint8)
        kw = dict(obs=g["obs"].t)
    elif form == "frames":
        g["frames"] = Guarded((R * N * po.FRAME_BYTES,), torch.uint8)
        g["fidx"] = Guarded((N, 4), torch.int32)
        kw = dict(frames=g["frames"].t, fidx=g["fidx"].t, ring_slots=R)
    act = torch.from_numpy(run["acts"][t]).to(DEV)
    hip().pong_step(g["state"].t, act, *(g[k].t for k in OUTS), g["ep_acc"].t, N, po.SEED, run["abs_steps"][t],
                    run["max_steps"], False, None, **kw)
    torch.cuda.synchronize()
    _check_guards(g)
    out = _download(g)
    assert np.array_equal(_bits(out["state"].reshape(N, po.STATE)), _bits(run["states"][t + 1])), (form, t)
    for k in OUTS:
        assert np.array_equal(_bits(out[k]), _bits(run[k][t])), (form, t, k)
    return out


def check_ring_launch(out, state_after, abs_step, n):
    """One ring launch into an all-sentinel ring: the new frame in its slot, nothing else."""
    frames = out["frames"].reshape(R, n, po.FRAME_BYTES)
    slot = abs_step % R
    assert np.array_equal(frames[slot], po.frame(state_after[:, po.HIST:])), "the ring's new frame"
    assert (np.delete(frames, slot, 0) == BYTE_SENTINEL).all(), "ring bytes outside the written slot"
    assert np.array_equal(out["fidx"], po.ring_rows(state_after[:, po.VALID], abs_step, R, n)), "fidx"


@pytest.mark.parametrize("case", list(po.CASES))
def test_full_replay_thread_per_env(cuda, case):
    run = full_run(case, "hist")
    check_full(run)
    assert np.array_equal(_bits(run["hist"]), _bits(run["states"][:, :, po.HIST:])), "hist_out rows vs state slots 16..31"
    for t in render_steps(run):
        after = run["states"][t + 1]
        out = relaunch(run, t, "obs")
        assert np.array_equal(out["obs"], po.render(after[:, po.HIST:])), f"obs bytes after step {t}"
        out = relaunch(run, t, "frames")
        check_ring_launch(out, after, run["abs_steps"][t], N)


@pytest.mark.parametrize("case", list(po.CASES))
def test_full_replay_frame_ring(cuda, case):
    run = full_run(case, "ring")
    check_full(run)
    other = full_run(case, "hist")
    for k in ("states", "ep_acc") + OUTS:
        assert np.array_equal(_bits(run[k]), _bits(other[k])), f"{k}: ring form vs thread-per-env form"
    want = np.stack([po.ring_rows(run["states"][t][:, po.VALID], po.STEP0 + t, R, N) for t in range(S + 1)])
    assert np.array_equal(run["fidx"], want), "fidx of every step"
    assert (want[0] == want[0][:, :1]).all() and any(len(np.unique(r)) == 4 for r in want[-1])  # reset: one frame
    frames = run["frames"].reshape(R, N, po.FRAME_BYTES)
    for t in range(S + 1 - R, S + 1):  # the ring ends holding the frames of the last R steps
        assert np.array_equal(frames[(po.STEP0 + t) % R], po.frame(run["states"][t][:, po.HIST:])), t


# ------------------------------------------------------------------ b: step-counter forms
def counter_run(form, with_base):
    """Reset + 8 steps at counters CARRY_BASE ..: as host offset + device base, or as one host value."""
    steps = 8
    acts = po.actions(steps, N, po.CARRY_ACT_SEED)
    g = dict(state=Guarded((N * po.STATE,)), states=Guarded((steps + 1, N, po.STATE)), ep_acc=Guarded((N, 4), fill=PREFILL),
             **_outs((steps, N)))
    if form == "frames":
        g["frames"] = Guarded((R * N * po.FRAME_BYTES,), torch.uint8)
        g["fidx"] = Guarded((steps + 1, N, 4), torch.int32)
    else:
        g["hist"] = Guarded((steps + 1, N, 16))
    base = torch.full((1,), po.CARRY_BASE, dtype=torch.int64, device=DEV) if with_base else None
    spare = _outs((N,))
    dummy = torch.zeros(N, dtype=torch.int32, device=DEV)
    for t in range(steps + 1):
        kw = dict(frames=g["frames"].t, fidx=g["fidx"].t[t], ring_slots=R) if form == "frames" else dict(hist=g["hist"].t[t])
        outs = [spare[k].t for k in OUTS] if t == 0 else [g[k].t[t - 1] for k in OUTS]
        act = dummy if t == 0 else torch.from_numpy(acts[t - 1]).to(DEV)
        hip().pong_step(g["state"].t, act, *outs, g["ep_acc"].t, N, po.SEED, t if with_base else po.CARRY_BASE + t,
                        po.CARRY_MAX_STEPS, t == 0, base, **kw)
        g["states"].t[t].copy_(g["state"].t.view(N, po.STATE))
    torch.cuda.synchronize()
    _check_guards({**g, **spare})
    run = _download(g)
    run["acts"] = acts
    return run


@pytest.mark.parametrize("form", ["hist", "frames"])
def test_step_counter_forms_agree_across_the_carry(cuda, form):
    a, b = counter_run(form, True), counter_run(form, False)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{k}: (step, step_base) vs (step + base, None)"
    steps = len(a["acts"])
    abs_steps = [po.CARRY_BASE + 1 + t for t in range(steps)]
    assert abs_steps[0] < 2 ** 32 <= abs_steps[-1]
    rp = po.replay(a["states"], a["acts"], po.SEED, abs_steps, po.CARRY_MAX_STEPS, reset_step=po.CARRY_BASE)
    assert po.assert_replay(a["states"], a, rp) <= po.MAX_SKIP_SHARE
    assert (a["done"][po.CARRY_MAX_STEPS - 1] == 1).all()  # resets drawn with the high counter word set
    assert np.array_equal(a["ep_acc"].astype(np.float64), po.expected_ep_acc(PREFILL, a, rp))
    if form == "frames":
        want = np.stack([po.ring_rows(a["states"][t][:, po.VALID], po.CARRY_BASE + t, R, N) for t in range(steps + 1)])
        assert np.array_equal(a["fidx"], want)
    else:
        assert np.array_equal(_bits(a["hist"]), _bits(a["states"][:, :, po.HIST:]))


# ------------------------------------------------------------------ c: injected boundary states
NI = 96


def injected_launch(form, state, act, max_steps, ep_acc=True, head_action=None):
    """One ``reset_all = 0`` launch of ``form`` over the injected ``state``; ``head_action``: the
    head-fused kernel, with a zero ``part`` and a bias of 50 on that action."""
    g = dict(state=Guarded((NI * po.STATE,), fill=state.reshape(-1)), **_outs((NI,)))
    if ep_acc:
        g["ep_acc"] = Guarded((NI, 4), fill=PREFILL)
    acc = g["ep_acc"].t if ep_acc else None
    kw = {}
    if form in ("obs", "head"):
        g["obs"] = Guarded((NI, 21, 21, 64), torch.uint8)
        kw = dict(obs=g["obs"].t)
    elif form == "frames":
        g["frames"] = Guarded((R * NI * po.FRAME_BYTES,), torch.uint8)
        g["fidx"] = Guarded((NI, 4), torch.int32)
        kw = dict(frames=g["frames"].t, fidx=g["fidx"].t, ring_slots=R)
    else:
        g["hist"] = Guarded((NI, 16))
        kw = dict(hist=g["hist"].t)
    outs = [g[k].t for k in OUTS]
    if form == "head":
        A, F = 6, 512
        hp = torch.zeros(A * F + A + F + 1, device=DEV)
        hp[A * F + head_action] = 50.0
        g.update(act=Guarded((NI,), torch.int32), logp=Guarded((NI,)), value=Guarded((NI,)),
                 h=Guarded((NI * F,), torch.bfloat16))
        hip().pong_head_step(torch.zeros(NI * F, device=DEV), 1, torch.zeros(F, device=DEV), hp, A, g["h"].t, g["act"].t,
                             g["logp"].t, g["value"].t, 1, 0, None, g["state"].t, *outs, acc, g["obs"].t, NI, po.INJ_SEED,
                             po.INJ_STEP, None, int(max_steps))
    else:
        hip().pong_step(g["state"].t, torch.from_numpy(act).to(DEV), *outs, acc, NI, po.INJ_SEED, po.INJ_STEP,
                        int(max_steps), False, None, **kw)
    torch.cuda.synchronize()
    _check_guards(g)
    h = g.pop("h", None)
    out = _download(g)
    if h is not None:
        assert (h.t == 0).all()
    out["state"] = out["state"].reshape(NI, po.STATE)
    return out


def check_injected(out, form, state, act, max_steps):
    """A launch with one time limit for all rows against the oracle: replay, ep_acc, renders."""
    states = np.stack([state, out["state"]])
    outs = {k: out[k][None] for k in OUTS}
    rp = po.replay(states, act[None], po.INJ_SEED, [po.INJ_STEP], int(max_steps))
    po.assert_replay(states, outs, rp)
    if "ep_acc" in out:
        assert np.array_equal(out["ep_acc"].astype(np.float64), po.expected_ep_acc(PREFILL, outs, rp))
        idle = out["done"] == 0
        assert np.array_equal(_bits(out["ep_acc"][idle]), _bits(np.tile(np.asarray(PREFILL, np.float32), (NI, 1))[idle]))
    if form in ("obs", "head"):
        assert np.array_equal(out["obs"], po.render(out["state"][:, po.HIST:])), "obs bytes"
    elif form == "frames":
        check_ring_launch(out, out["state"], po.INJ_STEP, NI)
    else:
        assert np.array_equal(_bits(out["hist"]), _bits(out["state"][:, po.HIST:]))


@pytest.mark.parametrize("form", ["hist", "obs", "frames"])
def test_injected_boundary_states(cuda, form):
    state, act, ms, rows = po.scenario_inputs(NI)
    merged = {k: np.zeros((1, NI), np.float32) for k in OUTS}
    after = np.zeros_like(state)
    for limit in np.unique(ms):
        out = injected_launch(form, state, act, limit)
        check_injected(out, form, state, act, limit)
        bare = injected_launch(form, state, act, limit, ep_acc=False)  # ep_acc=None is accepted
        for k in ("state",) + OUTS:
            assert np.array_equal(_bits(bare[k]), _bits(out[k])), k
        pick = ms == limit
        after[pick] = out["state"][pick]
        for k in OUTS:
            merged[k][0][pick] = out[k][pick]
    po.assert_scenarios(np.stack([state, after]), merged, act, rows)  # every row under its scenario's own limit
    ends = {s.name for s, d in zip(po.SCENARIOS, merged["done"][0]) if d > 0}
    assert ends == {"agent_win", "opponent_win", "time_limit", "time_limit_with_point"}


@pytest.mark.parametrize("action", [2, 3])  # up, down
def test_injected_boundary_states_head_fused(cuda, action):
    state, _, _, _ = po.scenario_inputs(NI)
    out = injected_launch("head", state, None, po.INJ_MAX_STEPS, head_action=action)
    assert (out["act"] == action).all()  # the other five share exp(-50)
    assert np.allclose(out["logp"], 0.0, atol=1e-6) and (out["value"] == 0).all()
    check_injected(out, "head", state, out["act"], po.INJ_MAX_STEPS)
    same = injected_launch("obs", state, out["act"], po.INJ_MAX_STEPS)
    for k in ("state", "obs", "ep_acc") + OUTS:
        assert np.array_equal(_bits(out[k]), _bits(same[k])), k


# ------------------------------------------------------------------ d: trainer metrics
def test_trainer_metrics_match_the_buffers_across_epoch_boundaries(cuda):
    """PixelA2CTrainer on its default path (frame ring, fused head, one eager update, then
    captured graphs): metrics() and the episode_sums() deltas, rebuilt on the host from ``rew`` and
    ``done`` with the partial returns carried across epochs.  Rewards are +-1 and 0: every sum is
    exact.  The time limit is set before the first update; nothing is captured before it."""
    from relayrl_prototype_amd.runtime.pixel_trainer import PixelA2CConfig, PixelA2CTrainer

    E, T, limit = 64, 5, 7
    tr = PixelA2CTrainer(PixelA2CConfig(num_envs=E, rollout_len=T, seed=3), device=cuda)
    assert tr.ring is not None and tr.fused_head and not tr._graphs and tr.updates == 0
    tr.env.max_steps = limit
    ret, ln = np.zeros(E), np.zeros(E, np.int64)
    n = sum_ret = sum_len = 0.0
    for epoch in range(4):
        tr.train_epoch()
        torch.cuda.synchronize()
        rew, done = tr.rew.clone().cpu().numpy().astype(np.float64), tr.done.clone().cpu().numpy()
        n_e = s_e = 0.0
        for t in range(T):
            ret += rew[t]
            ln += 1
            d = done[t] > 0
            assert (ln[d] == limit).all() and (ln < limit)[~d].all()
            n_e += d.sum()
            s_e += ret[d].sum()
            sum_len += ln[d].sum()
            ret[d], ln[d] = 0.0, 0
        assert tr.episode_sums() == (n_e, s_e), epoch
        n, sum_ret = n + n_e, sum_ret + s_e
    assert tr._graphs, "the later updates replay captured graphs"
    assert n == E * ((4 * T) // limit) and (ln == (4 * T) % limit).all()
    m = tr.metrics()
    assert m["Episodes"] == n
    assert m["AverageEpRet"] == sum_ret / n
    assert m["EpLen"] == sum_len / n == limit
