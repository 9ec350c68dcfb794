"""Pixel policy evaluation on the GPU: ``rrl_pong_eval_step`` (csrc/kernels/pong.hip) driven step by
step through ``DevicePong.eval_step`` -- conv stack, fc split-K GEMM, head + env step + render --
against the host oracle of tests/pong_oracle.py, the slot bookkeeping rebuilt from the trace
(tests/pixel_eval_helpers.py) and the model's own head; then the driver and the trainer above it.

a. constant policy (all head parameters zero: every logit ties, the lowest index wins), natural
   21-point endings, E = 2, frame ring;  b. the freeze of an env after its E-th episode;
c. time limit, E = 3, s2d observations;  d. a real network: logits and first argmax bitwise;
e. sampled mode bitwise ``DeviceNatureCNN.act``;  f. the trainer is left as it was;  g. refusals.

Every output sits in a sentinel-filled ``Guarded`` buffer whose guards must survive.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import pong_oracle as po
from guarded import DEV, INT_SENTINEL, Guarded
from pixel_eval_helpers import rebuild_slots

pytestmark = pytest.mark.gpu

N = 37   # no multiple of 4, a partial 128-row fc tile, odd ring rows
R = 5    # ring slots
A = 6
OUTS = ("rew", "done", "fin_ret", "fin_len")
POLL = 32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _model(seed, zero_head):
    from relayrl_prototype_amd.models.nature_cnn import CNNSpec, DeviceNatureCNN

    spec = CNNSpec(act_dim=A)
    params = spec.init(seed)
    if zero_head:
        params[spec.offsets()["head"]:] = 0.0
    return DeviceNatureCNN(spec, DEV, max_batch=N, params=params)


@lru_cache(maxsize=None)
def run(case):
    """One evaluation of N envs driven by the test itself, everything recorded on the device and
    downloaded once."""
    from relayrl_prototype_amd.envs.pong import DevicePong, FrameRing
    from relayrl_prototype_amd.models.nature_cnn import FC_IN, HIDDEN

    c = dict(constant=dict(E=2, max_steps=6750, S=992, ring=True, zero_head=True, greedy=True),
             limit=dict(E=3, max_steps=24, S=80, ring=False, zero_head=True, greedy=True),
             network=dict(E=1, max_steps=40, S=44, ring=True, zero_head=False, greedy=True),
             sampled=dict(E=1, max_steps=40, S=8, ring=True, zero_head=False, greedy=False))[case]
    E, S, ms = c["E"], c["S"], c["max_steps"]
    m = _model(0, c["zero_head"])
    env = DevicePong(N, DEV, po.SEED, ms)
    g = dict(state=Guarded((N * po.STATE,)), states=Guarded((S + 1, N, po.STATE)), **{k: Guarded((S, N)) for k in OUTS},
             **{k + "0": Guarded((N,)) for k in OUTS},
             # slots: an extra row E that no episode may reach
             ep_ret=Guarded((E + 1, N)), ep_len=Guarded((E + 1, N), torch.int32), ep_code=Guarded((E + 1, N), torch.int32),
             ep_cnt=Guarded((N,), torch.int32, fill=0), remaining=Guarded((1,), torch.int32, fill=N),
             cnts=Guarded((S, N), torch.int32), rems=Guarded((S,), torch.int32),
             # the slot tensors after every step
             rets=Guarded((S, E + 1, N)), lens=Guarded((S, E + 1, N), torch.int32), codes=Guarded((S, E + 1, N), torch.int32),
             tr_act=Guarded((S, N), torch.int32), tr_logits=Guarded((S, N, A)), tr_rew=Guarded((S, N)),
             tr_done=Guarded((S, N)))
    env.state = g["state"].t
    env.rew, env.done, env.fin_ret, env.fin_len = (g[k + "0"].t for k in OUTS)
    env.step_count = po.STEP0
    ring = None
    if c["ring"]:
        ring = FrameRing(N, R, DEV)
        g["frames"] = Guarded((R * N * po.FRAME_BYTES,), torch.uint8)
        g["fidx"] = Guarded((S + 1, N, 4), torch.int32)
        ring.frames = g["frames"].t
        env.reset(ring=(ring, g["fidx"].t[0]))
        frozen_frames = torch.zeros(R, N, po.FRAME_BYTES, dtype=torch.uint8, device=DEV)  # at the env's freeze
    else:
        g["obs"] = Guarded((N, 21, 21, 64), torch.uint8)
        env.reset(g["obs"].t)
        obs_at = {}
    g["states"].t[0].copy_(env.state.view(N, po.STATE))
    fc_b, hp = m.head_params()
    a3, wfc = m._rows(m.a3, 0, N, FC_IN), m.shadow[m.o["wfc"]:m.o["bfc"]]
    ref_logits = torch.zeros(S, N, A, device=DEV)
    ref_act = torch.full((S, N), INT_SENTINEL, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(2, N, device=DEV)
    was_frozen = torch.zeros(N, dtype=torch.bool, device=DEV)
    for t in range(S):
        cur = g["fidx"].t[t] if ring is not None else g["obs"].t
        x = ring.obs(cur) if ring is not None else cur
        if case == "network":    # the model's own head on the pre-step observation
            ref_logits[t] = m.logits(x)[0]
        elif case == "sampled":  # the rollout's draw for the same observation, seed and step
            m.act(x, 0, ref_act[t], scratch[0], scratch[1], 77, 1000 + t)
        m.forward(x, 0, fc=False, store_acts=False)
        used = int(m.h.fc_nt_part(a3, wfc, m._fc_part, N, HIDDEN, FC_IN, m.fc_splits(N)))
        env.fin_ret, env.fin_len = g["fin_ret"].t[t], g["fin_len"].t[t]
        if ring is not None:
            g["fidx"].t[t + 1].copy_(cur)  # the step rewrites the rows of the envs that step
        out = g["fidx"].t[t + 1] if ring is not None else cur
        env.eval_step(m._fc_part, used, fc_b, hp, A, 77, 1000 + t, po.STEP0 + 1 + t, out, E, g["ep_cnt"].t,
                      g["ep_ret"].t, g["ep_len"].t, g["ep_code"].t, g["remaining"].t, greedy=c["greedy"], ring=ring,
                      trace=(g["tr_act"].t[t], g["tr_logits"].t[t], g["tr_rew"].t[t], g["tr_done"].t[t]),
                      rew_out=g["rew"].t[t], done_out=g["done"].t[t])
        g["states"].t[t + 1].copy_(env.state.view(N, po.STATE))
        g["cnts"].t[t].copy_(g["ep_cnt"].t)
        g["rems"].t[t].copy_(g["remaining"].t[0])
        for k, rec in (("ep_ret", "rets"), ("ep_len", "lens"), ("ep_code", "codes")):
            g[rec].t[t].copy_(g[k].t)
        if ring is not None:
            now = g["ep_cnt"].t >= E
            frozen_frames = torch.where((now & ~was_frozen)[None, :, None], ring.frames.view(R, N, -1), frozen_frames)
            was_frozen = now
        elif t in (0, 23, 24, 71):  # the first step, the last of an episode, a reset's observation, the last step
            obs_at[t] = g["obs"].t.clone()
    torch.cuda.synchronize()
    for k, b in g.items():
        assert b.guards_intact(), f"{k}: the kernel wrote outside its buffer"
    out = {k: b.t.cpu().numpy() for k, b in g.items()}
    out.update(E=E, S=S, max_steps=ms, model=m, abs_steps=[po.STEP0 + 1 + t for t in range(S)],
               ref_logits=ref_logits.cpu().numpy(), ref_act=ref_act.cpu().numpy())
    if ring is not None:
        out["frozen_frames"] = frozen_frames.cpu().numpy().reshape(-1)
    else:
        out["obs_at"] = {t: o.cpu().numpy() for t, o in obs_at.items()}
    return out


def check_bookkeeping(r):
    """Replay of the stepped cells, and slots / counters against their host rebuild."""
    E = r["E"]
    hb = rebuild_slots(r["tr_rew"], r["tr_done"], E)
    act = hb.active
    # the trace is written exactly where the env stepped
    assert (r["tr_act"][act] != INT_SENTINEL).all() and (r["tr_act"][~act] == INT_SENTINEL).all()
    for k in ("tr_rew", "tr_done"):
        assert not np.isnan(r[k][act]).any() and np.isnan(r[k][~act]).all(), k
    assert not np.isnan(r["tr_logits"][act]).any() and np.isnan(r["tr_logits"][~act]).all()
    for k in ("rew", "done"):
        assert np.array_equal(_bits(r[k][act]), _bits(r["tr_" + k][act])), k
    # teacher-forced replay of the stepped cells (a frozen env's row is no step: excluded)
    acts = np.where(act, r["tr_act"], 0)
    rp = po.replay(r["states"], acts, po.SEED, r["abs_steps"], r["max_steps"], reset_step=po.STEP0)
    near = ~po.compared(rp.margin) & act
    rp.margin = np.where(act, rp.margin, po.EPS / 2)  # not compared
    po.assert_replay(r["states"], r, rp)
    share = near.sum() / act.sum()
    print(f"{act.sum()} stepped cells, {share:.2e} within {po.EPS} of a threshold, "
          f"{(rp.margin[act] == 0).mean():.2%} exactly on one; all envs done after {int(act.any(1).sum())} steps")
    assert share <= po.MAX_SKIP_SHARE
    for k in OUTS:  # the env's own reset-time buffers are never written
        assert np.isnan(r[k + "0"]).all(), k
    # slots, counters
    assert np.array_equal(r["cnts"], hb.ep_cnt) and np.array_equal(r["ep_cnt"], hb.ep_cnt[-1])
    assert np.array_equal(r["rems"], hb.remaining) and r["remaining"][0] == hb.remaining[-1] == 0
    assert (hb.ep_cnt[-1] == E).all()
    assert np.array_equal(r["ep_ret"][:E].astype(np.float64), hb.ep_ret)
    assert np.array_equal(r["ep_len"][:E], hb.ep_len) and np.array_equal(r["ep_code"][:E], hb.ep_code)
    assert np.isnan(r["ep_ret"][E]).all() and (r["ep_len"][E] == INT_SENTINEL).all() and \
        (r["ep_code"][E] == INT_SENTINEL).all(), "a slot beyond E was written"
    return hb, rp


def check_freeze(r, hb):
    """From the step an env finishes its E-th episode on, nothing of it changes."""
    act = hb.active
    st = r["states"]
    idle = ~act
    assert idle.any()
    assert np.array_equal(_bits(st[1:][idle]), _bits(st[:-1][idle])), "a frozen env's state row moved"
    assert np.array_equal(r["state"].reshape(N, po.STATE), st[-1])
    if "fidx" in r:
        assert np.array_equal(r["fidx"][1:][idle], r["fidx"][:-1][idle]), "a frozen env's fidx row moved"
        assert np.array_equal(r["frames"], r["frozen_frames"]), "a frozen env's ring frames were rewritten"
    # at every step: slot k is written exactly when k < ep_cnt, and then holds its final value
    written = np.arange(r["E"] + 1)[None, :, None] < hb.ep_cnt[:, None, :]          # [S, E + 1, N]
    assert np.array_equal(~np.isnan(r["rets"]), written), "ep_ret slots vs ep_cnt"
    for k, rec in (("ep_len", "lens"), ("ep_code", "codes")):
        assert np.array_equal(r[rec] != INT_SENTINEL, written), f"{k} slots vs ep_cnt"
        assert (r[rec] == r[k][None])[written].all(), f"a written {k} slot changed later"
    assert (_bits(r["rets"]) == _bits(r["ep_ret"])[None])[written].all(), "a written ep_ret slot changed later"


# ------------------------------------------------------------------ a, b
def test_constant_policy_natural_endings(cuda):
    r = run("constant")
    assert (r["tr_logits"][~np.isnan(r["tr_logits"])] == 0).all(), "zero head parameters: every logit is 0"
    hb, rp = check_bookkeeping(r)
    assert (r["tr_act"][hb.active] == 0).all(), "all logits tie: the lowest index"
    assert (r["ep_code"][:2] == 1).all()
    assert (hb.points.max(-1) == 21).all(), "every episode ended on its 21st point"
    ends = rp.rec.over[hb.active & (r["tr_done"] > 0)]
    assert np.isin(ends, (po.OVER_AGENT, po.OVER_OPP)).all() and len(ends) == 2 * N


def test_frozen_envs_are_left_alone(cuda):
    r = run("constant")
    hb = rebuild_slots(r["tr_rew"], r["tr_done"], r["E"])
    first, last = hb.active.sum(0).min(), hb.active.sum(0).max()
    assert first < last < r["S"], "envs freeze at different steps, all before the run ends"
    check_freeze(r, hb)


def test_driver_stops_on_the_device_counter(cuda):
    """evaluate_pixel_policy on the same model, seed and counters: the same tensors, and it stops at
    the first poll after the last env finished."""
    from relayrl_prototype_amd.runtime.evaluate import evaluate_pixel_policy

    r = run("constant")
    done_at = int(rebuild_slots(r["tr_rew"], r["tr_done"], 2).active.any(1).sum())
    res = evaluate_pixel_policy(r["model"], 2, N, greedy=True, seed=po.SEED, step0=po.STEP0, max_episode_steps=6750,
                                poll_every=POLL)
    assert res.steps == -(-done_at // POLL) * POLL, (res.steps, done_at)
    assert int(res.remaining.item()) == 0 and (res.ep_cnt == 2).all()
    assert np.array_equal(_bits(res.ep_ret.cpu().numpy()), _bits(r["ep_ret"][:2]))
    assert np.array_equal(res.ep_len.cpu().numpy(), r["ep_len"][:2])
    assert np.array_equal(res.ep_code.cpu().numpy(), r["ep_code"][:2])
    s = res.stats()
    assert s["episodes"] == 2 * N and s["truncated_share"] == 0.0
    # (float64 means of the same integers in two summation orders: the last bit may differ)
    assert s["mean_return"] == pytest.approx(r["ep_ret"][:2].astype(np.float64).mean(), rel=1e-12, abs=0)


# ------------------------------------------------------------------ c
def test_time_limit_s2d_observations(cuda):
    r = run("limit")
    hb, rp = check_bookkeeping(r)
    assert hb.active[:72].all() and not hb.active[72:].any(), "3 episodes of 24 steps"
    assert (r["ep_code"][:3] == 2).all() and (r["ep_len"][:3] == 24).all()
    assert (r["tr_act"][:72] == 0).all()
    check_freeze(r, hb)
    assert sorted(r["obs_at"]) == [0, 23, 24, 71]
    for t, obs in r["obs_at"].items():
        assert np.array_equal(obs, po.render(r["states"][t + 1][:, po.HIST:])), f"obs bytes after step {t}"
    assert np.array_equal(r["obs"], po.render(r["states"][72][:, po.HIST:])), "a frozen env's observation"


# ------------------------------------------------------------------ d
def test_real_network_logits_and_argmax_are_the_models(cuda):
    r = run("network")
    hb, _ = check_bookkeeping(r)
    act = hb.active
    assert act[:40].all() and not act[40:].any() and (r["ep_code"][:1] == 2).all()
    assert np.array_equal(_bits(r["tr_logits"][act]), _bits(r["ref_logits"][act])), "logits vs DeviceNatureCNN.logits"
    assert np.array_equal(r["tr_act"][act], r["ref_logits"][act].argmax(-1)), "the first argmax of the device logits"
    assert len(np.unique(r["tr_act"][act])) >= 2, "one action only: the argmax check is vacuous, pick another seed"
    check_freeze(r, hb)


# ------------------------------------------------------------------ e
def test_sampled_mode_draws_what_act_draws(cuda):
    r = run("sampled")
    assert (r["ref_act"] >= 0).all()
    assert np.array_equal(r["tr_act"], r["ref_act"])
    assert len(np.unique(r["tr_act"])) >= 2
    rp = po.replay(r["states"], r["tr_act"], po.SEED, r["abs_steps"], r["max_steps"], reset_step=po.STEP0)
    po.assert_replay(r["states"], r, rp)


# ------------------------------------------------------------------ f
def test_trainer_is_left_as_it_was(cuda):
    from relayrl_prototype_amd.runtime.pixel_trainer import PixelA2CConfig, PixelA2CTrainer

    def trainer():
        return PixelA2CTrainer(PixelA2CConfig(num_envs=64, rollout_len=5, seed=3, max_episode_steps=8), device=cuda)

    a, b = trainer(), trainer()
    evals = []
    for u in range(4):
        a.train_epoch()
        b.train_epoch()
        if u in (1, 3):
            evals.append(b.evaluate(episodes=1, num_envs=37))
    torch.cuda.synchronize()
    assert a._graphs and b._graphs, "the later updates replay captured graphs"
    for name in ("params", "m", "v", "step_t", "shadow"):  # compared as bits
        ta, tb = getattr(a.model, name), getattr(b.model, name)
        bits = {4: torch.int32, 2: torch.int16, 8: torch.int64}[ta.element_size()]
        assert torch.equal(ta.view(bits), tb.view(bits)), name
    assert torch.equal(a.env.state.view(torch.int32), b.env.state.view(torch.int32))
    assert torch.equal(a.env.ep_acc, b.env.ep_acc) and torch.equal(a.sample_t, b.sample_t)
    assert torch.equal(a.env.step_t, b.env.step_t) and a.env.step_count == 1 + 4 * 5
    assert a.metrics() == b.metrics()
    e0, e1 = evals
    assert e0.step0 == 0 and e1.step0 > e0.step0 and e0.seed == e1.seed == b.eval_seed
    for e in evals:
        s = e.stats()
        assert s["episodes"] == 37 and s["mean_length"] == 8.0 and s["truncated_share"] == 1.0
    with pytest.raises(ValueError, match="num_envs"):
        b.evaluate(episodes=1, num_envs=65)


# ------------------------------------------------------------------ g
def test_argument_refusals(cuda):
    """Host-side checks only: every call is refused before a launch (the buffers keep their fill)."""
    from relayrl_prototype_amd.ops import hip

    F, E = 512, 2
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    i32 = torch.int32

    def call(E=E, max_steps=10, slots_n=N, trace=4, A=A):
        tr = [z(N, dt=i32), z(N, A), z(N), z(N)][:trace]
        kw = dict(zip(("tr_act", "tr_logits", "tr_rew", "tr_done"), tr))
        hip().pong_eval_step(z(N * F), 1, z(F), z(A * F + A + F + 1), A, True, 1, 0, state, z(N), z(N), z(N), z(N),
                             z(N, 21, 21, 64, dt=torch.uint8), N, 1, 7, max_steps, E, z(N, dt=i32),
                             z(max(E, 1), slots_n), z(max(E, 1), N, dt=i32), z(max(E, 1), N, dt=i32),
                             torch.full((1,), N, dtype=i32, device=DEV), **kw)

    state = torch.full((N * po.STATE,), 3.0, device=DEV)
    for kw in (dict(E=0), dict(max_steps=0), dict(trace=3), dict(slots_n=N - 1), dict(A=9)):
        with pytest.raises(RuntimeError):
            call(**kw)
    torch.cuda.synchronize()
    assert (state == 3.0).all(), "a refused call launched"
