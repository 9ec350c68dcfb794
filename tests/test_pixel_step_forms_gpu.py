"""The three one-workgroup-per-env PongSynth kernels against each other.  ``pong_step_render_kernel``,
``pong_head_step_render_kernel`` and ``pong_eval_step_kernel`` are one body (csrc/kernels/pong.hip
``pong_env_workgroup``) that differs in where the action comes from and in what thread 0 does after
the physics.  So, from one seed and one starting step, and fed the same fc partials,

(i)   ``DeviceNatureCNN.act`` then ``DevicePong.step``,
(ii)  ``DevicePong.step_head`` and
(iii) ``DevicePong.eval_step(greedy=False)``

write the same bits after every step: state, rewards, dones, finished-episode totals, the picture
(s2d observations, or ring frames and frame rows) and the actions; (i) and (ii) also the same episode
accumulators.  It holds while no env has finished its E evaluation episodes (asserted at the end).
Every output sits in a sentinel-filled ``Guarded`` buffer whose guards must survive.
"""
import pytest
import torch

import pong_oracle as po
from guarded import DEV, Guarded
from test_pixel_evaluate_gpu import A, N, R, _model

pytestmark = pytest.mark.gpu

T = 12         # steps
MAX_STEPS = 5  # every env is reset at steps 5 and 10 of the window
E = 4          # more episodes than 12 steps of <= 5 can finish: no env freezes
OUTS = ("state", "rew", "done", "fin_ret", "fin_len")
FORMS = ("act + step", "step_head", "eval_step")


def _same_bits(a, b):
    bits = {1: torch.uint8, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(bits), b.view(bits))


@pytest.mark.parametrize("form", ["s2d", "ring"])
def test_the_three_step_kernels_write_the_same_bits(cuda, form):
    from relayrl_prototype_amd.envs.pong import DevicePong, FrameRing

    m = _model(0, zero_head=False)
    fc_b, hp = m.head_params()
    envs, bufs, rings = [], [], []
    for _ in FORMS:
        env = DevicePong(N, DEV, po.SEED, MAX_STEPS)
        g = dict(state=Guarded((N * po.STATE,)), ep_acc=Guarded((N, 4), fill=0.0), act=Guarded((N,), torch.int32),
                 **{k: Guarded((N,)) for k in OUTS[1:]})
        env.state, env.ep_acc = g["state"].t, g["ep_acc"].t
        env.rew, env.done, env.fin_ret, env.fin_len = (g[k].t for k in OUTS[1:])
        env.step_count = po.STEP0
        if form == "ring":
            ring = FrameRing(N, R, DEV)
            g["frames"] = Guarded((R * N * po.FRAME_BYTES,), torch.uint8)
            g["fidx"] = Guarded((N, 4), torch.int32)
            ring.frames = g["frames"].t
            env.reset(ring=(ring, g["fidx"].t))
        else:
            ring = None
            g["obs"] = Guarded((N, 21, 21, 64), torch.uint8)
            env.reset(g["obs"].t)
        envs.append(env)
        bufs.append(g)
        rings.append(ring)
    picture = ("frames", "fidx") if form == "ring" else ("obs",)
    out = [g["fidx" if form == "ring" else "obs"].t for g in bufs]
    ev = dict(ep_cnt=Guarded((N,), torch.int32, fill=0), ep_ret=Guarded((E, N)), ep_len=Guarded((E, N), torch.int32),
              ep_code=Guarded((E, N), torch.int32), remaining=Guarded((1,), torch.int32, fill=N),
              tr_logits=Guarded((N, A)), tr_rew=Guarded((N,)), tr_done=Guarded((N,)))
    logp, value = Guarded((2, N)), Guarded((2, N))
    resets, actions = 0, set()
    for t in range(T):
        step = po.STEP0 + 1 + t  # the reset took step STEP0
        assert envs[0].step_count == envs[1].step_count == step, "eval_step's host step is the others' absolute step"
        x = rings[0].obs(out[0]) if form == "ring" else out[0]
        m.act(x, 0, bufs[0]["act"].t, logp.t[0], value.t[0], 77, 1000 + t)
        part, used, hid = m.forward_fc_partials(x, 0)
        envs[0].step(bufs[0]["act"].t, out[0], ring=rings[0])
        envs[1].step_head(part, used, fc_b, hp, A, hid, bufs[1]["act"].t, logp.t[1], value.t[1], 77, 1000 + t, None,
                          out[1], ring=rings[1])
        envs[2].eval_step(part, used, fc_b, hp, A, 77, 1000 + t, step, out[2], E, ev["ep_cnt"].t, ev["ep_ret"].t,
                          ev["ep_len"].t, ev["ep_code"].t, ev["remaining"].t, greedy=False, ring=rings[2],
                          trace=(bufs[2]["act"].t, ev["tr_logits"].t, ev["tr_rew"].t, ev["tr_done"].t))
        torch.cuda.synchronize()
        for k in OUTS + picture + ("act",):
            for j in (1, 2):
                assert _same_bits(bufs[0][k].t, bufs[j][k].t), f"step {t}: {k} of {FORMS[j]} differs from {FORMS[0]}"
        assert _same_bits(bufs[0]["ep_acc"].t, bufs[1]["ep_acc"].t), f"step {t}: ep_acc"
        assert _same_bits(logp.t[0], logp.t[1]) and _same_bits(value.t[0], value.t[1]), f"step {t}: logp / value"
        resets += int((bufs[0]["done"].t != 0).sum())
        actions.update(bufs[0]["act"].t.tolist())
    print(f"{form}: {resets} resets, actions {sorted(actions)}")
    for g in bufs + [ev, dict(logp=logp, value=value)]:
        for k, b in g.items():
            assert b.guards_intact(), f"{k}: a kernel wrote outside its buffer"
    assert int(ev["ep_cnt"].t.max()) < E, "an env froze: the forms are only equal while every env steps"
    assert resets >= 1 and bufs[0]["ep_acc"].t[:, 0].sum() == resets
    assert len(actions) >= 2 and min(actions) >= 0 and max(actions) < A
