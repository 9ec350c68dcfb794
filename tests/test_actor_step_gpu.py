"""The actor kernels against each other.  The rollout, evaluation and DQN kernels are assembled from
one step (csrc/kernels/actor_step.h): the same Philox coordinates, resets, observation tile and
forward pass.  So, from one seed and one ``step0``,

a. ``evaluate(greedy=0)`` traces bit for bit what ``rollout`` writes (CartPole: many resets;
   LunarLanderSynth: a shaped reward, which two separately written kernels once contracted
   differently; HalfCheetah: ``evaluate_cont`` against ``rollout_cont``), in the tile-stride form
   at 517 envs;
b. ``dqn_rollout(epsilon=0)`` fills its ring with what ``evaluate(greedy=1)`` traces.

Both hold over the window in which no env has finished its E evaluation episodes (``window_bufs``
asserts it).  The one-workgroup-per-tile rollout kernel is not compared: it sums the layer-2
partials in another order.
"""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import dqn_rollout, dqn_rollout_grid

import rollout_oracle as ro
from guarded import INT_SENTINEL, Guarded
from test_dqn_gpu import guarded_ring
from test_evaluate_gpu import CASES, WINDOW_E, launch as evaluate_launch, window_bufs, window_run
from test_rollout_episodes_gpu import launch as rollout_launch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    differ = int((got.view(np.int32) != want.view(np.int32)).sum())
    print(f"{what}: {differ} of {got.size} cells differ")
    assert differ == 0, what


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("name", ["CartPole-v1", "LunarLanderSynth-v0", "HalfCheetahSynth-v0"])
def test_sampled_evaluation_traces_the_rollout(cuda, name, H):
    c, N = CASES[name], 517
    bufs, T = window_bufs(window_run(name, N, H, 0))
    roll = rollout_launch(name, "tile", N, T, H, c["seed"], c["step0"], c["max_steps"])
    assert_same_bits(bufs["obs"], roll["obs"], f"{name} H={H} tr_obs")
    assert_same_bits(bufs["act"], roll["act"], f"{name} H={H} tr_act")
    assert_same_bits(bufs["rew"], roll["rew"], f"{name} H={H} tr_rew")
    assert np.array_equal(bufs["done"] == 1, roll["done"] != 0), "tr_done"
    assert np.isin(bufs["done"], (0, 1)).all() and (roll["done"] != 0).any()


@pytest.mark.parametrize("name", ["CartPole-v1", "Acrobot-v1"])
def test_greedy_dqn_rollout_fills_the_ring_with_the_evaluation_trace(cuda, name):
    e, c, N, H = ro.env_of(name), CASES[name], 81, 64
    T = c["T"]
    bufs, _ = window_bufs(evaluate_launch(name, N, H, WINDOW_E[name], T + 1, 1))
    g, ring = guarded_ring(T, N, e.D)
    persist = (Guarded((N, e.NS)), Guarded((N,), torch.int32), Guarded((N,)))
    stats = Guarded((dqn_rollout_grid(N), 8), fill=float(INT_SENTINEL))
    rc = dqn_rollout(e.env_id, ro.case_params(e, H, DEV), H, T, 0, ring, persist[0].t, persist[1].t, persist[2].t,
                     stats.t, seed=c["seed"], step0=c["step0"], epsilon=0.0, reset_all=True,
                     max_steps=c["max_steps"])
    torch.cuda.synchronize()
    assert rc == 0 and all(b.guards_intact() for b in list(g.values()) + list(persist) + [stats])
    assert_same_bits(g["obs"].t.cpu().numpy(), bufs["obs"][:T], f"{name} ring obs")
    assert_same_bits(g["act"].t.cpu().numpy(), bufs["act"], f"{name} ring act")
    assert_same_bits(g["rew"].t.cpu().numpy(), bufs["rew"], f"{name} ring rew")
