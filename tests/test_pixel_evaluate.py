"""Pixel policy evaluation, the parts that need no GPU: the launcher's acceptance of the pixel
presets and checkpoints, the CPU oracle path's refusal, the host-side slot rebuild the GPU test
relies on, and the float32 stand-in figures its constant-policy cases are sized by."""
import math

import numpy as np
import pytest
import torch

import pong_oracle as po
from pixel_eval_helpers import rebuild_slots
from relayrl_prototype_amd.runtime import launcher
from relayrl_prototype_amd.runtime.evaluate import EvalResult


class StubTrainer:
    """What run_preset needs of a trainer, with a canned evaluation."""

    def __init__(self):
        self.epochs, self.eval_calls = 0, []

    def train_epoch(self):
        self.epochs += 1

    def metrics(self):
        return {"Updates": self.epochs, "EnvSteps": 10 * self.epochs}

    def evaluate(self, episodes=1, num_envs=None, greedy=True):
        self.eval_calls.append((self.epochs, episodes, num_envs, greedy))
        ret = torch.tensor([[3.0, -1.0, 5.0, 1.0]]) + self.epochs
        return EvalResult(ret, torch.full((1, 4), 40, dtype=torch.int32), torch.ones(1, 4, dtype=torch.int32))


def test_eval_every_runs_for_the_pixel_preset(tmp_path, monkeypatch):
    made = []

    def factory(preset, comm, dev, overrides):
        assert preset.kind == "pixel"
        made.append(StubTrainer())
        return made[-1]

    monkeypatch.setattr(launcher, "_make_trainer", factory)
    rows = []
    launcher.run_preset("pong-a2c", 4, str(tmp_path), eval_every=2, eval_episodes=1, eval_envs=4, on_metrics=rows.append)
    (tr,) = made
    assert tr.eval_calls == [(2, 1, 4, True), (4, 1, 4, True)]
    assert len(rows) == 4
    assert all(set(launcher.EVAL_COLUMNS) <= set(r) for r in rows)
    assert math.isnan(rows[0]["EvalAverageEpRet"])                      # before the first evaluation
    assert rows[1]["EvalAverageEpRet"] == rows[2]["EvalAverageEpRet"] == 4.0  # mean(3, -1, 5, 1) + 2
    assert rows[3]["EvalAverageEpRet"] == 6.0 and rows[3]["EvalEpisodes"] == 4.0 and rows[3]["EvalEpLen"] == 40.0
    assert rows[3]["EvalMinEpRet"] == 3.0 and rows[3]["EvalMaxEpRet"] == 9.0


@pytest.mark.parametrize("name", ["cartpole-reinforce-host"])
def test_eval_every_is_still_refused_for_host_presets(tmp_path, monkeypatch, name):
    monkeypatch.setattr(launcher, "_make_trainer", lambda *a: pytest.fail("a trainer was built"))
    with pytest.raises(NotImplementedError, match="--eval-every"):
        launcher.run_preset(name, 1, str(tmp_path), eval_every=1)
    kinds = {p.kind for p in launcher.PRESETS.values()}
    assert {"vec", "pixel"} <= kinds


def test_run_evaluate_recognises_a_pixel_checkpoint(monkeypatch):
    pixel = {"trainer": {"cfg": {"env": "PongSynth-v0", "max_episode_steps": 6750}, "updates": 7,
                         "model": {"params": torch.zeros(8)}}, "epoch": 7}
    assert launcher.is_pixel_checkpoint(pixel["trainer"])
    assert not launcher.is_pixel_checkpoint({"cfg": {"env": "CartPole-v1"}, "model": {}})       # another env
    assert not launcher.is_pixel_checkpoint({"cfg": {"env": "PongSynth-v0"}, "params": 0})      # the CPU path's
    assert not launcher.is_pixel_checkpoint({"epoch": 3, "weights": torch.zeros(4)})
    seen = []

    def stub(st, tr, per_env, n, stochastic, seed, max_episode_steps):
        seen.append((tr["updates"], per_env, n, stochastic, seed, max_episode_steps))
        return {"env": tr["cfg"]["env"], "episodes": per_env * n}

    monkeypatch.setattr(launcher, "_evaluate_pixel_checkpoint", stub)
    out = launcher.evaluate_checkpoint_state(pixel, "ck", episodes=100, num_envs=64, stochastic=True, seed=5)
    assert seen == [(7, 2, 50, True, 5, None)] and out == {"env": "PongSynth-v0", "episodes": 100}
    assert "hidden" not in out
    for other in ({"trainer": {"epoch": 3, "weights": torch.zeros(4)}},
                  {"trainer": {"cfg": {"env": "CartPole-v1"}, "model": {"params": torch.zeros(8)}}}):
        with pytest.raises(ValueError, match="not a VecTrainer checkpoint"):
            launcher.evaluate_checkpoint_state(other, "ck")
    assert len(seen) == 1
    with pytest.raises(ValueError, match="--episodes"):
        launcher.evaluate_checkpoint_state(pixel, "ck", episodes=0)


def test_cpu_oracle_path_of_the_pixel_trainer_refuses():
    from relayrl_prototype_amd.runtime.pixel_trainer import PixelA2CConfig, PixelA2CTrainer

    tr = PixelA2CTrainer(PixelA2CConfig(num_envs=2, rollout_len=2), device="cpu")
    assert not tr.on_gpu and tr.eval_step0 == 0
    with pytest.raises(NotImplementedError, match="pixel"):
        tr.evaluate(episodes=1)
    with pytest.raises(NotImplementedError, match="pixel"):
        tr.evaluate(episodes=1, num_envs=64)  # refused before the num_envs check
    assert tr.eval_step0 == 0


def test_eval_step_has_no_cpu_path(monkeypatch):
    from relayrl_prototype_amd import ops
    from relayrl_prototype_amd.envs.pong import DevicePong

    monkeypatch.setattr(ops, "_HIP", None)
    monkeypatch.setattr(ops, "_HIP_ERR", ImportError("not built"))
    with pytest.raises(ops.NativeExtensionMissing):
        DevicePong(4, "cpu")


# ------------------------------------------------------------------ the slot rebuild
def test_rebuild_slots_on_hand_written_traces():
    nan = float("nan")
    # 1: one env, E = 2, time limits of 3 steps; a third episode's steps are not read
    r = rebuild_slots([[0], [1], [0], [-1], [0], [0], [nan], [nan]], [[0], [0], [1], [0], [0], [1], [nan], [nan]], 2)
    assert r.ep_ret[:, 0].tolist() == [1.0, -1.0] and r.ep_len[:, 0].tolist() == [3, 3]
    assert r.ep_code[:, 0].tolist() == [2, 2]
    assert r.ep_cnt[:, 0].tolist() == [0, 0, 1, 1, 1, 2, 2, 2] and r.remaining.tolist() == [1, 1, 1, 1, 1, 0, 0, 0]
    assert r.active[:, 0].tolist() == [True] * 6 + [False] * 2
    # 2: a 21-point ending is code 1, also when the opponent's points are interleaved with the agent's
    rew = [[-1.0]] * 20 + [[1.0]] + [[-1.0]] + [[0.0]]
    done = [[0.0]] * 21 + [[1.0]] + [[0.0]]
    r = rebuild_slots(rew, done, 1)
    assert (r.ep_ret[0, 0], r.ep_len[0, 0], r.ep_code[0, 0]) == (-20.0, 22, 1)
    assert r.points[0, 0].tolist() == [21, 1] and not r.active[22, 0] and r.remaining[-1] == 0
    # 3: two envs finishing at different steps; an unfinished slot stays unwritten
    rew = np.array([[1, 0], [0, 0], [0, -1], [nan, 0], [nan, 0]], float)
    done = np.array([[0, 0], [1, 0], [1, 1], [nan, 0], [nan, 0]], float)
    r = rebuild_slots(rew, done, 2)
    assert r.ep_cnt.tolist() == [[0, 0], [1, 0], [2, 1], [2, 1], [2, 1]] and r.remaining.tolist() == [2, 2, 1, 1, 1]
    assert r.ep_ret[:, 0].tolist() == [1.0, 0.0] and r.ep_len[:, 0].tolist() == [2, 1]
    assert r.ep_ret[0, 1] == -1.0 and r.ep_len[0, 1] == 3 and np.isnan(r.ep_ret[1, 1]) and r.ep_len[1, 1] == -1
    assert r.ep_code[:, 1].tolist() == [2, -1]
    assert r.active.tolist() == [[True, True], [True, True], [True, True], [False, True], [False, True]]


# ------------------------------------------------------------------ the float32 stand-in
def test_stand_in_figures_of_the_constant_policy_cases():
    """What the GPU cases are sized by: NOOP play of 37 envs, from the float32 oracle."""
    n = 37
    sim = po.simulate(n, np.zeros((944, n), np.int32), po.SEED, po.STEP0, 6750)
    r = rebuild_slots(sim["rew"], sim["done"], 2)
    # the last env finishes in step 938 (counted from 0): 939 steps are played
    assert int(r.active.any(1).sum()) == 939 and r.remaining[938] == 0 and r.remaining[937] == 1
    assert (r.ep_code == 1).all() and (r.points.max(-1) == 21).all()
    assert (r.ep_len.min(), r.ep_len.max()) == (248, 569)
    assert (r.ep_ret.min(), r.ep_ret.max()) == (-21.0, -14.0)
    sim = po.simulate(n, np.zeros((76, n), np.int32), po.SEED, po.STEP0, 24)
    r = rebuild_slots(sim["rew"], sim["done"], 3)
    assert int(r.active.any(1).sum()) == 72 and (r.ep_len == 24).all() and (r.ep_code == 2).all()
    assert (r.ep_ret.min(), r.ep_ret.max()) == (-3.0, 1.0)
