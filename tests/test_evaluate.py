"""Policy evaluation, the parts that need no GPU: the float64 greedy-action oracle, the EvalResult
statistics, the command line, and the loud failures (unsupported trainers, missing extension)."""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd import ops
from relayrl_prototype_amd.ops import MLPSpec
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.evaluate import STAT_FIELDS, EvalResult
from relayrl_prototype_amd.runtime.launcher import EVAL_COLUMNS, build_parser, eval_columns


def test_greedy_from_logits_hand_built_with_a_tie():
    logits = torch.tensor([[0.0, 1.0, 0.5],    # plain
                           [2.0, 2.0, -1.0],   # tie of the first two: the lowest index
                           [-3.0, -1.0, -1.0],  # tie of the last two
                           [7.0, 7.0, 7.0],    # all equal
                           [-5.0, -9.0, -4.75]], dtype=torch.float64)
    act, gap = ref.greedy_from_logits(logits)
    assert act.tolist() == [1, 0, 1, 0, 2]
    assert gap.tolist() == [0.5, 0.0, 0.0, 0.0, 0.25]
    act, gap = ref.greedy_from_logits(torch.tensor([[3.0]]))
    assert act.tolist() == [0] and gap.tolist() == [float("inf")]


def test_greedy_actions_ref_builds_the_logits_in_float64():
    D, H, A = 4, 64, 3
    p = MLPSpec(D, H, A).init(torch.Generator().manual_seed(0))
    obs = torch.randn(5, 7, D, generator=torch.Generator().manual_seed(1))
    act, gap = ref.greedy_actions_ref(p, obs, A, H)
    assert act.shape == gap.shape == (5, 7) and gap.dtype == torch.float64
    W1, b1, W2, b2, W3, b3 = (t.double() for t in ref.unflatten(p, D, H, A)[:6])
    x = obs.reshape(-1, D).double()
    logits = torch.relu(torch.relu(x @ W1.t() + b1) @ W2.t() + b2) @ W3.t() + b3
    assert torch.equal(act.reshape(-1), logits.argmax(-1))
    top = logits.sort(-1, descending=True).values
    assert torch.equal(gap.reshape(-1), top[:, 0] - top[:, 1])
    # the dtype it is given: a float32 run agrees wherever the float64 gap is clear
    a32, g32 = ref.greedy_actions_ref(p, obs, A, H, dtype=torch.float32)
    assert g32.dtype == torch.float32 and torch.equal(a32[gap > 1e-4], act[gap > 1e-4])


def test_eval_result_statistics_against_numpy():
    rng = np.random.default_rng(3)
    E, N = 3, 41
    ret = rng.normal(20, 7, (E, N)).astype(np.float32)
    ln = rng.integers(1, 501, (E, N)).astype(np.int32)
    code = rng.integers(1, 3, (E, N)).astype(np.int32)
    res = EvalResult(torch.from_numpy(ret), torch.from_numpy(ln), torch.from_numpy(code), greedy=False, seed=5,
                     step0=9)
    r64 = ret.astype(np.float64)
    want = dict(episodes=E * N, mean_return=r64.mean(), std_return=r64.std(), min_return=r64.min(),
                max_return=r64.max(), mean_length=ln.astype(np.float64).mean(), truncated_share=(code == 2).mean())
    assert set(want) == set(STAT_FIELDS)
    assert res.episodes == E * N and isinstance(res.episodes, int)
    for k, v in want.items():
        assert getattr(res, k) == pytest.approx(v, rel=1e-12, abs=0), k
    assert res.min_return <= res.mean_return <= res.max_return
    d = res.to_dict()
    assert {k: d[k] for k in STAT_FIELDS} == res.stats() and (d["greedy"], d["seed"], d["step0"]) == (False, 5, 9)
    with pytest.raises(AttributeError):
        res.median_return
    cols = eval_columns(res)
    assert tuple(cols) == EVAL_COLUMNS
    assert cols["EvalAverageEpRet"] == res.mean_return and cols["EvalEpisodes"] == E * N
    assert cols["EvalEpLen"] == res.mean_length and cols["EvalStdEpRet"] == res.std_return


def test_command_line_of_evaluate_and_the_eval_flags():
    ap = build_parser()
    a = ap.parse_args(["evaluate", "--checkpoint", "runs/ck"])
    assert (a.cmd, a.checkpoint, a.episodes, a.num_envs, a.stochastic, a.seed, a.max_episode_steps) == (
        "evaluate", "runs/ck", 100, 1024, False, 0, None)
    a = ap.parse_args(["evaluate", "--checkpoint", "d", "--episodes", "7", "--num-envs", "3", "--stochastic",
                       "--seed", "11", "--max-episode-steps", "60"])
    assert (a.episodes, a.num_envs, a.stochastic, a.seed, a.max_episode_steps) == (7, 3, True, 11, 60)
    with pytest.raises(SystemExit):
        ap.parse_args(["evaluate"])  # --checkpoint is required
    t = ap.parse_args(["train"])
    assert (t.eval_every, t.eval_episodes, t.eval_envs) == (0, 1, None)  # off by default
    t = ap.parse_args(["train", "--eval-every", "5", "--eval-episodes", "2", "--eval-envs", "512"])
    assert (t.eval_every, t.eval_episodes, t.eval_envs) == (5, 2, 512)


def test_episodes_are_spread_over_whole_episodes_per_env():
    from relayrl_prototype_amd.runtime.launcher import spread_episodes

    assert spread_episodes(100, 1024) == (1, 100)
    assert spread_episodes(100, 64) == (2, 50)
    assert spread_episodes(64, 32) == (2, 32)
    assert spread_episodes(1, 1) == (1, 1)
    for episodes in range(1, 200):
        for num_envs in (1, 3, 16, 64, 1000):
            per_env, n = spread_episodes(episodes, num_envs)
            assert 1 <= n <= num_envs and episodes <= per_env * n < episodes + per_env


def test_evaluate_of_a_non_vec_checkpoint_is_refused(tmp_path):
    from relayrl_prototype_amd.runtime.launcher import run_evaluate
    from relayrl_prototype_amd.utils.checkpoint import save_checkpoint

    save_checkpoint(str(tmp_path), {"trainer": {"epoch": 3, "weights": torch.zeros(4)}})
    with pytest.raises(ValueError, match="not a VecTrainer checkpoint"):
        run_evaluate(str(tmp_path))


def test_unsupported_trainers_say_so():
    from relayrl_prototype_amd.api.server import TrainingServer
    from relayrl_prototype_amd.runtime.actor_learner import ActorLearner
    from relayrl_prototype_amd.runtime.engine import EngineAlgorithm, RemoteEngineAlgorithm
    from relayrl_prototype_amd.runtime.host_trainer import HostVecTrainer
    from relayrl_prototype_amd.runtime.pixel_trainer import PixelA2CTrainer

    # evaluate() of these needs nothing of the instance: it refuses before touching it
    for cls, word in ((HostVecTrainer, "host-env"), (PixelA2CTrainer, "pixel"), (ActorLearner, "actor-learner"),
                      (RemoteEngineAlgorithm, "multi-rank")):
        with pytest.raises(NotImplementedError, match=word):
            cls.evaluate(object.__new__(cls), episodes=1)

    class Holder:
        def __init__(self, trainer):
            self.trainer = trainer

    with pytest.raises(NotImplementedError, match="host-env"):  # the engine forwards to its trainer
        EngineAlgorithm.evaluate(Holder(object.__new__(HostVecTrainer)), episodes=2, num_envs=4)
    srv = object.__new__(TrainingServer)
    srv.engine = None
    with pytest.raises(NotImplementedError, match="agent uploads"):
        srv.evaluate()


def test_eval_every_is_refused_for_a_preset_without_device_envs(tmp_path):
    from relayrl_prototype_amd.runtime.launcher import run_preset

    with pytest.raises(NotImplementedError, match="--eval-every"):  # before any trainer is built
        run_preset("cartpole-reinforce-host", 1, str(tmp_path), eval_every=1)


def test_evaluate_policy_op_raises_without_the_extension(monkeypatch):
    monkeypatch.setattr(ops, "_HIP", None)
    monkeypatch.setattr(ops, "_HIP_ERR", ImportError("not built"))
    with pytest.raises(ops.NativeExtensionMissing):
        ops.evaluate_policy_op(0, torch.zeros(17538), 128, 1, 16)


def test_evaluate_policy_op_has_no_cpu_path():
    """With the extension loaded a CPU tensor is refused, not scored by some PyTorch stand-in."""
    with pytest.raises((ValueError, ops.NativeExtensionMissing), match="GPU tensor|not built"):
        ops.evaluate_policy_op(0, torch.zeros(17538), 128, 1, 16)
