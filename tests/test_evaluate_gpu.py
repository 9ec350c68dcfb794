"""The fused evaluation kernels (csrc/kernels/evaluate.hip) against the float64 host oracles of
tests/rollout_oracle.py and ops/reference.py:

a. physics and resets of a traced window, greedy and sampled, all five envs (``ro.replay``);
b. completion: every env runs exactly E episodes, the trace stops where the last one ends, the
   outputs are the episode sums of the kernel's own trace, ep_code against the oracle's ``term``;
c. greedy discrete actions against the float64 argmax at the device's own observations;
d. greedy continuous actions against the fp32 oracle's mu; determinism; seeds;
e. sampled mode against the fp32 policy oracle's draws;
f. VecTrainer.evaluate, its isolation from training, and the ``evaluate`` command.

517 envs (33 tiles, ragged last tile) run with grids sized for 2 CUs, so that 16 waves stride over
the tiles; 40 envs run one tile per workgroup.  Every output is the middle of a sentinel-guarded
tensor, and trace tensors start as sentinels, so an unwritten row shows.

MountainCar-v0 in (c): its observations (|pos| <= 1.2, |vel| <= 0.07) are too small to move the
argmax off the output bias for any seed tried, so it is compared against the oracle without the
two-action condition.
"""
import json
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import EvalTrace, MLPSpec, evaluate_policy_op, hip
from relayrl_prototype_amd.ops import reference as ref

import rollout_oracle as ro
from guarded import INT_SENTINEL, Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = {k: dict(v) for k, v in ro.CASES.items()}
# with the greedy policy some landers hover to the 1000-step limit; at 60 both endings occur
CASES["LunarLanderSynth-v0"]["max_steps"] = 60
# episodes per env of the traced window (a, c, d, e): enough that no env finishes inside it
WINDOW_E = {name: 7 if name == "CartPole-v1" else 3 for name in CASES}
SHAPES = [(517, 128), (517, 64), (40, 128)]  # (N, H); N = 517 runs under set_cu_limit(2)
GAP = 3e-4            # three times the 1e-4 logit tolerance of test_forward_value_logits_eval
MAX_GAP_SKIP = 0.02   # at most 2 % of the compared cells may have a smaller float64 gap
MIN_ACTION_SHARE = 0.10


@contextmanager
def cu_limit(N):
    h = hip()
    old = h.set_cu_limit(2) if N > 256 else None
    try:
        yield
    finally:
        if old is not None:
            h.set_cu_limit(old)


def seeded_params(name, H, s):
    e = ro.env_of(name)
    return MLPSpec(e.D, H, e.A, gaussian=e.continuous).init(torch.Generator().manual_seed(s))


def launch(name, N, H, E, Tc, greedy, seed=None, params=None):
    """One evaluation launch into guarded buffers (``Tc = 0``: null trace pointers); the buffers as
    numpy arrays.  ``params``: flat CPU weights (default: the case's)."""
    e, c = ro.env_of(name), CASES[name]
    seed = c["seed"] if seed is None else seed
    params = ro.case_params(e, H) if params is None else params
    g = dict(ep_ret=Guarded((E, N)), ep_len=Guarded((E, N), torch.int32), ep_code=Guarded((E, N), torch.int32))
    trace = None
    if Tc > 0:
        g.update(tr_obs=Guarded((Tc, N, e.D)),
                 tr_act=Guarded((Tc, N, e.A)) if e.continuous else Guarded((Tc, N), torch.int32),
                 tr_rew=Guarded((Tc, N)), tr_done=Guarded((Tc, N)))
        trace = EvalTrace(g["tr_obs"].t, g["tr_act"].t, g["tr_rew"].t, g["tr_done"].t)
    consts = torch.from_numpy(e.constants()).to(DEV) if e.continuous else None
    with cu_limit(N):
        evaluate_policy_op(e.env_id, params.to(DEV), H, E, N, greedy=greedy, seed=seed, step0=c["step0"],
                           max_steps=c["max_steps"], env_consts=consts,
                           out=(g["ep_ret"].t, g["ep_len"].t, g["ep_code"].t), trace=trace)
        torch.cuda.synchronize()
    for k, b in g.items():
        assert b.guards_intact(), f"{k}: the kernel wrote outside its buffer"
    out = {k: b.t.cpu().numpy() for k, b in g.items()}
    out.update(env=e, name=name, N=N, H=H, E=E, Tc=Tc, greedy=greedy, seed=seed, step0=c["step0"],
               max_steps=c["max_steps"], params=params)
    return out


@lru_cache(maxsize=None)
def window_run(name, N, H, greedy):
    """The first T steps of the case, traced with Tc = T + 1 (``tr_obs`` then has the row replay needs)."""
    return launch(name, N, H, WINDOW_E[name], CASES[name]["T"] + 1, greedy)


def window_bufs(run):
    """The traced window in the rollout buffers' layout, after asserting that no env finished
    inside it (so that every row of the window was written)."""
    T = run["Tc"] - 1
    total = run["ep_len"].sum(0)
    assert total.min() >= T + 1, f"an env finished its episodes after {total.min()} steps, inside the window {T + 1}"
    bufs = dict(obs=run["tr_obs"], act=run["tr_act"][:T], rew=run["tr_rew"][:T], done=run["tr_done"][:T], tobs=None)
    for k, b in bufs.items():
        assert b is None or not np.isnan(b.astype(np.float64)).any(), f"{k}: unwritten cells inside the window"
    if not run["env"].continuous:
        assert (bufs["act"] != INT_SENTINEL).all()
    return bufs, T


def check_outputs(run):
    E, N = run["E"], run["N"]
    assert np.isfinite(run["ep_ret"]).all(), "an ep_ret cell was not written"
    assert ((run["ep_len"] >= 1) & (run["ep_len"] <= run["max_steps"])).all()
    assert np.isin(run["ep_code"], (1, 2)).all()
    assert run["ep_ret"].shape == run["ep_len"].shape == run["ep_code"].shape == (E, N)


# ------------------------------------------------------------------ a: physics and resets
@pytest.mark.parametrize("greedy", [1, 0])
@pytest.mark.parametrize("N,H", SHAPES)
@pytest.mark.parametrize("name", list(CASES))
def test_window_replay(cuda, name, N, H, greedy):
    run = window_run(name, N, H, greedy)
    check_outputs(run)
    bufs, T = window_bufs(run)
    c = CASES[name]
    rp = ro.replay(name, bufs, c["seed"], c["step0"], c["max_steps"], has_tobs=False)
    share = ro.assert_replay(name, bufs, rp)
    ends = int((bufs["done"] > 0).sum())
    print(f"{name} N={N} H={H} greedy={greedy}: {share:.4%} of {T * N} cells within {ro.EPS} of a threshold, "
          f"{ends} episode ends (each followed by a checked reset)")
    # the greedy H = 128 landers hover past the 40-step window; every other case ends episodes in it
    assert ends > 0 or (name == "LunarLanderSynth-v0" and greedy and H == 128)


# ------------------------------------------------------------------ b: completion
COMPLETION = [(N, H, g) for N, H in SHAPES for g in (1,)] + [(517, 128, 0)]


def check_completion(run):
    """Everything (b) asks of one traced launch with Tc = E * max_steps."""
    e, E, N, Tc = run["env"], run["E"], run["N"], run["Tc"]
    assert Tc == E * run["max_steps"]
    check_outputs(run)
    total = run["ep_len"].sum(0)  # S: the steps env n ran
    written = np.arange(Tc)[:, None] < total[None, :]
    # exactly S rows are written, the rest still hold the sentinel
    for k in ("tr_rew", "tr_done"):
        assert np.array_equal(~np.isnan(run[k]), written), f"{k}: written rows != sum(ep_len)"
    assert np.array_equal(~np.isnan(run["tr_obs"]), np.repeat(written[:, :, None], e.D, 2)), "tr_obs rows"
    if e.continuous:
        assert np.array_equal(~np.isnan(run["tr_act"]), np.repeat(written[:, :, None], e.A, 2)), "tr_act rows"
    else:
        assert np.array_equal(run["tr_act"] != INT_SENTINEL, written), "tr_act rows"
        assert ((run["tr_act"][written] >= 0) & (run["tr_act"][written] < e.A)).all()
    rew = np.where(written, run["tr_rew"], 0).astype(np.float32)
    done = np.where(written, run["tr_done"], 0).astype(np.float32)
    assert np.isin(done, (0, 1)).all()
    # exactly E episode ends, the last of them in row S - 1
    assert np.array_equal(done.sum(0), np.full(N, E))
    assert (done[total - 1, np.arange(N)] == 1).all()
    # ep_ret / ep_len are the episode sums of the kernel's own trace: the same fp32 additions
    st = ro.episode_stats(rew, done)
    ep = st["episodes"]
    assert st["n_done"] == E * N
    order = np.lexsort((ep["t"], ep["env"]))  # by env, then by time: episode k of env n
    k = np.tile(np.arange(E), N)
    envs, ts = ep["env"][order], ep["t"][order]
    assert np.array_equal(envs, np.repeat(np.arange(N), E))
    assert np.array_equal(run["ep_len"][k, envs], ep["len"][order])
    got, want = run["ep_ret"][k, envs], ep["ret"][order].astype(np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "ep_ret vs the fp32 running sums of tr_rew"
    # ep_code == 2 exactly where len == max_steps and the oracle's term is false
    bufs = dict(obs=np.where(np.isnan(run["tr_obs"]), 0, run["tr_obs"]),
                act=np.where(written[..., None], run["tr_act"], 0) if e.continuous else np.where(written, run["tr_act"], 0),
                rew=rew, done=done)
    rp = ro.replay(e, bufs, run["seed"], run["step0"], run["max_steps"], has_tobs=False)
    term, margin = rp["term"][ts, envs], rp["margin"][ts, envs]
    code = np.where((ep["len"][order] == run["max_steps"]) & ~term, 2, 1)
    sure = margin > ro.EPS
    assert np.array_equal(run["ep_code"][k, envs][sure], code[sure]), "ep_code vs the oracle"
    share = float((rp["margin"][written] <= ro.EPS).mean())  # as assert_replay counts it: over all cells
    assert share <= ro.MAX_SKIP_SHARE, f"{share:.4%} of the cells lie within {ro.EPS} of a threshold"
    return set(np.unique(run["ep_code"]))


@pytest.mark.parametrize("N,H,greedy", COMPLETION)
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_completion(cuda, name, E, N, H, greedy):
    run = launch(name, N, H, E, E * CASES[name]["max_steps"], greedy)
    codes = check_completion(run)
    if not ro.env_of(name).terminates or name in ("MountainCar-v0", "Acrobot-v1"):
        assert codes == {2}  # 9 steps reach neither the flag nor the bar
    elif name == "LunarLanderSynth-v0" and greedy:
        assert codes == {1, 2}, "at 60 steps both endings occur: touchdowns and the time limit"
    else:  # the greedy H = 128 poles all fall before step 12; the sampled landers all come down before 60
        assert codes <= {1, 2}
    # with null trace pointers the three outputs are bitwise the same
    bare = launch(name, N, H, E, 0, greedy)
    for k in ("ep_ret", "ep_len", "ep_code"):
        assert np.array_equal(np.ascontiguousarray(run[k]).view(np.int32), np.ascontiguousarray(bare[k]).view(np.int32)), k


# ------------------------------------------------------------------ c: greedy actions, discrete
# (name, H, init seed or None for the case's weights, two-action condition)
GREEDY = [("CartPole-v1", 128, 5, True), ("Acrobot-v1", 128, 2, True), ("LunarLanderSynth-v0", 64, 2, True),
          ("LunarLanderSynth-v0", 128, 2, True), ("MountainCar-v0", 128, None, False)]


def check_greedy_discrete(run, two_actions):
    e = run["env"]
    written = ~np.isnan(run["tr_rew"])
    assert written.any()
    obs = torch.from_numpy(np.where(np.isnan(run["tr_obs"]), 0, run["tr_obs"]))
    act, gap = ref.greedy_actions_ref(run["params"], obs, e.A, run["H"])
    act, gap = act.numpy()[written], gap.numpy()[written]
    clear = gap > GAP
    skipped = float((~clear).mean())
    assert skipped <= MAX_GAP_SKIP, f"{skipped:.2%} of the cells have a float64 gap below {GAP}"
    assert np.array_equal(run["tr_act"][written][clear], act[clear]), "tr_act vs the float64 argmax"
    shares = np.bincount(act, minlength=e.A) / act.size
    print(f"{run['name']} H={run['H']}: float64 action shares {np.round(shares, 3)}, skipped {skipped:.2%}")
    if two_actions:  # a constant policy would prove nothing
        assert (shares >= MIN_ACTION_SHARE).sum() >= 2, shares
    return shares, skipped


# Acrobot at N = 40 is left out: the float64 oracle itself puts 22 of those 1,000 cells (2.2 %) under
# the gap, which the 2 % cap does not allow; its 517 envs (1.88 % on the CPU oracle) carry the check.
@pytest.mark.parametrize("name,H,s,two_actions,N",
                         [c + (N,) for c in GREEDY for N in (517, 40) if (c[0], N) != ("Acrobot-v1", 40)])
def test_greedy_actions_discrete(cuda, name, H, s, two_actions, N):
    params = None if s is None else seeded_params(name, H, s)
    run = launch(name, N, H, WINDOW_E[name], CASES[name]["T"] + 1, 1, params=params)
    check_outputs(run)
    check_greedy_discrete(run, two_actions)


# ------------------------------------------------------------------ d: greedy actions, continuous
CHEETAH = "HalfCheetahSynth-v0"


@pytest.mark.parametrize("N,H", SHAPES)
def test_greedy_actions_continuous(cuda, N, H):
    run = window_run(CHEETAH, N, H, 1)
    bufs, T = window_bufs(run)
    e = run["env"]
    for t in range(T):
        mu = ref.mlp_forward_ref(3, run["params"], torch.from_numpy(bufs["obs"][t]), e.A, H)["logits"]
        torch.testing.assert_close(torch.from_numpy(bufs["act"][t]), mu, rtol=1e-4, atol=1e-4)
    again = launch(CHEETAH, N, H, run["E"], run["Tc"], 1)
    for k in ("ep_ret", "ep_len", "ep_code", "tr_obs", "tr_act", "tr_rew", "tr_done"):
        assert np.array_equal(np.ascontiguousarray(run[k]).view(np.int32),
                              np.ascontiguousarray(again[k]).view(np.int32)), f"{k}: two launches of one seed differ"
    other = launch(CHEETAH, N, H, run["E"], run["Tc"], 1, seed=run["seed"] + 1)
    assert not np.array_equal(other["tr_obs"][0], run["tr_obs"][0]), "another seed, the same resets"


# ------------------------------------------------------------------ e: sampled mode
@pytest.mark.parametrize("N,H", SHAPES)
@pytest.mark.parametrize("name", list(CASES))
def test_sampled_actions(cuda, name, N, H):
    run = window_run(name, N, H, 0)
    bufs, T = window_bufs(run)
    e = run["env"]
    greedy = window_run(name, N, H, 1)
    assert not np.array_equal(greedy["tr_act"][:T], run["tr_act"][:T]), "the greedy and the sampled run agree"
    if e.continuous:
        assert np.isfinite(bufs["act"]).all()
        return
    differ = 0
    for t in range(T):
        r = ref.mlp_forward_ref(1, run["params"], torch.from_numpy(bufs["obs"][t]), e.A, H, seed=run["seed"],
                                step=run["step0"] + t)
        differ += int((r["act"].numpy() != bufs["act"][t]).sum())
    assert differ <= max(1, 0.02 * T * N), differ  # a draw within rounding of a cdf step may go either way


# ------------------------------------------------------------------ f: trainer level
def small_trainer(cuda):
    from relayrl_prototype_amd.runtime.vec_trainer import VecTrainer, VecTrainerConfig

    return VecTrainer(VecTrainerConfig(num_envs=256, rollout_len=16, train_vf_iters=2, seed=4), device=cuda)


def test_trainer_evaluate(cuda):
    tr = small_trainer(cuda)
    res = tr.evaluate(episodes=2, num_envs=96)
    assert res.ep_ret.shape == res.ep_len.shape == res.ep_code.shape == (2, 96)
    assert res.episodes == 2 * 96 and res.greedy
    assert res.min_return <= res.mean_return <= res.max_return and res.std_return >= 0
    ln = res.ep_len.cpu().numpy()
    assert ln.min() >= 1 and ln.max() <= tr.max_steps
    assert 1 <= res.mean_length <= tr.max_steps and 0 <= res.truncated_share <= 1
    assert res.mean_return == res.mean_length  # CartPole pays 1 per step
    # the same weights again: other resets (the stream's counter has moved on)
    res2 = tr.evaluate(episodes=2, num_envs=96)
    assert res2.step0 == res.step0 + 2 * tr.max_steps and res2.seed == res.seed != tr.env_seed
    assert not torch.equal(res.ep_len, res2.ep_len)
    assert tr.evaluate().ep_ret.shape == (1, 256)  # defaults: one episode in as many envs as it trains


def test_evaluate_leaves_training_untouched(cuda):
    def run(with_eval):
        tr = small_trainer(cuda)
        for _ in range(3):
            tr.train_epoch()
            if with_eval:
                tr.evaluate(episodes=1, num_envs=48).stats()
        torch.cuda.synchronize()
        return {k: t.detach().cpu().clone() for k, t in
                dict(pi=tr.pi.params, vf=tr.vf.params, state=tr.state, ep_len=tr.ep_len, ep_ret=tr.ep_ret,
                     ep_stats=tr.ep_stats).items()}

    a, b = run(True), run(False)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_evaluate_command_on_a_trainer_checkpoint(cuda, tmp_path, capsys):
    from relayrl_prototype_amd.runtime.launcher import main
    from relayrl_prototype_amd.utils.checkpoint import save_checkpoint

    tr = small_trainer(cuda)
    tr.train_epoch()
    save_checkpoint(str(tmp_path), {"trainer": tr.state_dict(), "epoch": 1})
    assert main(["evaluate", "--checkpoint", str(tmp_path), "--episodes", "64", "--num-envs", "32", "--seed", "3"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["episodes"] == 64 and out["env"] == "CartPole-v1" and out["hidden"] == 128 and out["greedy"] is True
    assert out["min_return"] <= out["mean_return"] <= out["max_return"] <= 500
    # the printed score is the one of the trainer's weights
    from relayrl_prototype_amd.runtime.evaluate import evaluate_policy

    same = evaluate_policy("CartPole-v1", tr.pi.params, 128, 2, 32, seed=3)
    assert same.mean_return == out["mean_return"]
    assert main(["evaluate", "--checkpoint", str(tmp_path), "--episodes", "8", "--stochastic"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["episodes"] == 8 and out["greedy"] is False


def test_train_eval_every_logs_the_eval_columns(cuda, tmp_path):
    """``train --eval-every 2``: every row of progress.txt carries the Eval* columns, NaN before the first
    evaluation and the latest values afterwards; without the flag no such column exists."""
    import glob

    from relayrl_prototype_amd.runtime.launcher import EVAL_COLUMNS, run_preset

    ov = dict(num_envs=256, rollout_len=16, train_vf_iters=2, seed=4)

    def rows(out, **kw):
        run_preset("cartpole-reinforce-baseline", 5, str(out), dict(ov), **kw)
        (path,) = glob.glob(str(out / "**" / "progress.txt"), recursive=True)
        lines = [ln.rstrip("\n").split("\t") for ln in open(path)]
        return lines[0], [dict(zip(lines[0], map(float, r))) for r in lines[1:]]

    head, r = rows(tmp_path / "on", eval_every=2, eval_episodes=2, eval_envs=48)
    assert len(r) == 5 and set(EVAL_COLUMNS) <= set(head)
    assert all(np.isnan(r[0][k]) for k in EVAL_COLUMNS)  # epoch 1: nothing evaluated yet
    for k in EVAL_COLUMNS:
        assert np.isfinite(r[1][k]) and r[2][k] == r[1][k] and r[4][k] == r[3][k], k  # carried between evaluations
    assert r[1]["EvalEpisodes"] == r[3]["EvalEpisodes"] == 96
    assert r[3]["EvalMinEpRet"] <= r[3]["EvalAverageEpRet"] <= r[3]["EvalMaxEpRet"]
    assert r[1]["EvalAverageEpRet"] == r[1]["EvalEpLen"]  # CartPole pays 1 per step
    assert any(r[3][k] != r[1][k] for k in EVAL_COLUMNS), "the second evaluation repeats the first"
    head_off, r_off = rows(tmp_path / "off")
    assert not set(EVAL_COLUMNS) & set(head_off) and [c for c in head if c not in EVAL_COLUMNS] == head_off
    # evaluation does not touch training: the training columns agree with the run without it
    for a, b in zip(r, r_off):
        for k in ("AverageEpRet", "LossPi", "LossV", "Entropy", "EnvSteps"):
            assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), k
