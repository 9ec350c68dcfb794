#!/usr/bin/env python3
"""Pixel policy evaluation (runtime/evaluate.py ``evaluate_pixel_policy``) on one MI355X, one JSON
line per measurement on stdout (and appended to ``--out``):

* ``eval_step``     -- ms per evaluation step at ``--num-envs`` envs: conv stack (no a1 / a2 stores)
  + fc split-K GEMM + the fused greedy head / env step / render kernel, launched eagerly.  Taken as
  the slope between two evaluations cut by a time limit of ``--k-lo`` and ``--k-hi`` steps (every
  env then plays exactly that many), so the set-up of an evaluation (env, ring, reset) drops out.
* ``rollout_step``  -- ms per training rollout step of the same build and size: the trainer's
  ``Rollout`` phase with ``phase_timing`` (eager launches like the evaluation's; device time of T
  steps plus the bootstrap value forward, divided by T), and by T + 1 as the lower bound that
  counts the bootstrap forward as a whole step.
* ``evaluate``      -- total time and env-steps/s of ``evaluate(episodes=1)`` for a freshly
  initialised policy, once per ``--poll`` value (the steps between two reads of the device
  counter): env-steps counts the steps the envs played (the sum of the episode lengths), the wall
  time includes the tail in which finished envs still pass through the conv stack.

The arms of a comparison alternate (A B B A) after a warm-up.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=2048)
    ap.add_argument("--rollout-len", type=int, default=5)
    ap.add_argument("--k-lo", type=int, default=100)
    ap.add_argument("--k-hi", type=int, default=500)
    ap.add_argument("--updates", type=int, default=40, help="phase-timed training updates per window")
    ap.add_argument("--poll", default="8,32,128,512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pong_evaluate_bench needs a GPU: a CPU timing says nothing about the MI355X")
    from relayrl_prototype_amd.runtime.evaluate import evaluate_pixel_policy
    from relayrl_prototype_amd.runtime.pixel_trainer import PixelA2CConfig, PixelA2CTrainer

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, T = a.num_envs, a.rollout_len
    base = dict(bench="pong_evaluate", num_envs=N, tag=a.tag, device=torch.cuda.get_device_name(0))
    tr = PixelA2CTrainer(PixelA2CConfig(num_envs=N, rollout_len=T, phase_timing=True), device=dev)
    m, row0 = tr.model, T * N

    def eval_k(k):  # every env plays exactly k steps: one episode cut by the time limit
        return evaluate_pixel_policy(m, 1, N, seed=11, max_episode_steps=k, row0=row0, poll_every=10 ** 9)

    def rollout_window():
        tr.timer.device_ms.clear()
        tr.timer.wall.clear()
        for _ in range(a.updates):
            tr.train_epoch()
        return tr.timer.columns()["RolloutMs"] / a.updates

    for _ in range(3):  # warm-up: code objects, allocator blocks, the trainer's eager path
        tr.train_epoch()
    eval_k(a.k_lo)
    slopes, rolls = [], []
    for arm in ("eval", "roll", "roll", "eval") * 2:
        if arm == "eval":
            lo, _ = timed(lambda: eval_k(a.k_lo))
            hi, _ = timed(lambda: eval_k(a.k_hi))
            slopes.append((hi - lo) / (a.k_hi - a.k_lo))
        else:
            rolls.append(rollout_window())
    emit(dict(base, arm="eval_step", ms_per_step=round(statistics.median(slopes), 5),
              ms_min=round(min(slopes), 5), ms_max=round(max(slopes), 5), windows=len(slopes), k_lo=a.k_lo, k_hi=a.k_hi,
              timing="host clock around a synchronised call, slope between two step counts"), a.out)
    med = statistics.median(rolls)
    emit(dict(base, arm="rollout_step", rollout_phase_ms=round(med, 5), ms_per_step=round(med / T, 5),
              ms_per_step_counting_bootstrap=round(med / (T + 1), 5), ms_min=round(min(rolls) / T, 5),
              ms_max=round(max(rolls) / T, 5), windows=len(rolls), updates=a.updates, rollout_len=T,
              fused_head=bool(tr.fused_head), frame_ring=tr.ring is not None,
              timing="device events around the Rollout phase (T steps + the bootstrap value forward) / T"), a.out)
    # whole evaluations of the freshly initialised policy (the trainer has made a few updates: rebuilt)
    del tr, m
    torch.cuda.empty_cache()
    tr = PixelA2CTrainer(PixelA2CConfig(num_envs=N, rollout_len=T), device=dev)
    polls = [int(p) for p in a.poll.split(",") if p]
    times = {p: [] for p in polls}
    info = {}
    for p in polls:  # warm-up of every arm
        evaluate_pixel_policy(tr.model, 1, N, seed=tr.eval_seed, row0=T * N, poll_every=p)
    for _ in range(a.reps):
        for p in polls + polls[::-1]:
            ms, res = timed(lambda: evaluate_pixel_policy(tr.model, 1, N, seed=tr.eval_seed, row0=T * N, poll_every=p))
            times[p].append(ms)
            info[p] = res
    for p in polls:
        res = info[p]
        st = res.stats()
        played = float(res.ep_len.sum().item())
        ms = statistics.median(times[p])
        emit(dict(base, arm="evaluate", poll_every=p, ms_total=round(ms, 3), ms_min=round(min(times[p]), 3),
                  ms_max=round(max(times[p]), 3), reps=len(times[p]), steps_launched=res.steps,
                  longest_episode=int(res.ep_len.max().item()), env_steps_played=played,
                  env_steps_per_sec=round(played / (ms * 1e-3), 1),
                  launched_env_steps_per_sec=round(res.steps * N / (ms * 1e-3), 1), mean_return=st["mean_return"],
                  mean_length=st["mean_length"], truncated_share=st["truncated_share"]), a.out)


if __name__ == "__main__":
    main()
