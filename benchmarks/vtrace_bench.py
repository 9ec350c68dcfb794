#!/usr/bin/env python3
"""Cost of the V-trace off-policy correction (ActorLearnerConfig.correction) on one MI355X.

The LunarLander actor-learner preset (2048 envs x 128 steps, 80 value iterations) at world 1 with
``phase_timing``: one engine per arm in one process, alternating A B B A after warm-up, every window
``--steps`` steps closed by a device synchronise.  One JSON line per window on stdout (and appended to
``--out``): env-steps/s, ms per step and the device ms per step of the learner's phases (Learn,
PolicyEval, Scan, ValueFwd, Optimize) and of the rollout.  ``--arms none`` alone also runs on a checkout
that predates the ``correction`` field (the none-versus-parent comparison).
"""
import argparse
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

PHASES = ("LearnMs", "PolicyEvalMs", "ScanMs", "ValueFwdMs", "OptimizeMs", "RolloutMs")


def make_engine(arm, dev):
    from relayrl_prototype_amd.runtime.actor_learner import ActorLearner, ActorLearnerConfig
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    kw = dict(PRESETS["lunarlander-reinforce-baseline"].overrides, phase_timing=True)
    names = {f.name for f in dataclasses.fields(ActorLearnerConfig)}
    if "correction" in names:
        kw["correction"] = arm
    elif arm != "none":
        raise SystemExit("this checkout has no ActorLearnerConfig.correction: only --arms none runs here")
    return ActorLearner(ActorLearnerConfig(**{k: v for k, v in kw.items() if k in names}), device=dev)


def window(al, steps):
    al.metrics()  # resets the phase timers
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        al.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    m = al.metrics()
    rec = {"env_steps_per_s": round(steps * al.cfg.rollout_len * al.cfg.num_envs / dt, 1),
           "step_ms": round(1e3 * dt / steps, 4), "steps": steps}
    rec.update({k: round(m[k] / steps, 5) for k in PHASES if k in m})
    rec.update({k: m[k] for k in ("MeanRho", "MeanAbsLogRatio") if k in m})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="none,vtrace")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vtrace_bench needs a GPU: a CPU timing says nothing about the MI355X")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    arms = a.arms.split(",")
    eng = {arm: make_engine(arm, dev) for arm in arms}
    for al in eng.values():
        window(al, a.warmup)
    for _ in range(a.rounds):
        for arm in arms + arms[::-1]:  # A B B A
            rec = dict(window(eng[arm], a.steps), bench="vtrace_actor_learner_step", correction=arm, tag=a.tag,
                       device=torch.cuda.get_device_name(0))
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    for al in eng.values():
        al.finish()


if __name__ == "__main__":
    main()
