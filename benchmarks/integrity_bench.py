#!/usr/bin/env python3
"""Cost of the rollout integrity check (ActorLearnerConfig.integrity) on one MI355X.

(a) The payload checksum kernel (csrc/kernels/checksum.hip) on one actor's payload of the
    actor-learner bench shape (LunarLanderSynth-v0, 2048 envs x 128 steps) and on a 10x smaller one:
    device-event time per launch, GB/s from the bytes the shapes give, and that rate as a share of the
    ~6.3 TB/s achievable HBM read rate.  Two arms: ``rotating`` walks over enough distinct copies of the
    payload to exceed the 256 MiB Infinity Cache (every launch reads HBM), ``resident`` re-reads one copy
    (what a learner sees right after the rollout or the P2P receive wrote it).
(b) ``ActorLearner.step()`` with integrity off and lagged: two engines in one process, alternating
    A B B A after warm-up, every window at least ``--window-s`` seconds and ended by a device
    synchronise.  The spread of the repeated identical arms is reported beside the difference.

One JSON line per record on stdout (and appended to ``--out``).  ``--arms off`` alone also runs on a
checkout that predates the ``integrity`` field (the off-versus-parent comparison).
"""
import argparse
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

HBM_READ_TBS = 6.3        # achievable HBM read rate of the MI355X
L3_BYTES = 256 << 20      # Infinity Cache


def payload_segments(N, T, D, dev, gen):
    """One actor's payload in ActorLearner's order: obs [T*N, D], final obs [N, D], act int32 [T, N],
    logp, rew, done [T, N], tobs [T, N, D], header float64[10]."""
    f = lambda *s: torch.randn(*s, device=dev, generator=gen)
    return [f(T * N, D), f(N, D), torch.randint(0, 4, (T, N), device=dev, generator=gen, dtype=torch.int32),
            f(T, N), f(T, N), f(T, N), f(T, N, D), torch.randn(10, device=dev, generator=gen, dtype=torch.float64)]


def bench_kernel(N, T, D, dev, reps, emit):
    from relayrl_prototype_amd import ops

    gen = torch.Generator(device=dev).manual_seed(0)
    one = payload_segments(N, T, D, dev, gen)
    nbytes = sum(s.numel() * s.element_size() for s in one)
    ncopies = L3_BYTES * 2 // nbytes + 2
    copies = [one] + [[s.clone() for s in one] for _ in range(ncopies - 1)]
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    want = ops.payload_checksum([s.cpu() for s in one])
    assert torch.equal(ops.payload_checksum(one, out=out).cpu(), want), "kernel disagrees with the oracle"
    for arm, sets in (("rotating", copies), ("resident", [one])):
        for i in range(max(20, len(sets))):
            ops.payload_checksum(sets[i % len(sets)], out=out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            ops.payload_checksum(sets[i % len(sets)], out=out)
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps  # checksum + finishing launch, back to back on one stream
        gbs = nbytes / (us * 1e-6) / 1e9
        emit({"bench": "checksum_kernel", "arm": arm, "num_envs": N, "rollout_len": T, "obs_dim": D,
              "payload_bytes": nbytes, "distinct_copies": len(sets), "launches": reps, "us_per_launch": round(us, 3),
              "GBps": round(gbs, 1), "share_of_6.3TBps_hbm_read": round(gbs / (HBM_READ_TBS * 1e3), 4),
              "matches_oracle": True})


def make_engine(a, arm, dev):
    from relayrl_prototype_amd.parallel.comm import Comm
    from relayrl_prototype_amd.runtime.actor_learner import ActorLearner, ActorLearnerConfig

    kw = dict(env=a.env, num_envs=a.num_envs, rollout_len=a.rollout_len, with_baseline=True, gamma=0.98, lam=0.97,
              pi_lr=3e-4, vf_lr=1e-3, train_vf_iters=a.vf_iters, learner_acts=True, stall_timeout_s=0.0, seed=1)
    if "integrity" in {f.name for f in dataclasses.fields(ActorLearnerConfig)}:
        kw["integrity"] = arm
    elif arm != "off":
        raise SystemExit("this checkout has no ActorLearnerConfig.integrity: only --arms off runs here")
    return ActorLearner(ActorLearnerConfig(**kw), Comm(collectives=False), device=dev)


def window(al, seconds, min_steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        al.step()
        n += 1
        if n >= min_steps and n % 4 == 0:  # the clock is read without a sync; the window ends with one
            if time.perf_counter() - t0 >= seconds:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, n


def bench_step(a, dev, emit):
    arms = a.arms.split(",")
    eng = {arm: make_engine(a, arm, dev) for arm in arms}
    for al in eng.values():
        for _ in range(a.warmup):
            al.step()
    torch.cuda.synchronize()
    order = arms + arms[::-1]  # A B B A
    ms = {arm: [] for arm in arms}
    steps = 0
    for _ in range(a.rounds):
        for arm in order:
            t, n = window(eng[arm], a.window_s, a.min_steps)
            ms[arm].append(round(t, 4))
            steps += n
    for al in eng.values():
        al.finish()
    rec = {"bench": "actor_learner_step", "env": a.env, "num_envs": a.num_envs, "rollout_len": a.rollout_len,
           "train_vf_iters": a.vf_iters, "window_s": a.window_s, "order": order, "rounds": a.rounds, "steps": steps,
           "tag": a.tag}
    mean = {}
    for arm in arms:
        v = ms[arm]
        mean[arm] = sum(v) / len(v)
        rec[f"{arm}_ms_per_step"] = v
        rec[f"{arm}_mean_ms"] = round(mean[arm], 4)
        rec[f"{arm}_spread_pct"] = round((max(v) - min(v)) / mean[arm] * 100, 3)  # identical arms, run to run
    if "off" in mean and "lagged" in mean:
        rec["lagged_over_off_pct"] = round((mean["lagged"] / mean["off"] - 1) * 100, 3)
        m = eng["lagged"].metrics()
        rec.update(IntegrityChecked=m["IntegrityChecked"], IntegrityMismatches=m["IntegrityMismatches"])
    emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="LunarLanderSynth-v0")
    ap.add_argument("--num-envs", type=int, default=2048)
    ap.add_argument("--rollout-len", type=int, default=128)
    ap.add_argument("--vf-iters", type=int, default=80)
    ap.add_argument("--arms", default="off,lagged")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--min-steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=400)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("integrity_bench needs a GPU: a CPU timing says nothing about the MI355X")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if not a.skip_kernel:
        from relayrl_prototype_amd import _native

        D = _native.VecEnv(a.env, 1, 0, 1).obs_dim
        bench_kernel(a.num_envs, a.rollout_len, D, dev, a.kernel_reps, emit)
        bench_kernel(max(a.num_envs // 10, 1), a.rollout_len, D, dev, a.kernel_reps, emit)
    bench_step(a, dev, emit)


if __name__ == "__main__":
    main()
