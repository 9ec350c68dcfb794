#!/usr/bin/env python3
"""Time to score a policy on whole episodes, on one MI355X: the fused evaluation kernel against the
only way a checkout without it can.

Arms, per workload (CartPole-v1 at 4,096 and 32,768 envs, HalfCheetahSynth-v0 at 16,384 envs; one
episode per env, the env's own time limit, H = 128, seeded initial weights):

* ``evaluate``  -- one ``evaluate`` / ``evaluate_cont`` launch into three [1, N] tensors, then the
  float64 statistics (one synchronising read).  ``--modes`` picks sampled and / or greedy actions.
* ``rollout``   -- ``rollout`` / ``rollout_cont`` with ``T = max_steps`` and ``reset_all`` into full
  ``[T + 1][N][D]`` buffers, ``done`` and ``rew`` copied to the host, and each env's first episode
  picked out of ``done`` there.  Sampled actions only: the rollout kernels have no greedy mode.

The sampled ``evaluate`` arm and the ``rollout`` arm are given the same seed, so they run the same
episodes; ``lengths_match`` says the two agree on every episode length.  The arms alternate A B B A
after a warm-up; one JSON line per window on stdout (and appended to ``--out``) with the median and
the spread of the repeats, the bytes each path allocates, and ``tile_wait_share``: the share of a
tile's steps spent waiting for its longest episode, sum over 16-env tiles of (max - mean length) over
the sum of the maxima, read from ``ep_len``.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

WORKLOADS = [("CartPole-v1", 4096), ("CartPole-v1", 32768), ("HalfCheetahSynth-v0", 16384)]
H = 128
SEED, STEP0 = 12345, 0


class Workload:
    def __init__(self, env, N, dev):
        from relayrl_prototype_amd import _native
        from relayrl_prototype_amd.ops import MLPSpec, hip
        from relayrl_prototype_amd.runtime.vec_trainer import CONTINUOUS_DEVICE_ENVS, DEVICE_ENVS

        self.env, self.N, self.dev, self.h = env, N, dev, hip()
        self.env_id = DEVICE_ENVS[env]
        self.continuous = env in CONTINUOUS_DEVICE_ENVS
        self.D, self.A, self.NS, self.max_steps = self.h.env_dims(self.env_id)
        self.params = MLPSpec(self.D, H, self.A, gaussian=self.continuous).init(
            torch.Generator().manual_seed(7)).to(dev)
        self.consts = (torch.tensor(_native.env_constants(env), dtype=torch.float32, device=dev)
                       if self.continuous else None)
        self.bufs = None

    # ---- the fused kernel
    def evaluate(self, greedy):
        from relayrl_prototype_amd.ops import evaluate_policy_op
        from relayrl_prototype_amd.runtime.evaluate import EvalResult

        out = evaluate_policy_op(self.env_id, self.params, H, 1, self.N, greedy=greedy, seed=SEED, step0=STEP0,
                                 max_steps=self.max_steps, env_consts=self.consts)
        res = EvalResult(*out[:3], greedy=greedy)
        st = res.stats()  # the synchronising read
        nbytes = sum(t.numel() * t.element_size() for t in out[:3])
        return st["mean_return"], res.ep_len, nbytes

    # ---- the rollout kernels, full buffers, host-side extraction
    def alloc_rollout(self):
        N, T, D, dev = self.N, self.max_steps, self.D, self.dev
        act = torch.empty(T, N, self.A, device=dev) if self.continuous else torch.empty(T, N, dtype=torch.int32,
                                                                                          device=dev)
        self.bufs = dict(state=torch.empty(N, self.NS, device=dev), ep_len=torch.empty(N, dtype=torch.int32, device=dev),
                         ep_ret=torch.empty(N, device=dev), obs=torch.empty(T + 1, N, D, device=dev), act=act,
                         logp=torch.empty(T, N, device=dev), rew=torch.empty(T, N, device=dev),
                         done=torch.empty(T, N, device=dev),
                         ep_stats=torch.empty(self.h.rollout_grid(N), 8, device=dev))
        return sum(t.numel() * t.element_size() for t in self.bufs.values())

    def rollout(self):
        nbytes = self.alloc_rollout()  # a scoring call owns no buffers: allocation is part of its cost
        b = self.bufs
        args = (H, b["state"], b["ep_len"], b["ep_ret"], b["obs"], b["act"], b["logp"], b["rew"], b["done"], None,
                b["ep_stats"], SEED, STEP0, True, self.max_steps)
        if self.continuous:
            self.h.rollout_cont(self.env_id, self.params, self.consts, *args)
        else:
            self.h.rollout(self.env_id, self.params, *args)
        done = b["done"].cpu().numpy() > 0  # synchronises
        rew = b["rew"].cpu().numpy()
        first = done.argmax(0)  # every env ends an episode within max_steps rows
        inside = np.arange(done.shape[0])[:, None] <= first[None, :]
        ret = np.where(inside, rew, 0).sum(0, dtype=np.float64)
        self.bufs = None
        return float(ret.mean()), first + 1, nbytes


def tile_wait_share(ep_len):
    """sum over 16-env tiles of (max - mean length) / sum of the maxima."""
    ln = np.asarray(ep_len, np.float64).reshape(-1)
    pad = (-len(ln)) % 16
    tiles = np.concatenate([ln, np.full(pad, np.nan)]).reshape(-1, 16)
    mx, mean = np.nanmax(tiles, 1), np.nanmean(tiles, 1)
    return float((mx - mean).sum() / mx.sum()), float(mx.mean()), float(ln.mean())


def window(w, arm, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mean, lens, nbytes = w.rollout() if arm == "rollout" else w.evaluate(arm == "evaluate_greedy")
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
        if len(times) >= 5 and sum(times) > 2000.0:  # a long call needs no 50 repeats: 5 and two seconds do
            break
    reps = len(times)
    lens =lens.cpu().numpy().reshape(-1) if torch.is_tensor(lens) else np.asarray(lens)
    share, tile_max, mean_len = tile_wait_share(lens)
    rec = dict(arm=arm, env=w.env, num_envs=w.N, episodes=w.N, max_steps=w.max_steps, ms_median=round(statistics.median(times), 4),
               ms_min=round(min(times), 4), ms_max=round(max(times), 4), reps=reps, bytes_allocated=int(nbytes),
               mean_return=mean, mean_length=mean_len, mean_tile_max_length=tile_max, tile_wait_share=round(share, 4))
    return rec, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="sampled,greedy", help="evaluate arms: sampled, greedy")
    ap.add_argument("--reps", type=int, default=5, help="repeats per window of the rollout arm")
    ap.add_argument("--eval-reps", type=int, default=50, help="repeats per window of an evaluate arm (a short call)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_bench needs a GPU: a CPU timing says nothing about the MI355X")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    arms = ["evaluate_" + m for m in a.modes.split(",") if m] + ["rollout"]
    for env, N in WORKLOADS:
        w = Workload(env, N, dev)
        lens = {}
        for arm in arms:  # warm-up: code objects, the allocator's blocks, pinned staging
            _, lens[arm] = window(w, arm, 1)
        match = bool(np.array_equal(lens["evaluate_sampled"], lens["rollout"])) if "evaluate_sampled" in lens else None
        for _ in range(a.rounds):
            for arm in arms + arms[::-1]:  # A B B A
                rec, _ = window(w, arm, a.reps if arm == "rollout" else a.eval_reps)
                rec.update(bench="evaluate_policy", lengths_match=match, tag=a.tag, device=torch.cuda.get_device_name(0))
                line = json.dumps(rec)
                print(line, flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        del w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
