#!/usr/bin/env python3
"""DQN throughput on one MI355X at the shape of the ``cartpole-dqn`` preset (1,024 envs x 4 steps,
batch 1,024, 4 updates per epoch, H = 128, eager launches).

One JSON line:

* ``env_steps_per_s`` / ``grad_steps_per_s``: ``DQNTrainer.train_epoch()`` end to end (wall clock
  around ``--epochs`` epochs after ``--warmup``, the ring filled and learning under way);
* ``*_us``: microseconds per launch of the three kernels from HIP events around ``--iters`` back-to-back
  launches each (median of ``--reps`` windows): ``dqn_rollout``, ``dqn_targets``, ``mlp_grad(Q_TD)``.
  Launches are eager, so a figure is bounded below by the host's issue interval: a spread of a few
  hundredths of a microsecond between windows says the kernel, not the host, set it;
* ``mlp_grad_pg_cat_us``: ``mlp_grad(PG_CAT)`` at the same B, D, H and A on the fp32-MFMA kernel Q_TD
  uses (the value-grad mode switched to 0 for the reading): the two share everything but the head.

    python benchmarks/dqn_bench.py --out profiles/dqn_bench.jsonl

``--prioritized`` adds, from the same process, the ``cartpole-dqn-per`` preset (prioritised replay):
``per_epoch_us`` / ``per_env_steps_per_s`` / ``per_grad_steps_per_s`` beside the uniform figures, and the
microseconds per launch of ``per_insert``, ``dqn_targets_per``, ``mlp_grad_q_td_weighted`` and ``per_update``
(``per_insert`` and ``per_update`` are one workgroup each: their time is latency, not throughput).  The
line goes to ``profiles/dqn_per_bench.jsonl`` unless ``--out`` names another file.

``--n-step K [K ...]`` adds, from the same process, what n-step returns cost: the microseconds per launch of
``dqn_targets`` at ``n_step = 1`` and at every K on the same trained ring, uniform (``targets_n<K>_us``) and
prioritised (``targets_per_n<K>_us``), and the epoch of both DQN presets at ``n_step = 1`` and at the first K
(``epoch_n<K>_us`` / ``epoch_per_n<K>_us``).  The line goes to ``profiles/dqn_nstep_bench.jsonl`` unless
``--out`` names another file.

``--dueling`` adds, from the same process, the dueling head against the plain one at the shapes of
``cartpole-dqn`` (``uniform``) and ``cartpole-dqn-nstep`` (``per_n3``; with the dueling head it is the
``cartpole-dqn-dueling`` preset): ``epoch_<shape>_<plain|dueling>_us`` and the microseconds per launch of
``dqn_rollout``, ``dqn_targets`` and ``mlp_grad`` (``<kernel>_<shape>_<plain|dueling>_us``).  The line goes to
``profiles/dqn_dueling_bench.jsonl`` unless ``--out`` names another file.

``--noisy`` adds, from the same process, NoisyNet exploration: the microseconds per launch of ``noisy_compose``
with one job (the actor's, per rollout) and with three (per update) and of ``noisy_grad``, at the net of the
``cartpole-dqn-noisy`` preset, and the epoch of that preset against ``cartpole-dqn-dueling``
(``epoch_noisy_us`` / ``epoch_dueling_us``).  The line goes to ``profiles/dqn_noisy_bench.jsonl`` unless ``--out``
names another file.  ``--noisy-learning EPOCHS`` instead records, for seeds 1..3 of both presets, the greedy mean
return over 256 episodes every 100 epochs: one line per run in ``profiles/dqn_noisy_learning.jsonl``.

``--quantiles NQ`` adds, from the same process, the quantile-regression head (QR-DQN, ``quantiles = NQ``) against the
scalar one at the shapes of ``cartpole-dqn`` (``uniform``) and ``cartpole-dqn-nstep`` (``per_n3``; with ``NQ = 8`` it
is the ``cartpole-dqn-quantile`` preset): ``epoch_<shape>_<scalar|quantile>_us`` and the microseconds per launch of
``dqn_rollout``, ``dqn_targets`` and ``mlp_grad`` (``<kernel>_<shape>_<scalar|quantile>_us``).  The line goes to
``profiles/dqn_quantile_bench.jsonl`` unless ``--out`` names another file.  ``--quantile-learning EPOCHS`` instead
records, for seeds 1..3 of ``cartpole-dqn-nstep`` and ``cartpole-dqn-quantile``, the greedy mean return over 256
episodes every 100 epochs: one line per run in ``profiles/dqn_quantile_learning.jsonl``.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def event_us(fn, iters, reps):
    """Median over ``reps`` windows of the mean microseconds of ``iters`` back-to-back calls."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / iters)
    return round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)


def per_records(a, dev, event_us):
    """The prioritised preset: epoch wall clock and the four launches prioritised replay adds or changes."""
    from relayrl_prototype_amd.ops import GradHead, dqn_targets, mlp_grad, per_insert, per_update
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    cfg = DQNConfig(**PRESETS["cartpole-dqn-per"].overrides)
    tr = DQNTrainer(cfg, device=dev)
    for _ in range(a.warmup):
        tr.train_epoch()
    assert tr.updates > 0, "the warm-up must reach learning_starts"
    torch.cuda.synchronize()
    u0, t0 = tr.updates, time.perf_counter()
    for _ in range(a.epochs):
        tr.train_epoch()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    N, T, B, C = cfg.num_envs, cfg.rollout_len, cfg.batch_size, cfg.buffer_slots
    rec = dict(per_preset="cartpole-dqn-per", per_alpha=cfg.per_alpha, per_tree_leaves=tr.per.P2,
               per_env_steps_per_s=round(a.epochs * N * T / el, 1),
               per_grad_steps_per_s=round((tr.updates - u0) / el, 1), per_epoch_us=round(1e6 * el / a.epochs, 2))
    filled = min(tr.slots_written, C) * N

    def insert():  # the same slots every time: timing only
        per_insert(tr.per, C, N, T, 0)

    def targets():
        dqn_targets(tr.q.params, tr.target, cfg.hidden, tr.A, tr.ring, filled, cfg.gamma, cfg.double_q, tr.sample_seed,
                    7, B, tree=tr.per.tree, beta=0.7, out=(tr.Xb, tr.act_b, tr.y, tr.idx, tr.w, tr.wmax))

    def grad_q():
        mlp_grad(GradHead.Q_TD, tr.q.params, tr.Xb, tr.A, cfg.hidden, act=tr.act_b, ret=tr.y, clip_eps=cfg.huber_delta,
                 grad_slab=tr.slab, loss_slab=tr.loss, row_w=tr.w, w_norm=tr.wmax, td_abs=tr.td_abs)

    def update():
        per_update(tr.per, tr.idx, tr.td_abs, cfg.per_alpha, cfg.per_eps)

    for name, fn in (("per_insert", insert), ("dqn_targets_per", targets), ("mlp_grad_q_td_weighted", grad_q),
                     ("per_update", update)):
        fn()
        torch.cuda.synchronize()
        med, lo, hi = event_us(fn, a.iters, a.reps)
        rec[name + "_us"] = med
        rec[name + "_us_range"] = [lo, hi]
    return rec


def nstep_records(a, dev, event_us):
    """n-step returns against one-step in one process: the targets launch, uniform and prioritised, and the epoch."""
    from relayrl_prototype_amd.ops import dqn_targets
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    rec = dict(n_steps=list(a.n_step))
    for preset, tag in (("cartpole-dqn", ""), ("cartpole-dqn-per", "per_")):
        for n in (1, a.n_step[0]):
            cfg = DQNConfig(**dict(PRESETS[preset].overrides, n_step=n))
            tr = DQNTrainer(cfg, device=dev)
            for _ in range(a.warmup):
                tr.train_epoch()
            assert tr.updates > 0, "the warm-up must reach learning_starts"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.epochs):
                tr.train_epoch()
            torch.cuda.synchronize()
            rec[f"epoch_{tag}n{n}_us"] = round(1e6 * (time.perf_counter() - t0) / a.epochs, 2)
        # the launch alone, on the ring of the trainer just measured: the same rows are sampled for every n
        N, B, C = cfg.num_envs, cfg.batch_size, cfg.buffer_slots
        filled = min(tr.slots_written, C) * N
        newest = (tr.cursor - 1) % C
        out = (tr.Xb, tr.act_b, tr.y, tr.idx, tr.w, tr.wmax) if tr.per is not None else (tr.Xb, tr.act_b, tr.y, None)
        kw = dict(tree=tr.per.tree, beta=0.7) if tr.per is not None else {}
        for n in [1] + [k for k in a.n_step if k != 1]:
            def targets():
                dqn_targets(tr.q.params, tr.target, cfg.hidden, tr.A, tr.ring, filled, cfg.gamma, cfg.double_q,
                            tr.sample_seed, 7, B, out=out, n_step=n, newest=newest, **kw)

            targets()
            torch.cuda.synchronize()
            med, lo, hi = event_us(targets, a.iters, a.reps)
            rec[f"targets_{tag}n{n}_us"] = med
            rec[f"targets_{tag}n{n}_us_range"] = [lo, hi]
    return rec


def dueling_records(a, dev, event_us):
    """The dueling head against the plain one in one process, at the shapes of ``cartpole-dqn`` (uniform, one-step)
    and ``cartpole-dqn-nstep`` (prioritised, 3-step: with ``dueling`` it is the ``cartpole-dqn-dueling`` preset):
    the epoch, and the three launches that stage the Q-network."""
    from relayrl_prototype_amd.ops import dqn_rollout, dqn_targets, mlp_grad
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    assert PRESETS["cartpole-dqn-dueling"].overrides == dict(PRESETS["cartpole-dqn-nstep"].overrides, dueling=True)
    rec = {}
    for preset, tag in (("cartpole-dqn", "uniform"), ("cartpole-dqn-nstep", "per_n3")):
        for dueling in (False, True):
            cfg = DQNConfig(**dict(PRESETS[preset].overrides, dueling=dueling))
            tr = DQNTrainer(cfg, device=dev)
            for _ in range(a.warmup):
                tr.train_epoch()
            assert tr.updates > 0, "the warm-up must reach learning_starts"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.epochs):
                tr.train_epoch()
            torch.cuda.synchronize()
            key = f"{tag}_{'dueling' if dueling else 'plain'}"
            rec[f"epoch_{key}_us"] = round(1e6 * (time.perf_counter() - t0) / a.epochs, 2)
            N, T, B, C = cfg.num_envs, cfg.rollout_len, cfg.batch_size, cfg.buffer_slots
            filled = min(tr.slots_written, C) * N
            duel = dict(dueling=True) if dueling else {}
            tkw = dict(duel)
            gkw = {}
            out = (tr.Xb, tr.act_b, tr.y, None)
            if tr.per is not None:
                tkw.update(tree=tr.per.tree, beta=0.7)
                gkw = dict(row_w=tr.w, w_norm=tr.wmax, td_abs=tr.td_abs)
                out = (tr.Xb, tr.act_b, tr.y, tr.idx, tr.w, tr.wmax)
            if cfg.n_step > 1:
                tkw.update(n_step=cfg.n_step, newest=(tr.cursor - 1) % C)

            def rollout():  # the same slot and step every time: timing only
                dqn_rollout(tr.env_id, tr.q.params, cfg.hidden, T, 0, tr.ring, tr.state, tr.ep_len, tr.ep_ret,
                            tr.ep_stats, seed=tr.env_seed, step0=0, epsilon=0.1, reset_all=False,
                            max_steps=tr.max_steps, **duel)

            def targets():
                dqn_targets(tr.q.params, tr.target, cfg.hidden, tr.A, tr.ring, filled, cfg.gamma, cfg.double_q,
                            tr.sample_seed, 7, B, out=out, **tkw)

            def grad_q():
                mlp_grad(tr.head, tr.q.params, tr.Xb, tr.A, cfg.hidden, act=tr.act_b, ret=tr.y,
                         clip_eps=cfg.huber_delta, grad_slab=tr.slab, loss_slab=tr.loss, **gkw)

            for name, fn in (("dqn_rollout", rollout), ("dqn_targets", targets), ("mlp_grad", grad_q)):
                fn()
                torch.cuda.synchronize()
                med, lo, hi = event_us(fn, a.iters, a.reps)
                rec[f"{name}_{key}_us"] = med
                rec[f"{name}_{key}_us_range"] = [lo, hi]
    return rec


def quantile_records(a, dev, event_us):
    """The quantile head (``quantiles = a.quantiles``) against the scalar one in one process, at the shapes of
    ``cartpole-dqn`` (uniform, one-step) and ``cartpole-dqn-nstep`` (prioritised, 3-step: with 8 quantiles it is the
    ``cartpole-dqn-quantile`` preset): the epoch, and the three launches that stage the Q-network."""
    from relayrl_prototype_amd.ops import dqn_rollout, dqn_targets, mlp_grad
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    assert PRESETS["cartpole-dqn-quantile"].overrides == dict(PRESETS["cartpole-dqn-nstep"].overrides, quantiles=8)
    rec = dict(quantiles=a.quantiles)
    for preset, tag in (("cartpole-dqn", "uniform"), ("cartpole-dqn-nstep", "per_n3")):
        for NQ in (0, a.quantiles):
            cfg = DQNConfig(**dict(PRESETS[preset].overrides, quantiles=NQ))
            tr = DQNTrainer(cfg, device=dev)
            for _ in range(a.warmup):
                tr.train_epoch()
            assert tr.updates > 0, "the warm-up must reach learning_starts"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.epochs):
                tr.train_epoch()
            torch.cuda.synchronize()
            key = f"{tag}_{'quantile' if NQ else 'scalar'}"
            rec[f"epoch_{key}_us"] = round(1e6 * (time.perf_counter() - t0) / a.epochs, 2)
            N, T, B, C = cfg.num_envs, cfg.rollout_len, cfg.batch_size, cfg.buffer_slots
            filled = min(tr.slots_written, C) * N
            qr = dict(quantiles=NQ) if NQ else {}
            tkw = dict(qr)
            gkw = dict(qr)
            out = (tr.Xb, tr.act_b, tr.y, None)
            if tr.per is not None:
                tkw.update(tree=tr.per.tree, beta=0.7)
                gkw.update(row_w=tr.w, w_norm=tr.wmax, td_abs=tr.td_abs)
                out = (tr.Xb, tr.act_b, tr.y, tr.idx, tr.w, tr.wmax)
            if cfg.n_step > 1:
                tkw.update(n_step=cfg.n_step, newest=(tr.cursor - 1) % C)

            def rollout():  # the same slot and step every time: timing only
                dqn_rollout(tr.env_id, tr.q.params, cfg.hidden, T, 0, tr.ring, tr.state, tr.ep_len, tr.ep_ret,
                            tr.ep_stats, seed=tr.env_seed, step0=0, epsilon=0.1, reset_all=False,
                            max_steps=tr.max_steps, **qr)

            def targets():
                dqn_targets(tr.q.params, tr.target, cfg.hidden, tr.A, tr.ring, filled, cfg.gamma, cfg.double_q,
                            tr.sample_seed, 7, B, out=out, **tkw)

            def grad_q():
                mlp_grad(tr.head, tr.q.params, tr.Xb, tr.A, cfg.hidden, act=tr.act_b, ret=tr.y,
                         clip_eps=cfg.huber_delta, grad_slab=tr.slab, loss_slab=tr.loss, **gkw)

            for name, fn in (("dqn_rollout", rollout), ("dqn_targets", targets), ("mlp_grad", grad_q)):
                fn()
                torch.cuda.synchronize()
                med, lo, hi = event_us(fn, a.iters, a.reps)
                rec[f"{name}_{key}_us"] = med
                rec[f"{name}_{key}_us_range"] = [lo, hi]
    return rec


def quantile_learning(a, dev):
    """Greedy mean return over 256 episodes every 100 epochs, seeds 1..3, ``cartpole-dqn-nstep`` and
    ``cartpole-dqn-quantile``: one JSON line per run."""
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    lines = []
    for preset in ("cartpole-dqn-nstep", "cartpole-dqn-quantile"):
        for seed in (1, 2, 3):
            cfg = DQNConfig(**dict(PRESETS[preset].overrides, seed=seed))
            tr = DQNTrainer(cfg, device=dev)
            curve = []
            for epoch in range(1, a.quantile_learning + 1):
                tr.train_epoch()
                if epoch % 100 == 0:
                    curve.append(round(tr.evaluate(episodes=1, num_envs=256).stats()["mean_return"], 1))
            lines.append(json.dumps(dict(preset=preset, quantiles=cfg.quantiles, n_step=cfg.n_step, seed=seed,
                                         eval_every=100, env_steps_per_epoch=cfg.num_envs * cfg.rollout_len,
                                         greedy_mean_return_256=curve)))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


def noisy_records(a, dev, event_us):
    """NoisyNet exploration in one process: the two new launches at the preset's net, and the epoch of
    ``cartpole-dqn-noisy`` against ``cartpole-dqn-dueling``."""
    from relayrl_prototype_amd.ops import noisy_compose, noisy_grad
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    assert PRESETS["cartpole-dqn-noisy"].overrides == dict(PRESETS["cartpole-dqn-dueling"].overrides, noisy=True,
                                                           eps_start=0.0, eps_end=0.0)
    rec = {}
    for preset, tag in (("cartpole-dqn-dueling", "dueling"), ("cartpole-dqn-noisy", "noisy")):
        cfg = DQNConfig(**PRESETS[preset].overrides)
        tr = DQNTrainer(cfg, device=dev)
        for _ in range(a.warmup):
            tr.train_epoch()
        assert tr.updates > 0, "the warm-up must reach learning_starts"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.epochs):
            tr.train_epoch()
        torch.cuda.synchronize()
        rec[f"epoch_{tag}_us"] = round(1e6 * (time.perf_counter() - t0) / a.epochs, 2)
    spec, key = tr.q.spec, tr.noise_seed  # the noisy trainer's
    rec.update(noisy_params=spec.P, noisy_slabs=int(tr.slab.shape[0]), noisy_sigma_mean_abs=tr.metrics()["SigmaMeanAbs"])

    def compose1():  # the same draw every time: timing only
        noisy_compose(tr.theta, (0,), (7,), spec, key, out=tr.actor_w)

    def compose3():
        noisy_compose((tr.theta, tr.target, tr.theta), (1, 2, 3), (7, 7, 7), spec, key, out=tr.update_w)

    def grad():
        noisy_grad(tr.slab, 1, 7, spec, key, out=tr.theta_grad)

    for name, fn in (("noisy_compose_1job", compose1), ("noisy_compose_3jobs", compose3), ("noisy_grad", grad)):
        fn()
        torch.cuda.synchronize()
        med, lo, hi = event_us(fn, a.iters, a.reps)
        rec[name + "_us"] = med
        rec[name + "_us_range"] = [lo, hi]
    return rec


def noisy_learning(a, dev):
    """Greedy mean return over 256 episodes every 100 epochs, seeds 1..3, ``cartpole-dqn-dueling`` and
    ``cartpole-dqn-noisy``: one JSON line per run."""
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    lines = []
    for preset in ("cartpole-dqn-dueling", "cartpole-dqn-noisy"):
        for seed in (1, 2, 3):
            cfg = DQNConfig(**dict(PRESETS[preset].overrides, seed=seed))
            tr = DQNTrainer(cfg, device=dev)
            curve = []
            for epoch in range(1, a.noisy_learning + 1):
                tr.train_epoch()
                if epoch % 100 == 0:
                    curve.append(round(tr.evaluate(episodes=1, num_envs=256).stats()["mean_return"], 1))
            rec = dict(preset=preset, noisy=bool(cfg.noisy), dueling=bool(cfg.dueling), n_step=cfg.n_step, seed=seed,
                       eval_every=100, env_steps_per_epoch=cfg.num_envs * cfg.rollout_len, greedy_mean_return_256=curve)
            if cfg.noisy:
                rec["sigma_mean_abs"] = round(tr.metrics()["SigmaMeanAbs"], 5)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--prioritized", action="store_true", help="also measure the cartpole-dqn-per preset")
    ap.add_argument("--n-step", type=int, nargs="+", default=[], metavar="K",
                    help="also measure n-step returns at every K against one-step")
    ap.add_argument("--dueling", action="store_true", help="also measure the dueling head against the plain one")
    ap.add_argument("--noisy", action="store_true", help="also measure NoisyNet exploration against cartpole-dqn-dueling")
    ap.add_argument("--noisy-learning", type=int, default=0, metavar="EPOCHS",
                    help="record greedy-return curves of cartpole-dqn-noisy and cartpole-dqn-dueling instead")
    ap.add_argument("--quantiles", type=int, default=0, metavar="NQ",
                    help="also measure the quantile head (QR-DQN) with NQ quantiles against the scalar one")
    ap.add_argument("--quantile-learning", type=int, default=0, metavar="EPOCHS",
                    help="record greedy-return curves of cartpole-dqn-quantile and cartpole-dqn-nstep instead")
    a = ap.parse_args()
    if a.quantiles < 0 or 2 * a.quantiles > 16:
        raise SystemExit("--quantiles takes 1 .. 8 (CartPole has 2 actions and the kernels hold 16 outputs)")
    if any(k < 1 for k in a.n_step):
        raise SystemExit("--n-step takes values >= 1")
    if (a.prioritized or a.n_step or a.dueling or a.noisy or a.noisy_learning or a.quantiles
            or a.quantile_learning) and not a.out:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                             "dqn_quantile_learning.jsonl" if a.quantile_learning else
                             "dqn_quantile_bench.jsonl" if a.quantiles else
                             "dqn_noisy_learning.jsonl" if a.noisy_learning else
                             "dqn_noisy_bench.jsonl" if a.noisy else
                             "dqn_dueling_bench.jsonl" if a.dueling else
                             "dqn_nstep_bench.jsonl" if a.n_step else "dqn_per_bench.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("dqn_bench needs a GPU: a CPU timing says nothing about the MI355X")
    from relayrl_prototype_amd.ops import GradHead, dqn_rollout, dqn_targets, mlp_grad, set_value_grad_mode
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.noisy_learning:
        return noisy_learning(a, dev)
    if a.quantile_learning:
        return quantile_learning(a, dev)
    cfg = DQNConfig(**PRESETS["cartpole-dqn"].overrides)
    tr = DQNTrainer(cfg, device=dev)
    for _ in range(a.warmup):
        tr.train_epoch()
    assert tr.updates > 0, "the warm-up must reach learning_starts"
    torch.cuda.synchronize()
    u0, t0 = tr.updates, time.perf_counter()
    for _ in range(a.epochs):
        tr.train_epoch()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    N, T, B = cfg.num_envs, cfg.rollout_len, cfg.batch_size
    rec = dict(bench="dqn", preset="cartpole-dqn", env=cfg.env, num_envs=N, rollout_len=T, batch_size=B,
               hidden=cfg.hidden, updates_per_epoch=cfg.updates_per_epoch, epochs=a.epochs,
               env_steps_per_s=round(a.epochs * N * T / el, 1), grad_steps_per_s=round((tr.updates - u0) / el, 1),
               epoch_us=round(1e6 * el / a.epochs, 2))

    filled = min(tr.slots_written, cfg.buffer_slots) * N

    def rollout():  # the same slot and step every time: timing only
        dqn_rollout(tr.env_id, tr.q.params, cfg.hidden, T, 0, tr.ring, tr.state, tr.ep_len, tr.ep_ret, tr.ep_stats,
                    seed=tr.env_seed, step0=0, epsilon=0.1, reset_all=False, max_steps=tr.max_steps)

    def targets():
        dqn_targets(tr.q.params, tr.target, cfg.hidden, tr.A, tr.ring, filled, cfg.gamma, cfg.double_q, tr.sample_seed,
                    7, B, out=(tr.Xb, tr.act_b, tr.y, None))

    def grad_q():
        mlp_grad(GradHead.Q_TD, tr.q.params, tr.Xb, tr.A, cfg.hidden, act=tr.act_b, ret=tr.y, clip_eps=cfg.huber_delta,
                 grad_slab=tr.slab, loss_slab=tr.loss)

    adv = torch.randn(B, device=dev)

    def grad_pg():
        mlp_grad(GradHead.PG_CAT, tr.q.params, tr.Xb, tr.A, cfg.hidden, act=tr.act_b, adv=adv, grad_slab=tr.slab,
                 loss_slab=tr.loss)

    old = set_value_grad_mode(0)  # PG_CAT on the fp32-MFMA kernel, like Q_TD
    try:
        for name, fn in (("dqn_rollout", rollout), ("dqn_targets", targets), ("mlp_grad_q_td", grad_q),
                         ("mlp_grad_pg_cat", grad_pg)):
            fn()
            torch.cuda.synchronize()
            med, lo, hi = event_us(fn, a.iters, a.reps)
            rec[name + "_us"] = med
            rec[name + "_us_range"] = [lo, hi]
    finally:
        set_value_grad_mode(old)
    if a.prioritized:
        rec.update(per_records(a, dev, event_us))
    if a.n_step:
        rec.update(nstep_records(a, dev, event_us))
    if a.dueling:
        rec.update(dueling_records(a, dev, event_us))
    if a.noisy:
        rec.update(noisy_records(a, dev, event_us))
    if a.quantiles:
        rec.update(quantile_records(a, dev, event_us))
    rec.update(iters=a.iters, reps=a.reps, tag=a.tag, device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
