"""Categorical policies of more than 16 actions: microseconds per launch of ``mlp_forward(CAT_SAMPLE)`` and
``mlp_grad(PG_CAT)`` at D = 8, H = 128, B = 1,024 and 65,536, for A = 16 on the replicated heads (mlp_forward.hip,
mlp_grad.hip; no bf16x6 instance takes 16 actions) and A = 18 and 64 on the wide output layer (mlp_cat_wide.hip), all
in one process.

Each figure is the median over ``--reps`` windows of HIP events around ``--iters`` back-to-back launches, after a
warm-up of every shape; the range over the windows goes with it.  One JSON line per (B, A) is printed and appended to
``profiles/mlp_wide_actions_bench.jsonl`` (``--out``).  No threshold: the figures are recorded.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def event_us(fn, iters, reps):
    """Median, min and max over ``reps`` windows of the mean microseconds of ``iters`` back-to-back calls."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mlp_wide_actions_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_actions_bench needs a GPU: a CPU timing says nothing about the MI355X")
    from relayrl_prototype_amd.ops import FwdMode, GradHead, MLPSpec, grad_slabs, mlp_forward, mlp_grad

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D, H = 8, 128
    for B in (1024, 65536):
        for A in (16, 18, 64):
            gen = torch.Generator().manual_seed(A)
            pp, X = MLPSpec(D, H, A).init(gen).to(dev), torch.randn(B, D, generator=gen).to(dev)
            act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32).to(dev)
            adv = torch.randn(B, generator=gen).to(dev)
            out = dict(act=torch.empty(B, dtype=torch.int32, device=dev), logp=torch.empty(B, device=dev),
                       entropy=torch.empty(B, device=dev))
            ns = grad_slabs(B, dev)
            slab, loss = torch.empty(ns, pp.numel(), device=dev), torch.empty(ns, 8, device=dev)

            def fwd():
                mlp_forward(FwdMode.CAT_SAMPLE, pp, X, A, H, seed=1, step=2, out=out)

            def grad():
                mlp_grad(GradHead.PG_CAT, pp, X, A, H, act=act, adv=adv, grad_slab=slab, loss_slab=loss)

            rec = dict(bench="mlp_wide_actions", B=B, D=D, H=H, A=A,
                       kernels="mlp_cat_wide" if A > 16 else "mlp_forward / mlp_grad")
            for name, fn in (("mlp_forward_cat_sample", fwd), ("mlp_grad_pg_cat", grad)):
                for _ in range(a.warmup):
                    fn()
                torch.cuda.synchronize()
                med, lo, hi = event_us(fn, a.iters, a.reps)
                rec[name + "_us"] = med
                rec[name + "_us_range"] = [lo, hi]
            rec.update(iters=a.iters, reps=a.reps, tag=a.tag, device=torch.cuda.get_device_name(0))
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
