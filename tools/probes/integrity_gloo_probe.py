"""Rollout integrity across a real device-tensor P2P: two gloo ranks share cuda:0.

Rank 0 learns only, rank 1 acts only.  Every rollout (payload on the device, header with the raw
64-bit checksum columns) crosses gloo send / recv into the learner's shard batch, where the
checksum kernel recomputes the sums and the verify kernel compares them, the sequence number and
the weight version.  Prints one JSON line from rank 0; a failed check raises (exit code != 0).

    torchrun --nproc-per-node 2 --master-addr 127.0.0.1 tools/probes/integrity_gloo_probe.py --integrity strict
"""
import argparse
import json
import os

import torch
import torch.distributed as dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--integrity", choices=("off", "lagged", "strict"), default="strict")
    ap.add_argument("--max-lag", type=int, default=1)
    ap.add_argument("--env", default="LunarLanderSynth-v0")
    ap.add_argument("--num-envs", type=int, default=512)
    ap.add_argument("--rollout-len", type=int, default=32)
    a = ap.parse_args()
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    from relayrl_prototype_amd.parallel.comm import Comm
    from relayrl_prototype_amd.runtime.actor_learner import ActorLearner, ActorLearnerConfig

    cfg = ActorLearnerConfig(env=a.env, num_envs=a.num_envs, rollout_len=a.rollout_len, train_vf_iters=4, seed=3,
                             max_lag=a.max_lag, learner_ranks=1, learner_acts=False, integrity=a.integrity,
                             stall_timeout_s=60.0)
    al = ActorLearner(cfg, Comm(), device="cuda:0")
    versions = []
    for _ in range(a.steps):
        al.step()
        if al.is_learner:
            versions.append([int(x) for x in al.b_hdr[:, 7].tolist()])
    al.finish()
    m = al.metrics()
    if al.is_learner:
        ck = al.b_hdr.view(torch.int64)[:, 10:12].cpu()
        print(json.dumps({"integrity": a.integrity, "max_lag": a.max_lag, "steps": a.steps, "versions": versions,
                          "ActorSeqs": m.get("ActorSeqs"), "IntegrityChecked": m.get("IntegrityChecked"),
                          "IntegrityMismatches": m.get("IntegrityMismatches"),
                          "checksum_columns_nonzero": bool((ck != 0).all()), "backend": "gloo",
                          "device": torch.cuda.get_device_name(0)}), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    os._exit(0)


if __name__ == "__main__":
    main()
