"""The bench.py driver contract on a real GPU, including the multi-rank launch.

The driver runs ``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N``
on an 8-GPU node over RCCL.  Here two ranks share the one GPU of the test box over gloo
(RRL_FORCE_DEVICE pins both to cuda:0), which exercises the same code path: rendezvous,
per-rank envs, gradient all-reduce every optimiser step, max-over-ranks timing and a single
JSON line from rank 0.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _json_lines(out):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def test_bench_single_gpu_contract(cuda):
    r = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--full", "--num-envs", "2048",
                        "--vf-iters", "4", "--ttt-seeds", "1", "--ttt-ref-seeds", "1", "--ref-cpu-seconds", "0",
                        "--convergence", "off"],
                       cwd=REPO, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = _json_lines(r.stdout)
    assert len(recs) == 1
    rec = recs[0]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in rec, k
    assert rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["value"] > 0
    assert rec["config"]["global_batch"] == 2048 * 64
    assert "time_to_threshold_s" in rec  # the second half of the metric, on by default on one GPU


def test_bench_plain_run_is_headline_only_and_dumps_outputs(cuda, tmp_path):
    """Without --full: warm-up, the timed steps and the record -- no secondary measurement -- and
    --dump-outputs writes what the last timed epoch left as float32 / float64 .npy files."""
    import numpy as np

    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--num-envs",
                        "2048", "--vf-iters", "4", "--dump-outputs", str(out)],
                       cwd=REPO, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = _json_lines(r.stdout)
    assert len(recs) == 1
    rec = recs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 2 and rec["value"] > 0 and rec["ms_per_step"] > 0
    # ms_per_step is the time of one timed step (rounded to 1 us: < 1 % of an epoch of >= 0.1 ms)
    assert rec["value"] == pytest.approx(2048 * 64 / (rec["ms_per_step"] * 1e-3), rel=1e-2)
    for k in ("time_to_threshold_s", "phase_ms_per_step", "host_env_path", "pong_a2c", "pong_a2c_big", "convergence",
              "actor_learner", "reference_equivalent_cpu"):
        assert k not in rec, k
    arrays = {p.name[:-4]: np.load(p) for p in out.iterdir()}
    assert {"pi_params", "vf_params", "ep_stats", "env_state", "ep_len", "ep_ret", "env_columns", "obs", "act",
            "logp", "rew", "done"} == set(arrays)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) < 64 << 20
    cols = arrays["env_columns"]
    assert cols.shape == (1024,) and (np.diff(cols) > 0).all() and cols[-1] < 2048
    assert arrays["obs"].shape == (65, 1024, 4) and arrays["logp"].shape == (64, 1024)
    assert arrays["env_state"].shape[0] == 2048
    # the sampled columns are the rollout the epoch learned from: CartPole pays 1 per step
    assert (arrays["rew"] == 1.0).all() and set(np.unique(arrays["act"])) <= {0.0, 1.0}


def test_bench_two_ranks_gloo_shared_gpu(cuda):
    env = dict(os.environ, RRL_DIST_BACKEND="gloo", RRL_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", "bench.py", "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--full", "--num-envs", "1024", "--vf-iters", "4", "--al-num-envs", "256",
           "--al-rollout-len", "32", "--al-vf-iters", "8", "--multi-ttt-seeds", "1", "--ttt-max-s", "15"]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=115)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = _json_lines(r.stdout)
    assert len(recs) == 1, r.stdout  # rank 0 only
    rec = recs[0]
    assert rec["n_gpus"] == 2 and rec["value"] > 0
    assert rec["config"]["parallelism"] == "dp2"
    assert rec["config"]["global_batch"] == 2 * 1024 * 64  # weak scaling: per-rank envs fixed
    # world > 1 records carry both halves of the metric, 1 seed here
    assert "time_to_threshold_s" in rec and rec["time_to_threshold"]["tuned"]["seeds"] == 1
    # the collective preflight ran first (gloo: nothing to capture, so eager collectives)
    assert rec["preflight"]["rccl_ok"] is True and rec["graphs"] is False
    # the secondary actor -> learner phase ran on the GPU: device-env rollouts on both ranks, the
    # remote rollout received into the learner's shard batch (K = 2), weights sent back with lag 1
    al = rec["actor_learner"]
    assert "error" not in al, al
    assert al["K"] == 2 and al["L"] == 1 and al["versions_ok"] is True and al["env_steps_per_s"] > 0
    assert al["per_rank"][0]["role"] == "learner" and al["per_rank"][1]["role"] == "actor"
    assert al["gather_ms"][0] > 0 and al["weight_recv_ms"][1] is not None


def test_bench_two_rccl_ranks(cuda):
    """``bench.py --gpus 2`` without a launcher: it starts torch.distributed.run itself, one
    rank per GPU over RCCL (the driver's scaling run).  Needs two visible GPUs."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (the 1-GPU box rehearses the rank logic over gloo above)")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("RRL_DIST_BACKEND", None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--num-envs",
                        "2048", "--vf-iters", "4"], cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = _json_lines(r.stdout)
    assert len(recs) == 1
    rec = recs[0]
    assert rec["n_gpus"] == 2 and rec["backend"] == "nccl" and rec["rccl_world"] == 2
    assert rec["config"]["parallelism"] == "dp2" and len(rec["per_rank_env_steps_per_s"]) == 2


def test_preflight_child_captures_a_real_rccl_all_reduce(cuda):
    """The preflight child on one MI355X with a one-rank RCCL communicator: init, 70 KB all-reduce,
    P2P self-ring, and an all-reduce captured into a hipGraph, replayed 3x, bitwise vs eager."""
    r = subprocess.run([sys.executable, "-m", "relayrl_prototype_amd.parallel.preflight", "--port", str(_free_port()),
                        "--rank", "0", "--world", "1", "--backend", "nccl", "--device", "0", "--timeout-s", "40"],
                       cwd=REPO, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True,
                       timeout=100)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RRL_PREFLIGHT ")]
    assert line, (r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(line[0][len("RRL_PREFLIGHT "):])
    assert res["rccl_ok"] and res["graphs_ok"] and res["stage"] == "done", res
    assert r.returncode == 0


def test_bench_gloo_capture_failure_injected(cuda):
    """VERDICT r5 #3 'done means': two gloo ranks on the one GPU with an injected capture failure
    still produce a valid line, with graphs false and the preflight recorded."""
    env = dict(os.environ, RRL_DIST_BACKEND="gloo", RRL_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0",
               RRL_PREFLIGHT_INJECT="capture")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", "bench.py", "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--num-envs", "1024", "--vf-iters", "4", "--actor-learner", "off", "--no-ttt",
           "--phase-steps", "0"]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = _json_lines(r.stdout)
    assert len(recs) == 1, r.stdout
    rec = recs[0]
    assert rec["value"] > 0 and rec["graphs"] is False
    assert rec["preflight"]["rccl_ok"] is True and rec["preflight"]["graphs_ok"] is False
