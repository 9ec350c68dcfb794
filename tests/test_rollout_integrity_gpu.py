"""Rollout integrity on the GPU: the checksum and verify kernels (csrc/kernels/checksum.hip) against
the numpy oracle, bit for bit, and ActorLearner's ``integrity`` modes on cuda:0 with injected faults."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from relayrl_prototype_amd import RolloutIntegrityError, ops
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.parallel.comm import Comm
from relayrl_prototype_amd.runtime.actor_learner import HDR, ActorLearner, ActorLearnerConfig
from relayrl_prototype_amd.utils import faults

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 20) + 3
COUNTS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 1027, BIG]
FAULT_BIT = {"stale": "seq", "skip": "seq", "mix": "checksum", "tear": "checksum"}


@pytest.fixture(scope="module")
def words(cuda):
    """Full-range random 32-bit words, on the host (int32 view) and in a 16-byte-aligned device
    allocation; never written after this."""
    w = np.random.default_rng(0).integers(0, 1 << 32, size=BIG + 8, dtype=np.uint64).astype(np.uint32).view(np.int32)
    host = torch.from_numpy(w.copy())
    dev = host.to(cuda)
    assert dev.data_ptr() % 16 == 0
    return host, dev


def _same(dev_segs, host_segs):
    got = ops.payload_checksum(dev_segs)
    assert got.is_cuda and got.dtype == torch.int64
    want = ref.payload_checksum_ref(host_segs)
    assert torch.equal(got.cpu(), want), (got.cpu().tolist(), want.tolist())
    return got


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_kernel_matches_oracle_for_every_count_and_start_offset(words, off):
    host, dev = words
    for n in COUNTS:
        _same([dev[off:off + n]], [host[off:off + n]])
        _same([dev[off:off + n].view(torch.float32)], [host[off:off + n]])


@pytest.mark.parametrize("nseg", [1, 2, 8])
def test_kernel_mixed_dtype_segments(words, nseg):
    host, dev = words
    # segments of odd lengths that start at elements 1, 2, 3, ... of the allocation, int32 / float32 alternating
    cuts = np.linspace(1, 3001, nseg + 1).astype(int) + np.arange(nseg + 1)
    hs = [host[cuts[i]:cuts[i + 1]] for i in range(nseg)]
    ds = [dev[cuts[i]:cuts[i + 1]] for i in range(nseg)]
    ds = [d.view(torch.float32) if i % 2 else d for i, d in enumerate(ds)]
    got = _same(ds, hs)
    whole = ops.payload_checksum([dev[cuts[0]:cuts[-1]]])
    assert torch.equal(got, whole)  # splitting changes nothing
    if nseg > 1:
        assert not torch.equal(ops.payload_checksum(ds[::-1]), got)
    # a float64 header row counts as pairs of words
    h = torch.tensor([3.0, -0.0, 1e300, 7.0], dtype=torch.float64)
    _same(ds[:7] + [h.to(dev.device)], hs[:7] + [h])


def test_kernel_counts_special_floats_as_their_bits(words):
    bits = np.array([0x80000000, 0x00000000, 0x7FC00001, 0x7FC00002, 0xFFC00001, 0x7F800001, 0xFF800000,
                     0x7F800000, 0x00000001], dtype=np.uint32)
    bits = np.tile(bits, 29)[:257]
    host = torch.from_numpy(bits.view(np.int32).copy())
    dev = host.cuda().view(torch.float32)
    assert torch.isnan(dev).any() and torch.isinf(dev).any()
    got = _same([dev], [host])
    canon = torch.where(torch.isnan(dev), torch.full_like(dev, float("nan")), dev)
    assert not torch.equal(ops.payload_checksum([canon]), got)  # distinct NaN payloads are distinct


def test_kernel_result_is_independent_of_the_grid_and_repeatable(words):
    host, dev = words
    segs = [dev[1:BIG], dev[2:1029].view(torch.float32)]
    want = ref.payload_checksum_ref([host[1:BIG], host[2:1029]])
    h = ops.hip()
    prev = h.set_cu_limit(0)
    try:
        res = []
        for lim in (1, 7, 0):
            h.set_cu_limit(lim)
            res.append(ops.payload_checksum(segs).cpu())
            res.append(ops.payload_checksum(segs).cpu())  # a second call: the sums are re-zeroed
    finally:
        h.set_cu_limit(prev)
    for r in res:
        assert torch.equal(r, want)


def test_kernel_rejects_bad_arguments(words):
    host, dev = words
    x = dev[:24].reshape(4, 6)
    assert torch.equal(ops.payload_checksum([x.t()]).cpu(), ref.payload_checksum_ref([host[:24].reshape(4, 6).t()]))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.payload_checksum([torch.zeros(4, dtype=torch.int16, device=dev.device)])
    with pytest.raises(ValueError, match="segments"):
        ops.payload_checksum([dev[:4]] * 9)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.hip().payload_checksum([x.t()], torch.zeros(2, dtype=torch.int64, device=dev.device))
    with pytest.raises(ValueError, match="is on cpu"):
        ops.payload_checksum([dev[:4], host[:4]])


@pytest.mark.parametrize("K", [1, 3])
def test_verify_kernel_status_bits(cuda, K):
    sums = torch.arange(1, 2 * K + 1, dtype=torch.int64).reshape(K, 2) * ((1 << 61) + 12345)
    hdr = torch.zeros(K, HDR, dtype=torch.float64)
    hdr[:, 0], hdr[:, 7] = 9.0, 5.0
    hdr.view(torch.int64)[:, 10:12] = sums

    def run(h, s, seq=9, lo=4, hi=5):
        st = ops.payload_verify(s.to(cuda), h.to(cuda), seq, lo, hi)
        assert st.dtype == torch.int32 and st.is_cuda
        assert st.cpu().tolist() == ops.payload_verify(s, h, seq, lo, hi).tolist()
        return st.cpu().tolist()

    assert run(hdr, sums) == [0] * K
    assert run(hdr, sums, lo=5, hi=5) == [0] * K and run(hdr, sums, lo=4, hi=4) == [4] * K
    j = K - 1
    bad_sum = sums.clone()
    bad_sum[j, 1] ^= 1 << 40
    want = [0] * K
    want[j] = 1
    assert run(hdr, bad_sum) == want
    h2 = hdr.clone()
    h2[j, 0] = 8.0
    want[j] = 2
    assert run(h2, sums) == want
    h4 = hdr.clone()
    h4[j, 7] = 6.0
    want[j] = 4
    assert run(h4, sums) == want
    h7 = h2.clone()
    h7[j, 7] = 3.0
    want[j] = 7
    assert run(h7, bad_sum) == want


# ---------------------------------------------------------------------- ActorLearner on cuda:0
def _make(integrity, env="LunarLanderSynth-v0", n=512, algo="reinforce"):
    cfg = ActorLearnerConfig(env=env, num_envs=n, rollout_len=32, algo=algo, train_vf_iters=4, train_pi_iters=2,
                             seed=3, learner_acts=True, integrity=integrity)
    return ActorLearner(cfg, Comm(collectives=False), device="cuda:0")


@pytest.fixture
def rollout_fault():
    yield faults.set_rollout_fault
    faults.set_rollout_fault(None)


def _first_epoch_buffers(al):
    torch.cuda.synchronize()
    out = {k: getattr(al, k).clone() for k in ("b_obs", "b_act", "b_logp", "b_rew", "b_done", "b_hdr")}
    if al.b_tobs is not None:
        out["b_tobs"] = al.b_tobs.clone()
    return out


def _assert_bitwise_equal_payload(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if k == "b_hdr":
            x, y = x[:, :10].contiguous().view(torch.int64), y[:, :10].contiguous().view(torch.int64)
        else:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


@pytest.mark.parametrize("env,n,algo", [("LunarLanderSynth-v0", 512, "reinforce"), ("HalfCheetahSynth-v0", 1024, "ppo")])
def test_actor_learner_clean_lagged_run(cuda, env, n, algo, rollout_fault):
    off = _make("off", env, n, algo)
    off.step()
    ref_bufs = _first_epoch_buffers(off)
    off.finish()
    assert off.b_hdr.view(torch.int64)[:, 10:].abs().sum().item() == 0
    al = _make("lagged", env, n, algo)
    assert al.actor.kind == "device" and (al.b_act.dtype == torch.float32) == (algo == "ppo")
    al.step()
    _assert_bitwise_equal_payload(_first_epoch_buffers(al), ref_bufs)
    # the header carries the oracle's sums of the slot it arrived with
    slot = al._slot(0)
    want = ref.payload_checksum_ref([p.cpu() for p in slot[:-1] if p is not None] + [slot[-1][:10].cpu()])
    assert torch.equal(al.b_hdr.view(torch.int64)[0, 10:].cpu(), want)
    for _ in range(3):
        al.step()
    al.finish()
    m = al.metrics()
    assert m["IntegrityChecked"] == 4 and m["IntegrityMismatches"] == 0 and m["ActorSeqs"] == [4.0]
    if algo == "ppo":  # float actions and tobs are covered: a payload swap in this layout is caught at once
        st = _make("strict", env, n, algo)
        st.step()
        rollout_fault("0:1:mix")
        with pytest.raises(RolloutIntegrityError, match="bits=checksum "):
            st.step()
        st.watchdog.close()


@pytest.mark.parametrize("kind", ["stale", "mix", "tear", "skip"])
@pytest.mark.parametrize("mode", ["strict", "lagged"])
def test_actor_learner_detects_every_fault(cuda, mode, kind, rollout_fault):
    al = _make(mode)
    al.step()
    al.step()
    rollout_fault(f"0:2:{kind}")
    if mode == "strict":
        torch.cuda.synchronize()
        before = al.learner.pi.params.clone()
        with pytest.raises(RolloutIntegrityError) as ei:
            al.step()
        torch.cuda.synchronize()
        assert torch.equal(al.learner.pi.params.view(torch.int32), before.view(torch.int32))
    else:
        al.step()  # read one step late
        with pytest.raises(RolloutIntegrityError) as ei:
            al.step()
    msg = str(ei.value)
    assert "actor 0" in msg and "epoch 2" in msg, msg
    assert f"bits={FAULT_BIT[kind]}" in msg or f"+{FAULT_BIT[kind]}" in msg, msg
    if kind in ("mix", "tear"):
        assert "bits=checksum " in msg, msg
    al.watchdog.close()


# ---------------------------------------------------------------------- two gloo ranks on cuda:0
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_gloo_ranks_share_the_gpu_strict(cuda):
    """The only place the raw 64-bit header columns cross a real device-tensor P2P."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", "tools/probes/integrity_gloo_probe.py",
           "--steps", "3", "--integrity", "strict", "--max-lag", "1"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=REPO)
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(rec) == 1, r.stdout
    assert rec[0]["IntegrityMismatches"] == 0 and rec[0]["IntegrityChecked"] == 3, rec[0]
    assert rec[0]["ActorSeqs"] == [3.0] and rec[0]["versions"] == [[0], [0], [1]], rec[0]
    assert rec[0]["checksum_columns_nonzero"] is True
