"""Rollout integrity on the CPU: the numpy checksum oracle, and ActorLearner's ``integrity`` modes
in one process and over three gloo ranks, with the data-plane faults of utils/faults.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from relayrl_prototype_amd import RolloutIntegrityError, ops
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.parallel.comm import Comm
from relayrl_prototype_amd.runtime import actor_learner as alm
from relayrl_prototype_amd.runtime.actor_learner import HDR, ActorLearner, ActorLearnerConfig
from relayrl_prototype_amd.utils import faults

M64 = (1 << 64) - 1
FAULT_BIT = {"stale": "seq", "skip": "seq", "mix": "checksum", "tear": "checksum"}


def _sums(segments):
    s = ref.payload_checksum_ref(segments).numpy().view(np.uint64)
    return int(s[0]), int(s[1])


def _bigint(words, base=0):
    s1 = s2 = 0
    for i, w in enumerate(words):
        s1 += int(w)
        s2 += (base + i + 1) * int(w)
    return s1 & M64, s2 & M64


def _rand_words(n, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


# ---------------------------------------------------------------------- oracle properties
def test_any_single_bit_flip_changes_s1():
    w = _rand_words(37, 1)
    s1 = _sums([w])[0]
    for i in range(w.size):
        for b in range(32):
            x = w.copy()
            x[i] ^= np.uint32(1 << b)
            assert _sums([x])[0] != s1, (i, b)


def test_swap_of_unequal_words_keeps_s1_and_changes_s2():
    w = _rand_words(101, 2)
    a = _sums([w])
    for i, j in ((0, 1), (3, 77), (50, 100)):
        assert w[i] != w[j]
        x = w.copy()
        x[i], x[j] = w[j], w[i]
        b = _sums([x])
        assert b[0] == a[0] and b[1] != a[1], (i, j)


def test_segment_order_changes_s2():
    u, v = _rand_words(40, 3), _rand_words(24, 4)
    a, b = _sums([u, v]), _sums([v, u])
    assert a[0] == b[0] and a[1] != b[1]


@pytest.mark.parametrize("nseg", [1, 2, 8])
def test_split_into_segments_gives_identical_sums(nseg):
    w = _rand_words(1027, 5)
    cuts = [0] + sorted(np.random.default_rng(6).choice(np.arange(1, w.size), nseg - 1, replace=False).tolist()) + [w.size]
    segs = [w[cuts[i]:cuts[i + 1]] for i in range(nseg)]
    assert _sums(segs) == _sums([w]) == _bigint(w)


def test_s2_wraps_past_2_64_and_matches_bigint():
    w = _rand_words((1 << 20) + 3, 7)
    whole = _sums([w])
    assert _sums([w[:4099]]) == _bigint(w[:4099])
    words = w.tolist()
    exact = sum((i + 1) * x for i, x in enumerate(words))
    assert exact > M64  # the unreduced s2 does not fit 64 bits
    assert whole == (sum(words) & M64, exact & M64)
    # and an independent numpy formulation of the whole buffer (32-bit halves of the index)
    idx = np.arange(1, w.size + 1, dtype=np.uint64)
    w64 = w.astype(np.uint64)
    hi, lo = (idx >> np.uint64(32)), (idx & np.uint64(0xFFFFFFFF))
    s2 = int((((hi * w64) << np.uint64(32)) + lo * w64).sum(dtype=np.uint64))
    assert whole == (int(w64.sum(dtype=np.uint64)), s2)


def test_float_payloads_count_as_their_bits():
    bits = np.array([0x80000000, 0x00000000, 0x7FC00001, 0x7FC00002, 0xFF800000, 0x7F800000], dtype=np.uint32)
    t = torch.from_numpy(bits.view(np.float32).copy())
    assert _sums([t]) == _bigint(bits)
    i = torch.from_numpy(bits.view(np.int32).copy())
    h = torch.tensor([1.0, -2.5], dtype=torch.float64)
    got = ops.payload_checksum([t, None, i, h]).numpy().view(np.uint64)
    want = _bigint(np.concatenate([bits, bits, h.numpy().view(np.uint32)]))
    assert (int(got[0]), int(got[1])) == want


def test_noncontiguous_segment_is_checksummed_in_logical_order():
    x = torch.arange(24, dtype=torch.int32).reshape(4, 6)
    got = ops.payload_checksum([x.t()])
    assert torch.equal(got, ops.payload_checksum([x.t().contiguous()]))
    assert not torch.equal(got, ops.payload_checksum([x]))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.payload_checksum([torch.zeros(4, dtype=torch.int16)])
    with pytest.raises(ValueError, match="segments"):
        ops.payload_checksum([x] * 9)


def test_verify_reference_status_bits():
    K = 3
    hdr = torch.zeros(K, HDR, dtype=torch.float64)
    sums = torch.tensor([[5, -7], [1 << 62, 3], [0, 0]], dtype=torch.int64)
    hdr[:, 0], hdr[:, 7] = 4.0, 2.0
    hdr.view(torch.int64)[:, 10:12] = sums
    assert ops.payload_verify(sums, hdr, 4, 1, 2).tolist() == [0, 0, 0]
    hdr[1, 0] = 3.0
    hdr[2, 7] = 0.0
    bad = sums.clone()
    bad[0, 1] += 1
    assert ops.payload_verify(bad, hdr, 4, 1, 2).tolist() == [1, 2, 4]


# ---------------------------------------------------------------------- single process
def _make(integrity, seed=11):
    cfg = ActorLearnerConfig(env="CartPole-v1", num_envs=8, rollout_len=16, hidden=64, train_vf_iters=2,
                             num_threads=1, seed=seed, learner_acts=True, integrity=integrity)
    return ActorLearner(cfg, Comm(collectives=False), device="cpu")


@pytest.fixture
def rollout_fault():
    yield faults.set_rollout_fault
    faults.set_rollout_fault(None)


@pytest.fixture(scope="module")
def off_first_epoch():
    """Buffers of the integrity="off" run after its first step: the reference the other modes share."""
    al = _make("off")
    al.step()
    al.finish()
    return {k: getattr(al, k).clone() for k in ("b_obs", "b_act", "b_rew", "b_hdr")}


@pytest.mark.parametrize("mode", ["lagged", "strict"])
def test_clean_run_checks_every_slot_and_leaves_the_data_alone(mode, off_first_epoch):
    al = _make(mode)
    al.step()
    for k in ("b_obs", "b_act", "b_rew"):
        assert torch.equal(getattr(al, k).view(torch.int32), off_first_epoch[k].view(torch.int32)), k
    assert torch.equal(al.b_hdr[:, :10].contiguous().view(torch.int64),
                       off_first_epoch["b_hdr"][:, :10].contiguous().view(torch.int64))
    assert torch.equal(off_first_epoch["b_hdr"][:, 10:], torch.zeros(1, 2, dtype=torch.float64))
    assert al.b_hdr.view(torch.int64)[0, 10:].tolist() != [0, 0]
    for _ in range(3):
        al.step()
    al.finish()
    m = al.metrics()
    assert m["IntegrityChecked"] == 4 and m["IntegrityMismatches"] == 0
    assert m["ActorSeqs"] == [4.0]
    assert al._seen_seq == {0: 4}


@pytest.mark.parametrize("kind", ["stale", "mix", "tear", "skip"])
def test_strict_raises_in_the_faulty_step_before_the_weights_change(kind, rollout_fault):
    al = _make("strict")
    al.step()
    al.step()
    rollout_fault(f"0:2:{kind}")
    before = al.learner.pi.params.clone()
    with pytest.raises(RolloutIntegrityError) as ei:
        al.step()
    msg = str(ei.value)
    assert f"bits={FAULT_BIT[kind]}" in msg or f"+{FAULT_BIT[kind]}" in msg, msg
    assert "actor 0" in msg and "epoch 2" in msg and "seq expected 3" in msg, msg
    if kind in ("mix", "tear"):
        assert "bits=checksum " in msg and "received 3" in msg, msg  # only the checksum bit
    assert torch.equal(al.learner.pi.params.view(torch.int32), before.view(torch.int32))
    assert al.integrity_mismatches == 1
    al.watchdog.close()


@pytest.mark.parametrize("kind", ["stale", "mix", "tear", "skip"])
@pytest.mark.parametrize("follow", [True, False])
def test_lagged_raises_within_one_step(kind, follow, rollout_fault):
    al = _make("lagged")
    al.step()
    al.step()
    rollout_fault(f"0:2:{kind}")
    al.step()  # the faulty epoch: its status is read one step late
    with pytest.raises(RolloutIntegrityError) as ei:
        al.step() if follow else al.finish()
    msg = str(ei.value)
    assert "epoch 2" in msg and (f"bits={FAULT_BIT[kind]}" in msg or f"+{FAULT_BIT[kind]}" in msg), msg
    al.watchdog.close()


def test_off_does_not_notice_a_stale_rollout(rollout_fault):
    al = _make("off")
    al.step()
    al.step()
    rollout_fault("0:2:stale")
    al.step()
    al.step()
    al.finish()
    assert "IntegrityChecked" not in al.metrics()


def test_seq_continues_after_load_state_dict():
    a = _make("strict")
    for _ in range(3):
        a.step()
    a.finish()
    sd = a.state_dict()
    assert sd["epoch"] == 3
    b = _make("strict", seed=12)
    b.load_state_dict(sd)
    b.step()
    b.finish()
    assert b.b_hdr[0, 0].item() == 4.0
    m = b.metrics()
    assert m["IntegrityChecked"] == 1 and m["IntegrityMismatches"] == 0 and m["ActorSeqs"] == [4.0]


def test_config_rejects_an_unknown_mode():
    with pytest.raises(ValueError, match="integrity"):
        _make("sometimes")
    assert alm.INTEGRITY_MODES == ("off", "lagged", "strict")


# ---------------------------------------------------------------------- three gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, q, lag, fault):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        torch.set_num_threads(1)
        import torch.distributed as dist

        from relayrl_prototype_amd.parallel.comm import init_distributed

        comm = init_distributed(backend="gloo")
        if fault:
            faults.set_rollout_fault(fault)
        cfg = ActorLearnerConfig(env="CartPole-v1", num_envs=8, rollout_len=16, hidden=64, train_vf_iters=2,
                                 train_pi_iters=2, num_threads=1, seed=5, max_lag=lag, learner_ranks=1,
                                 learner_acts=False, integrity="strict")
        al = ActorLearner(cfg, comm, device="cpu")
        versions = []
        try:
            for _ in range(3):
                al.step()
                if al.is_learner:
                    versions.append([int(x) for x in al.b_hdr[:, 7].tolist()])
        except RolloutIntegrityError as e:
            q.put((rank, "integrity", str(e)))
            q.close()
            q.join_thread()
            os._exit(3)  # the peers are blocked on this rank: the parent ends them
        al.finish()
        m = al.metrics()
        q.put((rank, "ok", (m.get("ActorSeqs"), versions, m.get("IntegrityChecked"), m.get("IntegrityMismatches"))))
        dist.destroy_process_group()
    except Exception:
        import traceback

        q.put((rank, "error", traceback.format_exc()))


def _spawn(lag, fault):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_gloo_worker, args=(r, 3, port, q, lag, fault)) for r in range(3)]
    for p in ps:
        p.start()
    return ps, q


def _reap(ps):
    for p in ps:
        if p.is_alive():
            p.kill()
        p.join(timeout=10)


@pytest.mark.parametrize("lag", [0, 1])
def test_gloo_three_ranks_strict_clean(lag):
    ps, q = _spawn(lag, None)
    try:
        res = sorted((q.get(timeout=120) for _ in range(3)), key=lambda r: r[0])
        for p in ps:
            p.join(timeout=30)
    finally:
        _reap(ps)
    for r in res:
        assert r[1] == "ok", r
    seqs, versions, checked, bad = res[0][2]
    assert seqs == [3.0, 3.0]
    assert checked == 6 and bad == 0
    for k, vs in enumerate(versions):
        assert vs == [max(k - lag, 0)] * 2, (k, vs)


def test_gloo_stale_last_slot_is_reported_by_the_learner():
    ps, q = _spawn(1, "0:2:stale")
    try:
        while True:  # actors report nothing before the learner does: they wait for its weights
            r = q.get(timeout=120)
            if r[0] == 0:
                break
        assert r[1] == "integrity", r
        assert "actor 2" in r[2] and "seq" in r[2] and "epoch 2" in r[2], r[2]
        ps[0].join(timeout=30)
        assert ps[0].exitcode == 3
    finally:
        _reap(ps)  # no rank waits for a collective timeout
