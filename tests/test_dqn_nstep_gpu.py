"""n-step returns on the GPU: the n-step instances of the targets kernel (csrc/kernels/dqn.hip), uniform and
prioritised, against the float64 walk and target of ops/dqn.py, and the DQNTrainer with ``n_step`` (resume,
learning, the ``cartpole-dqn-nstep`` preset).  Every output buffer of a kernel under test is guarded."""
import os

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import MLPSpec, PriorityTree, ReplayRing, dqn_nstep_walk_ref, dqn_sample_rows_ref
from relayrl_prototype_amd.ops import dqn_targets, hip, per_insert, per_sample_rows_ref, per_tree_build, per_tree_leaves
from relayrl_prototype_amd.ops import per_update
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer

import dqn_nstep_oracle as dn
import dqn_oracle as do
from guarded import INT_SENTINEL, Guarded
from test_dqn_gpu import FWD_TOL, TRAINER, _bits, cu_limit, guarded_ring

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS_C, NS_N = 6, 17
CONFIGS = [(3 * NS_N, 2), (6 * NS_N, 5), (6 * NS_N, 2)]  # (filled, newest): the last one wraps
N_STEPS = (2, 3, 8)
BATCHES = (1, 65, 1000)
SEED, GAMMA, BETA = (3 << 32) | 5, 0.97, 0.7
# The done codes of the ring, the same for every case.  About one row in four ends an episode, half of them
# each way.  The seed was picked on the CPU, from the oracle alone, so that the samples of the cases below meet
# every walk ending and every walk length (Coverage.check asserts it again in every test).
DONE_SEED = 4
KINDS = ("full", "terminal", "truncation", "newest")


def host_ring(D, A, seed):
    gen = torch.Generator().manual_seed(seed)
    C, N = NS_C, NS_N
    u = torch.rand(C, N, generator=torch.Generator().manual_seed(DONE_SEED))
    done = torch.where(u < 0.125, 1.0, torch.where(u < 0.25, 2.0, 0.0))
    assert set(done.unique().tolist()) == {0.0, 1.0, 2.0}
    return ReplayRing(torch.randn(C, N, D, generator=gen), torch.randn(C, N, D, generator=gen),
                      torch.randint(0, A, (C, N), generator=gen, dtype=torch.int32), torch.randn(C, N, generator=gen),
                      done)


def device_ring(host):
    g, dev = guarded_ring(NS_C, NS_N, host.obs.shape[-1])
    for dst, src in zip(dev, host):
        dst.copy_(src)
    return g, dev


def walk_kinds(host, last, m, n, newest):
    """Why each walk ended, from the oracle's (last, m): the order of the loop's own tests."""
    done = host.done.reshape(-1).numpy()[last]
    return np.where(m == n, "full", np.where(done == 1, "terminal", np.where(done == 2, "truncation", "newest")))


class Coverage:
    """Walk endings and lengths the cases of one test met, by n."""

    def __init__(self):
        self.kinds = {n: set() for n in N_STEPS}
        self.ms = {n: set() for n in N_STEPS}

    def add(self, n, kinds, m, last, newest):
        self.kinds[n] |= set(kinds.tolist())
        self.ms[n] |= set(m.tolist())
        assert ((kinds != "newest") | (last // NS_N == newest)).all()

    def check(self):
        for n in N_STEPS:
            # a ring of C slots has no walk of more than C steps: n = 8 never runs its full length
            want = set(KINDS) if n <= NS_C else set(KINDS) - {"full"}
            assert self.kinds[n] == want, (n, self.kinds[n])
            assert self.ms[n] == set(range(1, min(n, NS_C) + 1)), (n, self.ms[n])


def check_targets(out, host, rows, filled, newest, n, online, target, H, A, double_q, cov):
    """idx, last, Xb, act_b exactly; y against the float64 walk and networks."""
    D = host.obs.shape[-1]
    Xb, act_b, y, idx = (o.t.cpu() for o in out[:4])
    got_last = out[-1].t.cpu()
    np.testing.assert_array_equal(idx.numpy(), rows)
    last, G, disc, m = dqn_nstep_walk_ref(rows, host, filled, newest, n, GAMMA, torch.float64)
    np.testing.assert_array_equal(got_last.numpy(), last)
    assert last.min() >= 0 and last.max() < filled and ((last - rows) % filled == (m - 1) * NS_N).all()
    cov.add(n, walk_kinds(host, last, m, n, newest), m, last, newest)
    r = torch.from_numpy(rows)
    assert torch.equal(Xb.view(torch.int32), host.obs.reshape(-1, D)[r].view(torch.int32))
    assert torch.equal(act_b, host.act.reshape(-1)[r])
    # y against the float64 oracle; any action within tol of the selecting net's maximum may be a*
    la = torch.from_numpy(last)
    nobs = host.nobs.reshape(-1, D)[la].double()
    qt = ref.trunk(target.double(), nobs, D, H, A)[0]
    sel = ref.trunk(online.double(), nobs, D, H, A)[0] if double_q else qt
    top = sel.max(-1, keepdim=True).values
    cand = sel >= top - (FWD_TOL["atol"] + FWD_TOL["rtol"] * top.abs())
    boot = (host.done.reshape(-1)[la] != 1).double()
    ys = torch.from_numpy(G).unsqueeze(-1) + (torch.from_numpy(disc) * boot).unsqueeze(-1) * qt
    ok = ((y.double().unsqueeze(-1) - ys).abs() <= FWD_TOL["atol"] + FWD_TOL["rtol"] * ys.abs()) & cand
    assert bool(ok.any(-1).all()), (n, filled, newest, int((~ok.any(-1)).sum()))


def assert_same_bits(a, b):
    for x, y in zip(a, b):
        assert y.guards_intact() and np.array_equal(_bits(x.t.cpu().numpy()), _bits(y.t.cpu().numpy()))


# ------------------------------------------------------------------ 1. the uniform n-step instance
@pytest.mark.parametrize("double_q", [False, True])
@pytest.mark.parametrize("H,A", [(H, A) for H in (64, 128) for A in (2, 3, 4)])
def test_nstep_targets_walk_gather_and_target(cuda, H, A, double_q):
    D = 2 * A
    host = host_ring(D, A, 100 * H + A)
    g, ring = device_ring(host)
    online = MLPSpec(D, H, A).init(torch.Generator().manual_seed(11))
    target = MLPSpec(D, H, A).init(torch.Generator().manual_seed(12))
    cov = Coverage()

    def launch(B, filled, newest, upd, n):
        out = (Guarded((B, D)), Guarded((B,), torch.int32), Guarded((B,)), Guarded((B,), torch.int32),
               Guarded((B,), torch.int32))
        dqn_targets(online.to(DEV), target.to(DEV), H, A, ring, filled, GAMMA, double_q, SEED, upd, B,
                    out=tuple(o.t for o in out), n_step=n, newest=newest)
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in out) and all(b.guards_intact() for b in g.values())
        return out

    for n in N_STEPS:
        for B in BATCHES:
            for filled, newest in CONFIGS:
                upd = 2 ** 32 - 1 + B  # the update counter's high word matters
                out = launch(B, filled, newest, upd, n)
                rows = dqn_sample_rows_ref(SEED, upd, B, filled)
                check_targets(out, host, rows, filled, newest, n, online, target, H, A, double_q, cov)
                if B == 1000:  # two workgroups stride over the 16 slabs: the same bits
                    with cu_limit(2):
                        assert_same_bits(out, launch(B, filled, newest, upd, n))
    cov.check()
    for k, b in g.items():  # the ring is an input: not one bit of it changed
        assert np.array_equal(_bits(b.t.cpu().numpy()), _bits(getattr(host, k).numpy())), k


def test_nstep_targets_without_the_optional_outputs(cuda):
    """idx and last left out: y, Xb and act_b are those of the launch that writes them."""
    H, A, D, B, n = 64, 2, 4, 65, 3
    host = host_ring(D, A, 7)
    _, ring = device_ring(host)
    p, q = (MLPSpec(D, H, A).init(torch.Generator().manual_seed(s)).to(DEV) for s in (11, 12))
    filled, newest = CONFIGS[2]
    full = dqn_targets(p, q, H, A, ring, filled, GAMMA, True, SEED, 9, B, n_step=n, newest=newest)
    assert len(full) == 5 and full[4].dtype == torch.int32
    out = (Guarded((B, D)), Guarded((B,), torch.int32), Guarded((B,)))
    dqn_targets(p, q, H, A, ring, filled, GAMMA, True, SEED, 9, B, out=tuple(o.t for o in out) + (None,), n_step=n,
                newest=newest)
    torch.cuda.synchronize()
    for a, b in zip(full, out):
        assert b.guards_intact() and np.array_equal(_bits(a.cpu().numpy()), _bits(b.t.cpu().numpy()))


# ------------------------------------------------------------------ 2. the prioritised n-step instance
def device_tree(filled, seed):
    """A tree in guarded device buffers whose first ``filled`` leaves the tree kernels set: per_insert at pmax = 1,
    then per_update of every row with a random |td|."""
    L = NS_C * NS_N
    gt, gp = Guarded((2 * per_tree_leaves(L),), fill=0.0), Guarded((1,), fill=np.float32(1.0))
    pt = PriorityTree(gt.t, gp.t, L)
    assert per_insert(pt, NS_C, NS_N, filled // NS_N, 0) == 0
    td = np.random.default_rng(seed).uniform(0.0, 4.0, filled).astype(np.float32)
    per_update(pt, torch.arange(filled, dtype=torch.int32, device=DEV), torch.from_numpy(td).to(DEV), 0.6, 1e-3)
    torch.cuda.synchronize()
    leaves = pt.leaves.cpu()
    assert gt.guards_intact() and bool((leaves[:filled] > 0).all()) and bool((leaves[filled:] == 0).all())
    assert leaves[:filled].unique().numel() > filled // 2, "the priorities are not uniform"
    assert torch.equal(gt.t.cpu().view(torch.int32), per_tree_build(leaves).view(torch.int32))
    return gt, pt


@pytest.mark.parametrize("double_q", [False, True])
@pytest.mark.parametrize("H,A", [(H, A) for H in (64, 128) for A in (2, 3, 4)])
def test_prioritised_nstep_targets(cuda, H, A, double_q):
    D = 2 * A
    host = host_ring(D, A, 100 * H + A)
    g, ring = device_ring(host)
    online = MLPSpec(D, H, A).init(torch.Generator().manual_seed(11))
    target = MLPSpec(D, H, A).init(torch.Generator().manual_seed(12))
    cov = Coverage()

    def launch(tree, B, filled, newest, upd, n):
        out = (Guarded((B, D)), Guarded((B,), torch.int32), Guarded((B,)), Guarded((B,), torch.int32), Guarded((B,)),
               Guarded((1,)))
        kw = {}
        if n > 1:
            out += (Guarded((B,), torch.int32),)
            kw = dict(n_step=n, newest=newest)
        dqn_targets(online.to(DEV), target.to(DEV), H, A, ring, filled, GAMMA, double_q, SEED, upd, B, tree=tree,
                    beta=BETA, out=tuple(o.t for o in out), **kw)
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in out) and all(b.guards_intact() for b in g.values())
        return out

    trees = {filled: device_tree(filled, filled) for filled in sorted({f for f, _ in CONFIGS})}
    for n in N_STEPS:
        for B in BATCHES:
            for filled, newest in CONFIGS:
                upd = 2 ** 32 - 1 + B
                gt, pt = trees[filled]
                before = gt.big.clone()
                out = launch(pt.tree, B, filled, newest, upd, n)
                assert torch.equal(gt.big.view(torch.int32), before.view(torch.int32)), "the sampler wrote to the tree"
                rows = per_sample_rows_ref(pt.tree, SEED, upd, B, filled)
                assert rows.max() < filled
                check_targets(out, host, rows, filled, newest, n, online, target, H, A, double_q, cov)
                # n_step leaves the draw and its weights alone: the one-step launch's bits
                one = launch(pt.tree, B, filled, newest, upd, 1)
                for i in (0, 1, 3, 4, 5):  # Xb, act_b, idx, w, wmax
                    assert np.array_equal(_bits(out[i].t.cpu().numpy()), _bits(one[i].t.cpu().numpy())), i
                if B == 1000:
                    with cu_limit(2):
                        assert_same_bits(out, launch(pt.tree, B, filled, newest, upd, n))
    cov.check()


# ------------------------------------------------------------------ 3. refusals
def _sentinels_only(bufs):
    for b in bufs:
        whole = b.big.cpu()
        if not (bool(torch.isnan(whole).all()) if whole.dtype.is_floating_point else bool((whole == INT_SENTINEL).all())):
            return False
    return True


def test_nstep_entry_points_refuse_bad_arguments(cuda):
    """n_step = 0, newest = filled / N and filled % N != 0: the entry points' codes raise, and nothing is written."""
    D, H, A, B = 4, 64, 2, 8
    host = host_ring(D, A, 1)
    _, ring = device_ring(host)
    p = MLPSpec(D, H, A).init(torch.Generator().manual_seed(1)).to(DEV)
    _, pt = device_tree(NS_C * NS_N, 1)
    h = hip()
    N = NS_N
    bad = [(0, 0, 6 * N), (3, 6, 6 * N), (3, 3, 3 * N), (3, -1, 6 * N), (3, 0, 3 * N + 1)]  # (n_step, newest, filled)
    for n, newest, filled in bad:
        out = (Guarded((B, D)), Guarded((B,), torch.int32), Guarded((B,)), Guarded((B,), torch.int32),
               Guarded((B,), torch.int32))
        with pytest.raises(RuntimeError, match="code -[24]"):
            h.dqn_targets(p, p, H, A, ring.obs, ring.nobs, ring.act, ring.rew, ring.done, filled, 0.9, True, 1, 0,
                          *(o.t for o in out[:4]), n_step=n, newest=newest, last=out[4].t)
        with pytest.raises(ValueError):  # the wrapper says why before it launches
            dqn_targets(p, p, H, A, ring, filled, 0.9, True, 1, 0, B, out=tuple(o.t for o in out), n_step=n,
                        newest=newest)
        w, wmax = Guarded((B,)), Guarded((1,))
        with pytest.raises(RuntimeError, match="code -[24]"):
            h.dqn_targets(p, p, H, A, ring.obs, ring.nobs, ring.act, ring.rew, ring.done, filled, 0.9, True, 1, 0,
                          *(o.t for o in out[:4]), tree=pt.tree, beta=0.5, w=w.t, wmax=wmax.t, n_step=n, newest=newest,
                          last=out[4].t)
        torch.cuda.synchronize()
        assert _sentinels_only(out + (w, wmax)), (n, newest, filled)
    with pytest.raises(ValueError, match="newest"):
        dqn_targets(p, p, H, A, ring, 6 * N, 0.9, True, 1, 0, B, n_step=3)
    # the sound calls, for contrast; n_step = 1 with the walk's arguments is the one-step launch
    out = tuple(Guarded(s, d) for s, d in (((B, D), torch.float32), ((B,), torch.int32), ((B,), torch.float32),
                                           ((B,), torch.int32), ((B,), torch.int32)))
    h.dqn_targets(p, p, H, A, ring.obs, ring.nobs, ring.act, ring.rew, ring.done, 6 * N, 0.9, True, 1, 0,
                  *(o.t for o in out[:4]), n_step=1, newest=5, last=out[4].t)
    one = dqn_targets(p, p, H, A, ring, 6 * N, 0.9, True, 1, 0, B)
    torch.cuda.synchronize()
    for a, b in zip(one, out):
        assert b.guards_intact() and np.array_equal(_bits(a.cpu().numpy()), _bits(b.t.cpu().numpy()))
    assert torch.equal(out[4].t, out[3].t)


# ------------------------------------------------------------------ 4. trainer
NAMES = ["online", "m", "v", "step", "target", "obs", "nobs", "act", "rew", "done", "state", "ep_len", "ep_ret", "tree",
         "pmax"]


@pytest.mark.parametrize("prioritized", [False, True])
def test_nstep_trainer_resume_is_bitwise(cuda, prioritized):
    kw = dict(TRAINER, n_step=3, prioritized=prioritized, per_beta_epochs=4)
    a = DQNTrainer(DQNConfig(**kw), device=cuda)
    for _ in range(6):
        a.train_epoch()
    b = DQNTrainer(DQNConfig(**kw), device=cuda)
    for _ in range(3):
        b.train_epoch()
    sd = b.state_dict()
    assert sd["cfg"]["n_step"] == 3 and set(sd) == set(DQNTrainer(DQNConfig(**dict(kw, n_step=1)), device=cuda).state_dict())
    c = DQNTrainer(DQNConfig(**kw), device=cuda)
    c.q.params.add_(1.0)  # other weights until the load
    c.load_state_dict(sd)
    for _ in range(3):
        c.train_epoch()
    torch.cuda.synchronize()
    assert a.counters() == c.counters() and a.updates == 12 and a.cursor == 0 and a.slots_written == 24
    for n, x, y in zip(NAMES, a.snapshot_tensors(), c.snapshot_tensors()):
        assert torch.equal(x, y), f"{n} differs after the resume"
    m = a.metrics()
    assert m["NStep"] == 3 and m["Updates"] == 12 and np.isfinite(m["LossQ"]) and np.isfinite(m["QVals"])
    assert bool(torch.isfinite(a.q.params).all())


@pytest.mark.parametrize("prioritized", [False, True])
def test_n_step_one_is_the_default_trainer_and_three_is_not(cuda, prioritized):
    kw = dict(TRAINER, prioritized=prioritized, per_beta_epochs=4)
    trainers = [DQNTrainer(DQNConfig(**kw), device=cuda), DQNTrainer(DQNConfig(**kw, n_step=1), device=cuda),
                DQNTrainer(DQNConfig(**kw, n_step=3), device=cuda)]
    for _ in range(6):
        for tr in trainers:
            tr.train_epoch()
    torch.cuda.synchronize()
    d, one, three = trainers
    assert d.metrics()["NStep"] == 1 and d.counters() == one.counters() == three.counters() and d.updates == 12
    for n, x, y in zip(NAMES, d.snapshot_tensors(), one.snapshot_tensors()):
        assert torch.equal(x, y), f"{n}: n_step = 1 is not the default trainer"
    assert not torch.equal(d.q.params, three.q.params)


# ------------------------------------------------------------------ 5. learning
def test_nstep_trainer_learns_cartpole_like_the_cpu_oracle(cuda):
    """The CPU oracle loop with three-step returns (tests/dqn_nstep_oracle.py) at the small shape, 600 epochs =
    1194 updates: see dqn_nstep_oracle.ORACLE_RETURNS_N3 for the greedy mean return over 256 episodes of seeds
    1..5.  The GPU trainer after the same number of updates must reach 80 % of the lowest, the bar of
    test_dqn_gpu.test_trainer_learns_cartpole_like_the_cpu_oracle."""
    tr = DQNTrainer(DQNConfig(**do.SMALL, n_step=3, seed=1), device=cuda)
    for _ in range(do.SMALL_EPOCHS):
        tr.train_epoch()
    assert tr.updates == 1194
    got = tr.evaluate(episodes=1, num_envs=do.EVAL_EPISODES).stats()["mean_return"]
    floor = 0.8 * min(dn.ORACLE_RETURNS_N3.values())
    print(f"GPU greedy mean return {got:.2f}, floor {floor:.2f}, oracle {dn.ORACLE_RETURNS_N3}")
    assert got >= floor, (got, floor)


# ------------------------------------------------------------------ 6. CLI
def test_nstep_preset_trains_evaluates_and_checkpoints(cuda, tmp_path):
    from relayrl_prototype_amd.runtime.launcher import EVAL_COLUMNS, ckpt_dir, run_evaluate, run_preset

    small = {k: v for k, v in TRAINER.items() if k != "max_episode_steps"}
    rows = []
    last = run_preset("cartpole-dqn-nstep", 4, str(tmp_path), overrides=small, eval_every=2, checkpoint_every=4,
                      eval_episodes=1, eval_envs=32, on_metrics=rows.append)
    assert len(rows) == 4 and last["Epoch"] == 4 and last["Updates"] == 8 and last["NStep"] == 3
    assert 0.4 <= last["Beta"] <= 1.0 and last["PriorityMax"] >= 1.0
    for k in EVAL_COLUMNS:
        assert np.isfinite(rows[1][k]) and np.isfinite(last[k]), k
    ck = ckpt_dir(str(tmp_path), "cartpole-dqn-nstep", 0)
    assert os.path.exists(os.path.join(ck, "state.json"))
    out = run_evaluate(ck, episodes=64, num_envs=32)
    assert out["env"] == "CartPole-v1" and out["hidden"] == 64 and out["episodes"] == 64 and out["greedy"]
    assert out["checkpoint_epoch"] == 4 and 8.0 <= out["mean_return"] <= 500.0
