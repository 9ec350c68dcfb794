"""Prioritised replay on the GPU: the priority sum tree kernels (csrc/kernels/per.hip), the prioritised
instance of the targets kernel (dqn.hip), the importance-weighted Q_TD head (mlp_grad.hip) and the
prioritised DQNTrainer, against the host oracles (ops/per.py, ops/reference.py, tests/per_oracle.py).
Every output buffer of a kernel under test is guarded."""
import os

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import GradHead, MLPSpec, PriorityTree, dqn_targets, hip, mlp_grad, reduce_slabs
from relayrl_prototype_amd.ops import per_insert, per_sample_rows_ref, per_tree_build, per_tree_leaves, per_update
from relayrl_prototype_amd.ops import per_weights_ref
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer

import dqn_oracle as do
import per_oracle as po
from guarded import INT_SENTINEL, Guarded
from test_dqn_gpu import FWD_TOL, TGT_C, TGT_N, TGT_T, TRAINER, _bits, _q_td_case, cu_limit, random_ring

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def guarded_tree(leaves, pmax):
    """A host-built tree over ``leaves`` and a pmax, both in guarded device buffers."""
    L = len(leaves)
    gt, gp = Guarded((2 * per_tree_leaves(L),)), Guarded((1,), fill=np.float32(pmax))
    gt.t.copy_(per_tree_build(torch.as_tensor(np.asarray(leaves, np.float32))))
    return gt, gp, PriorityTree(gt.t, gp.t, L)


def random_leaves(L, filled, seed):
    p = np.zeros(L, np.float32)
    p[:filled] = np.random.default_rng(seed).uniform(0.05, 3.0, filled).astype(np.float32)
    return p


# ------------------------------------------------------------------ 1. insert
@pytest.mark.parametrize("C,N,T", [(6, 17, 3), (8, 16, 4), (8, 320, 4)])
def test_insert_sets_the_range_and_keeps_the_invariant(cuda, C, N, T):
    """L = 102 (P2 = 128), L = P2 = 128, and 1,280 inserted leaves (more than the workgroup has
    threads, P2 = 4096): first, middle and last slot0, with a pmax that is not the default."""
    L = C * N
    for slot0 in sorted({0, (C // T // 2) * T, C - T}):
        leaves = random_leaves(L, L, 10 * C + slot0)
        leaves[::5] = 0.0  # rows never written
        pmax = np.float32(2.75) + np.float32(slot0) * np.float32(0.1)
        gt, gp, pt = guarded_tree(leaves, pmax)
        assert per_insert(pt, C, N, T, slot0) == 0
        torch.cuda.synchronize()
        assert gt.guards_intact() and gp.guards_intact()
        got = pt.leaves.cpu().numpy()
        lo, hi = slot0 * N, (slot0 + T) * N
        assert (_bits(got[lo:hi]) == _bits(np.array([pmax]))).all()
        assert np.array_equal(_bits(got[:lo]), _bits(leaves[:lo])) and np.array_equal(_bits(got[hi:]), _bits(leaves[hi:]))
        assert torch.equal(gt.t.cpu().view(torch.int32), per_tree_build(torch.from_numpy(got)).view(torch.int32))
        assert _bits(gp.t.cpu().numpy())[0] == _bits(np.array([pmax]))[0]


@pytest.mark.parametrize("T,slot0", [(3, 6), (3, 4), (4, 0), (3, 2)])
def test_insert_refuses_a_range_that_would_wrap(cuda, T, slot0):
    C, N = 6, 17
    gt, gp = Guarded((2 * 128,)), Guarded((1,), fill=np.float32(1.5))
    assert per_insert(PriorityTree(gt.t, gp.t, C * N), C, N, T, slot0) < 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(gt.big).all()), "a refused insert wrote to the tree"
    with pytest.raises(ValueError):
        per_insert(PriorityTree(gt.t, gp.t, C * N), C, N + 1, 3, 0)  # the tree covers another ring


# ------------------------------------------------------------------ 2. sample + targets
W_ERR = [0.0]  # the largest fp32-vs-float64 relative error of w seen by the cases below


@pytest.mark.parametrize("double_q", [False, True])
@pytest.mark.parametrize("H,A", [(H, A) for H in (64, 128) for A in (2, 3, 4)])
def test_prioritised_targets_sample_gather_weigh(cuda, H, A, double_q):
    D = 2 * A
    L = TGT_C * TGT_N
    host, g, ring = random_ring(D, A, 100 * H + A)
    online = MLPSpec(D, H, A).init(torch.Generator().manual_seed(11))
    target = MLPSpec(D, H, A).init(torch.Generator().manual_seed(12))
    seed, gamma, beta = (3 << 32) | 5, 0.97, 0.7

    def launch(tree, filled, upd, B):
        out = (Guarded((B, D)), Guarded((B,), torch.int32), Guarded((B,)), Guarded((B,), torch.int32), Guarded((B,)),
               Guarded((1,)))
        dqn_targets(online.to(DEV), target.to(DEV), H, A, ring, filled, gamma, double_q, seed, upd, B, tree=tree,
                    beta=beta, out=tuple(o.t for o in out))
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in out) and all(b.guards_intact() for b in g.values())
        return out

    for B in (1, 63, 65, 1000):
        for filled in (1, TGT_N * TGT_T, L):
            upd = 2 ** 32 - 1 + B  # the update counter's high word matters
            leaves = random_leaves(L, filled, filled + B)
            gt, _, pt = guarded_tree(leaves, 1.0)
            tree_before = gt.big.clone()
            out = launch(pt.tree, filled, upd, B)
            assert torch.equal(gt.big.view(torch.int32), tree_before.view(torch.int32)), "the sampler wrote to the tree"
            Xb, act_b, y, idx, w, wmax = (o.t.cpu() for o in out)
            want = per_sample_rows_ref(pt.tree, seed, upd, B, filled)
            np.testing.assert_array_equal(idx.numpy(), want)
            assert want.max() < filled and (leaves[want] > 0).all()
            rows = torch.from_numpy(want)
            assert torch.equal(Xb.view(torch.int32), host.obs.reshape(-1, D)[rows].view(torch.int32))
            assert torch.equal(act_b, host.act.reshape(-1)[rows])
            # y against the float64 oracle; any action within tol of the selecting net's maximum may be a*
            nobs = host.nobs.reshape(-1, D)[rows].double()
            qt = ref.trunk(target.double(), nobs, D, H, A)[0]
            sel = ref.trunk(online.double(), nobs, D, H, A)[0] if double_q else qt
            top = sel.max(-1, keepdim=True).values
            cand = sel >= top - (FWD_TOL["atol"] + FWD_TOL["rtol"] * top.abs())
            boot = (host.done.reshape(-1)[rows] != 1).double()
            ys = host.rew.reshape(-1)[rows].double().unsqueeze(-1) + gamma * boot.unsqueeze(-1) * qt
            ok = ((y.double().unsqueeze(-1) - ys).abs() <= FWD_TOL["atol"] + FWD_TOL["rtol"] * ys.abs()) & cand
            assert bool(ok.any(-1).all()), (B, filled, int((~ok.any(-1)).sum()))
            # the importance weights against float64, and their maximum bit for bit
            w64 = per_weights_ref(pt.tree, want, filled, beta)
            torch.testing.assert_close(w.double(), w64, **FWD_TOL)
            W_ERR[0] = max(W_ERR[0], float(((w.double() - w64).abs() / w64).max()))
            assert _bits(wmax.numpy())[0] == _bits(w.numpy()).max() and float(wmax) == float(w.max())
            again = [launch(pt.tree, filled, upd, B)]  # a second launch: the same bits
            if B == 1000:  # two workgroups stride over the 16 slabs: the same bits
                with cu_limit(2):
                    again.append(launch(pt.tree, filled, upd, B))
            for other in again:
                for a, b in zip(out, other):
                    assert np.array_equal(_bits(a.t.cpu().numpy()), _bits(b.t.cpu().numpy()))
    print(f"largest relative error of w so far: {W_ERR[0]:.3e}")


def test_prioritised_targets_refuse_bad_arguments(cuda):
    D, H, A, B = 4, 64, 2, 8
    L = TGT_C * TGT_N
    _, _, ring = random_ring(D, A, 1)
    p = MLPSpec(D, H, A).init(torch.Generator().manual_seed(1)).to(DEV)
    _, _, pt = guarded_tree(random_leaves(L, L, 1), 1.0)

    def outs(idx=True):
        return (torch.empty(B, D, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(B, device=DEV),
                torch.empty(B, dtype=torch.int32, device=DEV) if idx else None, torch.empty(B, device=DEV),
                torch.empty(1, device=DEV))

    dqn_targets(p, p, H, A, ring, L, 0.9, True, 1, 0, B, tree=pt.tree, beta=0.5, out=outs())  # the sound call
    for filled, hid, tree in ((0, H, pt.tree), (L + 1, H, pt.tree), (1, 96, pt.tree), (1, H, pt.tree[:-2]),
                              (1, H, torch.zeros(512, device=DEV)), (1, H, pt.tree.double())):
        with pytest.raises(RuntimeError):
            dqn_targets(p, p, hid, A, ring, filled, 0.9, True, 1, 0, B, tree=tree, beta=0.5, out=outs())
    with pytest.raises(ValueError):
        dqn_targets(p, p, H, A, ring, 1, 0.9, True, 1, 0, B, tree=pt.tree, beta=0.5, out=outs(idx=False))
    with pytest.raises(ValueError):
        dqn_targets(p, p, H, A, ring, 1, 0.9, True, 1, 0, B, tree=pt.tree, beta=0.0, out=outs())
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. update
@pytest.mark.parametrize("L", [102, 2560])
def test_update_takes_the_maximum_over_duplicates(cuda, L):
    """B = 1000 batch rows over L ring rows (102: every touched row many times; 2560: P2 = 4096), |td| of 0,
    large values, an infinity and a NaN."""
    B, alpha, eps, pmax0 = 1000, 0.6, 1e-3, np.float32(2.25)
    rng = np.random.default_rng(L)
    touchable = np.flatnonzero(np.arange(L) % 7 != 3)  # rows 3, 10, 17, ... stay untouched
    idx = rng.choice(touchable, B).astype(np.int32)
    td = np.abs(rng.standard_normal(B)).astype(np.float32) * np.float32(2.0)
    td[:6] = [0.0, 1e3, 3e7, 0.0, np.inf, 1e-8]
    td[500] = np.nan
    idx[7] = idx[500]  # the NaN row shares its leaf with a finite one
    leaves0 = random_leaves(L, L, 5)
    v64 = (td.astype(np.float64) + eps) ** alpha
    v64[~np.isfinite(td)] = float(pmax0)
    want = {}
    for r, v in zip(idx, v64):
        want[int(r)] = max(want.get(int(r), 0.0), v)
    touched = np.array(sorted(want))
    assert len(touched) < len(touchable) or L == 102
    runs = []
    for _ in range(2):
        gt, gp, pt = guarded_tree(leaves0, pmax0)
        per_update(pt, torch.from_numpy(idx).to(DEV), torch.from_numpy(td).to(DEV), alpha, eps)
        torch.cuda.synchronize()
        assert gt.guards_intact() and gp.guards_intact()
        runs.append((gt.t.cpu(), gp.t.cpu()))
    tree, pmax = runs[0]
    assert torch.equal(tree.view(torch.int32), runs[1][0].view(torch.int32)), "two runs differ"
    assert torch.equal(pmax.view(torch.int32), runs[1][1].view(torch.int32))
    P2 = per_tree_leaves(L)
    got = tree.numpy()[P2:P2 + L]
    exp = np.array([want[int(r)] for r in touched])
    np.testing.assert_allclose(got[touched].astype(np.float64), exp, **FWD_TOL)
    err = float((np.abs(got[touched] - exp) / exp).max())
    print(f"largest relative error of the new leaves, L = {L}: {err:.3e}")
    assert _bits(got[idx[500]])[()] >= _bits(np.array(pmax0))[()]  # the NaN row took pmax (or its finite twin's more)
    assert got[idx[4]] >= pmax0 and np.isfinite(tree.numpy()).all()  # so did the infinity; nothing non-finite got in
    rest = np.setdiff1d(np.arange(L), touched)
    assert len(rest) > 0 and np.array_equal(_bits(got[rest]), _bits(leaves0[rest])), "an untouched leaf changed"
    assert (tree.numpy()[P2 + L:] == 0).all()
    assert torch.equal(tree.view(torch.int32), per_tree_build(torch.from_numpy(got.copy())).view(torch.int32))
    assert _bits(pmax.numpy())[0] == _bits(np.array([max(pmax0, got[touched].max())], np.float32))[0]
    with pytest.raises(RuntimeError):
        per_update(pt, torch.from_numpy(idx).to(DEV), torch.from_numpy(td[:10]).to(DEV), alpha, eps)  # td_abs too short


# ------------------------------------------------------------------ 4. the weighted Q_TD head
@pytest.mark.parametrize("H,A", [(H, A) for H in (64, 128) for A in (2, 3, 4)])
def test_weighted_q_td_head_matches_float64_autograd(cuda, H, A):
    """The shapes and tolerances of test_dqn_gpu.test_q_td_head_matches_float64_autograd, with random
    positive weights normalised by their maximum."""
    delta = 0.75
    for D in (2, 4, 6, 8):
        for B in (1, 64, 65, 4100):
            pp, X, act, y = _q_td_case(D, H, A, B, delta, 1000 * D + B)
            w = torch.rand(B, generator=torch.Generator().manual_seed(B + D)) * 3.0 + 0.05
            wn = w.max().reshape(1)
            args = (GradHead.Q_TD, pp.to(DEV), X.to(DEV), A, H)
            kw = dict(act=act.to(DEV), ret=y.to(DEV), clip_eps=delta)
            ns = int(hip().mlp_grad_slabs(B))
            gs, gl, gtd = Guarded((ns, pp.numel())), Guarded((ns, 8), fill=float(INT_SENTINEL)), Guarded((B,))
            slab, loss = mlp_grad(*args, **kw, grad_slab=gs.t, loss_slab=gl.t, row_w=w.to(DEV), w_norm=wn.to(DEV),
                                  td_abs=gtd.t)
            torch.cuda.synchronize()
            assert gs.guards_intact() and gl.guards_intact() and gtd.guards_intact()
            assert bool((gl.t[:, 6:] == INT_SENTINEL).all())
            g64, st = ref.mlp_grad_ref(int(GradHead.Q_TD), pp, X, A, H, act=act, ret=y, inv_B=1.0 / B, clip_eps=delta,
                                       dtype=torch.float64, row_w=w, w_norm=wn)
            g = reduce_slabs(slab).cpu().double()
            scale = g64.abs().max().item() + 1e-12
            err = (g - g64).abs().max().item()
            assert err <= 2e-4 * scale + 1e-6, (err, scale)  # test_kernels_gpu.test_grad_matches_autograd
            ls = loss.sum(0).cpu()
            assert abs(ls[0].item() - st["loss"]) <= 1e-3 * (abs(st["loss"]) + 1)
            assert abs(ls[4].item() - st["v"]) <= 1e-3 * (abs(st["v"]) + 1)
            assert int(ls[5].item()) == B and (ls[1:4] == 0).all()
            torch.testing.assert_close(gtd.t.cpu().double(), st["td_abs"], **FWD_TOL)
            # weights == 1 with w_norm = 1: bitwise the unweighted slabs
            ones, one = torch.ones(B, device=DEV), torch.ones(1, device=DEV)
            s1, l1 = mlp_grad(*args, **kw, row_w=ones, w_norm=one)
            s0, l0 = mlp_grad(*args, **kw)
            assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)), "unit weights changed the gradient"
            assert torch.equal(l0[:, :6].view(torch.int32), l1[:, :6].view(torch.int32))


def test_weighted_head_leaves_rows_past_nvalid_alone(cuda):
    D, H, A, B, nv, delta = 4, 128, 2, 4100, 3001, 1.0
    pp, X, act, y = _q_td_case(D, H, A, B, delta, 5)
    w = torch.rand(B, generator=torch.Generator().manual_seed(2)) + 0.5
    Xp, actp, yp, wp = X.clone(), act.clone(), y.clone(), w.clone()
    Xp[nv:], yp[nv:], actp[nv:], wp[nv:] = float("nan"), float("nan"), 99, float("nan")
    nvalid = torch.tensor([nv], dtype=torch.int32, device=DEV)
    wn = w[:nv].max().reshape(1)
    gtd = Guarded((B,))  # the payload starts as NaN sentinels
    slab, loss = mlp_grad(GradHead.Q_TD, pp.to(DEV), Xp.to(DEV), A, H, act=actp.to(DEV), ret=yp.to(DEV), clip_eps=delta,
                          nvalid=nvalid, inv_B_dev=torch.tensor([1.0 / nv], device=DEV), row_w=wp.to(DEV),
                          w_norm=wn.to(DEV), td_abs=gtd.t)
    torch.cuda.synchronize()
    td = gtd.t.cpu()
    assert gtd.guards_intact() and bool(torch.isnan(td[nv:]).all()), "a row past nvalid wrote td_abs"
    g64, st = ref.mlp_grad_ref(int(GradHead.Q_TD), pp, X[:nv], A, H, act=act[:nv], ret=y[:nv], inv_B=1.0 / nv,
                               clip_eps=delta, dtype=torch.float64, row_w=w[:nv], w_norm=wn)
    torch.testing.assert_close(td[:nv].double(), st["td_abs"], **FWD_TOL)
    g = reduce_slabs(slab).cpu().double()
    assert bool(torch.isfinite(slab).all())
    assert (g - g64).abs().max().item() <= 2e-4 * (g64.abs().max().item() + 1e-12) + 1e-6


# ------------------------------------------------------------------ 5. trainer
PER_TRAINER = dict(TRAINER, prioritized=True, per_beta_epochs=4)
NAMES = ["online", "m", "v", "step", "target", "obs", "nobs", "act", "rew", "done", "state", "ep_len", "ep_ret", "tree",
         "pmax"]


def _state(tr):
    return [t.clone() for t in tr.snapshot_tensors()], dict(tr.counters())


def _tree_is_sound(tr):
    return torch.equal(tr.per.tree.view(torch.int32), per_tree_build(tr.per.leaves).view(torch.int32))


def test_prioritised_trainer_resume_is_bitwise(cuda):
    a = DQNTrainer(DQNConfig(**PER_TRAINER), device=cuda)
    assert len(a.snapshot_tensors()) == len(NAMES) and float(a.per.pmax) == 1.0 and _tree_is_sound(a)
    for k in range(6):
        a.train_epoch()
        assert _tree_is_sound(a), f"the tree lost its invariant in epoch {k}"
    b = DQNTrainer(DQNConfig(**PER_TRAINER), device=cuda)
    for _ in range(3):
        b.train_epoch()
    before, counters = _state(b)
    assert b.evaluate(episodes=2, num_envs=33).stats()["episodes"] == 66
    after, counters2 = _state(b)
    assert counters == counters2 and all(torch.equal(x, y) for x, y in zip(before, after)), "evaluate() changed state"
    sd = b.state_dict()
    assert set(sd["per"]) == {"leaves", "pmax"} and sd["per"]["leaves"].shape == (8 * 64,)
    c = DQNTrainer(DQNConfig(**PER_TRAINER), device=cuda)
    c.q.params.add_(1.0)  # other weights and another tree until the load
    c.per.tree.fill_(3.0)
    c.per.pmax.fill_(9.0)
    c.load_state_dict(sd)
    assert torch.equal(c.per.tree.view(torch.int32), b.per.tree.view(torch.int32)) and torch.equal(c.per.pmax, b.per.pmax)
    for _ in range(3):
        c.train_epoch()
    torch.cuda.synchronize()
    assert a.counters() == c.counters() and a.updates == 12 and a.cursor == 0 and a.slots_written == 24
    for n, x, y in zip(NAMES, a.snapshot_tensors(), c.snapshot_tensors()):
        assert torch.equal(x, y), f"{n} differs after the resume"
    # the priorities moved: every row was inserted, the sampled ones re-weighed, pmax grew or stayed
    leaves = a.per.leaves
    assert bool((leaves > 0).all()) and leaves.unique().numel() > 2 and float(a.per.pmax) >= float(leaves.max())
    m = a.metrics()
    assert m["Beta"] == pytest.approx(1.0) and m["PriorityMax"] == float(a.per.pmax) and np.isfinite(m["LossQ"])
    # a uniform trainer refuses nothing it accepted before, and cannot take priorities it has no tree for
    u = DQNTrainer(DQNConfig(**TRAINER), device=cuda)
    assert "Beta" not in u.metrics() and "per" not in u.state_dict() and len(u.snapshot_tensors()) == 13
    with pytest.raises(ValueError):
        c.load_state_dict(u.state_dict())


def test_default_config_is_the_uniform_trainer_bit_for_bit(cuda):
    a = DQNTrainer(DQNConfig(**TRAINER), device=cuda)
    b = DQNTrainer(DQNConfig(**TRAINER, prioritized=False), device=cuda)
    for _ in range(4):
        a.train_epoch()
        b.train_epoch()
    torch.cuda.synchronize()
    assert a.per is None and b.per is None and a.counters() == b.counters() and a.updates == 8
    for n, x, y in zip(NAMES, a.snapshot_tensors(), b.snapshot_tensors()):
        assert torch.equal(x, y), n
    sd = a.state_dict()
    c = DQNTrainer(DQNConfig(**TRAINER), device=cuda)
    c.load_state_dict(sd)  # a uniform checkpoint loads into a uniform trainer
    assert torch.equal(c.q.params, a.q.params)


# ------------------------------------------------------------------ 6. learning
def test_prioritised_trainer_learns_cartpole_like_the_cpu_oracle(cuda):
    """The CPU oracle loop with prioritised replay (tests/per_oracle.py: the same algorithm, Philox draws
    and fp32 tree, float64 networks) at the small shape, 600 epochs = 1194 updates: see
    per_oracle.ORACLE_RETURNS for the greedy mean return over 256 episodes of seeds 1..5 (a random
    policy: about 22).  The GPU trainer after the same number of updates must reach 80 % of the lowest."""
    tr = DQNTrainer(DQNConfig(**po.SMALL_PER, seed=1), device=cuda)
    for _ in range(do.SMALL_EPOCHS):
        tr.train_epoch()
    assert tr.updates == 1194 and _tree_is_sound(tr)
    got = tr.evaluate(episodes=1, num_envs=do.EVAL_EPISODES).stats()["mean_return"]
    floor = 0.8 * min(po.ORACLE_RETURNS.values())
    print(f"GPU greedy mean return {got:.2f}, floor {floor:.2f}, oracle {po.ORACLE_RETURNS}")
    assert got >= floor, (got, floor)


# ------------------------------------------------------------------ 7. CLI
def test_per_preset_trains_evaluates_and_checkpoints(cuda, tmp_path):
    from relayrl_prototype_amd.runtime.launcher import EVAL_COLUMNS, ckpt_dir, run_evaluate, run_preset

    small = {k: v for k, v in TRAINER.items() if k != "max_episode_steps"}
    rows = []
    last = run_preset("cartpole-dqn-per", 4, str(tmp_path), overrides=small, eval_every=2, checkpoint_every=4,
                      eval_episodes=1, eval_envs=32, on_metrics=rows.append)
    assert len(rows) == 4 and last["Epoch"] == 4 and last["Updates"] == 8
    assert 0.4 <= last["Beta"] <= 1.0 and last["PriorityMax"] >= 1.0
    for k in EVAL_COLUMNS:
        assert np.isfinite(rows[1][k]) and np.isfinite(last[k]), k
    ck = ckpt_dir(str(tmp_path), "cartpole-dqn-per", 0)
    assert os.path.exists(os.path.join(ck, "state.json"))
    out = run_evaluate(ck, episodes=64, num_envs=32)
    assert out["env"] == "CartPole-v1" and out["hidden"] == 64 and out["episodes"] == 64 and out["greedy"]
    assert out["checkpoint_epoch"] == 4 and 8.0 <= out["mean_return"] <= 500.0
