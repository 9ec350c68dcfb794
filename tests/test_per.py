"""Prioritised replay on the CPU: the sum tree's torch build and host oracles (ops/per.py), the
prioritised sampler, the importance-weighted Q_TD reference head, the public plumbing (config, beta
schedule, preset, engine resolution, the CPU form of ``dqn_targets``) and the oracle training loop
whose result is the yardstick of the GPU learning test (tests/test_per_gpu.py)."""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import GradHead, MLPSpec, PriorityTree, ReplayRing, dqn_targets, mlp_grad
from relayrl_prototype_amd.ops import per_insert, per_sample_rows_ref, per_tree_build, per_tree_leaves, per_update
from relayrl_prototype_amd.ops import per_weights_ref
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, beta_at, dqn_seeds

import dqn_oracle as do
import per_oracle as po

C, N = 6, 17  # the ring of the sampling tests: L = 102, P2 = 128


def tree_over(leaves):
    return per_tree_build(torch.as_tensor(np.asarray(leaves, dtype=np.float32)))


def priorities(kind, filled, L=C * N, seed=0):
    rng = np.random.default_rng(seed)
    p = np.zeros(L, np.float32)
    if kind == "flat":
        p[:filled] = 1.0
    elif kind == "skewed":  # eight decades, a few rows carry nearly all the mass
        p[:filled] = np.exp(rng.uniform(-9.0, 9.0, filled)).astype(np.float32)
    else:
        p[:filled] = rng.uniform(0.05, 3.0, filled).astype(np.float32)
    return p


# ------------------------------------------------------------------ the tree
def test_tree_build_is_one_fp32_add_per_node():
    assert [per_tree_leaves(n) for n in (1, 2, 3, 102, 128, 129, 1280)] == [1, 2, 4, 128, 128, 256, 2048]
    with pytest.raises(ValueError):
        per_tree_leaves(0)
    for n in (1, 2, 102, 128, 1280):
        leaves = priorities("random", n, n, seed=n)
        t = tree_over(leaves).numpy()
        P2 = per_tree_leaves(n)
        assert t.shape == (2 * P2,) and t.dtype == np.float32 and t[0] == 0
        np.testing.assert_array_equal(t[P2:P2 + n], leaves)
        assert (t[P2 + n:] == 0).all()
        i = np.arange(1, P2)
        np.testing.assert_array_equal(t[i], t[2 * i] + t[2 * i + 1])  # numpy fp32 adds: the same bits
        assert abs(float(t[1]) - float(leaves.astype(np.float64).sum())) <= 1e-5 * leaves.sum()


def test_insert_and_update_references():
    pt = PriorityTree.allocate(C, N, "cpu")
    assert pt.P2 == 128 and pt.L == 102 and float(pt.pmax) == 1.0 and float(pt.tree.sum()) == 0.0
    pt.pmax.fill_(2.5)
    assert per_insert(pt, C, N, 3, 3) == 0
    want = np.zeros(102, np.float32)
    want[3 * N:] = 2.5
    np.testing.assert_array_equal(pt.leaves.numpy(), want)
    assert torch.equal(pt.tree, tree_over(want))
    before = pt.tree.clone()
    for T, slot0 in ((3, 6), (3, 4), (4, 0), (3, 2)):  # the wrapping ranges dqn_rollout refuses
        assert per_insert(pt, C, N, T, slot0) < 0 and torch.equal(pt.tree, before)
    # update: the maximum over the duplicates, not with the old leaf; a NaN takes pmax; pmax grows
    idx = torch.tensor([60, 61, 60, 62, 63, 60], dtype=torch.int32)
    td = torch.tensor([0.5, 0.0, 2.0, float("nan"), 40.0, 1.0])
    per_update(pt, idx, td, 0.6, 1e-3)
    leaves = pt.leaves.numpy()
    f = lambda x: np.float32(x + 1e-3) ** np.float32(0.6)  # noqa: E731
    np.testing.assert_allclose(leaves[60:64], [f(2.0), f(0.0), 2.5, f(40.0)], rtol=1e-6)
    assert leaves[60] < 2.5  # lowered: no maximum with the old value
    want[60:64] = leaves[60:64]
    np.testing.assert_array_equal(leaves, want)
    assert torch.equal(pt.tree, tree_over(leaves)) and float(pt.pmax) == float(leaves[63]) > 2.5
    assert np.isfinite(pt.tree.numpy()).all()
    with pytest.raises(ValueError):
        per_update(pt, idx, td, -0.1, 1e-3)
    with pytest.raises(ValueError):
        per_update(pt, idx, td, 0.6, 0.0)


# ------------------------------------------------------------------ sampling
@pytest.mark.parametrize("kind", ["flat", "skewed", "random"])
@pytest.mark.parametrize("filled", [1, 51, 102])
def test_samples_land_on_written_rows_of_positive_priority(kind, filled):
    p = priorities(kind, filled, seed=filled)
    t = tree_over(p)
    for B in (1, 63, 65, 1000):
        for u in (None, 0.0, float(po.U_MAX)):  # Philox draws, and every draw forced to an extreme
            for upd in (0, 2 ** 32 + 5):
                rows = per_sample_rows_ref(t, (3 << 32) | 5, upd, B, filled, u=u)
                assert rows.dtype == np.int64 and rows.shape == (B,)
                assert rows.min() >= 0 and rows.max() < filled, (B, u, rows.max())
                assert (p[rows] > 0).all(), (B, u)


def test_sampler_depends_on_seed_update_and_not_on_the_uniform_draws():
    t = tree_over(priorities("random", 102))
    a = per_sample_rows_ref(t, 1234, 7, 64, 102)
    np.testing.assert_array_equal(a, per_sample_rows_ref(t, 1234, 7, 64, 102))
    for other in (per_sample_rows_ref(t, 1234, 8, 64, 102), per_sample_rows_ref(t, 1235, 7, 64, 102),
                  per_sample_rows_ref(t, 1234, 7 + 2 ** 32, 64, 102), per_sample_rows_ref(t, 1234 + 2 ** 32, 7, 64, 102)):
        assert (a != other).mean() > 0.1
    with pytest.raises(ValueError):
        per_sample_rows_ref(t, 1, 0, 4, 0)
    with pytest.raises(ValueError):
        per_sample_rows_ref(t[:-1], 1, 0, 4, 1)


def test_sampled_frequencies_follow_the_priorities():
    """40 updates of B = 1000 over random priorities: the largest |frequency - p_i / sum p| stays below
    1e-3 (stratified sampling: far tighter than 40,000 independent draws would be)."""
    p = priorities("random", 102, seed=3)
    t = tree_over(p)
    cnt = np.zeros(102)
    for upd in range(40):
        cnt += np.bincount(per_sample_rows_ref(t, 77, upd, 1000, 102), minlength=102)
    dev = np.abs(cnt / cnt.sum() - p.astype(np.float64) / p.astype(np.float64).sum()).max()
    print("largest deviation of the sampled frequency:", dev)
    assert dev < 1e-3, dev


# ------------------------------------------------------------------ weighted Q_TD head
def _weighted_huber_autograd(pp, X, act, y, w, wn, A, H, delta):
    p = pp.double().clone().requires_grad_(True)
    q = ref.trunk(p, X.double(), X.shape[1], H, A)[0].gather(-1, act.long().unsqueeze(-1)).squeeze(-1)
    li = torch.nn.functional.huber_loss(q, y.double(), reduction="none", delta=delta) * (w.double() / wn)
    li.mean().backward()
    return p.grad, li.detach(), q.detach()


@pytest.mark.parametrize("D,H,A,B,delta", [(4, 64, 2, 65, 1.0), (8, 128, 4, 33, 0.5), (6, 64, 3, 1, 2.0)])
def test_weighted_q_td_reference_matches_float64_autograd(D, H, A, B, delta):
    torch.manual_seed(B)
    pp = MLPSpec(D, H, A).init(torch.Generator().manual_seed(6))
    X = torch.randn(B, D)
    act = torch.randint(0, A, (B,), dtype=torch.int32)
    q = ref.trunk(pp, X, D, H, A)[0].gather(-1, act.long().unsqueeze(-1)).squeeze(-1)
    y = q + torch.tensor([0.3, -0.3, 1.7, -1.7, 0.0])[torch.arange(B) % 5] * delta
    w = torch.rand(B) * 2.0 + 0.1
    wn = w.max().reshape(1)
    g64, li, q64 = _weighted_huber_autograd(pp, X, act, y, w, float(wn), A, H, delta)
    g, st = ref.mlp_grad_ref(int(GradHead.Q_TD), pp, X, A, H, act=act, ret=y, clip_eps=delta, dtype=torch.float64,
                             row_w=w, w_norm=wn)
    torch.testing.assert_close(g, g64, rtol=1e-12, atol=1e-14)
    assert abs(st["loss"] - li.sum().item()) <= 1e-12 * (1 + li.sum().item()) and st["count"] == B
    torch.testing.assert_close(st["td_abs"], (q64 - y.double()).abs(), rtol=1e-12, atol=1e-14)
    # the fp32 path of the CPU op, with td_abs written in place
    td = torch.full((B,), -1.0)
    g32, ls = mlp_grad(GradHead.Q_TD, pp, X, A, H, act=act, ret=y, clip_eps=delta, row_w=w, w_norm=wn, td_abs=td)
    scale = g64.abs().max().item() + 1e-12
    assert (g32[0].double() - g64).abs().max().item() <= 2e-4 * scale + 1e-6
    assert abs(ls[0, 0].item() - li.sum().item()) <= 1e-3 * (li.sum().item() + 1) and int(ls[0, 5]) == B
    torch.testing.assert_close(td.double(), (q64 - y.double()).abs(), rtol=1e-4, atol=1e-4)
    # all-ones weights with w_norm = 1: bitwise the unweighted head
    for dtype in (torch.float32, torch.float64):
        g0, s0 = ref.mlp_grad_ref(int(GradHead.Q_TD), pp, X, A, H, act=act, ret=y, clip_eps=delta, dtype=dtype)
        g1, s1 = ref.mlp_grad_ref(int(GradHead.Q_TD), pp, X, A, H, act=act, ret=y, clip_eps=delta, dtype=dtype,
                                  row_w=torch.ones(B), w_norm=torch.ones(1))
        assert torch.equal(g0, g1) and s0["loss"] == s1["loss"]
    with pytest.raises(ValueError):
        mlp_grad(GradHead.Q_TD, pp, X, A, H, act=act, ret=y, row_w=w)  # w_norm missing
    with pytest.raises(ValueError):
        mlp_grad(GradHead.PG_CAT, pp, X, A, H, act=act, adv=y, row_w=w, w_norm=wn)


# ------------------------------------------------------------------ plumbing
def test_beta_schedule_and_config_refusals():
    cfg = DQNConfig(per_beta_start=0.4, per_beta_end=1.0, per_beta_epochs=100)
    assert not cfg.prioritized and (cfg.per_alpha, cfg.per_eps) == (0.6, 1e-3)
    assert beta_at(cfg, 0) == 0.4 and beta_at(cfg, 50) == pytest.approx(0.7)
    assert beta_at(cfg, 100) == pytest.approx(1.0) and beta_at(cfg, 10 ** 6) == pytest.approx(1.0)
    assert beta_at(DQNConfig(per_beta_epochs=0), 0) == 1.0
    for bad in (dict(per_alpha=-0.1), dict(per_beta_start=0.0), dict(per_beta_start=1.5), dict(per_beta_end=0.0),
                dict(per_beta_end=1.01), dict(per_eps=0.0), dict(per_eps=-1.0), dict(prioritized="maybe")):
        with pytest.raises(ValueError):
            DQNConfig(**bad)
    assert DQNConfig(prioritized="true").prioritized is True and DQNConfig(prioritized="False").prioritized is False
    assert DQNConfig(per_alpha=0.0, per_beta_start=1.0).per_alpha == 0.0


def test_preset_and_engine_resolution_reach_the_config():
    from relayrl_prototype_amd.runtime import engine as eng
    from relayrl_prototype_amd.runtime.launcher import PRESETS, _filter

    base, per = PRESETS["cartpole-dqn"], PRESETS["cartpole-dqn-per"]
    assert per.kind == "vec" and per.overrides["prioritized"] is True
    assert {k: v for k, v in per.overrides.items() if k in base.overrides} == base.overrides
    extra = set(per.overrides) - set(base.overrides)
    assert extra == {"prioritized", "per_alpha", "per_beta_start", "per_beta_end", "per_beta_epochs", "per_eps"}
    cfg = DQNConfig(**per.overrides)  # every override is a DQNConfig field
    assert cfg.prioritized and cfg == DQNConfig(**dict(base.overrides, prioritized=True))  # the defaults
    # --set prioritized=true on the old preset
    assert DQNConfig(**_filter(DQNConfig, dict(base.overrides, prioritized=True))).prioritized
    spec = eng.resolve_engine("DQN", 4, 2, {}, {}, {"prioritized": "true", "per_alpha": 0.5, "per_beta_epochs": 10},
                              engine="vec")
    assert spec.algo == "dqn" and spec.trainer["prioritized"] == "true"
    cfg = DQNConfig(**eng._filter(DQNConfig, spec.trainer))
    assert cfg.prioritized is True and cfg.per_alpha == 0.5 and cfg.per_beta_epochs == 10
    assert not DQNConfig(**eng._filter(DQNConfig, eng.resolve_engine("DQN", 4, 2, {}, {}, {}, engine="vec").trainer)).prioritized


def test_prioritised_targets_on_the_cpu():
    D, H, A, gamma, beta, B = 4, 64, 2, 0.9, 0.7, 64
    gen = torch.Generator().manual_seed(5)
    ring = ReplayRing(torch.randn(C, N, D, generator=gen), torch.randn(C, N, D, generator=gen),
                      torch.randint(0, A, (C, N), generator=gen, dtype=torch.int32), torch.randn(C, N, generator=gen),
                      torch.randint(0, 3, (C, N), generator=gen).float())
    online = MLPSpec(D, H, A).init(torch.Generator().manual_seed(11))
    target = MLPSpec(D, H, A).init(torch.Generator().manual_seed(12))
    filled = 51
    p = priorities("random", filled, seed=8)
    t = tree_over(p)
    Xb, act_b, y, idx, w, wmax = dqn_targets(online, target, H, A, ring, filled, gamma, True, 3, 9, B, tree=t, beta=beta)
    rows = per_sample_rows_ref(t, 3, 9, B, filled)
    np.testing.assert_array_equal(idx.numpy(), rows)
    assert torch.equal(Xb, ring.obs.reshape(-1, D)[idx]) and torch.equal(act_b, ring.act.reshape(-1)[idx])
    want_w = (filled * p[rows].astype(np.float64) / float(t[1])) ** -beta
    np.testing.assert_allclose(w.numpy(), want_w, rtol=1e-5)
    np.testing.assert_allclose(per_weights_ref(t, rows, filled, beta).numpy(), want_w, rtol=1e-12)
    assert wmax.shape == (1,) and float(wmax) == float(w.max())
    # the targets are the uniform form's at the same rows
    nobs = ring.nobs.reshape(-1, D)[idx]
    qt = ref.trunk(target, nobs, D, H, A)[0]
    astar = ref.greedy_from_logits(ref.trunk(online, nobs, D, H, A)[0])[0]
    boot = (ring.done.reshape(-1)[idx] != 1).float()
    torch.testing.assert_close(y, ring.rew.reshape(-1)[idx] + gamma * boot * qt.gather(-1, astar.unsqueeze(-1)).squeeze(-1))
    # into caller's tensors
    out = (torch.zeros(B, D), torch.zeros(B, dtype=torch.int32), torch.zeros(B), torch.zeros(B, dtype=torch.int32),
           torch.zeros(B), torch.zeros(1))
    dqn_targets(online, target, H, A, ring, filled, gamma, True, 3, 9, B, out=out, tree=t, beta=beta)
    assert torch.equal(out[3].long(), idx) and torch.equal(out[4], w) and torch.equal(out[5], wmax)
    for bad in (None, 0.0, 1.5):
        with pytest.raises(ValueError):
            dqn_targets(online, target, H, A, ring, filled, gamma, True, 3, 9, B, tree=t, beta=bad)
    # without a tree nothing changed: four results
    assert len(dqn_targets(online, target, H, A, ring, filled, gamma, True, 3, 9, B)) == 4


# ------------------------------------------------------------------ oracle training loop
def test_per_oracle_loop_learns_cartpole_at_the_small_shape():
    """The lowest of the five recorded seeds (per_oracle.ORACLE_RETURNS) must be reproduced to within 20 %
    (BLAS builds may order float64 sums differently) and beat three times a random policy's 22 steps; and
    the oracle's tree keeps the invariant of the device tree all the way."""
    assert sorted(po.ORACLE_RETURNS) == [1, 2, 3, 4, 5] and min(po.ORACLE_RETURNS.values()) >= 66.0
    seed = min(po.ORACLE_RETURNS, key=po.ORACLE_RETURNS.get)
    cfg = DQNConfig(**po.SMALL_PER, seed=seed)
    params, updates, pt = po.oracle_dqn_per(cfg, do.SMALL_EPOCHS)
    assert updates == 1194
    r = do.greedy_return(params, cfg.hidden, dqn_seeds(seed)[2])
    print(f"PER oracle greedy return, seed {seed}:", r)
    assert r >= 66.0 and r >= 0.8 * po.ORACLE_RETURNS[seed]
    assert torch.equal(pt.tree, per_tree_build(pt.leaves)) and bool((pt.leaves > 0).all())
    assert float(pt.pmax) >= float(pt.leaves.max()) and np.isfinite(pt.tree.numpy()).all()
