"""The dueling head on the CPU, in float64: the combine of ops/reference.py against a closed form and against
the folded plain net (tests/dqn_dueling_oracle.py: an oracle that shares no code with it), the HEAD_Q_DUEL
gradient against autograd, the dueling TD targets against the plain targets of the folded nets, and the
DQNConfig field, the preset, the checkpoint key and the engine resolution."""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import GradHead, MLPSpec, ReplayRing, dqn_targets, dqn_targets_ref
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.ops.per import per_tree_build
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig

import dqn_dueling_oracle as dd

F64 = torch.float64
ACTIONS = (1, 2, 4, 15)


# ------------------------------------------------------------------ 1. the combine
def test_dueling_q_closed_form():
    out = torch.tensor([[1.0, 2.0, 6.0, 10.0], [-3.0, 0.0, 3.0, -1.0]], dtype=F64)  # adv x 3, then V
    want = torch.tensor([[10 - 3 + 1, 10 - 3 + 2, 10 - 3 + 6], [-1 - 0 - 3, -1 - 0 + 0, -1 - 0 + 3]], dtype=F64)
    assert torch.equal(ref.dueling_q(out, 3), want)
    gen = torch.Generator().manual_seed(1)
    for A in ACTIONS:
        o = torch.randn(5, 7, A + 1, generator=gen, dtype=F64)
        q = ref.dueling_q(o, A)
        assert q.shape == (5, 7, A) and q.dtype == F64
        assert float((q.mean(-1) - o[..., A]).abs().max()) <= 1e-14  # mean_a Q == V
        assert torch.equal(q.argmax(-1), o[..., :A].argmax(-1))
        if A == 1:
            # Q == V: (V - adv) + adv rounds twice, each within half an ulp of max(|V|, |V - adv|)
            bound = 2.3e-16 * (o[..., 1].abs() + (o[..., 1] - o[..., 0]).abs())
            assert bool(((q[..., 0] - o[..., 1]).abs() <= bound).all())
    assert ref.dueling_q(torch.randn(3, 4), 3).dtype == torch.float32
    with pytest.raises(ValueError, match="outputs"):
        ref.dueling_q(torch.zeros(2, 3), 3)


# ------------------------------------------------------------------ 2. fold equivalence
@pytest.mark.parametrize("A", ACTIONS)
def test_dueling_net_equals_its_folded_plain_net(A):
    D, H = min(2 * A, 16), 64
    gen = torch.Generator().manual_seed(10 + A)
    p = MLPSpec(D, H, A + 1).init(gen).double()
    X = torch.randn(257, D, generator=gen, dtype=F64)
    folded = dd.fold(p, D, H, A)
    assert folded.numel() == MLPSpec(D, H, A).P
    plain = ref.trunk(folded, X, D, H, A)[0]
    duel = ref.dueling_q(ref.trunk(p, X, D, H, A + 1)[0], A)
    err = float((plain - duel).abs().max())
    print(f"A = {A}: fold vs combine {err:.2e}")
    assert err <= 1e-12


# ------------------------------------------------------------------ 3. HEAD_Q_DUEL against autograd
def _huber(diff, delta):
    ad = diff.abs()
    return torch.where(ad <= delta, 0.5 * diff * diff, delta * (ad - 0.5 * delta))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("A", ACTIONS)
def test_q_duel_reference_gradient_matches_autograd(A, weighted):
    D, H, B, delta, inv_B = min(2 * A, 16), 64, 37, 0.75, 1.0 / 41
    gen = torch.Generator().manual_seed(20 + A)
    spec = MLPSpec(D, H, A + 1)
    p = spec.init(gen).double()
    X = torch.randn(B, D, generator=gen, dtype=F64)
    act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
    q0 = ref.dueling_q(ref.trunk(p, X, D, H, A + 1)[0], A).gather(-1, act.long().unsqueeze(-1)).squeeze(-1)
    y = q0 + torch.tensor([0.3, -0.3, 1.7, -1.7, 0.0], dtype=F64)[torch.arange(B) % 5] * delta
    kw = {}
    w = torch.ones(B, dtype=F64)
    if weighted:
        row_w = torch.rand(B, generator=gen, dtype=F64) + 0.1
        w_norm = row_w.max().reshape(1)
        kw = dict(row_w=row_w, w_norm=w_norm)
        w = row_w / w_norm
    g, st = ref.mlp_grad_ref(ref.HEAD_Q_DUEL, p, X, A, H, act=act, ret=y, inv_B=inv_B, clip_eps=delta, dtype=F64, **kw)
    # the explicit loss, written out on the unflattened net without the combine's helper
    pa = p.clone().requires_grad_(True)
    W1, b1, W2, b2, W3, b3, _ = ref.unflatten(pa, D, H, A + 1)
    h2 = torch.relu(torch.relu(X @ W1.t() + b1) @ W2.t() + b2)
    out = h2 @ W3.t() + b3
    adv, val = out[:, :A], out[:, A]
    q = val + adv.gather(-1, act.long().unsqueeze(-1)).squeeze(-1) - adv.mean(-1)
    li = w * _huber(q - y, delta)
    (li.sum() * inv_B).backward()
    err = float((g - pa.grad).abs().max())
    print(f"A = {A}, weighted = {weighted}: reference vs autograd {err:.2e}")
    assert err <= 1e-12
    li, q = li.detach(), q.detach()
    assert abs(st["loss"] - float(li.sum())) <= 1e-12 * (1 + abs(float(li.sum())))
    assert abs(st["v"] - float(q.sum())) <= 1e-12 * (1 + abs(float(q.sum()))) and st["count"] == B
    assert float((st["td_abs"] - (q - y).abs()).abs().max()) <= 1e-12
    # the two invariants of the head
    o = spec.offsets()
    db3 = g[o["b3"]:o["b3"] + A + 1]
    dq = w * (q - y).clamp(-delta, delta) * inv_B
    assert abs(float(db3[:A].sum())) <= 1e-12, "the advantage rows' bias gradient sums to 0"
    assert abs(float(db3[A] - dq.sum())) <= 1e-12, "the value row's bias gradient is sum(dq)"


def test_q_duel_through_the_cpu_op():
    """ops.mlp_grad on CPU tensors is the reference, td_abs included; the weights are the Q heads' alone."""
    from relayrl_prototype_amd.ops import mlp_grad

    D, H, A, B = 4, 64, 2, 9
    gen = torch.Generator().manual_seed(3)
    p = MLPSpec(D, H, A + 1).init(gen)
    X, act, y = torch.randn(B, D, generator=gen), torch.randint(0, A, (B,), generator=gen, dtype=torch.int32), torch.randn(B, generator=gen)
    row_w, td = torch.rand(B, generator=gen) + 0.5, torch.zeros(B)
    g, ls = mlp_grad(GradHead.Q_DUEL, p, X, A, H, act=act, ret=y, clip_eps=1.0, row_w=row_w, w_norm=row_w.max().reshape(1),
                     td_abs=td)
    want, st = ref.mlp_grad_ref(ref.HEAD_Q_DUEL, p, X, A, H, act=act, ret=y, clip_eps=1.0, row_w=row_w,
                                w_norm=row_w.max().reshape(1))
    assert g.shape == (1, MLPSpec(D, H, A + 1).P) and torch.equal(g[0], want) and torch.equal(td, st["td_abs"])
    assert int(GradHead.Q_DUEL) == ref.HEAD_Q_DUEL == 6
    with pytest.raises(ValueError, match="15"):
        mlp_grad(GradHead.Q_DUEL, p, X, 16, H, act=act, ret=y)
    with pytest.raises(ValueError, match="Q_DUEL"):
        mlp_grad(GradHead.PG_CAT, p, X, A, H, act=act, adv=y, td_abs=td)


# ------------------------------------------------------------------ 4. targets against the folded nets
TC, TN, TA, TD_, TH = 6, 5, 3, 4, 64


def _ring_and_nets(seed):
    gen = torch.Generator().manual_seed(seed)
    ring = ReplayRing(torch.randn(TC, TN, TD_, generator=gen), torch.randn(TC, TN, TD_, generator=gen),
                      torch.randint(0, TA, (TC, TN), generator=gen, dtype=torch.int32), torch.randn(TC, TN, generator=gen),
                      torch.randint(0, 3, (TC, TN), generator=gen).float())
    ring.done[0, 0] = 1.0
    assert set(ring.done.unique().tolist()) == {0.0, 1.0, 2.0}
    online = MLPSpec(TD_, TH, TA + 1).init(gen).double()
    target = MLPSpec(TD_, TH, TA + 1).init(gen).double()
    return ring, online, target


@pytest.mark.parametrize("double_q", [False, True])
@pytest.mark.parametrize("form", ["uniform", "tree", "nstep"])
def test_dueling_targets_equal_the_plain_targets_of_the_folded_nets(form, double_q):
    ring, online, target = _ring_and_nets(31)
    # a* cannot flip between the two computations: every row's top-two advantage gap is far above rounding
    nobs = ring.nobs.reshape(-1, TD_).double()
    for net in (online, target):
        gap = ref.greedy_from_logits(ref.trunk(net, nobs, TD_, TH, TA + 1)[0][:, :TA])[1]
        assert float(gap.min()) > 1e-6, float(gap.min())
    fo, ft = dd.fold(online, TD_, TH, TA), dd.fold(target, TD_, TH, TA)
    B, filled = 64, TC * TN
    kw = {}
    if form == "tree":
        leaves = torch.rand(filled, generator=torch.Generator().manual_seed(5)) + 0.05
        kw = dict(tree=per_tree_build(leaves), beta=0.6)
    if form == "nstep":
        kw = dict(n_step=3, newest=2)
    a = dqn_targets_ref(online, target, TH, TA, ring, filled, 0.9, double_q, 7, 3, B, F64, dueling=True, **kw)
    b = dqn_targets_ref(fo, ft, TH, TA, ring, filled, 0.9, double_q, 7, 3, B, F64, **kw)
    assert len(a) == len(b) == {"uniform": 4, "tree": 6, "nstep": 5}[form]
    for i, (x, y) in enumerate(zip(a, b)):
        if i == 2:
            err = float((x - y).abs().max())
            print(f"{form}, double_q = {double_q}: y vs the folded nets {err:.2e}")
            assert x.dtype == F64 and err <= 1e-12
        else:
            assert torch.equal(x, y), i
    # the selection is on the advantages and it matters: single Q and double Q disagree somewhere
    other = dqn_targets_ref(online, target, TH, TA, ring, filled, 0.9, not double_q, 7, 3, B, F64, dueling=True, **kw)
    assert not torch.equal(other[2], a[2])
    # the CPU op is the reference
    got = dqn_targets(online, target, TH, TA, ring, filled, 0.9, double_q, 7, 3, B, dtype=F64, dueling=True, **kw)
    assert all(torch.equal(x, y) for x, y in zip(got, a))


def test_dueling_targets_check_the_parameter_count():
    ring, online, target = _ring_and_nets(32)
    plain = MLPSpec(TD_, TH, TA).init(torch.Generator().manual_seed(1)).double()
    want_d, want_p = MLPSpec(TD_, TH, TA + 1).P, MLPSpec(TD_, TH, TA).P
    for fn in (dqn_targets_ref, dqn_targets):
        with pytest.raises(ValueError, match=f"{want_p} floats.*{want_d}"):
            fn(plain, plain, TH, TA, ring, 8, 0.9, True, 1, 0, 4, dueling=True)
        with pytest.raises(ValueError, match=f"{want_d} floats.*{want_p}"):
            fn(online, target, TH, TA, ring, 8, 0.9, True, 1, 0, 4)
        with pytest.raises(ValueError, match="online"):
            fn(plain, target, TH, TA, ring, 8, 0.9, True, 1, 0, 4, dueling=True)
        fn(None, target, TH, TA, ring, 8, 0.9, False, 1, 0, 4, dueling=True)  # single Q reads no online net
    big = MLPSpec(TD_, TH, 17).init(torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="15"):
        dqn_targets_ref(big, big, TH, 16, ring, 8, 0.9, False, 1, 0, 4, dueling=True)


# ------------------------------------------------------------------ 5. config and plumbing
def test_config_parses_dueling():
    assert DQNConfig().dueling is False and DQNConfig(dueling=True).dueling is True
    for word, want in (("true", True), ("0", False), (" Yes ", True), ("false", False), ("1", True), ("no", False)):
        assert DQNConfig(dueling=word).dueling is want, word
    for bad in ("maybe", "2", ""):
        with pytest.raises(ValueError, match="dueling"):
            DQNConfig(dueling=bad)
    with pytest.raises(ValueError, match="prioritized"):  # the field it was modelled on still says its own name
        DQNConfig(prioritized="maybe")
    assert DQNConfig(dueling="true").to_dict()["dueling"] is True
    cfg = DQNConfig(**DQNConfig(dueling=True, prioritized=True, n_step=3).to_dict())  # round trip of a checkpoint's cfg
    assert cfg.dueling and cfg.prioritized and cfg.n_step == 3


def test_more_than_fifteen_actions_are_refused():
    from relayrl_prototype_amd.ops.dqn import check_q_params
    from relayrl_prototype_amd.runtime import dqn_trainer

    assert dqn_trainer.MAX_DUELING_ACTIONS == 15
    check_q_params(torch.zeros(MLPSpec(4, 64, 16).P), 4, 64, 15, True)
    check_q_params(torch.zeros(MLPSpec(4, 64, 16).P), 4, 64, 16, False)
    with pytest.raises(ValueError, match="15"):
        check_q_params(torch.zeros(MLPSpec(4, 64, 17).P), 4, 64, 16, True)
    from relayrl_prototype_amd.ops import mlp_grad

    with pytest.raises(ValueError, match="15"):
        mlp_grad(GradHead.Q_DUEL, torch.zeros(MLPSpec(4, 64, 17).P), torch.zeros(2, 4), 16, 64,
                 act=torch.zeros(2, dtype=torch.int32), ret=torch.zeros(2))


def test_dueling_preset_and_engine_resolution():
    from relayrl_prototype_amd.runtime import engine as eng
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    p, nstep = PRESETS["cartpole-dqn-dueling"], PRESETS["cartpole-dqn-nstep"]
    assert p.kind == "vec" and p.overrides == dict(nstep.overrides, dueling=True)
    assert "dueling" not in nstep.overrides
    cfg = DQNConfig(**p.overrides)  # every override is a DQNConfig field
    assert cfg.dueling and cfg.n_step == 3 and cfg.prioritized and cfg.double_q and cfg.algo == "dqn"
    spec = eng.resolve_engine("DQN", 4, 2, {}, {}, {"dueling": "true"}, engine="vec")
    assert spec.trainer["dueling"] == "true"
    cfg = DQNConfig(**eng._filter(DQNConfig, spec.trainer))  # what make_trainer builds
    assert cfg.dueling is True and cfg.env == "CartPole-v1" and not cfg.prioritized


def test_evaluate_checkpoint_state_reads_the_dueling_key(monkeypatch):
    """An old checkpoint's cfg has no such key: a plain net.  A dueling one passes the flag on."""
    from relayrl_prototype_amd.runtime import evaluate as ev
    from relayrl_prototype_amd.runtime.launcher import evaluate_checkpoint_state

    seen = []

    class Res:
        def to_dict(self):
            return {"mean_return": 1.0}

    def fake(env, params, hidden, episodes, num_envs, **kw):
        seen.append(kw)
        return Res()

    monkeypatch.setattr(ev, "evaluate_policy", fake)
    old = DQNConfig().to_dict()
    del old["dueling"]
    st = {"cfg": old, "learner": {"pi": {"params": torch.zeros(3)}}, "epoch": 2}
    evaluate_checkpoint_state(st, episodes=4, num_envs=4)
    st["cfg"] = DQNConfig(dueling=True).to_dict()
    evaluate_checkpoint_state(st, episodes=4, num_envs=4)
    assert [kw["dueling"] for kw in seen] == [False, True]
    with pytest.raises(ValueError, match="stochastic"):
        evaluate_checkpoint_state(st, episodes=4, num_envs=4, stochastic=True)


def test_evaluate_policy_refuses_a_stochastic_dueling_policy():
    from relayrl_prototype_amd.runtime.evaluate import evaluate_policy

    p = torch.zeros(MLPSpec(4, 64, 3).P)
    with pytest.raises(ValueError, match="greedily"):
        evaluate_policy("CartPole-v1", p, 64, 1, 4, greedy=False, dueling=True, device="cpu")
    with pytest.raises(ValueError, match="discrete"):
        evaluate_policy("HalfCheetahSynth-v0", p, 64, 1, 4, dueling=True, device="cpu")


# ------------------------------------------------------------------ oracle training loop
def test_dueling_oracle_loop_starts_from_the_trainer_init_and_moves():
    """The helper's loop: 20 epochs at the small shape update 38 times, from MLPSpec(D, H, A + 1)'s seeded init."""
    import dqn_oracle as do

    cfg = DQNConfig(**dict(do.SMALL, learning_starts=512), seed=2, dueling=True)
    p, u = dd.oracle_dqn_dueling(cfg, 20)
    init = MLPSpec(4, cfg.hidden, 3).init(torch.Generator().manual_seed(2)).double()
    assert u == 38 and p.shape == init.shape and not torch.equal(p, init) and bool(torch.isfinite(p).all())
    assert sorted(dd.ORACLE_RETURNS_DUEL) == [1, 2, 3, 4, 5] and min(dd.ORACLE_RETURNS_DUEL.values()) > 0
    assert np.isfinite(dd.greedy_return_dueling(p, cfg.hidden, 9, episodes=8))
