"""The quantile-regression head (QR-DQN) on the CPU, in float64: the HEAD_Q_QR reference gradient against autograd
of the written-out loss (tests/dqn_quantile_oracle.py: oracles that share no code with the reference), the
quantile TD targets against a written-out loop, and the DQNConfig field, the preset, the checkpoint key, the engine
resolution and every refusal."""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import GradHead, MLPSpec, ReplayRing, dqn_nstep_walk_ref, dqn_sample_rows_ref
from relayrl_prototype_amd.ops import dqn_targets, dqn_targets_ref, mlp_grad
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.ops.per import per_sample_rows_ref, per_tree_build
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig

import dqn_quantile_oracle as dq

F64 = torch.float64
SHAPES = [(2, 8), (4, 4), (3, 5), (2, 1), (1, 16)]  # (A, NQ)


# ------------------------------------------------------------------ 1. the sums
def test_quantile_q_sums_action_major():
    out = torch.arange(12, dtype=F64).reshape(2, 6)  # A = 2, NQ = 3
    assert torch.equal(ref.quantile_q(out, 2, 3), torch.tensor([[3.0, 12.0], [21.0, 30.0]], dtype=F64))
    gen = torch.Generator().manual_seed(1)
    for A, NQ in SHAPES:
        o = torch.randn(7, A * NQ, generator=gen, dtype=F64)
        s = ref.quantile_q(o, A, NQ)
        assert s.shape == (7, A) and s.dtype == F64
        assert float((s - dq.quantile_sums(o, A, NQ)).abs().max()) <= 1e-14
    o32 = torch.randn(5, 16, generator=gen)  # fp32: ascending, one add each
    want = o32[:, 0:8].clone()
    acc = want[:, 0]
    for i in range(1, 8):
        acc = acc + o32[:, i]
    assert torch.equal(ref.quantile_q(o32, 2, 8)[:, 0], acc) and ref.quantile_q(o32, 2, 8).dtype == torch.float32
    with pytest.raises(ValueError, match="outputs"):
        ref.quantile_q(torch.zeros(2, 5), 2, 3)


# ------------------------------------------------------------------ 2. HEAD_Q_QR against autograd
def _qr_case(A, NQ, seed, B=23, D=None, kappa=0.75):
    D = D or min(2 * A + 1, 16)
    H = 64
    gen = torch.Generator().manual_seed(seed)
    p = MLPSpec(D, H, A * NQ).init(gen).double()
    X = torch.randn(B, D, generator=gen, dtype=F64)
    act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
    out = dq.forward64(p, X, D, H, A * NQ)
    theta = torch.stack([out[b, int(act[b]) * NQ:(int(act[b]) + 1) * NQ] for b in range(B)])
    # targets on a quantile exactly (u = 0), inside the Huber zone, and beyond +-kappa
    off = torch.tensor([0.0, 0.3, -0.3, 1.7, -1.7], dtype=F64)[(torch.arange(B).unsqueeze(1) + torch.arange(NQ)) % 5]
    T = theta.flip(-1) + off * kappa
    T[0] = theta[0]  # row 0: T_j = theta_j, so u_jj = 0 for every j
    return p, X, act, T, D, H, kappa


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("A,NQ", SHAPES)
def test_q_qr_reference_gradient_matches_autograd(A, NQ, weighted):
    p, X, act, T, D, H, kappa = _qr_case(A, NQ, 20 + A + NQ)
    B, inv_B = X.shape[0], 1.0 / 41
    kw, w = {}, torch.ones(B, dtype=F64)
    if weighted:
        row_w = torch.rand(B, generator=torch.Generator().manual_seed(3), dtype=F64) + 0.1
        w_norm = row_w.max().reshape(1)
        kw, w = dict(row_w=row_w, w_norm=w_norm), row_w / w_norm
    g, st = ref.mlp_grad_ref(ref.HEAD_Q_QR, p, X, A, H, act=act, ret=T, inv_B=inv_B, clip_eps=kappa, dtype=F64,
                             quantiles=NQ, **kw)
    pa = p.clone().requires_grad_(True)
    rho = dq.qr_loss_rows(dq.forward64(pa, X, D, H, A * NQ), act, T, A, NQ, kappa)
    ((w * rho).sum() * inv_B).backward()
    err = float((g - pa.grad).abs().max())
    print(f"A = {A}, NQ = {NQ}, weighted = {weighted}: reference vs autograd {err:.2e}")
    assert err <= 1e-12
    rho = rho.detach()
    # the td_abs = rho contract: the UNWEIGHTED row loss, whatever the weights
    assert float((st["td_abs"] - rho).abs().max()) <= 1e-12
    tot = float((w * rho).sum())
    assert abs(st["loss"] - tot) <= 1e-12 * (1 + abs(tot)) and st["count"] == B
    out = dq.forward64(p, X, D, H, A * NQ)
    s_act = dq.quantile_sums(out, A, NQ)[torch.arange(B), act.long()]
    assert abs(st["v"] - float((s_act / NQ).sum())) <= 1e-12 * (1 + abs(float(s_act.sum())))
    # every output that is not a quantile of the taken action has gradient 0: its b3 entry is exactly 0
    b3 = MLPSpec(D, H, A * NQ).offsets()["b3"]
    taken = set(int(a) for a in act)
    for a in range(A):
        if a not in taken:
            assert bool((g[b3 + a * NQ:b3 + (a + 1) * NQ] == 0).all())


def test_q_qr_closed_form_at_one_quantile():
    """NQ = 1: tau = 1/2 and the row loss is 0.5 * huber(u) / kappa."""
    p, X, act, T, D, H, kappa = _qr_case(2, 1, 5)
    _, st = ref.mlp_grad_ref(ref.HEAD_Q_QR, p, X, 2, H, act=act, ret=T, clip_eps=kappa, dtype=F64, quantiles=1)
    out = dq.forward64(p, X, D, H, 2)
    u = T[:, 0] - out[torch.arange(X.shape[0]), act.long()]
    hub = torch.where(u.abs() <= kappa, 0.5 * u * u, kappa * (u.abs() - 0.5 * kappa))
    assert float((st["td_abs"] - 0.5 * hub / kappa).abs().max()) <= 1e-14
    assert float(u.abs().min()) == 0.0 and float(u.abs().max()) > kappa  # both zones and u = 0 are among the rows


def test_q_qr_through_the_cpu_op():
    """ops.mlp_grad on CPU tensors is the reference, td_abs included."""
    A, NQ, D, H, B = 2, 8, 4, 64, 9
    gen = torch.Generator().manual_seed(3)
    p = MLPSpec(D, H, A * NQ).init(gen)
    X, act = torch.randn(B, D, generator=gen), torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
    T = torch.randn(B, NQ, generator=gen)
    row_w, td = torch.rand(B, generator=gen) + 0.5, torch.zeros(B)
    kw = dict(act=act, ret=T, clip_eps=1.0, row_w=row_w, w_norm=row_w.max().reshape(1))
    g, ls = mlp_grad(GradHead.Q_QR, p, X, A, H, td_abs=td, quantiles=NQ, **kw)
    want, st = ref.mlp_grad_ref(ref.HEAD_Q_QR, p, X, A, H, quantiles=NQ, **kw)
    assert g.shape == (1, MLPSpec(D, H, A * NQ).P) and torch.equal(g[0], want) and torch.equal(td, st["td_abs"])
    assert float(ls[0, 5]) == B and abs(float(ls[0, 0]) - st["loss"]) <= 1e-5 * (1 + abs(st["loss"]))
    assert int(GradHead.Q_QR) == ref.HEAD_Q_QR == 7
    nv = torch.tensor([5], dtype=torch.int32)  # the device-side batch shape, on the CPU path
    g5, _ = mlp_grad(GradHead.Q_QR, p, X, A, H, quantiles=NQ, nvalid=nv, inv_B=1.0 / B, **kw)
    w5, _ = ref.mlp_grad_ref(ref.HEAD_Q_QR, p, X[:5], A, H, act=act[:5], ret=T[:5], clip_eps=1.0, row_w=row_w[:5],
                             w_norm=kw["w_norm"], inv_B=1.0 / B, quantiles=NQ)
    assert torch.equal(g5[0], w5)


def test_q_qr_refusals():
    D, H, B = 4, 64, 3
    X, act = torch.zeros(B, D), torch.zeros(B, dtype=torch.int32)
    p16 = torch.zeros(MLPSpec(D, H, 16).P)
    for fn in (lambda **k: mlp_grad(GradHead.Q_QR, p16, X, k.pop("A", 2), H, act=act, **k),
               lambda **k: ref.mlp_grad_ref(ref.HEAD_Q_QR, p16, X, k.pop("A", 2), H, act=act, **k)):
        with pytest.raises(ValueError, match="16"):
            fn(A=3, ret=torch.zeros(B, 8), quantiles=8)  # 24 outputs
        with pytest.raises(ValueError, match="quantiles"):
            fn(ret=torch.zeros(B, 8), quantiles=0)  # the head without its quantiles
        with pytest.raises(ValueError, match="quantiles"):
            fn(ret=torch.zeros(B, 8), quantiles=-1)
        with pytest.raises(ValueError, match="threshold"):
            fn(ret=torch.zeros(B, 8), quantiles=8, clip_eps=0.0)
    with pytest.raises(ValueError, match="quantiles"):  # quantiles with another head
        mlp_grad(GradHead.Q_TD, p16, X, 16, H, act=act, ret=torch.zeros(B), quantiles=2)
    with pytest.raises(ValueError, match=f"{MLPSpec(D, H, 2).P} floats.*{MLPSpec(D, H, 16).P}"):  # a scalar net
        mlp_grad(GradHead.Q_QR, torch.zeros(MLPSpec(D, H, 2).P), X, 2, H, act=act, ret=torch.zeros(B, 8), quantiles=8)
    with pytest.raises(ValueError, match="targets"):
        mlp_grad(GradHead.Q_QR, p16, X, 2, H, act=act, ret=torch.zeros(B), quantiles=8)


# ------------------------------------------------------------------ 3. targets against the written-out loop
TC, TN, TD_, TH = 6, 5, 4, 64


def _ring_and_nets(seed, A, NQ):
    gen = torch.Generator().manual_seed(seed)
    ring = ReplayRing(torch.randn(TC, TN, TD_, generator=gen), torch.randn(TC, TN, TD_, generator=gen),
                      torch.randint(0, A, (TC, TN), generator=gen, dtype=torch.int32), torch.randn(TC, TN, generator=gen),
                      torch.randint(0, 3, (TC, TN), generator=gen).float())
    ring.done[0, 0] = 1.0
    assert set(ring.done.unique().tolist()) == {0.0, 1.0, 2.0}
    online = MLPSpec(TD_, TH, A * NQ).init(gen).double()
    target = MLPSpec(TD_, TH, A * NQ).init(gen).double()
    return ring, online, target


@pytest.mark.parametrize("double_q", [False, True])
@pytest.mark.parametrize("form", ["uniform", "tree", "nstep"])
@pytest.mark.parametrize("A,NQ", [(2, 8), (3, 5), (1, 16)])
def test_quantile_targets_equal_the_written_out_loop(A, NQ, form, double_q):
    ring, online, target = _ring_and_nets(31 + A, A, NQ)
    B, filled, gamma, seed, upd = 48, TC * TN, 0.9, 7, 3
    kw = {}
    if form == "tree":
        leaves = torch.rand(filled, generator=torch.Generator().manual_seed(5)) + 0.05
        kw = dict(tree=per_tree_build(leaves), beta=0.6)
    if form == "nstep":
        kw = dict(n_step=3, newest=2)
    got = dqn_targets_ref(online, target, TH, A, ring, filled, gamma, double_q, seed, upd, B, F64, quantiles=NQ, **kw)
    assert len(got) == {"uniform": 4, "tree": 6, "nstep": 5}[form]
    rows = per_sample_rows_ref(kw["tree"], seed, upd, B, filled) if form == "tree" else \
        dqn_sample_rows_ref(seed, upd, B, filled)
    if form == "nstep":
        last, G, disc, _ = dqn_nstep_walk_ref(rows, ring, filled, 2, 3, gamma, F64)
    else:
        last, G, disc = rows, ring.rew.reshape(-1)[torch.from_numpy(rows)].double().numpy(), np.full(B, gamma)
    want = dq.qr_targets_loop(online, target, TH, A, NQ, ring, last, G, disc, double_q)
    y = got[2]
    err = float((y - want).abs().max())
    print(f"A = {A}, NQ = {NQ}, {form}, double_q = {double_q}: y vs the loop {err:.2e}")
    assert y.shape == (B, NQ) and y.dtype == F64 and err <= 1e-12
    # everything but y equals the scalar call on the same ring (sampling does not see the nets)
    plain = tuple(MLPSpec(TD_, TH, A).init(torch.Generator().manual_seed(s)).double() for s in (1, 2))
    base = dqn_targets_ref(plain[0], plain[1], TH, A, ring, filled, gamma, double_q, seed, upd, B, F64, **kw)
    for i, (x, b) in enumerate(zip(got, base)):
        if i != 2:
            assert torch.equal(x, b), i
    # the selection is on the sums and it matters: single Q and double Q disagree somewhere (A > 1)
    if A > 1:
        other = dqn_targets_ref(online, target, TH, A, ring, filled, gamma, not double_q, seed, upd, B, F64,
                                quantiles=NQ, **kw)
        assert not torch.equal(other[2], y)
    # the CPU op is the reference
    op = dqn_targets(online, target, TH, A, ring, filled, gamma, double_q, seed, upd, B, dtype=F64, quantiles=NQ, **kw)
    assert all(torch.equal(x, b) for x, b in zip(op, got))
    out = (torch.zeros(B, TD_, dtype=F64), torch.zeros(B, dtype=torch.int32), torch.zeros(B, NQ, dtype=F64),
           torch.zeros(B, dtype=torch.int64))
    if form == "tree":
        out += (torch.zeros(B, dtype=F64), torch.zeros(1, dtype=F64))
    dqn_targets(online, target, TH, A, ring, filled, gamma, double_q, seed, upd, B, out=out, dtype=F64, quantiles=NQ, **kw)
    assert torch.equal(out[2], y)


def test_quantile_targets_refusals():
    A, NQ = 2, 8
    ring, online, target = _ring_and_nets(32, A, NQ)
    plain = MLPSpec(TD_, TH, A).init(torch.Generator().manual_seed(1)).double()
    want_q, want_p = MLPSpec(TD_, TH, A * NQ).P, MLPSpec(TD_, TH, A).P
    for fn in (dqn_targets_ref, dqn_targets):
        with pytest.raises(ValueError, match=f"{want_p} floats.*{want_q}"):
            fn(plain, plain, TH, A, ring, 10, 0.9, True, 1, 0, 4, quantiles=NQ)
        with pytest.raises(ValueError, match=f"{want_q} floats.*{want_p}"):
            fn(online, target, TH, A, ring, 10, 0.9, True, 1, 0, 4)
        with pytest.raises(ValueError, match="online"):
            fn(plain, target, TH, A, ring, 10, 0.9, True, 1, 0, 4, quantiles=NQ)
        fn(None, target, TH, A, ring, 10, 0.9, False, 1, 0, 4, quantiles=NQ)  # single Q reads no online net
        with pytest.raises(ValueError, match="quantiles.*dueling|dueling.*quantiles"):
            fn(online, target, TH, A, ring, 10, 0.9, True, 1, 0, 4, quantiles=NQ, dueling=True)
        with pytest.raises(ValueError, match="16"):
            fn(online, target, TH, 3, ring, 10, 0.9, True, 1, 0, 4, quantiles=NQ)
        with pytest.raises(ValueError, match="quantiles"):
            fn(online, target, TH, A, ring, 10, 0.9, True, 1, 0, 4, quantiles=-1)


# ------------------------------------------------------------------ 4. config and plumbing
def test_config_parses_quantiles():
    assert DQNConfig().quantiles == 0 and DQNConfig(quantiles=8).quantiles == 8
    for word, want in (("8", 8), (" 4 ", 4), ("0", 0), (16, 16), (2.0, 2)):
        assert DQNConfig(quantiles=word).quantiles == want, word
    for bad in ("eight", "", None, 2.5, "2.5"):
        with pytest.raises(ValueError, match="quantiles"):
            DQNConfig(quantiles=bad)
    for bad in (-1, "-3", 17):
        with pytest.raises(ValueError, match="quantiles"):
            DQNConfig(quantiles=bad)
    with pytest.raises(ValueError, match="n_step"):  # the field it was modelled on still says its own name
        DQNConfig(n_step="three")
    with pytest.raises(ValueError, match="quantiles.*dueling"):
        DQNConfig(quantiles=4, dueling=True)
    with pytest.raises(ValueError, match="quantiles.*dueling"):
        DQNConfig(quantiles="4", dueling="true")
    DQNConfig(quantiles=0, dueling=True)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="huber_delta"):
            DQNConfig(quantiles=4, huber_delta=bad)
    DQNConfig(quantiles=0, huber_delta=0.0)  # the scalar head's business, as before
    assert DQNConfig(quantiles="8").to_dict()["quantiles"] == 8
    cfg = DQNConfig(**DQNConfig(quantiles=8, prioritized=True, n_step=3, noisy=True).to_dict())  # a checkpoint's cfg
    assert cfg.quantiles == 8 and cfg.prioritized and cfg.n_step == 3 and cfg.noisy and not cfg.dueling


def test_check_q_params_takes_quantiles():
    from relayrl_prototype_amd.ops.dqn import check_q_params, check_quantiles

    check_q_params(torch.zeros(MLPSpec(4, 64, 16).P), 4, 64, 2, False, quantiles=8)
    check_q_params(torch.zeros(MLPSpec(4, 64, 16).P), 4, 64, 16, False, quantiles=1)
    check_q_params(torch.zeros(MLPSpec(4, 64, 2).P), 4, 64, 2, False)  # quantiles = 0: as before
    with pytest.raises(ValueError, match="floats.*quantiles = 8"):
        check_q_params(torch.zeros(MLPSpec(4, 64, 2).P), 4, 64, 2, False, quantiles=8)
    with pytest.raises(ValueError, match="16"):
        check_q_params(torch.zeros(MLPSpec(4, 64, 16).P), 4, 64, 4, False, quantiles=5)
    with pytest.raises(ValueError, match="dueling"):
        check_q_params(torch.zeros(MLPSpec(4, 64, 16).P), 4, 64, 2, True, quantiles=8)
    assert check_quantiles(2, "8") == 8 and check_quantiles(16, 0) == 0
    with pytest.raises(ValueError, match=">= 0"):
        check_quantiles(2, -2)


def test_quantile_preset_and_engine_resolution():
    from relayrl_prototype_amd.runtime import engine as eng
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    p, nstep = PRESETS["cartpole-dqn-quantile"], PRESETS["cartpole-dqn-nstep"]
    assert p.kind == "vec" and p.overrides == dict(nstep.overrides, quantiles=8)
    assert "quantiles" not in nstep.overrides and "quantiles" not in PRESETS["cartpole-dqn"].overrides
    cfg = DQNConfig(**p.overrides)  # every override is a DQNConfig field
    assert cfg.quantiles == 8 and cfg.n_step == 3 and cfg.prioritized and cfg.double_q and not cfg.dueling
    for name in ("cartpole-dqn", "cartpole-dqn-per", "cartpole-dqn-nstep"):  # --set quantiles=8
        assert DQNConfig(**dict(PRESETS[name].overrides, quantiles="8")).quantiles == 8
    for name in ("cartpole-dqn-dueling", "cartpole-dqn-noisy"):  # the dueling presets refuse it
        with pytest.raises(ValueError, match="dueling"):
            DQNConfig(**dict(PRESETS[name].overrides, quantiles="8"))
    spec = eng.resolve_engine("DQN", 4, 2, {}, {}, {"quantiles": "8"}, engine="vec")
    assert spec.trainer["quantiles"] == "8"
    cfg = DQNConfig(**eng._filter(DQNConfig, spec.trainer))  # what make_trainer builds
    assert cfg.quantiles == 8 and cfg.env == "CartPole-v1" and not cfg.prioritized


def test_evaluate_checkpoint_state_reads_the_quantiles_key(monkeypatch):
    """An old checkpoint's cfg has no such key: a scalar net.  A quantile one passes the count on."""
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
    del old["quantiles"]
    st = {"cfg": old, "learner": {"pi": {"params": torch.zeros(3)}}, "epoch": 2}
    evaluate_checkpoint_state(st, episodes=4, num_envs=4)
    st["cfg"] = DQNConfig(quantiles=8).to_dict()
    evaluate_checkpoint_state(st, episodes=4, num_envs=4)
    assert [kw["quantiles"] for kw in seen] == [0, 8] and [kw["dueling"] for kw in seen] == [False, False]
    with pytest.raises(ValueError, match="stochastic"):
        evaluate_checkpoint_state(st, episodes=4, num_envs=4, stochastic=True)


def test_evaluate_policy_refuses_what_a_quantile_net_is_not():
    from relayrl_prototype_amd.runtime.evaluate import evaluate_policy

    p = torch.zeros(MLPSpec(4, 64, 16).P)
    with pytest.raises(ValueError, match="greedily"):
        evaluate_policy("CartPole-v1", p, 64, 1, 4, greedy=False, quantiles=8, device="cpu")
    with pytest.raises(ValueError, match="discrete"):
        evaluate_policy("HalfCheetahSynth-v0", p, 64, 1, 4, quantiles=8, device="cpu")
    with pytest.raises(ValueError, match="dueling"):
        evaluate_policy("CartPole-v1", p, 64, 1, 4, quantiles=8, dueling=True, device="cpu")
    with pytest.raises(ValueError, match="quantiles"):
        evaluate_policy("CartPole-v1", p, 64, 1, 4, quantiles=-1, device="cpu")


# ------------------------------------------------------------------ oracle training loop
def test_quantile_oracle_loop_starts_from_the_trainer_init_and_moves():
    """The helper's loop: 20 epochs at the small shape update 38 times, from MLPSpec(D, H, A * NQ)'s seeded init."""
    import dqn_oracle as do

    cfg = DQNConfig(**dict(do.SMALL, learning_starts=512), seed=2, quantiles=8)
    p, u = dq.oracle_dqn_quantile(cfg, 20)
    init = MLPSpec(4, cfg.hidden, 16).init(torch.Generator().manual_seed(2)).double()
    assert u == 38 and p.shape == init.shape and not torch.equal(p, init) and bool(torch.isfinite(p).all())
    assert sorted(dq.ORACLE_RETURNS_QR) == [1, 2, 3, 4, 5] and min(dq.ORACLE_RETURNS_QR.values()) > 0
    assert np.isfinite(dq.greedy_return_quantile(p, cfg.hidden, 8, 9, episodes=8))
