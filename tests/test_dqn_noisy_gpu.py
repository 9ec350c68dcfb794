"""NoisyNet exploration on the GPU: the compose and grad kernels (csrc/kernels/noisy.hip) against the host
references of ops/noisy.py (the noise within a derived tolerance of float64, everything after the noise bit for
bit), the device pipeline compose -> mlp_grad -> noisy_grad against float64 autograd, and the noisy DQNTrainer.
Every output buffer of a kernel under test is guarded."""
import os

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import GradHead, MLPSpec, evaluate_policy_op, hip, mlp_grad, noisy_compose
from relayrl_prototype_amd.ops import noisy_compose_ref, noisy_eps_ref, noisy_grad, noisy_num_units, noisy_sigma_init
from relayrl_prototype_amd.ops import noisy_units_ref
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime import dqn_trainer as dt
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer, dqn_noise_seed

import dqn_noisy_oracle as dn
import dqn_oracle as do
from guarded import Guarded
from test_dqn_gpu import TRAINER, cu_limit

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY = dn.KEY


def theta_of(spec, seed=3, sigma0=0.5):
    """[mu; sigma] with a sigma that differs from element to element (a constant would hide an index slip)."""
    g = torch.Generator().manual_seed(seed)
    sigma = noisy_sigma_init(spec, sigma0) * (0.5 + torch.rand(spec.P, generator=g))
    return torch.cat([spec.init(g), sigma])


def compose(thetas, roles, draws, spec, units=True):
    """One guarded launch -> (out [njobs, P], units [njobs, U] or None) on the host."""
    n = len(roles)
    out = Guarded((n, spec.P))
    un = Guarded((n, noisy_num_units(spec))) if units else None
    noisy_compose(thetas, roles, draws, spec, KEY, out=out.t, units_out=un.t if units else None)
    torch.cuda.synchronize()
    assert out.guards_intact() and (un is None or un.guards_intact())
    return out.t.cpu(), (un.t.cpu() if units else None)


# ------------------------------------------------------------------ 1. the noise
@pytest.mark.parametrize("D,H,A", dn.SHAPES)
def test_unit_factors_are_the_float64_normals(cuda, D, H, A):
    spec = MLPSpec(D, H, A)
    theta = theta_of(spec).to(DEV)
    worst = 0.0
    for draw in dn.DRAWS:
        for roles in ((0, 1, 2), (3,)):
            _, units = compose(theta, roles, (draw,) * len(roles), spec)
            for k, role in enumerate(roles):
                f = units[k].double().numpy()
                n64 = noisy_units_ref(KEY, role, draw, spec, np.float64)[0]
                worst = max(worst, float(np.abs(np.sign(f) * f * f - n64).max()))
    print(f"max |sgn(f) f^2 - n64| = {worst:.3e}")
    assert worst <= dn.UNIT_TOL


# ------------------------------------------------------------------ 2. compose, given the noise
@pytest.mark.parametrize("D,H,A", dn.SHAPES)
def test_compose_is_bitwise_given_the_units(cuda, D, H, A):
    spec = MLPSpec(D, H, A)
    P = spec.P
    th = [theta_of(spec, s) for s in (3, 4, 5)]
    dev = [t.to(DEV) for t in th]
    roles, draws = (1, 2, 3), (2 ** 32 + 5, 7, 2 ** 63 - 1)
    out, units = compose(dev, roles, draws, spec)
    for k in range(3):
        eps = noisy_eps_ref(units[k], spec)
        assert torch.equal(out[k], th[k][:P] + th[k][P:] * eps), k  # torch fp32 on the CPU: a multiply, an add
        assert torch.equal(out[k], noisy_compose_ref(th[k], units[k], spec))
        one, one_units = compose(dev[k], (roles[k],), (draws[k],), spec)  # three jobs == three launches
        assert torch.equal(one[0], out[k]) and torch.equal(one_units[0], units[k]), k
    with cu_limit(2):
        again, again_units = compose(dev, roles, draws, spec)
    assert torch.equal(again, out) and torch.equal(again_units, units), "the result depends on the grid"
    plain, _ = compose(dev, roles, draws, spec, units=False)  # units_out is optional
    assert torch.equal(plain, out)
    zero = torch.cat([th[0][:P], torch.zeros(P)]).to(DEV)  # sigma = 0: mu, bit for bit
    out0, _ = compose(zero, (0,), (1,), spec)
    assert torch.equal(out0[0], th[0][:P])


# ------------------------------------------------------------------ 3. grad
@pytest.mark.parametrize("D,H,A", dn.SHAPES)
def test_grad_is_bitwise(cuda, D, H, A):
    spec = MLPSpec(D, H, A)
    P = spec.P
    role, draw = 1, 2 ** 32 + 9
    _, units = compose(theta_of(spec).to(DEV), (role,), (draw,), spec)
    eps = noisy_eps_ref(units[0], spec)
    for nslab in (1, 2, 65):
        slab = torch.randn(nslab, P, generator=torch.Generator().manual_seed(nslab))
        g = slab[0].clone()
        for s in range(1, nslab):  # ascending, one fp32 add at a time
            g = g + slab[s]

        def launch():
            out = Guarded((2 * P,))
            noisy_grad(slab.to(DEV), role, draw, spec, KEY, out=out.t)
            torch.cuda.synchronize()
            assert out.guards_intact()
            return out.t.cpu()

        got = launch()
        assert torch.equal(got[:P], g), nslab
        assert torch.equal(got[P:], g * eps), nslab
        assert torch.equal(launch(), got), "two launches differ"
        with cu_limit(2):
            assert torch.equal(launch(), got), "the result depends on the grid"


# ------------------------------------------------------------------ 4. refusals
def test_refusals_write_nothing(cuda):
    h = hip()
    spec = MLPSpec(4, 64, 2)
    P, U = spec.P, noisy_num_units(spec)
    big = 2 * MLPSpec(16, 128, 16).P  # no refused call is short of memory either
    theta = torch.zeros(big, device=DEV)
    out, units, grad = Guarded((3, big // 2)), Guarded((3, 16 + 4 * 128 + 16)), Guarded((big,))
    slab = torch.zeros(2, big // 2, device=DEV)

    def comp(thetas=None, roles=(1,), D=4, H=64, A=2, o=out.t, u=units.t):
        thetas = [theta] * len(roles) if thetas is None else thetas
        return h.noisy_compose(thetas, list(roles), [0] * len(roles), D, H, A, KEY, o, u)

    def grd(s=slab, role=1, D=4, H=64, A=2, g=grad.t, nslab=2):
        return h.noisy_grad(s, role, 0, D, H, A, KEY, g, nslab)

    assert comp(o=None) == -1 and comp(thetas=[None]) == -1
    assert grd(s=None) == -1 and grd(g=None) == -1
    for D in (0, 17):
        assert comp(D=D) == -2 and grd(D=D) == -2
    for A in (0, 17):
        assert comp(A=A) == -2 and grd(A=A) == -2
    assert comp(roles=()) == -2 and comp(roles=(0, 1, 2, 3)) == -2
    assert grd(nslab=0) == -2
    for role in (-1, 4):
        assert comp(roles=(1, role)) == -2 and grd(role=role) == -2
    for H in (0, 32, 96, 256):
        assert comp(H=H) == -3 and grd(H=H) == -3
    with pytest.raises(ValueError, match="role"):
        noisy_compose(theta[:2 * P], (4,), (0,), spec, KEY)
    with pytest.raises(ValueError, match="theta"):
        noisy_compose(theta[:P], (1,), (0,), spec, KEY)
    with pytest.raises(RuntimeError):  # the binding sizes every tensor of a shape the kernel takes
        comp(thetas=[theta[:P]])
    with pytest.raises(RuntimeError):
        grd(s=slab.reshape(-1)[:P], nslab=2)
    torch.cuda.synchronize()
    for b in (out, units, grad):
        assert bool(torch.isnan(b.big).all()), "a refused call wrote"
    assert comp(roles=(0, 1, 2)) == 0 and grd() == 0  # the sound calls
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.t.reshape(-1)[:3 * P]).all()) and bool(torch.isfinite(grad.t[:2 * P]).all())
    assert bool(torch.isfinite(units.t.reshape(-1)[:3 * U]).all())


# ------------------------------------------------------------------ 5. end to end against float64 autograd
@pytest.mark.parametrize("dueling", [False, True], ids=["q_td", "q_duel"])
@pytest.mark.parametrize("H,A", [(H, A) for H in (64, 128) for A in (2, 3)])
def test_pipeline_matches_float64_autograd(cuda, H, A, dueling):
    """compose -> mlp_grad -> noisy_grad against autograd through W = mu + sigma * eps in float64, eps from the
    dumped unit factors.  The mu half is the quantity test_dqn_gpu._assert_q_td bounds and takes its tolerance,
    2e-4 * max|g64| + 1e-6; the sigma half is that gradient times eps, one exact multiple per element plus one
    rounding: the same rtol, the atol times max|eps|."""
    D, delta, role, draw = 4, 0.75, 1, 11
    AO = A + 1 if dueling else A
    head = GradHead.Q_DUEL if dueling else GradHead.Q_TD
    spec = MLPSpec(D, H, AO)
    P = spec.P
    theta = theta_of(spec, 6)
    for B in (1, 65):
        w, units = compose(theta.to(DEV), (role,), (draw,), spec)
        gen = torch.Generator().manual_seed(100 * B + A)
        X = torch.randn(B, D, generator=gen)
        act = torch.randint(0, A, (B,), generator=gen, dtype=torch.int32)
        eps = noisy_eps_ref(units[0].double(), spec)
        th64 = theta.double().requires_grad_(True)
        out = ref.trunk(th64[:P] + th64[P:] * eps, X.double(), D, H, AO)[0]
        q = (ref.dueling_q(out, A) if dueling else out).gather(-1, act.long().unsqueeze(-1)).squeeze(-1)
        # |diff| on both sides of delta, both signs, and 0
        y = (q + torch.tensor([0.3, -0.3, 1.7, -1.7, 0.0], dtype=torch.float64)[torch.arange(B) % 5] * delta).detach()
        diff = q - y
        huber = torch.where(diff.abs() <= delta, 0.5 * diff * diff, delta * (diff.abs() - 0.5 * delta))
        (g64,) = torch.autograd.grad(huber.mean(), th64)
        ns = int(hip().mlp_grad_slabs(B))
        slab = Guarded((ns, P))
        mlp_grad(head, w[0].to(DEV), X.to(DEV), A, H, act=act.to(DEV), ret=y.float().to(DEV), clip_eps=delta,
                 grad_slab=slab.t)
        got = Guarded((2 * P,))
        noisy_grad(slab.t, role, draw, spec, KEY, out=got.t)
        torch.cuda.synchronize()
        assert slab.guards_intact() and got.guards_intact()
        g = got.t.cpu().double()
        scale = g64[:P].abs().max().item() + 1e-12
        err = (g[:P] - g64[:P]).abs().max().item()
        assert err <= 2e-4 * scale + 1e-6, ("mu", B, err, scale)
        emax = eps.abs().max().item()
        scale_s = g64[P:].abs().max().item() + 1e-12
        err_s = (g[P:] - g64[P:]).abs().max().item()
        print(f"B = {B}: mu err {err:.3e} (scale {scale:.3e}), sigma err {err_s:.3e} (scale {scale_s:.3e}, max|eps| {emax:.3f})")
        assert err_s <= 2e-4 * scale_s + 1e-6 * emax, ("sigma", B, err_s, scale_s, emax)


# ------------------------------------------------------------------ 6. trainer wiring
def _recorded(monkeypatch):
    """Wrap the three big launches of the trainer module: every call records copies of the parameter tensors
    it received."""
    seen = {"rollout": [], "targets": [], "grad": []}
    ro, tg, mg = dt.dqn_rollout, dt.dqn_targets, dt.mlp_grad

    def rollout(env_id, params, *a, **kw):
        seen["rollout"].append((params.data_ptr(), params.clone()))
        return ro(env_id, params, *a, **kw)

    def targets(online, target, *a, **kw):
        seen["targets"].append((online.data_ptr(), online.clone(), target.data_ptr(), target.clone()))
        return tg(online, target, *a, **kw)

    def grad(head, params, *a, **kw):
        seen["grad"].append((params.data_ptr(), params.clone()))
        return mg(head, params, *a, **kw)

    monkeypatch.setattr(dt, "dqn_rollout", rollout)
    monkeypatch.setattr(dt, "dqn_targets", targets)
    monkeypatch.setattr(dt, "mlp_grad", grad)
    return seen


@pytest.mark.parametrize("double_q", [True, False])
def test_trainer_feeds_each_launch_its_own_sample(cuda, monkeypatch, double_q):
    seen = _recorded(monkeypatch)
    jobs = []  # (roles, draws, copies of the thetas at the time of the call) of every compose launch
    nc = dt.noisy_compose

    def compose_spy(thetas, roles, draws, *a, **kw):
        thetas = list(thetas) if isinstance(thetas, (list, tuple)) else [thetas] * len(roles)
        jobs.append((tuple(roles), tuple(draws), [t.clone() for t in thetas]))
        return nc(thetas, roles, draws, *a, **kw)

    monkeypatch.setattr(dt, "noisy_compose", compose_spy)
    kw = dict(TRAINER, noisy=True, double_q=double_q, eps_start=0.0, eps_end=0.0)
    tr = DQNTrainer(DQNConfig(**kw), device=cuda)
    spec, P, key = tr.q.spec, tr.q.P, dqn_noise_seed(kw["seed"])
    assert tr.theta.numel() == 2 * P and tr.target.numel() == 2 * P and tr.theta_m.numel() == 2 * P
    plain = DQNTrainer(DQNConfig(**TRAINER), device=cuda)
    assert torch.equal(tr.theta[:P], plain.q.params), "mu is not the plain trainer's seeded init"
    sigma0 = noisy_sigma_init(spec, 0.5).to(cuda)
    assert torch.equal(tr.theta[P:], sigma0) and torch.equal(tr.target, tr.theta)

    def sample(theta, role, draw):
        return noisy_compose(theta, (role,), (draw,), spec, key)[0]

    roles = (1, 2, 3) if double_q else (1, 2)  # no role-3 job without double Q
    for epoch in range(6):
        theta0, upd0 = tr.theta.clone(), tr.updates
        for k in seen:
            seen[k].clear()
        jobs.clear()
        tr.train_epoch()
        (ptr, w), = seen["rollout"]
        assert ptr == tr.actor_w.data_ptr() and torch.equal(w, sample(theta0, 0, epoch)), epoch
        assert jobs[0][:2] == ((0,), (epoch,)) and torch.equal(jobs[0][2][0], theta0)
        n = tr.updates - upd0
        assert n == 2 and len(seen["targets"]) == len(seen["grad"]) == n and len(jobs) == 1 + n
        for i in range(n):
            u = upd0 + i
            r, d, th = jobs[1 + i]
            assert r == roles and d == (u,) * len(roles)
            assert (not double_q or torch.equal(th[0], th[2])) and torch.equal(th[0], theta0) == (i == 0)
            on_ptr, on, tg_ptr, tg = seen["targets"][i]
            g_ptr, gw = seen["grad"][i]
            assert g_ptr == tr.update_w[0].data_ptr() and torch.equal(gw, sample(th[0], 1, u)), (epoch, i)
            assert tg_ptr == tr.update_w[1].data_ptr() and torch.equal(tg, sample(th[1], 2, u)), (epoch, i)
            if double_q:
                assert on_ptr == tr.update_w[2].data_ptr() and torch.equal(on, sample(th[2], 3, u)), (epoch, i)
            assert not torch.equal(gw, tg) and not torch.equal(gw, th[0][:P]) and not torch.equal(gw, w)
    # sigma learns, and its Adam state with it
    assert not torch.equal(tr.theta[P:], sigma0) and bool((tr.theta_m[P:] != 0).any())
    m = tr.metrics()
    assert m["Noisy"] is True and m["Epsilon"] == 0.0
    assert m["SigmaMeanAbs"] == pytest.approx(float(tr.theta[P:].abs().mean()), rel=1e-6)
    assert "SigmaMeanAbs" not in plain.metrics() and plain.metrics()["Noisy"] is False


def test_noisy_target_network_follows_its_schedule(cuda):
    tr = DQNTrainer(DQNConfig(**TRAINER, noisy=True), device=cuda)
    tr.rollout()
    prev = tr.target.clone()
    assert torch.equal(prev, tr.theta) and prev.numel() == 2 * tr.q.P
    P = tr.q.P
    for u in range(1, 8):
        tr.update()
        if u % 3 == 0:
            assert torch.equal(tr.target, tr.theta)
            assert not torch.equal(tr.target[:P], prev[:P]) and not torch.equal(tr.target[P:], prev[P:])
            prev = tr.target.clone()
        else:
            assert torch.equal(tr.target, prev)
            assert not torch.equal(tr.target[:P], tr.theta[:P]) and not torch.equal(tr.target[P:], tr.theta[P:])


# ------------------------------------------------------------------ 7. resume and evaluate
NAMES = ["online", "m", "v", "step", "target", "obs", "nobs", "act", "rew", "done", "state", "ep_len", "ep_ret", "tree",
         "pmax", "sigma", "m_sigma", "v_sigma", "target_sigma"]


def _state(tr):
    return [t.clone() for t in tr.snapshot_tensors()], dict(tr.counters())


def test_noisy_trainer_resume_is_bitwise_and_evaluate_scores_mu(cuda):
    extra = dict(prioritized=True, n_step=3, per_beta_epochs=4, dueling=True)
    kw = dict(TRAINER, noisy=True, **extra)
    a = DQNTrainer(DQNConfig(**kw), device=cuda)
    for _ in range(6):
        a.train_epoch()
    b = DQNTrainer(DQNConfig(**kw), device=cuda)
    for _ in range(3):
        b.train_epoch()
    assert len(b.snapshot_tensors()) == len(NAMES)
    before, counters = _state(b)
    step0 = b.eval_step0
    res = b.evaluate(episodes=2, num_envs=33)
    assert res.stats()["episodes"] == 66
    after, counters2 = _state(b)
    assert counters == counters2 and all(torch.equal(x, y) for x, y in zip(before, after)), "evaluate() changed state"
    P = b.q.P
    mu = b.theta[:P].clone()
    ep_ret, ep_len, ep_code, _ = evaluate_policy_op(b.env_id, mu, kw["hidden"], 2, 33, greedy=True, seed=b.eval_seed,
                                                    step0=step0, max_steps=b.max_steps, dueling=True)
    assert torch.equal(res.ep_ret, ep_ret) and torch.equal(res.ep_len, ep_len), "evaluate() is not the evaluator on mu"
    sd = b.state_dict()
    assert sd["cfg"]["noisy"] is True and torch.equal(sd["learner"]["pi"]["params"], mu.cpu())
    assert sd["learner"]["pi"]["m"].numel() == P and sd["learner"]["target"]["params"].numel() == P
    assert sorted(sd["noisy"]) == ["m", "sigma", "target_sigma", "v"] and sd["noisy"]["sigma"].numel() == P
    c = DQNTrainer(DQNConfig(**kw), device=cuda)
    c.theta.add_(1.0)  # other weights until the load
    c.target.zero_()
    c.theta_m.add_(1.0)
    c.load_state_dict(sd)
    for _ in range(3):
        c.train_epoch()
    torch.cuda.synchronize()
    assert a.counters() == c.counters() and a.updates == 12 and a.cursor == 0 and a.slots_written == 24
    for n, x, y in zip(NAMES, a.snapshot_tensors(), c.snapshot_tensors()):
        assert torch.equal(x, y), f"{n} differs after the resume"
    assert torch.equal(a.theta, c.theta) and torch.equal(a.target, c.target) and torch.equal(a.theta_v, c.theta_v)
    assert int(a.q.step.item()) == 12 and not torch.equal(a.theta, b.theta)
    # a noisy checkpoint and a plain trainer refuse each other by name
    plain = DQNTrainer(DQNConfig(**dict(TRAINER, **extra)), device=cuda)
    with pytest.raises(ValueError, match="noisy"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="noisy"):
        c.load_state_dict(plain.state_dict())
    old = plain.state_dict()
    del old["cfg"]["noisy"]  # a checkpoint from before the feature: a plain net
    with pytest.raises(ValueError, match="noisy"):
        c.load_state_dict(old)
    plain.load_state_dict(old)


# ------------------------------------------------------------------ 8. noisy=False is the trainer of before
def test_plain_trainer_calls_none_of_the_new_ops(cuda, monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("a plain trainer called a noisy op")

    ref_run = DQNTrainer(DQNConfig(**TRAINER), device=cuda)
    for _ in range(6):
        ref_run.train_epoch()
    for name in ("noisy_compose", "noisy_grad", "noisy_sigma_init"):
        monkeypatch.setattr(dt, name, boom)
    monkeypatch.setattr(hip(), "noisy_compose", boom)
    monkeypatch.setattr(hip(), "noisy_grad", boom)
    tr = DQNTrainer(DQNConfig(**TRAINER, noisy="false"), device=cuda)
    assert tr.theta is None and tr.target.numel() == tr.q.P
    for _ in range(6):
        tr.train_epoch()
    tr.evaluate(episodes=1, num_envs=8)
    torch.cuda.synchronize()
    assert tr.updates == 12 and len(tr.snapshot_tensors()) == 13
    for x, y in zip(tr.snapshot_tensors(), ref_run.snapshot_tensors()):
        assert torch.equal(x, y)
    sd = tr.state_dict()
    assert "noisy" not in sd and sd["cfg"]["noisy"] is False


# ------------------------------------------------------------------ 9. CLI
def test_noisy_preset_trains_evaluates_and_checkpoints(cuda, tmp_path):
    from relayrl_prototype_amd.runtime.launcher import EVAL_COLUMNS, ckpt_dir, run_evaluate, run_preset

    small = {k: v for k, v in TRAINER.items() if k != "max_episode_steps"}
    rows = []
    last = run_preset("cartpole-dqn-noisy", 4, str(tmp_path), overrides=small, eval_every=2, checkpoint_every=4,
                      eval_episodes=1, eval_envs=32, on_metrics=rows.append)
    assert len(rows) == 4 and last["Epoch"] == 4 and last["Updates"] == 8
    assert last["Noisy"] is True and last["Dueling"] is True and last["NStep"] == 3 and last["Epsilon"] == 0.0
    assert 0.0 < last["SigmaMeanAbs"] < 1.0
    for k in EVAL_COLUMNS:
        assert np.isfinite(rows[1][k]) and np.isfinite(last[k]), k
    ck = ckpt_dir(str(tmp_path), "cartpole-dqn-noisy", 0)
    assert os.path.exists(os.path.join(ck, "state.json"))
    out = run_evaluate(ck, episodes=64, num_envs=32)  # a noisy checkpoint's learner/pi/params is mu
    assert out["env"] == "CartPole-v1" and out["hidden"] == 64 and out["episodes"] == 64 and out["greedy"]
    assert out["checkpoint_epoch"] == 4 and 8.0 <= out["mean_return"] <= 500.0


# ------------------------------------------------------------------ 10. learning without epsilon
def test_noisy_trainer_learns_cartpole_without_epsilon(cuda):
    """The CPU oracle loop with noisy layers (tests/dqn_noisy_oracle.py: the same algorithm and Philox draws,
    float64 networks and noise) at do.SMALL with eps_start = eps_end = 0.  At noisy_sigma0 = 0.5 and 600 epochs its
    five seeds score 9.43, 9.57, 9.33, 11.96 and 9.46, which is no bar, so both sides run noisy_sigma0 = 0.7 for
    4,800 epochs = 9,594 updates (the oracle file has the search), where the oracle scores 216.63, 185.76, 395.91,
    144.53 and 234.09.  The GPU trainer at seed 1 must reach 80 % of the lowest."""
    tr = DQNTrainer(DQNConfig(**dn.NOISY_SMALL, seed=1, noisy_sigma0=dn.NOISY_SIGMA0), device=cuda)
    for _ in range(dn.NOISY_EPOCHS):
        tr.train_epoch()
    assert tr.updates == dn.NOISY_UPDATES == 9594
    got = tr.evaluate(episodes=1, num_envs=do.EVAL_EPISODES).stats()["mean_return"]
    floor = 0.8 * min(dn.ORACLE_RETURNS_NOISY.values())
    print(f"GPU greedy mean return {got:.2f}, floor {floor:.2f}, oracle {dn.ORACLE_RETURNS_NOISY}, "
          f"sigma {tr.metrics()['SigmaMeanAbs']:.4f}")
    assert floor >= 0.8 * 44.0 and got >= floor, (got, floor)
