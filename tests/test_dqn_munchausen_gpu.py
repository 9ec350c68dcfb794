"""Munchausen targets on the GPU: dqn_soft_targets_kernel (csrc/kernels/dqn.hip) against ``dqn_targets_ref`` in float64
within BOUND_FACTOR times the float32 reference's own error at the same case, every other output bit-equal to a
hard-max launch on the same ring, key and update, and the trainer built on it.  Every output buffer is guarded."""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import MLPSpec, ReplayRing, dqn_targets, dqn_targets_ref, hip
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, DQNTrainer

from guarded import DEV, Guarded
from test_dqn_gpu import TRAINER, guarded_ring
from test_dqn_quantile_gpu import same_bits, untouched
from test_per_gpu import guarded_tree, random_leaves

pytestmark = pytest.mark.gpu

C, N, B, BOUND_FACTOR = 6, 17, 65, 4.0  # 102 ring rows; a full workgroup pass of 64 batch rows plus one row in a second
GAMMA, BETA, SEED, UPDATE, ALPHA, CLIP = 0.97, 0.7, (3 << 32) | 5, 2 ** 32 + 7, 0.9, -1.0
# on the output layer, times sqrt(NQ) for the mean of NQ quantiles: Q-values a few units apart, so that the float64
# reference clips the bonus on 21 to 43 of the 65 rows at tau = 0.03, whatever the shape and the sampler
GAIN = 32.0
SHAPES = [(2, 0, 4, 64), (4, 0, 8, 128), (2, 8, 4, 128), (3, 5, 6, 64)]  # (A, NQ, D, H)


def soft_case(A, NQ, D, H, gain=GAIN):
    gain = gain * max(NQ, 1) ** 0.5
    gen = torch.Generator().manual_seed(1000 * H + 10 * A + NQ)
    host = ReplayRing(torch.randn(C, N, D, generator=gen), torch.randn(C, N, D, generator=gen),
                      torch.randint(0, A, (C, N), generator=gen, dtype=torch.int32), torch.randn(C, N, generator=gen),
                      torch.randint(0, 3, (C, N), generator=gen).float())
    assert all(set(host.done[c].unique().tolist()) == {0.0, 1.0, 2.0} for c in range(C))
    return host, MLPSpec(D, H, A * max(NQ, 1)).init(gen, out_gain=gain)


def launch(host, target, H, A, NQ, tree, n_step, **soft):
    g, ring = guarded_ring(C, N, host.obs.shape[-1])
    for dst, src in zip(ring, host):
        dst.copy_(src)
    out = (Guarded((B, ring.obs.shape[-1])), Guarded((B,), torch.int32), Guarded((B, NQ) if NQ else (B,)),
           Guarded((B,), torch.int32))
    kw = dict(quantiles=NQ, **soft)
    if tree is not None:
        out += (Guarded((B,)), Guarded((1,)))
        kw.update(tree=tree, beta=BETA)
    if n_step > 1:
        out += (Guarded((B,), torch.int32),)
        kw.update(n_step=n_step, newest=C - 1)
    dqn_targets(None, target.to(DEV), H, A, ring, C * N, GAMMA, False, SEED, UPDATE, B, out=tuple(o.t for o in out), **kw)
    torch.cuda.synchronize()
    assert all(o.guards_intact() for o in out) and all(b.guards_intact() for b in g.values())
    return out


def y_refs(host, target, H, A, NQ, tree, n_step, **soft):
    kw = dict(tree=tree, beta=BETA if tree is not None else None, n_step=n_step, newest=C - 1, quantiles=NQ, **soft)
    r64, r32 = (dqn_targets_ref(None, target, H, A, host, C * N, GAMMA, False, SEED, UPDATE, B, dtype=dt, **kw)
                for dt in (torch.float64, torch.float32))
    return r64[2], r64[3], BOUND_FACTOR * float((r32[2].double() - r64[2]).abs().max())


@pytest.mark.parametrize("tau", [0.03, 1.0])
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("sampler", ["uniform", "tree"])
@pytest.mark.parametrize("A,NQ,D,H", SHAPES)
def test_soft_targets(cuda, A, NQ, D, H, sampler, n_step, tau):
    host, target = soft_case(A, NQ, D, H)
    tree = guarded_tree(random_leaves(C * N, C * N, 7 + A), 1.0)[2].tree if sampler == "tree" else None
    soft = dict(munchausen=ALPHA, m_tau=tau, m_clip=CLIP)
    y64, rows, bound = y_refs(host, target, H, A, NQ, None if tree is None else tree.cpu(), n_step, **soft)
    if tau == 0.03:  # both sides of the clip, by the float64 reference
        out0 = ref.trunk(target.double(), host.obs.reshape(-1, D)[rows].double(), D, H, A * max(NQ, 1))[0]
        q0 = ref.quantile_q(out0, A, NQ) / NQ if NQ else out0
        taken = host.act.reshape(-1)[rows].long().unsqueeze(-1)
        clipped = ref.munchausen_terms(q0, tau)[0].gather(-1, taken).squeeze(-1) <= CLIP
        assert 4 * int(clipped.sum()) >= B and 4 * int((~clipped).sum()) >= B
    out = launch(host, target, H, A, NQ, tree, n_step, **soft)
    err = float((out[2].t.cpu().double() - y64).abs().max())
    print(f"A = {A} NQ = {NQ} H = {H} {sampler} n = {n_step} tau = {tau}: kernel error {err:.3e}, bound {bound:.3e}")
    assert bool(torch.isfinite(out[2].t).all()) and err <= bound
    hard = launch(host, target, H, A, NQ, tree, n_step)
    for i in range(len(out)):  # the soft target changes y alone
        assert i == 2 or same_bits(out[i], hard[i]), i


def test_soft_targets_tend_to_the_hard_max(cuda):
    """alpha = 0 is the hard-max launch itself; a clip of -1e-30 leaves no bonus and runs the soft kernel."""
    A, NQ, D, H, tau = 4, 0, 8, 128, 1e-3
    host, target = soft_case(A, NQ, D, H, gain=40.0)
    top = torch.topk(ref.trunk(target.double(), host.nobs.reshape(-1, D).double(), D, H, A)[0], 2, dim=-1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 20 * tau  # well separated
    hard = launch(host, target, H, A, NQ, None, 3)
    for soft in (dict(munchausen=0.0, m_tau=tau), dict(munchausen=ALPHA, m_tau=tau, m_clip=-1e-30)):
        bound = y_refs(host, target, H, A, NQ, None, 3, **soft)[2]
        out = launch(host, target, H, A, NQ, None, 3, **soft)
        err = float((out[2].t - hard[2].t).abs().max())
        assert err <= bound, (soft, err, bound)


@pytest.mark.parametrize("bad,match", [
    (dict(munchausen=1.5), "munchausen"), (dict(munchausen=-0.1), "munchausen"),
    (dict(munchausen=ALPHA, m_tau=0.0), "m_tau"), (dict(munchausen=ALPHA, m_clip=0.0), "m_clip"),
    (dict(munchausen=ALPHA, double_q=True), "double_q"), (dict(munchausen=ALPHA, dueling=True), "dueling"),
    (dict(munchausen=ALPHA, atoms=51, v_min=0.0, v_max=1.0), "atoms"),
])
def test_soft_target_refusals_write_nothing(cuda, bad, match):
    A, D, H = 2, 4, 64
    ring = guarded_ring(C, N, D)[1]
    net = MLPSpec(D, H, A).init(torch.Generator().manual_seed(1)).to(DEV)  # the rule is judged before the nets' sizes
    out = (Guarded((B, D)), Guarded((B,), torch.int32), Guarded((B,)), Guarded((B,), torch.int32))
    kw = dict(bad)
    double_q = kw.pop("double_q", False)
    with pytest.raises(ValueError, match=match):
        dqn_targets(net, net, H, A, ring, C * N, GAMMA, double_q, SEED, UPDATE, B, out=tuple(o.t for o in out), **kw)
    with pytest.raises(RuntimeError, match=match):  # the binding's own check
        hip().dqn_targets(net, net, H, A, *ring, C * N, GAMMA, double_q, SEED, UPDATE, *(o.t for o in out), **kw)
    torch.cuda.synchronize()
    untouched(*out)


def test_munchausen_preset_trains_resumes_evaluates_and_names_its_checkpoints(cuda, tmp_path):
    from relayrl_prototype_amd.runtime.launcher import ckpt_dir, run_evaluate, run_preset

    small = {k: v for k, v in TRAINER.items() if k != "max_episode_steps"}
    last = run_preset("cartpole-dqn-munchausen", 4, str(tmp_path), overrides=small, checkpoint_every=4)
    assert last["Epoch"] == 4 and last["Updates"] == 8 and last["NStep"] == 3 and np.isfinite(last["LossQ"])
    scored = run_evaluate(ckpt_dir(str(tmp_path), "cartpole-dqn-munchausen", 0), episodes=64, num_envs=32)
    assert scored["episodes"] == 64 and scored["checkpoint_epoch"] == 4 and 8.0 <= scored["mean_return"] <= 500.0
    kw = dict(TRAINER, double_q=False, prioritized=True, n_step=3, munchausen=ALPHA)
    a, b, c = (DQNTrainer(DQNConfig(**kw), device=cuda) for _ in range(3))
    for tr, epochs in ((a, 6), (b, 3)):
        for _ in range(epochs):
            tr.train_epoch()
    sd = b.state_dict()
    c.q.params.add_(1.0)  # other weights until the load
    c.load_state_dict(sd)
    for _ in range(3):
        c.train_epoch()
    torch.cuda.synchronize()
    assert a.counters() == c.counters() and a.updates > 0
    assert all(torch.equal(x, y) for x, y in zip(a.snapshot_tensors(), c.snapshot_tensors())), "the resume differs"
    hard = DQNTrainer(DQNConfig(**dict(kw, munchausen=0.0)), device=cuda)
    for tr, other in ((hard, sd), (c, hard.state_dict())):  # refused by name in both directions
        with pytest.raises(ValueError, match="munchausen"):
            tr.load_state_dict(other)
