"""Munchausen targets without a GPU: the soft-policy terms, ``dqn_targets_ref``, the rule, the presets and the config."""
import math

import pytest
import torch

from relayrl_prototype_amd.ops import dqn_targets
from relayrl_prototype_amd.ops import reference as ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig

from test_dqn_munchausen_gpu import C, N, soft_case  # the GPU test's host ring and target net


def test_munchausen_terms_by_hand():
    tlp, pi = ref.munchausen_terms(torch.tensor([1.0, 3.0, 2.0], dtype=torch.float64), 0.5)
    S = math.exp(-4.0) + 1.0 + math.exp(-2.0)  # d = -2, 0, -1 over tau = 0.5
    want_pi = torch.tensor([math.exp(-4.0) / S, 1.0 / S, math.exp(-2.0) / S], dtype=torch.float64)
    want_tlp = torch.tensor([-2.0, 0.0, -1.0], dtype=torch.float64) - 0.5 * math.log(S)
    assert torch.allclose(pi, want_pi, rtol=0, atol=1e-15) and torch.allclose(tlp, want_tlp, rtol=0, atol=1e-15)
    q = 30 * torch.randn(200, 5, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for tau in (1e-3, 0.03, 1.0):  # no overflow and no log of a vanished pi at any temperature
        tlp, pi = ref.munchausen_terms(q, tau)
        assert bool(torch.isfinite(tlp).all()) and bool((tlp <= 0).all())
        assert float((pi.sum(-1) - 1).abs().max()) <= 1e-14


@pytest.mark.parametrize("NQ,n_step", [(0, 1), (0, 3), (5, 3)])
def test_cpu_targets_tend_to_the_hard_max(NQ, n_step):
    """With a vanishing bonus the soft target goes to the hard-max one as tau -> 0 (on the quantile net: the quantiles
    of the action with the largest mean, which is what the hard-max target takes); alpha = 0 is the hard-max call."""
    ring, net = soft_case(3, NQ, 6, 64)
    args = (None, net, 64, 3, ring, C * N, 0.9, False, 1, 0, 12)
    kw = dict(dtype=torch.float64, quantiles=NQ, n_step=n_step, newest=C - 1)
    hard = dqn_targets(*args, **kw)
    assert torch.equal(dqn_targets(*args, munchausen=0.0, m_tau=1e-3, **kw)[2], hard[2])
    gaps = [float((dqn_targets(*args, munchausen=0.9, m_tau=tau, m_clip=-1e-30, **kw)[2] - hard[2]).abs().max())
            for tau in (1.0, 0.1, 1e-3)]
    assert gaps[0] > gaps[1] > gaps[2] and gaps[2] < 1e-9, gaps
    soft = dqn_targets(*args, munchausen=0.9, m_tau=0.03, **kw)
    assert soft[2].shape == hard[2].shape and not torch.equal(soft[2], hard[2])
    assert all(torch.equal(s, h) for i, (s, h) in enumerate(zip(soft, hard)) if i != 2)


@pytest.mark.parametrize("kw,match", [
    (dict(munchausen=1.5), "munchausen"), (dict(munchausen=-0.5), "munchausen"), (dict(munchausen="much"), "munchausen"),
    (dict(munchausen=0.9), "munchausen.*double_q"),  # double_q is on by default
    (dict(munchausen=0.9, double_q=False, m_tau=0.0), "m_tau"), (dict(munchausen=0.9, double_q=False, m_clip=0.0), "m_clip"),
    (dict(munchausen=0.9, double_q=False, dueling=True), "munchausen.*dueling"),
    (dict(munchausen=0.9, double_q=False, atoms=51, v_max=1.0), "munchausen.*atoms"),
])
def test_dqn_config_refuses_what_the_soft_target_does_not_build(kw, match):
    with pytest.raises(ValueError, match=match):
        DQNConfig(**kw)
    ring, net = soft_case(2, 0, 4, 64)
    with pytest.raises(ValueError, match="double_q"):  # the targets call has the same rule
        dqn_targets(net, net, 64, 2, ring, C * N, 0.9, True, 1, 0, 5, munchausen=0.9)


def test_presets_and_config_round_trip():
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    soft = dict(double_q=False, munchausen=0.9)
    assert PRESETS["cartpole-dqn-munchausen"].overrides == dict(PRESETS["cartpole-dqn-nstep"].overrides, **soft)
    assert PRESETS["cartpole-dqn-munchausen-qr"].overrides == dict(PRESETS["cartpole-dqn-quantile"].overrides, **soft)
    cfg = DQNConfig(double_q="false", munchausen="0.9", m_tau="0.05", m_clip=-2)  # a TrainingServer sends strings
    assert (cfg.munchausen, cfg.m_tau, cfg.m_clip) == (0.9, 0.05, -2.0)
    assert DQNConfig(**cfg.to_dict()) == cfg
    off = DQNConfig(m_clip=1.0)  # not judged while the soft target is off
    assert (off.munchausen, off.m_tau, DQNConfig().m_clip) == (0.0, 0.03, -1.0)
