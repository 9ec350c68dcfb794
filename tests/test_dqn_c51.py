"""The categorical (C51) head without a GPU: the rule for what is built and the host oracles of ops/reference.py."""
import numpy as np
import pytest
import torch

from relayrl_prototype_amd.models.mlp_spec import MLPSpec, c51_outputs
from relayrl_prototype_amd.ops import ReplayRing, dqn_targets
from relayrl_prototype_amd.ops import reference as ref

import dqn_c51_oracle as dc


@pytest.mark.parametrize("kw,match", [
    (dict(A=2, atoms=51, v_min=0, v_max=1, quantiles=4), "atoms.*quantiles"),
    (dict(A=2, atoms=51, v_min=0, v_max=1, dueling=True), "atoms.*dueling"),
    (dict(A=2, atoms=1, v_min=0, v_max=1), "atoms"),
    (dict(A=2, atoms=51, v_min=1, v_max=1), "v_min.*v_max"),
    (dict(A=2, atoms=65, v_min=0, v_max=1), "8 output tiles"),
    (dict(A=3, atoms=33, v_min=0, v_max=1), "8 output tiles"),
])
def test_c51_outputs_refuses_what_is_not_built(kw, match):
    with pytest.raises(ValueError, match=match):
        c51_outputs(**kw)


def test_c51_outputs_and_the_cpu_targets():
    assert c51_outputs(2, 51, 0, 100) == 102 and c51_outputs(4, 32, -1, 1) == 128 and c51_outputs(3, 17, -1, 1) == 51
    D, H, A, NA, B = 4, 64, 2, 5, 9
    gen = torch.Generator().manual_seed(1)
    ring = ReplayRing(torch.randn(3, 4, D, generator=gen), torch.randn(3, 4, D, generator=gen),
                      torch.randint(0, A, (3, 4), generator=gen, dtype=torch.int32), torch.randn(3, 4, generator=gen),
                      torch.randint(0, 3, (3, 4), generator=gen).float())
    net = MLPSpec(D, H, A * NA).init(gen)
    m = dqn_targets(net, net, H, A, ring, 12, 0.9, True, 1, 0, B, atoms=NA, v_min=-1.0, v_max=1.0)[2]  # the CPU reference
    assert m.shape == (B, NA) and torch.allclose(m.sum(-1), torch.ones(B), atol=1e-5)
    with pytest.raises(ValueError, match="floats"):
        dqn_targets(net, net, H, A, ring, 12, 0.9, True, 1, 0, B, atoms=NA + 1, v_min=-1.0, v_max=1.0)
    with pytest.raises(ValueError, match="quantiles"):
        dqn_targets(net, net, H, A, ring, 12, 0.9, True, 1, 0, B, atoms=NA, v_min=-1.0, v_max=1.0, quantiles=2)


@pytest.mark.parametrize("NA,v_min,v_max", [(51, 0.0, 100.0), (21, -1.0, 1.5), (3, -2.0, 2.0), (64, -10.0, 10.0)])
def test_projection_oracle(NA, v_min, v_max):
    """Mass is conserved to float64 rounding, the gather form equals the textbook l / u update wherever no b_j is an
    integer, and a terminal row (c = 0) puts all its mass at clamp(G)."""
    B = 40
    gen = torch.Generator().manual_seed(NA)
    p = torch.softmax(torch.randn(B, NA, generator=gen, dtype=torch.float64), -1)
    span = v_max - v_min
    G = v_min - 0.2 * span + 1.4 * span * torch.rand(B, generator=gen, dtype=torch.float64)  # past both ends too
    c = 0.97 * (torch.rand(B, generator=gen) < 0.7).double()                                 # 0: a terminal row
    m = ref.c51_project(p, G, c, v_min, v_max)
    assert float((m.sum(-1) - p.sum(-1)).abs().max()) <= 64 * 2.0 ** -52
    text, b = dc.project_textbook(p.numpy(), G.numpy(), c.numpy(), v_min, v_max)
    plain = (b != np.round(b)).all(-1)  # rows clamped at an end have an integer b_j
    assert plain.sum() >= 5
    np.testing.assert_allclose(m.numpy()[plain], text[plain], rtol=0, atol=1e-13)
    dropped = ~plain & (c.numpy() > 0)
    assert dropped.any() and (text[dropped].sum(-1) < 1 - 1e-6).all(), "the textbook form loses the clamped mass"
    term = c == 0
    dz = span / (NA - 1)
    bt = (G[term].clamp(v_min, v_max) - v_min) / dz
    want = (1 - (bt.unsqueeze(-1) - torch.arange(NA, dtype=torch.float64)).abs()).clamp(min=0)
    assert term.sum() >= 5 and torch.allclose(m[term], want, rtol=0, atol=1e-13)


def test_c51_q_float32_follows_float64():
    A, NA = 3, 21
    out = 3 * torch.randn(50, A * NA, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    q64, p64 = ref.c51_q(out, A, NA, -5.0, 7.0)
    z = torch.linspace(-5.0, 7.0, NA, dtype=torch.float64)
    want = torch.softmax(out.reshape(50, A, NA), -1)
    assert torch.allclose(p64, want, atol=1e-14) and torch.allclose(q64, (want * z).sum(-1), atol=1e-12)
    q32, p32 = ref.c51_q(out.float(), A, NA, -5.0, 7.0)
    assert q32.dtype == torch.float32 and float((q32.double() - q64).abs().max()) < 1e-5
    assert float((p32.double() - p64).abs().max()) < 1e-6


@pytest.mark.parametrize("kw,match", [
    (dict(atoms=51, v_min=0, v_max=1, quantiles=4), "atoms.*quantiles"),
    (dict(atoms=51, v_min=0, v_max=1, dueling=True), "atoms.*dueling"),
    (dict(atoms=51, v_min=0, v_max=1, noisy=True), "atoms.*noisy"),
    (dict(atoms=1, v_min=0, v_max=1), "atoms"),
    (dict(atoms=-3, v_min=0, v_max=1), "atoms"),
    (dict(atoms=2.5, v_min=0, v_max=1), "atoms"),
    (dict(atoms=51, v_min=1, v_max=1), "v_min.*v_max"),
    (dict(atoms=65, v_min=0, v_max=1), "8 output tiles"),
])
def test_dqn_config_refuses_what_the_categorical_head_does_not_build(kw, match):
    from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig

    with pytest.raises(ValueError, match=match):
        DQNConfig(**kw)
    from relayrl_prototype_amd.runtime.launcher import PRESETS
    c51 = dict(PRESETS["cartpole-dqn-nstep"].overrides, atoms=51, v_min=0.0, v_max=100.0)
    assert PRESETS["cartpole-dqn-c51"].overrides == c51 and DQNConfig().atoms == 0 and DQNConfig(atoms="51", v_max=1).atoms == 51
