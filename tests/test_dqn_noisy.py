"""NoisyNet exploration on the CPU: the DQNConfig fields and the preset, the structure of the noise reference
(ops/noisy.py), the normality of its unit normals, and the fp32 Box-Muller held to its derived bound against
float64 on the same Philox words, over every unit the GPU tests draw."""
import math

import numpy as np
import pytest
import torch

from relayrl_prototype_amd.ops import MLPSpec, noisy_compose, noisy_compose_ref, noisy_eps_ref, noisy_grad
from relayrl_prototype_amd.ops import noisy_grad_ref, noisy_num_units, noisy_sigma_init, noisy_units_ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig, dqn_noise_seed, dqn_seeds

import dqn_noisy_oracle as dn

KEY = dn.KEY


# ------------------------------------------------------------------ 1. config and preset
def test_config_parses_noisy():
    assert DQNConfig().noisy is False and DQNConfig().noisy_sigma0 == 0.5
    for word, want in (("true", True), ("false", False), (" Yes ", True), ("0", False)):
        assert DQNConfig(noisy=word).noisy is want, word
    with pytest.raises(ValueError, match="noisy"):
        DQNConfig(noisy="maybe")
    assert DQNConfig(noisy="true", noisy_sigma0="0.25").noisy_sigma0 == 0.25
    assert DQNConfig(noisy_sigma0=0).noisy_sigma0 == 0.0
    for bad in (-0.1, "-1", float("nan")):
        with pytest.raises(ValueError, match="noisy_sigma0"):
            DQNConfig(noisy_sigma0=bad)
    cfg = DQNConfig(**DQNConfig(noisy=True, dueling=True, noisy_sigma0=0.3).to_dict())  # a checkpoint's cfg
    assert cfg.noisy and cfg.dueling and cfg.noisy_sigma0 == 0.3


def test_noisy_preset_and_engine_resolution():
    from relayrl_prototype_amd.runtime import engine as eng
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    p, duel = PRESETS["cartpole-dqn-noisy"], PRESETS["cartpole-dqn-dueling"]
    assert p.kind == "vec" and p.overrides == dict(duel.overrides, noisy=True, eps_start=0.0, eps_end=0.0)
    assert "noisy" not in duel.overrides
    cfg = DQNConfig(**p.overrides)
    assert cfg.noisy and cfg.dueling and cfg.n_step == 3 and cfg.prioritized and cfg.noisy_sigma0 == 0.5
    spec = eng.resolve_engine("DQN", 4, 2, {}, {}, {"noisy": "true"}, engine="vec")
    cfg = DQNConfig(**eng._filter(DQNConfig, spec.trainer))
    assert cfg.noisy is True and not cfg.dueling


def test_noise_key_is_a_fourth_stream():
    for seed in (0, 1, 7, 2 ** 40 + 3):
        keys = dqn_seeds(seed)
        assert len(keys) == 3  # the tuple did not grow
        k = dqn_noise_seed(seed)
        assert 0 <= k < 2 ** 63 and (seed == 0 or k not in keys)
    assert dqn_noise_seed(1) != dqn_noise_seed(2)


# ------------------------------------------------------------------ 2. structure of the reference
def test_sigma_init_is_sigma0_over_sqrt_fan_in():
    spec = MLPSpec(6, 64, 3)
    s = noisy_sigma_init(spec, 0.5)
    o = spec.offsets()
    assert s.dtype == torch.float32 and s.numel() == spec.P
    assert torch.equal(s[:o["w2"]], torch.full((o["w2"],), 0.5 / math.sqrt(6)))  # W1 and b1
    assert torch.equal(s[o["w2"]:], torch.full((spec.P - o["w2"],), 0.5 / math.sqrt(64)))  # layers 2 and 3
    assert bool((noisy_sigma_init(spec, 0.0) == 0).all())
    with pytest.raises(ValueError, match="noisy_sigma0"):
        noisy_sigma_init(spec, -1.0)


@pytest.mark.parametrize("D,H,A", dn.SHAPES)
def test_eps_is_the_outer_product_of_the_unit_factors(D, H, A):
    spec = MLPSpec(D, H, A)
    U = noisy_num_units(spec)
    assert U == D + 4 * H + A
    n, f = noisy_units_ref(KEY, 1, 5, spec, np.float32)
    assert n.dtype == np.float32 and f.dtype == np.float32 and n.shape == f.shape == (U,)
    assert np.array_equal(f, np.copysign(np.sqrt(np.abs(n)), n))
    f = torch.from_numpy(f)
    eps = noisy_eps_ref(f, spec)
    assert eps.dtype == torch.float32 and eps.numel() == spec.P
    o = spec.offsets()
    cuts = [0, D, D + H, D + 2 * H, D + 3 * H, D + 4 * H, U]
    blk = [f[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    for l, (w, b, rows, cols) in enumerate((("w1", "b1", H, D), ("w2", "b2", H, H), ("w3", "b3", A, H))):
        f_in, f_out = blk[2 * l], blk[2 * l + 1]
        W = eps[o[w]:o[w] + rows * cols].view(rows, cols)
        assert torch.equal(W, f_out[:, None] * f_in[None, :]), w  # one fp32 multiply per weight
        assert torch.equal(eps[o[b]:o[b] + rows], f_out), b
    # the CPU path of the op is this reference
    theta = torch.cat([spec.init(torch.Generator().manual_seed(1)), noisy_sigma_init(spec, 0.5)])
    units = torch.zeros(1, U)
    out = noisy_compose(theta, (1,), (5,), spec, KEY, units_out=units)
    assert torch.equal(units[0], f) and torch.equal(out[0], theta[:spec.P] + theta[spec.P:] * eps)
    assert torch.equal(out[0], noisy_compose_ref(theta, f, spec))
    slab = torch.randn(3, spec.P, generator=torch.Generator().manual_seed(2))
    g = noisy_grad(slab, 1, 5, spec, KEY)
    want = (slab[0] + slab[1]) + slab[2]
    assert torch.equal(g[:spec.P], want) and torch.equal(g[spec.P:], want * eps)
    assert torch.equal(g, noisy_grad_ref(slab, eps))


def test_roles_and_draws_are_independent_samples():
    spec = MLPSpec(4, 128, 3)

    def n(role, draw):
        return noisy_units_ref(KEY, role, draw, spec)[0]

    roles = [n(r, 5) for r in range(4)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not np.any(roles[i] == roles[j]), (i, j)
    assert not np.any(n(1, 5) == n(1, 6))
    assert not np.any(n(1, 5) == n(1, 2 ** 32 + 5)), "the high counter word is ignored"
    assert np.array_equal(n(1, 5), n(1, 5))
    assert not np.any(n(1, 5) == noisy_units_ref(KEY ^ (1 << 40), 1, 5, spec)[0]), "the high key word is ignored"
    for bad in (-1, 4):
        with pytest.raises(ValueError, match="role"):
            noisy_units_ref(KEY, bad, 0, spec)
    # within one sample no two sides or layers share a stream: in2 and out1 have equal counts and differ
    D, H = spec.D, spec.H
    one = n(0, 0)
    assert not np.any(one[D:D + H] == one[D + H:D + 2 * H])


def test_unit_normals_are_standard_normal():
    """4,096 reference normals (8 draws of the 512 units of in2 .. in3 at H = 128): 5-sigma bounds on the mean
    (sd 1 / sqrt(n)) and the variance (sd sqrt(2 / n))."""
    spec = MLPSpec(4, 128, 3)
    x = np.concatenate([noisy_units_ref(KEY, 0, d, spec)[0][spec.D:spec.D + 512] for d in range(8)])
    assert x.size == 4096
    assert abs(x.mean()) <= 5 / math.sqrt(4096)
    assert abs(x.var() - 1.0) <= 5 * math.sqrt(2 / 4096)


# ------------------------------------------------------------------ 3. the fp32 noise against float64
def test_fp32_box_muller_is_within_its_bound_of_float64():
    """|n32 - n64| <= 2e-5 on the same Philox words: 1 - u0 is exact in fp32; the radius is at most
    sqrt(-2 ln 2^-24) = 5.77; the angle 2 pi u1 carries at most 2 * 2^-24 * 6.28 = 7.5e-7 absolute error, so the
    cosine is off by about 1e-6, about 6e-6 on n; a few ulp of relative error from logf, the multiply and sqrtf
    add about 2.5e-6; the bound is twice the sum.  Every unit, role and draw of the GPU tests' shapes is here,
    so the reference alone is known to pass before any GPU run; the factors are then within UNIT_TOL."""
    worst = worst_f = 0.0
    for D, H, A in dn.SHAPES:
        spec = MLPSpec(D, H, A)
        for role in range(4):
            for draw in dn.DRAWS:
                n64, _ = noisy_units_ref(KEY, role, draw, spec, np.float64)
                n32, f32 = noisy_units_ref(KEY, role, draw, spec, np.float32)
                assert np.isfinite(n32).all() and np.abs(n64).max() <= 5.77
                worst = max(worst, float(np.abs(n32.astype(np.float64) - n64).max()))
                f = f32.astype(np.float64)
                worst_f = max(worst_f, float(np.abs(np.sign(f) * f * f - n64).max()))
    print(f"max |n32 - n64| = {worst:.3e}, max |sgn(f) f^2 - n64| = {worst_f:.3e}")
    assert worst <= dn.N32_TOL and worst_f <= dn.UNIT_TOL


# ------------------------------------------------------------------ 4. the learning oracle's record
def test_oracle_returns_are_a_bar():
    """The GPU learning test asks for 80 % of the lowest of the five oracle returns: that is a bar only if the
    lowest is at least twice a random policy's 22."""
    assert sorted(dn.ORACLE_RETURNS_NOISY) == [1, 2, 3, 4, 5]
    assert min(dn.ORACLE_RETURNS_NOISY.values()) >= 44.0
    cfg = DQNConfig(**dn.NOISY_SMALL, noisy_sigma0=dn.NOISY_SIGMA0)
    assert cfg.noisy and cfg.eps_start == cfg.eps_end == 0.0
