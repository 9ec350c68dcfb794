"""Lambda-return targets without a GPU: the reference on a walk computed by hand, the two limits, the rule, the preset
and the config."""
import pytest
import torch

from relayrl_prototype_amd.ops import MLPSpec, ReplayRing, dqn_targets
from relayrl_prototype_amd.ops.dqn import dqn_lambda_y_ref
from relayrl_prototype_amd.runtime.dqn_trainer import DQNConfig

from test_dqn_lambda_gpu import C, N, NEWEST, REFUSALS, lam_case  # the GPU test's host ring, nets and refused calls


def hand_net(w3, b3):
    """Q(x) = w3 * relu(x) + b3 on MLPSpec(1, 64, 2): the only live path is input 0 -> unit 0 -> unit 0."""
    o, p = MLPSpec(1, 64, 2).offsets(), torch.zeros(MLPSpec(1, 64, 2).P, dtype=torch.float64)
    p[o["w1"]] = p[o["w2"]] = 1.0
    p[o["w3"]], p[o["w3"] + 64], p[o["b3"]], p[o["b3"] + 1] = *w3, *b3
    return p


def test_lambda_return_by_hand():
    """gamma = lam = 0.5: gl = g1 = 0.25.  Two envs walk slots 0, 1, 2 (rew 1, 2, 3; nobs 1, 0.25, 2); env 0 ends on a
    truncation (gb = 0.5), env 1 on a terminal (gb = 0).  Q_target(x) = [x + 0.5, 2 x]: V = 2, 0.75, 4."""
    nobs = torch.tensor([1.0, 0.25, 2.0, 9.0], dtype=torch.float64).reshape(4, 1, 1).expand(4, 2, 1)
    rew = torch.tensor([1.0, 2.0, 3.0, 9.0], dtype=torch.float64).reshape(4, 1).expand(4, 2)
    done = torch.tensor([[0.0, 0.0], [0.0, 0.0], [2.0, 1.0], [0.0, 0.0]])
    ring = ReplayRing(torch.zeros(4, 2, 1), nobs, torch.zeros(4, 2, dtype=torch.int32), rew, done)
    target, online = hand_net((1.0, 2.0), (0.5, 0.0)), hand_net((1.0, 0.0), (0.5, 0.0))
    tail = ([0, 1], 3, 3, 0.5, False, torch.float64)  # rows, newest, n_step, lam
    # t = 0.25 * 2 + 1 = 1.5;  0.25 * 0.75 + 2 = 2.1875;  0.5 * 4 + 3 = 5 or 0 * 4 + 3 = 3;  y = t0 + t1 / 4 + t2 / 16
    got = dqn_lambda_y_ref(None, target, 64, 2, ring, 8, 0.5, False, *tail)
    assert got.tolist() == [1.5 + 0.546875 + 0.3125, 1.5 + 0.546875 + 0.1875]
    # double Q: the online net always picks action 0, V = x + 0.5 = 1.5, 0.75, 2.5:  t = 1.375; 2.1875; 4.25 or 3
    got = dqn_lambda_y_ref(online, target, 64, 2, ring, 8, 0.5, True, *tail)
    assert got.tolist() == [1.375 + 0.546875 + 0.265625, 1.375 + 0.546875 + 0.1875]


@pytest.mark.parametrize("double_q,dueling", [(False, False), (True, True)])
def test_cpu_limits(double_q, dueling):
    ring, online, target = lam_case(3, 6, 128, dueling)
    args = (online, target, 128, 3, ring, C * N, 0.9, double_q, 1, 0, 40)
    kw = dict(dtype=torch.float64, dueling=dueling)
    nstep, zero, near, one = (dqn_targets(*args, n_step=3, newest=NEWEST, q_lambda=lam, **kw)
                              for lam in (1.0, 0.0, 1.0 - 2.0 ** -24, 1))
    assert float((zero[2] - dqn_targets(*args, **kw)[2]).abs().max()) < 1e-12  # lam = 0: the one-step target
    assert all(torch.equal(x, y) for i, (x, y) in enumerate(zip(zero, nstep)) if i != 2) and not torch.equal(zero[2], nstep[2])
    # lam -> 1: every term moves by at most 3 * (1 - lam) = 1.8e-7 of |rew| + |V| < 200
    assert 0.0 < float((near[2] - nstep[2]).abs().max()) < 4e-5 and torch.equal(one[2], nstep[2])
    assert torch.equal(nstep[2], dqn_targets(*args, n_step=3, newest=NEWEST, **kw)[2])  # the default is the n-step call


def test_config_preset_and_refusals():
    from relayrl_prototype_amd.runtime.launcher import PRESETS

    assert PRESETS["cartpole-dqn-lambda"].overrides == dict(PRESETS["cartpole-dqn-nstep"].overrides, n_step=5, q_lambda=0.7)
    cfg = DQNConfig(n_step="5", q_lambda="0.7", prioritized="true", dueling="true", noisy="true")  # strings from a server
    assert (cfg.n_step, cfg.q_lambda) == (5, 0.7) and DQNConfig(**cfg.to_dict()) == cfg and cfg.to_dict()["q_lambda"] == 0.7
    assert DQNConfig().q_lambda == 1.0 and DQNConfig(q_lambda=1, quantiles=8).q_lambda == 1.0  # 1 goes with every head
    ring, _, target = lam_case(2, 4, 64, False)
    for bad, match in REFUSALS + [(dict(q_lambda="nan"), "q_lambda")]:
        with pytest.raises(ValueError, match=match):  # the soft target goes without double_q
            DQNConfig(**dict(dict(n_step=3, double_q=False), **bad))
        with pytest.raises(ValueError, match=match):  # the targets call has the same rule
            dqn_targets(None, target, 64, 2, ring, C * N, 0.9, False, 1, 0, 5, **dict(dict(n_step=3, newest=NEWEST), **bad))
