"""DQN on the device: epsilon-greedy fused actor -> replay ring in HBM -> sampled TD updates.

One epoch (single rank, eager launches):

  1. ``dqn_rollout``: T steps x N envs of Q-network forward + epsilon-greedy action + env physics,
     written into T slots of a ring of ``buffer_slots`` (csrc/kernels/dqn.hip).  The host owns the
     epsilon schedule (linear, ``eps_start`` -> ``eps_end`` over ``eps_decay_epochs``) and the cursor.
  2. once ``slots_written * N >= learning_starts``: ``updates_per_epoch`` x
       ``dqn_targets``  sample + gather + TD target from the target (and online: double Q) network
       ``mlp_grad(Q_TD)``  fused forward + Huber head + backward  (csrc/kernels/mlp_grad.hip)
       ``adam_step``  slab-summing fused Adam
     and every ``target_update_every`` updates the target network copies the online one.

Every random draw is Philox at explicit coordinates (env streams: (env, global step); replay
samples: (batch row, update)), so a run is a pure function of the seed and ``state_dict()`` /
``load_state_dict()`` resume it bit for bit.  The API mirrors ``VecTrainer``.

``prioritized=True`` is prioritised experience replay (Schaul et al., proportional variant) on the
device: a priority sum tree over the ring's rows (csrc/kernels/per.hip, ops/per.py) in which every node
is one fp32 add of its children, so it is reproducible on any grid and rebuilt bit for bit from its
leaves.  The epoch becomes: rollout, ``per_insert`` of the slots just written (at the running maximum
priority), and per update ``dqn_targets`` (prioritised: rows from the tree, importance weights w and
their maximum), ``mlp_grad(Q_TD, row_w, w_norm, td_abs)``, Adam, ``per_update`` of the sampled rows to
``(|td| + per_eps)^per_alpha``.  The host owns the beta anneal (``beta_at``) like the epsilon schedule.

``n_step > 1`` turns the TD target into the n-step return.  The ring is time-major, so the successor of a
transition is the same env in the next slot: ``dqn_targets`` walks the sampled row forward through the ring
before the bootstrap forward pass, summing discounted rewards until n steps, an episode end (a terminal
drops the bootstrap, a truncation keeps it) or the newest slot, ``(cursor - 1) % buffer_slots``.  No row is
excluded from sampling and nothing new is stored: the actor, the ring, the samplers, the tree and the
checkpoint are those of one-step DQN, and ``n_step = 1`` runs its kernels.

``dueling=True`` is the dueling network of Wang et al. 2016: Q(s, a) = V(s) + A(s, a) - mean_a' A(s, a').  The
online and target nets are ``MLPSpec(D, H, A + 1)`` (output rows 0 .. A-1 the advantages, row A the state
value, so A <= 15); the actor and the evaluator act on the argmax of the advantage outputs, ``dqn_targets``
bootstraps from the dueling Q of the target net and the update is ``mlp_grad(Q_DUEL)``.  Both streams are
LINEAR on the shared trunk h2 (no separate stream hidden layers), so such a head folds exactly into a plain
A-output layer, ``W3'[a] = W3[a] + W3[A] - mean_k W3[k]`` (and ``b3'`` alike): the function class is that of
the plain net and what changes is the gradient, which moves the state value of every action with each sampled
transition.  Separate stream layers are left out.  It composes with ``double_q``, ``prioritized`` and
``n_step``; ``dueling=False`` launches the kernels it always launched.

``noisy=True`` is NoisyNet exploration (Fortunato et al. 2018, factorised Gaussian noise; ops/noisy.py has the
contract): all three layers are ``W = mu + sigma * eps``, ``theta = [mu; sigma]`` (2P, with Adam state of 2P) is what
is trained and ``target`` is a 2P copy.  The big kernels do not change: ``rollout()`` composes the role-0 sample
of draw = epoch (one for all envs and all T steps) into a buffer and hands that to ``dqn_rollout``; ``update()``
composes roles 1, 2 and 3 (the loss, the target net, the selecting net of double Q) at draw = updates in one
launch, and after ``dqn_targets`` and ``mlp_grad`` on those buffers ``noisy_grad`` turns the slabs into the
gradient of ``theta`` for Adam's ``grad=`` path.  ``epsilon`` still applies (the ``cartpole-dqn-noisy`` preset sets
it to 0), ``evaluate()`` scores ``mu``, and a checkpoint keeps ``mu`` where the plain parameters were
(``learner/pi``, ``learner/target``) and sigma with its Adam moments under ``noisy``.  ``noisy=False`` calls none of
this and launches the kernels it always launched.

``quantiles = NQ >= 1`` is the distributional head of QR-DQN (Dabney et al. 2018): the online and target nets are
``MLPSpec(D, H, A * NQ)``, output ``a * NQ + i`` the quantile of action ``a`` at level ``(2 i + 1) / (2 NQ)``, and
at most 16 outputs (CartPole: 8 quantiles, LunarLanderSynth: 4).  The actor and the evaluator act on the argmax of
the per-action quantile SUMS (``reference.quantile_q``: ascending adds, no division), ``dqn_targets`` writes
``y [B, NQ]``, the n-step target applied to each quantile of the target net at ``a*``, and the update is
``mlp_grad_qr``, the quantile-Huber loss with kappa = ``huber_delta`` (> 0).  With ``prioritized`` the priority is
the row's unweighted loss, as in Rainbow.  ``QVals`` is the mean of ``sum / NQ``.  It composes with ``double_q``,
``prioritized``, ``n_step`` and ``noisy`` (which only sees ``A * NQ`` outputs); ``quantiles`` with ``dueling`` is
refused: 16 outputs would leave CartPole 5 quantiles and the combination needs its own design.  ``quantiles = 0``
launches the kernels it always launched, with the arguments it always passed.

Left for later: quantiles with the dueling head, more than 16 outputs, per-env noise, several ranks, hipGraph
capture, serving the policy to agents (the trainer exposes no ``learner``, so a TrainingServer engine publishes no
model).
"""
from __future__ import annotations

from dataclasses import asdict, dataclass
from typing import Optional

import torch

from ..algorithms.core import FlatNet
from ..ops import GradHead, MLPSpec, ReplayRing, dqn_rollout, dqn_rollout_grid, dqn_targets, grad_slabs, hip, mlp_grad
from ..ops import mlp_grad_qr
from ..ops import PriorityTree, per_insert, per_update
from ..ops import adam_step, noisy_compose, noisy_grad, noisy_sigma_init
from ..parallel.comm import Comm
from .rollout_learn import episode_metrics
from .vec_trainer import CONTINUOUS_DEVICE_ENVS, DEVICE_ENVS


def _as_bool(name: str, value) -> bool:
    """A boolean field; hyperparameters of a TrainingServer arrive as strings ("true")."""
    if isinstance(value, str):
        word = value.strip().lower()
        if word not in ("true", "false", "1", "0", "yes", "no"):
            raise ValueError(f"{name} must be a boolean, got {value!r}")
        return word in ("true", "1", "yes")
    return bool(value)


MAX_DUELING_ACTIONS = 15  # the kernels hold 16 outputs, and the dueling net has one more than actions
MAX_Q_OUTPUTS = 16        # and the quantile net A * quantiles of them


@dataclass
class DQNConfig:
    env: str = "CartPole-v1"
    num_envs: int = 1024
    rollout_len: int = 4            # T: env steps per env and epoch
    hidden: int = 128
    algo: str = "dqn"
    buffer_slots: int = 256         # C: ring capacity in steps (C * num_envs transitions), a multiple of T
    batch_size: int = 1024
    updates_per_epoch: int = 4
    gamma: float = 0.99
    q_lr: float = 5e-4
    eps_start: float = 1.0
    eps_end: float = 0.05
    eps_decay_epochs: int = 500
    learning_starts: int = 8192     # transitions in the ring before the first update
    target_update_every: int = 100  # updates between target <- online copies
    double_q: bool = True
    huber_delta: float = 1.0
    seed: int = 1
    max_episode_steps: Optional[int] = None
    prioritized: bool = False       # prioritised experience replay (proportional variant)
    per_alpha: float = 0.6          # priority = (|td| + per_eps)^per_alpha
    per_beta_start: float = 0.4     # importance-weight exponent, annealed linearly by the host
    per_beta_end: float = 1.0
    per_beta_epochs: int = 500
    per_eps: float = 1e-3
    n_step: int = 1                 # n-step returns, formed from the ring at sample time (1: one-step TD)
    dueling: bool = False           # dueling head: A + 1 outputs, Q = V + A - mean A (needs A <= 15)
    noisy: bool = False             # NoisyNet exploration: W = mu + sigma * eps in all three layers
    noisy_sigma0: float = 0.5       # sigma starts at noisy_sigma0 / sqrt(fan_in)
    quantiles: int = 0              # QR-DQN: quantiles per action, A * quantiles <= 16 outputs (0: scalar DQN)

    def __post_init__(self):
        self.dueling = _as_bool("dueling", self.dueling)
        self.noisy = _as_bool("noisy", self.noisy)
        try:
            self.noisy_sigma0 = float(self.noisy_sigma0)
        except (TypeError, ValueError):
            raise ValueError(f"noisy_sigma0 must be a number, got {self.noisy_sigma0!r}") from None
        if not self.noisy_sigma0 >= 0.0:
            raise ValueError(f"noisy_sigma0 must be >= 0, got {self.noisy_sigma0}")
        try:  # hyperparameters of a TrainingServer arrive as strings ("3")
            n = int(self.n_step)
        except (TypeError, ValueError):
            raise ValueError(f"n_step must be an integer, got {self.n_step!r}") from None
        if isinstance(self.n_step, float) and n != self.n_step:
            raise ValueError(f"n_step must be an integer, got {self.n_step!r}")
        self.n_step = n
        try:
            nq = int(self.quantiles)
        except (TypeError, ValueError):
            raise ValueError(f"quantiles must be an integer, got {self.quantiles!r}") from None
        if isinstance(self.quantiles, float) and nq != self.quantiles:
            raise ValueError(f"quantiles must be an integer, got {self.quantiles!r}")
        self.quantiles = nq
        if not 0 <= self.quantiles <= MAX_Q_OUTPUTS:
            raise ValueError(f"quantiles must be in [0, {MAX_Q_OUTPUTS}], got {self.quantiles}")
        if self.quantiles > 0 and self.dueling:
            raise ValueError("quantiles > 0 with dueling=True is not built: 16 outputs would leave CartPole 5 "
                             "quantiles and the combination needs its own design; set quantiles=0 or dueling=False")
        if self.quantiles > 0 and not float(self.huber_delta) > 0.0:
            raise ValueError(f"quantiles needs huber_delta > 0 (the kappa of the quantile-Huber loss), got "
                             f"{self.huber_delta}")
        if not 1 <= self.n_step <= int(self.buffer_slots):
            raise ValueError(f"n_step must be in [1, buffer_slots = {self.buffer_slots}], got {self.n_step}")
        self.prioritized = _as_bool("prioritized", self.prioritized)
        for k in ("per_alpha", "per_beta_start", "per_beta_end", "per_eps"):
            setattr(self, k, float(getattr(self, k)))
        self.per_beta_epochs = int(self.per_beta_epochs)
        if not self.per_alpha >= 0.0:
            raise ValueError(f"per_alpha must be >= 0, got {self.per_alpha}")
        for k in ("per_beta_start", "per_beta_end"):
            if not 0.0 < getattr(self, k) <= 1.0:
                raise ValueError(f"{k} must be in (0, 1], got {getattr(self, k)}")
        if not self.per_eps > 0.0:
            raise ValueError(f"per_eps must be > 0, got {self.per_eps}")

    def to_dict(self):
        return asdict(self)


def dqn_seeds(seed: int) -> tuple:
    """(env, replay-sample, evaluation) Philox keys of a run: three streams that never share draws."""
    env = (int(seed) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
    return env, (env ^ 0x2545F4914F6CDD1D) & 0x7FFFFFFFFFFFFFFF, (env ^ 0x5851F42D4C957F2D) & 0x7FFFFFFFFFFFFFFF


def dqn_noise_seed(seed: int) -> int:
    """The fourth Philox key of a run: the NoisyNet unit normals (ops/noisy.py), a stream of their own."""
    return (dqn_seeds(seed)[0] ^ 0x14057B7EF767814F) & 0x7FFFFFFFFFFFFFFF


def epsilon_at(cfg: DQNConfig, epoch: int) -> float:
    """The exploration rate of (0-based) epoch ``epoch``: linear from eps_start to eps_end over eps_decay_epochs."""
    frac = min(1.0, epoch / cfg.eps_decay_epochs) if cfg.eps_decay_epochs > 0 else 1.0
    return float(cfg.eps_start + (cfg.eps_end - cfg.eps_start) * frac)


def beta_at(cfg: DQNConfig, epoch: int) -> float:
    """The importance-weight exponent of (0-based) epoch ``epoch``: linear from per_beta_start to per_beta_end
    over per_beta_epochs."""
    frac = min(1.0, epoch / cfg.per_beta_epochs) if cfg.per_beta_epochs > 0 else 1.0
    return float(cfg.per_beta_start + (cfg.per_beta_end - cfg.per_beta_start) * frac)


class DQNTrainer:
    def __init__(self, cfg: DQNConfig, comm: Optional[Comm] = None, device=None):
        self.cfg = cfg
        self.comm = comm or Comm()
        if self.comm.multi:
            raise ValueError("the DQN trainer is single-rank (world_size 1)")
        if cfg.env in CONTINUOUS_DEVICE_ENVS:
            raise ValueError(f"DQN needs a discrete action space; {cfg.env!r} is continuous")
        if cfg.env not in DEVICE_ENVS:
            raise ValueError(f"no device implementation of env {cfg.env!r}; have {list(DEVICE_ENVS)}")
        N, T, C, H = cfg.num_envs, cfg.rollout_len, cfg.buffer_slots, cfg.hidden
        if N < 1 or T < 1 or C < T or C % T:
            raise ValueError(f"buffer_slots ({C}) must be a positive multiple of rollout_len ({T})")
        if cfg.batch_size < 1 or cfg.updates_per_epoch < 0 or cfg.target_update_every < 1:
            raise ValueError("batch_size and target_update_every must be >= 1, updates_per_epoch >= 0")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("the DQN trainer runs the fused HIP actor: it needs a GPU device")
        self.env_id = DEVICE_ENVS[cfg.env]
        D, A, NS, max_steps = hip().env_dims(self.env_id)
        self.D, self.A, self.NS = D, A, NS
        self.max_steps = cfg.max_episode_steps or max_steps
        if cfg.dueling and A > MAX_DUELING_ACTIONS:
            raise ValueError(f"dueling needs A + 1 <= 16 outputs: {cfg.env!r} has {A} actions, at most "
                             f"{MAX_DUELING_ACTIONS} are supported")
        NQ = self.NQ = int(cfg.quantiles)
        if A * NQ > MAX_Q_OUTPUTS:
            raise ValueError(f"quantiles needs A * quantiles <= {MAX_Q_OUTPUTS} outputs: {cfg.env!r} has {A} actions, "
                             f"so at most {MAX_Q_OUTPUTS // A} quantiles; got {NQ}")
        # the online net: the seeded init of PGLearner's policy, with its fused-Adam state; the dueling net
        # has one output more, the state value (row A); the quantile net NQ outputs per action
        g = torch.Generator().manual_seed(int(cfg.seed))
        self.q = FlatNet(MLPSpec(D, H, A * NQ if NQ else A + 1 if cfg.dueling else A), cfg.q_lr, dev, g)
        self.head = GradHead.Q_QR if NQ else GradHead.Q_DUEL if cfg.dueling else GradHead.Q_TD
        # what the head adds to the actor's, the evaluator's and the targets' calls; a plain trainer passes what it
        # always passed.  The quantile head's gradient is an op of its own (_grad_qr)
        self._head_kw = dict(quantiles=NQ) if NQ else dict(dueling=True) if cfg.dueling else {}
        self.target = self.q.params.clone()
        self.theta = None
        if cfg.noisy:  # theta = [mu; sigma] with Adam state of 2P; the net's own tensors are its mu half
            P = self.q.P
            self.theta = torch.cat([self.q.params, noisy_sigma_init(self.q.spec, cfg.noisy_sigma0).to(dev)])
            self.theta_m, self.theta_v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
            self.theta_grad = torch.zeros_like(self.theta)
            self.q.params, self.q.m, self.q.v = self.theta[:P], self.theta_m[:P], self.theta_v[:P]
            self.target = self.theta.clone()
            self.actor_w = torch.zeros(1, P, device=dev)   # role 0, composed once per rollout
            self.update_w = torch.zeros(3, P, device=dev)  # roles 1, 2 (and 3), composed once per update
            self.noise_seed = dqn_noise_seed(cfg.seed)
        self.ring = ReplayRing.allocate(C, N, D, dev)
        self.state = torch.zeros(N, NS, device=dev)
        self.ep_len = torch.zeros(N, dtype=torch.int32, device=dev)
        self.ep_ret = torch.zeros(N, device=dev)
        self.ep_stats = torch.zeros(dqn_rollout_grid(N), 8, device=dev)
        B = cfg.batch_size
        self.Xb = torch.zeros(B, D, device=dev)
        self.act_b = torch.zeros(B, dtype=torch.int32, device=dev)
        self.y = torch.zeros((B, NQ) if NQ else (B,), device=dev)
        ns = grad_slabs(B, dev)
        self.slab = torch.zeros(ns, self.q.P, device=dev)
        self.loss = torch.zeros(ns, 8, device=dev)
        self.per = None
        if cfg.prioritized:
            self.per = PriorityTree.allocate(C, N, dev)
            self.idx = torch.zeros(B, dtype=torch.int32, device=dev)
            self.w = torch.zeros(B, device=dev)
            self.wmax = torch.zeros(1, device=dev)
            self.td_abs = torch.zeros(B, device=dev)
        self.last_beta = float(cfg.per_beta_start)
        self.env_seed, self.sample_seed, self.eval_seed = dqn_seeds(cfg.seed)
        self.eval_step0 = 0
        self.epoch = 0
        self.env_steps = 0
        self.updates = 0
        self.cursor = 0         # next ring slot to write
        self.slots_written = 0  # total, not capped at C
        self.last_epsilon = float(cfg.eps_start)
        self._first = True
        self._has_loss = False

    # ------------------------------------------------------------------ one epoch
    def epsilon(self, epoch: Optional[int] = None) -> float:
        """The exploration rate of epoch ``epoch`` (0-based; default: the next one)."""
        return epsilon_at(self.cfg, self.epoch if epoch is None else int(epoch))

    def rollout(self):
        cfg = self.cfg
        T = cfg.rollout_len
        self.last_epsilon = self.epsilon()
        self.last_beta = beta_at(cfg, self.epoch)  # the exponent of this epoch's updates
        rc = dqn_rollout(self.env_id, self._actor_params(), cfg.hidden, T, self.cursor, self.ring, self.state,
                         self.ep_len, self.ep_ret, self.ep_stats, seed=self.env_seed, step0=self.epoch * T,
                         epsilon=self.last_epsilon, reset_all=self._first, max_steps=self.max_steps, **self._head_kw)
        if rc != 0:
            raise RuntimeError(f"dqn_rollout refused slot {self.cursor} of {cfg.buffer_slots} (code {rc})")
        if self.per is not None:  # the new transitions enter at the running maximum priority
            rc = per_insert(self.per, cfg.buffer_slots, cfg.num_envs, T, self.cursor)
            if rc != 0:
                raise RuntimeError(f"per_insert refused slot {self.cursor} of {cfg.buffer_slots} (code {rc})")
        self._first = False
        self.cursor = (self.cursor + T) % cfg.buffer_slots
        self.slots_written += T

    def _actor_params(self) -> torch.Tensor:
        """What the actor acts on: the online net, or (noisy) its role-0 sample of this epoch, shared by all
        envs and all T steps of the launch."""
        if self.theta is None:
            return self.q.params
        noisy_compose(self.theta, (0,), (self.epoch,), self.q.spec, self.noise_seed, out=self.actor_w)
        return self.actor_w[0]

    def _update_params(self):
        """(selecting online net, target net, online net of the loss): the nets themselves, or (noisy) three
        independent samples at draw = the update index from one compose launch."""
        if self.theta is None:
            return self.q.params, self.target, self.q.params
        n = 3 if self.cfg.double_q else 2
        noisy_compose((self.theta, self.target, self.theta)[:n], (1, 2, 3)[:n], (self.updates,) * n, self.q.spec,
                      self.noise_seed, out=self.update_w[:n])
        select = self.update_w[2] if self.cfg.double_q else self.update_w[0]  # read only with double_q
        return select, self.update_w[1], self.update_w[0]

    def _apply(self):
        """One Adam step from the gradient slabs; (noisy) on [mu; sigma] from the slabs of the role-1 sample."""
        if self.theta is None:
            return self.q.apply(self.slab)
        q = self.q
        noisy_grad(self.slab, 1, self.updates, q.spec, self.noise_seed, out=self.theta_grad)
        adam_step(self.theta, self.theta_m, self.theta_v, q.step, q.ticket, q.lr, grad=self.theta_grad,
                  beta1=q.betas[0], beta2=q.betas[1], eps=q.eps, weight_decay=q.weight_decay)
        q.version += 1

    def _grad_qr(self, params):
        """The quantile head's gradient slabs of one batch (``mlp_grad_qr``), with the weights of prioritised replay
        where there are any."""
        per = {} if self.per is None else dict(row_w=self.w, w_norm=self.wmax, td_abs=self.td_abs)
        mlp_grad_qr(params, self.Xb, self.A, self.NQ, self.cfg.hidden, act=self.act_b, ret=self.y,
                    kappa=self.cfg.huber_delta, grad_slab=self.slab, loss_slab=self.loss, **per)

    def update(self):
        """One gradient step on a freshly sampled batch; the target network follows on its schedule."""
        cfg = self.cfg
        online, target, params = self._update_params()
        filled = min(self.slots_written, cfg.buffer_slots) * cfg.num_envs
        # n-step walks end at the slot the rollout wrote last: the one before the cursor
        nstep = dict(n_step=cfg.n_step, newest=(self.cursor - 1) % cfg.buffer_slots) if cfg.n_step > 1 else {}
        if self.per is None:
            dqn_targets(online, target, cfg.hidden, self.A, self.ring, filled, cfg.gamma, cfg.double_q,
                        self.sample_seed, self.updates, cfg.batch_size, out=(self.Xb, self.act_b, self.y, None),
                        **nstep, **self._head_kw)
            if self.NQ:
                self._grad_qr(params)
            else:
                mlp_grad(self.head, params, self.Xb, self.A, cfg.hidden, act=self.act_b, ret=self.y,
                         clip_eps=cfg.huber_delta, grad_slab=self.slab, loss_slab=self.loss)
            self._apply()
        else:
            dqn_targets(online, target, cfg.hidden, self.A, self.ring, filled, cfg.gamma, cfg.double_q,
                        self.sample_seed, self.updates, cfg.batch_size, tree=self.per.tree, beta=self.last_beta,
                        out=(self.Xb, self.act_b, self.y, self.idx, self.w, self.wmax), **nstep, **self._head_kw)
            if self.NQ:
                self._grad_qr(params)
            else:
                mlp_grad(self.head, params, self.Xb, self.A, cfg.hidden, act=self.act_b, ret=self.y,
                         clip_eps=cfg.huber_delta, grad_slab=self.slab, loss_slab=self.loss, row_w=self.w,
                         w_norm=self.wmax, td_abs=self.td_abs)
            self._apply()
            per_update(self.per, self.idx, self.td_abs, cfg.per_alpha, cfg.per_eps)
        self.updates += 1
        self._has_loss = True
        if self.updates % cfg.target_update_every == 0:
            self.target.copy_(self.q.params if self.theta is None else self.theta)

    def train_epoch(self):
        cfg = self.cfg
        self.rollout()
        self.epoch += 1
        self.env_steps += cfg.rollout_len * cfg.num_envs
        if self.slots_written * cfg.num_envs >= cfg.learning_starts:
            for _ in range(cfg.updates_per_epoch):
                self.update()

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, episodes: int = 1, num_envs: Optional[int] = None, greedy: bool = True):
        """Score the greedy policy of the online network: ``num_envs`` fresh envs x ``episodes`` whole
        episodes (the evaluator's argmax over "logits" is the greedy Q-policy).  It reads the weights
        and touches none of the training state or the ring; its Philox stream is its own.  A noisy net is
        scored at zero noise: on ``mu``, which ``self.q.params`` is."""
        if not greedy:
            raise ValueError("a DQN policy is evaluated greedily: softmax-of-Q is not this algorithm's policy")
        from ..ops import evaluate_policy_op
        from .evaluate import EvalResult

        E, N = int(episodes), int(num_envs or self.cfg.num_envs)
        step0 = self.eval_step0
        ep_ret, ep_len, ep_code, _ = evaluate_policy_op(self.env_id, self.q.params, self.cfg.hidden, E, N, greedy=True,
                                                        seed=self.eval_seed, step0=step0, max_steps=self.max_steps,
                                                        **self._head_kw)
        self.eval_step0 += E * self.max_steps
        return EvalResult(ep_ret, ep_len, ep_code, True, self.eval_seed, step0)

    # ------------------------------------------------------------------ metrics
    def metrics(self) -> dict:
        """Synchronising read of the last epoch's statistics."""
        ep = self.ep_stats.sum(0).tolist()
        mx = self.ep_stats[:, 3].max().item()
        mn = self.ep_stats[:, 4].min().item()
        out = {"Epoch": self.epoch}
        out.update(episode_metrics(self.comm, ep[0], ep[1], ep[2], mx, mn, ep[5]))
        nan = float("nan")
        loss_q = q_vals = nan
        if self._has_loss:
            ls = self.loss.sum(0).tolist()
            if ls[5] > 0:
                loss_q, q_vals = ls[0] / ls[5], ls[4] / ls[5]
        out.update(LossQ=loss_q, QVals=q_vals, Epsilon=self.last_epsilon, Updates=self.updates,
                   EnvSteps=self.env_steps, WorldSize=1, NStep=self.cfg.n_step, Dueling=bool(self.cfg.dueling),
                   Noisy=bool(self.cfg.noisy), Quantiles=int(self.cfg.quantiles))
        if self.theta is not None:
            out.update(SigmaMeanAbs=float(self.theta[self.q.P:].abs().mean().item()))
        if self.per is not None:
            out.update(Beta=self.last_beta, PriorityMax=float(self.per.pmax.item()))
        return out

    def episode_sums(self) -> tuple:
        """(finished episodes, sum of their returns) in the last epoch, from one device->host read."""
        n, s = self.ep_stats[:, :2].sum(0).tolist()
        return n, s

    def average_ep_return(self) -> float:
        n, s = self.episode_sums()
        return s / n if n > 0 else float("nan")

    # ------------------------------------------------------------------ state
    def snapshot_tensors(self):
        q = self.q
        P = q.P  # of a noisy trainer q.params / q.m / q.v and target[:P] are the mu halves
        target = self.target if self.theta is None else self.target[:P]
        ts = [q.params, q.m, q.v, q.step, target, *self.ring, self.state, self.ep_len, self.ep_ret]
        if self.per is not None:  # at the end: the names of the uniform trainer's tensors keep their places
            ts += [self.per.tree, self.per.pmax]
        if self.theta is not None:  # and the sigma halves after those
            ts += [self.theta[P:], self.theta_m[P:], self.theta_v[P:], self.target[P:]]
        return ts

    def counters(self) -> dict:
        return {"epoch": self.epoch, "env_steps": self.env_steps, "updates": self.updates, "cursor": self.cursor,
                "slots_written": self.slots_written, "_first": self._first}

    def set_counters(self, c: dict):
        self.epoch, self.env_steps, self.updates = int(c["epoch"]), int(c["env_steps"]), int(c["updates"])
        self.cursor, self.slots_written, self._first = int(c["cursor"]), int(c["slots_written"]), bool(c["_first"])

    def state_dict(self) -> dict:
        """Everything a bit-exact resume needs.  ``learner/pi/params`` is the online network, the
        layout ``launcher.evaluate_checkpoint_state`` reads."""
        sd = {"cfg": self.cfg.to_dict(),
              "learner": {"pi": self.q.state_dict(), "target": {"params": self.target[:self.q.P].cpu()}},
              "ring": {k: t.cpu() for k, t in self.ring._asdict().items()},
              "epoch": self.epoch, "env_steps": self.env_steps, "updates": self.updates, "cursor": self.cursor,
              "slots_written": self.slots_written, "eval_step0": self.eval_step0,
              "env_state": self.state.cpu(), "ep_len": self.ep_len.cpu(), "ep_ret": self.ep_ret.cpu()}
        if self.per is not None:  # the tree is a pure function of its leaves: load_state_dict rebuilds it
            sd["per"] = {"leaves": self.per.leaves.cpu(), "pmax": float(self.per.pmax.item())}
        if self.theta is not None:  # learner/pi and learner/target hold the mu halves: the evaluators read them
            P = self.q.P
            sd["noisy"] = {"sigma": self.theta[P:].cpu(), "m": self.theta_m[P:].cpu(), "v": self.theta_v[P:].cpu(),
                           "target_sigma": self.target[P:].cpu()}
        return sd

    def load_state_dict(self, sd: dict):
        """Resume from ``state_dict()``.  The Philox keys derive from ``cfg.seed``: build the trainer with the
        checkpoint's config (the launcher does, from the preset and its overrides) for a bit-exact resume."""
        got = int(sd["learner"]["pi"]["params"].numel())
        mine, theirs = int(self.cfg.quantiles), int(sd.get("cfg", {}).get("quantiles", 0) or 0)  # absent: scalar
        if mine != theirs:
            raise ValueError(f"this trainer has quantiles={mine} ({self.q.P} parameters); the checkpoint has "
                             f"quantiles={theirs} ({got} parameters): build the trainer with the checkpoint's "
                             "quantiles setting")
        mine = bool(self.cfg.dueling)
        theirs = sd.get("cfg", {}).get("dueling")  # absent in a checkpoint from before the dueling head: plain
        if got != self.q.P or (theirs is not None and bool(theirs) != mine):
            raise ValueError(f"this trainer has dueling={mine} ({self.q.P} parameters); the checkpoint has "
                             f"dueling={bool(theirs)} ({got} parameters): build the trainer with the checkpoint's "
                             "dueling setting")
        mine, theirs = bool(self.cfg.noisy), bool(sd.get("cfg", {}).get("noisy", False)) or "noisy" in sd
        if mine != theirs:
            raise ValueError(f"this trainer has noisy={mine}; the checkpoint has noisy={theirs}"
                             f"{'' if theirs else ' (no sigma)'}: build the trainer with the checkpoint's noisy setting")
        self.q.load_state_dict(sd["learner"]["pi"])
        self.target[:self.q.P].copy_(sd["learner"]["target"]["params"].to(self.device))
        if self.theta is not None:
            P, nz = self.q.P, sd["noisy"]
            for dst, k in ((self.theta, "sigma"), (self.theta_m, "m"), (self.theta_v, "v"),
                           (self.target, "target_sigma")):
                dst[P:].copy_(nz[k].to(self.device))
        for k, t in self.ring._asdict().items():
            src = sd["ring"][k]
            if tuple(src.shape) != tuple(t.shape):
                raise ValueError(f"checkpoint ring {k} is {tuple(src.shape)}, this trainer's {tuple(t.shape)}")
            t.copy_(src.to(self.device))
        self.set_counters({k: sd[k] for k in ("epoch", "env_steps", "updates", "cursor", "slots_written")} | {"_first": False})
        self.eval_step0 = int(sd.get("eval_step0", 0))
        self.state.copy_(sd["env_state"].to(self.device))
        self.ep_len.copy_(sd["ep_len"].to(self.device))
        self.ep_ret.copy_(sd["ep_ret"].to(self.device))
        if self.per is not None:
            if "per" not in sd:
                raise ValueError("a prioritised trainer cannot resume a checkpoint without priorities")
            self.per.load_leaves(sd["per"]["leaves"], sd["per"]["pmax"])
