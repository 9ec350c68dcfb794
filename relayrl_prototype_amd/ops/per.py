"""Prioritised experience replay (Schaul et al., proportional variant): the priority sum tree of
csrc/kernels/per.hip, its host oracles and the torch rebuild.

The ring has ``L = C * N`` rows (``ReplayRing``: row = slot * N + env) and ``P2`` is the smallest power
of two >= L.  ``tree`` is fp32 ``[2 * P2]``: node 1 the root, the leaf of row r at ``tree[P2 + r]``,
padding leaves and rows never written 0.  ``pmax`` (one float, 1.0 at the start) is the running maximum
of every leaf ever assigned.  After every op here each internal node is ONE fp32 add of its children,
``tree[i] == tree[2i] + tree[2i + 1]``: the tree is a pure function of its leaves, so a checkpoint keeps
the leaves and ``per_tree_build`` gives the same bits back, and ``per_sample_rows_ref`` predicts the rows
the kernel samples exactly.

* ``per_tree_build``: leaves -> tree in torch (CPU or GPU), log2(P2) strided adds.  The oracle of the
  tests and the rebuild of ``load_state_dict``.
* ``per_insert`` / ``per_update``: the two kernels; CPU tensors take ``per_insert_ref`` / ``per_update_ref``.
* ``per_sample_rows_ref`` / ``per_weights_ref``: what the prioritised ``dqn_targets`` samples and weighs.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import philox


def per_tree_leaves(L: int) -> int:
    """P2: the smallest power of two >= L (1 <= L <= 2^30)."""
    if L < 1 or L > 2 ** 30:
        raise ValueError(f"a priority tree needs 1 <= rows <= 2^30, got {L}")
    return 1 << (int(L) - 1).bit_length()


def per_tree_build(leaves: torch.Tensor) -> torch.Tensor:
    """fp32 ``[2 * P2]`` tree over ``leaves`` (``[n]``, n <= P2 = per_tree_leaves(n); the rest pads with 0):
    level by level ``t[h:n] = t[n:2n:2] + t[n+1:2n:2]``, one fp32 add per node; ``t[0]`` is 0."""
    leaves = leaves.reshape(-1).float()
    P2 = per_tree_leaves(leaves.numel())
    t = torch.zeros(2 * P2, dtype=torch.float32, device=leaves.device)
    t[P2:P2 + leaves.numel()] = leaves
    n = P2
    while n > 1:
        h = n // 2
        t[h:n] = t[n:2 * n:2] + t[n + 1:2 * n:2]
        n = h
    return t


class PriorityTree(NamedTuple):
    tree: torch.Tensor  # [2 * P2] fp32
    pmax: torch.Tensor  # [1] fp32
    L: int              # rows of the ring

    @staticmethod
    def allocate(C: int, N: int, device) -> "PriorityTree":
        P2 = per_tree_leaves(C * N)
        return PriorityTree(torch.zeros(2 * P2, device=device), torch.ones(1, device=device), C * N)

    @property
    def P2(self) -> int:
        return self.tree.numel() // 2

    @property
    def leaves(self) -> torch.Tensor:
        """The leaves of the ring's rows (a view)."""
        return self.tree[self.P2:self.P2 + self.L]

    def load_leaves(self, leaves: torch.Tensor, pmax) -> None:
        if leaves.numel() != self.L:
            raise ValueError(f"checkpoint has {leaves.numel()} priorities, this ring {self.L} rows")
        self.tree.copy_(per_tree_build(leaves.to(self.tree.device)))
        self.pmax.fill_(float(pmax))


def _wrap_code(C: int, N: int, T: int, slot0: int) -> int:
    if N < 1 or T < 1 or C < 1:
        return -2
    if slot0 < 0 or C % T != 0 or slot0 % T != 0 or slot0 + T > C:
        return -4
    return 0


def per_insert_ref(pt: PriorityTree, C: int, N: int, T: int, slot0: int) -> int:
    rc = _wrap_code(C, N, T, slot0)
    if rc:
        return rc
    leaves = pt.leaves.clone()
    leaves[slot0 * N:(slot0 + T) * N] = pt.pmax[0]
    pt.tree.copy_(per_tree_build(leaves))
    return 0


def per_insert(pt: PriorityTree, C: int, N: int, T: int, slot0: int) -> int:
    """Leaves of rows ``[slot0 * N, (slot0 + T) * N)`` <- pmax, ancestors refreshed.  Returns 0, or
    ``dqn_rollout``'s negative code (nothing written) for a range that would wrap."""
    from . import use_hip, hip

    if C * N != pt.L:
        raise ValueError(f"the tree covers {pt.L} rows, the ring has {C * N}")
    if not use_hip(pt.tree):
        return per_insert_ref(pt, C, N, T, slot0)
    return int(hip().per_insert(pt.tree, pt.pmax, int(C), int(N), int(T), int(slot0)))


def per_priorities_ref(td_abs, pmax: float, alpha: float, prio_eps: float) -> np.ndarray:
    """fp32 ``(|td| + eps)^alpha``; a non-finite one takes ``pmax``."""
    td = np.abs(np.asarray(td_abs, dtype=np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.power(td + np.float32(prio_eps), np.float32(alpha)).astype(np.float32)
    return np.where(np.isfinite(td) & np.isfinite(v), v, np.float32(pmax)).astype(np.float32)


def per_update_ref(pt: PriorityTree, idx, td_abs, alpha: float, prio_eps: float) -> None:
    idx = np.asarray(torch.as_tensor(idx).cpu(), dtype=np.int64)
    v = per_priorities_ref(torch.as_tensor(td_abs).detach().cpu().numpy(), float(pt.pmax[0]), alpha, prio_eps)
    ok = (idx >= 0) & (idx < pt.L)
    idx, v = idx[ok], v[ok]
    leaves = pt.leaves.cpu().numpy().copy()
    leaves[idx] = 0.0
    np.maximum.at(leaves, idx, v)  # the maximum over the duplicates, not with the old leaf
    pt.tree.copy_(per_tree_build(torch.from_numpy(leaves)).to(pt.tree.device))
    if v.size:
        pt.pmax.fill_(max(float(pt.pmax[0]), float(v.max())))


def per_update(pt: PriorityTree, idx: torch.Tensor, td_abs: torch.Tensor, alpha: float, prio_eps: float) -> None:
    """Leaf of every sampled row <- the maximum over its duplicates of ``(|td| + eps)^alpha``,
    ``pmax <- max(pmax, new leaves)``, ancestors refreshed."""
    from . import use_hip, hip

    if alpha < 0 or not prio_eps > 0:
        raise ValueError("per_update needs alpha >= 0 and prio_eps > 0")
    if not use_hip(pt.tree):
        return per_update_ref(pt, idx, td_abs, alpha, prio_eps)
    hip().per_update(pt.tree, pt.pmax, int(pt.L), idx, td_abs, float(alpha), float(prio_eps))


def per_sample_rows_ref(tree, seed: int, update: int, B: int, filled: int, u: Optional[float] = None) -> np.ndarray:
    """int64 [B]: the ring rows the prioritised ``dqn_targets`` reads for update ``update``, in numpy fp32:

        rnd   = philox((b, update_lo, update_hi, 1), seed);  total = tree[1];  seg = total / B
        m     = (b + u01(rnd.x)) * seg;  i = 1
        log2(P2) times:  l, r = tree[2i], tree[2i + 1];  (m >= l and r > 0) ? (m -= l, i = 2i + 1) : i = 2i
        row   = min(i - P2, filled - 1)

    ``u`` replaces every draw (the tests force 0 and the largest u01)."""
    t = np.ascontiguousarray(torch.as_tensor(tree).detach().cpu().numpy(), dtype=np.float32)
    P2 = t.size // 2
    if P2 < 1 or P2 & (P2 - 1) or t.size != 2 * P2:
        raise ValueError(f"a tree holds 2 * (a power of two) floats, got {t.size}")
    if filled < 1 or filled > P2:
        raise ValueError(f"filled must be in [1, {P2}], got {filled}")
    b = np.arange(B, dtype=np.uint32)
    n = b.shape
    if u is None:
        x = philox.philox4x32(b, np.full(n, update & 0xFFFFFFFF, np.uint32),
                              np.full(n, (update >> 32) & 0xFFFFFFFF, np.uint32), np.ones(n, np.uint32),
                              np.full(n, seed & 0xFFFFFFFF, np.uint32), np.full(n, (seed >> 32) & 0xFFFFFFFF, np.uint32))[0]
        uu = philox.u01(x)
    else:
        uu = np.full(n, u, np.float32)
    seg = np.float32(t[1]) / np.float32(B)
    m = (b.astype(np.float32) + uu) * seg
    assert m.dtype == np.float32
    i = np.ones(B, np.int64)
    for _ in range(P2.bit_length() - 1):
        l, r = t[2 * i], t[2 * i + 1]
        right = (m >= l) & (r > 0)
        m = np.where(right, m - l, m).astype(np.float32)
        i = np.where(right, 2 * i + 1, 2 * i)
    return np.minimum(i - P2, filled - 1)


def per_weights_ref(tree, rows, filled: int, beta: float, dtype=torch.float64) -> torch.Tensor:
    """``(filled * leaf / total)^-beta`` of ``rows`` in ``dtype``."""
    t = torch.as_tensor(tree).detach().cpu().to(dtype)
    P2 = t.numel() // 2
    leaf = t[P2 + torch.as_tensor(rows, dtype=torch.int64)]
    return (filled * leaf / t[1]) ** (-beta)
