"""Sentinel-guarded device tensors for the GPU tests: every output buffer of a kernel under test is
the middle of a larger tensor whose guard elements must survive the launch."""
import math

import numpy as np
import torch

GUARD = 64
INT_SENTINEL = -7
BYTE_SENTINEL = 0xA5  # no pixel value (0, 100, 255)
DEV = "cuda:0"


class Guarded:
    """A contiguous tensor with GUARD sentinel elements on both sides (NaN, -7 for ints, 0xA5 for bytes)."""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        n = math.prod(shape)
        self.sentinel = float("nan") if dtype.is_floating_point else (BYTE_SENTINEL if dtype == torch.uint8 else INT_SENTINEL)
        self.big = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device=DEV)
        self.t = self.big[GUARD:GUARD + n].view(shape)
        if fill is not None:  # else the payload starts as sentinels too: an unwritten cell shows
            self.t.copy_(torch.as_tensor(np.broadcast_to(np.asarray(fill), shape).copy()).to(dtype))

    def guards_intact(self):
        g = torch.cat([self.big[:GUARD], self.big[-GUARD:]])
        return bool(torch.isnan(g).all()) if self.big.dtype.is_floating_point else bool((g == self.sentinel).all())
