"""Rollout payload checksum and header verification (csrc/kernels/checksum.hip).

The payload of one actor -> learner rollout is one sequence of 32-bit words: the concatenation,
in order, of up to 8 segments.  ``payload_checksum`` returns the bits of

    s1 = sum_i w_i  mod 2^64          s2 = sum_i (i + 1) w_i  mod 2^64

as an ``int64[2]`` tensor.  Integer arithmetic over bit patterns: exact, independent of the launch
geometry, identical on every rank and on the CPU oracle (ops/reference.py, numpy uint64).
GPU tensors take the HIP kernel (no host sync, current stream); CPU tensors take the oracle.
A non-contiguous segment is checksummed in its logical (row-major) order, through a contiguous copy.
"""
from __future__ import annotations

import torch

from . import reference as ref
from .mlp import _hip_for

MAX_SEGMENTS = 8
STATUS_CHECKSUM, STATUS_SEQ, STATUS_VERSION = ref.STATUS_CHECKSUM, ref.STATUS_SEQ, ref.STATUS_VERSION
STATUS_NAMES = ((STATUS_CHECKSUM, "checksum"), (STATUS_SEQ, "seq"), (STATUS_VERSION, "version"))


def status_bits(status: int) -> str:
    """'checksum+seq' for status 3, 'ok' for 0."""
    return "+".join(n for b, n in STATUS_NAMES if status & b) or "ok"


def payload_checksum(segments, out=None) -> torch.Tensor:
    segs = [s for s in segments if s is not None]
    if not 1 <= len(segs) <= MAX_SEGMENTS:
        raise ValueError(f"payload_checksum takes 1..{MAX_SEGMENTS} segments, got {len(segs)}")
    dev = segs[0].device
    for i, s in enumerate(segs):
        if s.device != dev:
            raise ValueError(f"payload_checksum: segment {i} is on {s.device}, segment 0 on {dev}")
        if s.element_size() % 4:
            raise ValueError(f"payload_checksum: segment {i} has dtype {s.dtype}; the element size must be a "
                             "multiple of 4 bytes")
    if out is None:
        out = torch.empty(2, dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.numel() != 2 or out.device != dev or not out.is_contiguous():
        raise ValueError("payload_checksum: out must be a contiguous int64[2] tensor on the segments' device")
    h = _hip_for(segs[0])
    if h is None:
        out.copy_(ref.payload_checksum_ref(segs))
        return out
    h.payload_checksum([s.contiguous() for s in segs], out)
    return out


def payload_verify(sums, hdr, expected_seq: int, lo: int, hi: int, ck_col: int = 10, out=None) -> torch.Tensor:
    """``int32[K]`` status of K received headers ``hdr`` [K, HDR] (float64) against the recomputed
    ``sums`` [K, 2]: STATUS_CHECKSUM when the sums differ from the raw 64-bit header columns
    ``ck_col``, ``ck_col + 1``; STATUS_SEQ when column 0 != ``expected_seq``; STATUS_VERSION when
    column 7 is outside [``lo``, ``hi``]."""
    if hdr.dim() != 2 or hdr.dtype != torch.float64 or hdr.shape[1] < max(8, ck_col + 2):
        raise ValueError(f"payload_verify: hdr must be float64 [K, >= {max(8, ck_col + 2)}], got "
                         f"{hdr.dtype} {tuple(hdr.shape)}")
    K = hdr.shape[0]
    if sums.dtype != torch.int64 or sums.numel() != 2 * K or sums.device != hdr.device:
        raise ValueError("payload_verify: sums must be int64 [K, 2] on the header's device")
    if out is None:
        out = torch.empty(K, dtype=torch.int32, device=hdr.device)
    h = _hip_for(hdr)
    if h is None:
        out.copy_(ref.payload_verify_ref(sums, hdr, ck_col, expected_seq, lo, hi))
        return out
    h.payload_verify(sums.contiguous(), hdr.contiguous(), int(ck_col), int(expected_seq), int(lo), int(hi), out)
    return out
