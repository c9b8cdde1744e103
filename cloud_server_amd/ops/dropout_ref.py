"""The one definition of the dropout mask, in NumPy (the test reference) and in torch.

The mask is a pure function of (seed, layer, step, element), drawn from the counter RNG
the image ops already share between NumPy and the device (``preprocess.ops_ref.crng`` ==
``crng.h``), so it is never stored: the eager model, the HIP kernels (csrc/kernels/
dropout.hip) and a resumed job all redraw the same bits.

* ``drop_seed(cfg_seed, layer_index) = smix(uint64(cfg_seed) ^ (uint64(layer_index + 1) << 32))``
  with ``layer_index = LayerPlan.index``.
* Element ``(b, f)`` of a per-rank batch with ``F`` features per sample has the counter
  ``j = (b * world + rank) * F + f``: ``b * world + rank`` is the row's place in the global
  batch as ``BatchStream`` lays it out (``take[rank::world]``), so world-N data parallelism
  draws exactly the mask of one process at batch ``N * B``.
* ``r = crng(drop_seed, step & 0xFFFFFFFF, j)`` with ``step`` the number of completed
  training steps; the element is kept iff ``(r >> 8) < T``, ``T = round(keep_prob * 2^24)``
  clamped to ``[1, 2^24]`` (an integer compare: exact on every side).
* ``y = keep ? a * s : 0`` with ``s = float32(1 / keep_prob)``; backward ``da = keep ? dy * s : 0``.
"""
from __future__ import annotations

import numpy as np
import torch

from ..preprocess.ops_ref import _smix, crng

_M64 = (1 << 64) - 1


def drop_seed(cfg_seed: int, layer_index: int) -> int:
    z = np.array((int(cfg_seed) & _M64) ^ (((int(layer_index) + 1) << 32) & _M64), dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(_smix(z))


def keep_threshold(keep_prob: float) -> int:
    return min(max(int(round(float(keep_prob) * (1 << 24))), 1), 1 << 24)


def keep_scale(keep_prob: float) -> float:
    """``s`` as the float32 every implementation multiplies by."""
    return float(np.float32(1.0 / float(keep_prob)))


def keep_mask(seed: int, step: int, B: int, F: int, keep_prob: float, world: int = 1,
              rank: int = 0) -> np.ndarray:
    """bool [B, F]: the kept elements of one rank's batch at ``step`` (``seed`` = drop_seed)."""
    b = np.arange(B, dtype=np.uint64)[:, None]
    f = np.arange(F, dtype=np.uint64)[None, :]
    j = (b * np.uint64(world) + np.uint64(rank)) * np.uint64(F) + f
    r = crng(seed, np.uint64(int(step) & 0xFFFFFFFF), j)
    return (r >> np.uint64(8)) < np.uint64(keep_threshold(keep_prob))


# ---------------------------------------------------------------------------- torch
def _s64(v: int) -> int:
    """A 64-bit constant as the signed value with the same bits."""
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


def _lsr(z: torch.Tensor, k: int) -> torch.Tensor:
    """Logical right shift of int64 bits (``>>`` on int64 is arithmetic)."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _smix_torch(z: torch.Tensor) -> torch.Tensor:
    z = z + _s64(0x9E3779B97F4A7C15)
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def crng_torch(seed: int, step: torch.Tensor, j: torch.Tensor) -> torch.Tensor:
    """``ops_ref.crng`` from device ops alone (int64 arithmetic wraps like uint64): int64
    draws in [0, 2^32) for the int64 tensors ``step`` (< 2^32) and ``j`` (broadcast)."""
    z = _smix_torch((step << 32) | j) ^ _s64(int(seed))
    return _lsr(_smix_torch(z), 32)


def keep_mask_torch(seed: int, step: torch.Tensor, B: int, F: int, keep_prob: float, world: int = 1,
                    rank: int = 0) -> torch.Tensor:
    """bool [B, F] on ``step``'s device; ``step`` is a one-element int64 tensor."""
    dev = step.device
    b = torch.arange(B, dtype=torch.int64, device=dev)[:, None]
    f = torch.arange(F, dtype=torch.int64, device=dev)[None, :]
    j = (b * world + rank) * F + f
    r = crng_torch(seed, step.to(torch.int64) & 0xFFFFFFFF, j)
    return (r >> 8) < keep_threshold(keep_prob)
