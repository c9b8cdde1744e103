"""The one definition of the learning-rate schedule: NumPy float32, float64 and torch forms.

The rate of a step is a pure function of the step counter, evaluated on the device by the
launch that applies the update (``opt_step_lr`` in csrc/kernels/optim_common.h), so it moves
inside a replayed multi-step graph, needs no host sync and no checkpoint state, and is exact
across resume, packed jobs and data parallelism — like the counter-RNG dropout masks
(``ops/dropout_ref.py``).

* ``t`` is the 1-based step: the device counter after the head advanced it.  Under
  ``async_ps`` it is the owner's 1-based apply count, which is what TF's ``global_step`` is
  under asynchronous replicas.
* ``g = max(t - 1, 0)`` is TF's ``global_step`` convention: the first update uses g = 0.
* ``lr`` is the base rate, ``TrainConfig.effective_lr``.  With S = ``decay_steps``,
  r = ``decay_rate``, α = ``alpha``, W = ``warmup_steps``::

      constant      m = 1
      exponential   x = staircase ? float(g // S) : float(g) / float(S)      m = powf(r, x)
      inverse_time  x as above                                                m = 1 / (1 + r * x)
      cosine        x = float(min(g, S)) / float(S)       m = α + (1 − α) * 0.5 * (1 + cosf(π * x))
      warm-up       if g < W:  m = m * (float(g + 1) / float(W))
      lr_t = lr * m        (Adam: its bias correction is then applied to lr_t, with t)

* The stair index is an INTEGER division of the counter — never the floor of a float
  product or quotient (``3 * fl(1/3)`` floors to the wrong stair).
* Every float operation is fp32, in the order written (the device compiles the multiplier
  with contraction off); π is ``float32(pi)``.  ``mult_f64`` is the same formula in float64:
  the oracle the fp32 forms are tested against.
* The ``constant`` type without warm-up is no schedule at all: every path then runs exactly
  the code it ran before schedules existed (``active`` is False, ``to_c`` returns None).

The schedule object is ``models.dsl.LrSchedule`` (any object with its attributes works).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

# LrKind of csrc/kernels/optim_common.h (4: the constant type under a warm-up)
KINDS = {"constant": 0, "exponential": 1, "inverse_time": 2, "cosine": 3}
KIND_WARMUP_ONLY = 4
_PI32 = np.float32(math.pi)


class LrSchedC(C.Structure):
    """``csa::LrSched`` (24 bytes), passed to the ``*_sched`` entry points by pointer."""
    _fields_ = [("kind", C.c_int), ("staircase", C.c_int), ("decay_steps", C.c_int), ("warmup_steps", C.c_int),
                ("rate", C.c_float), ("alpha", C.c_float)]


def active(sched) -> bool:
    """False when the schedule is the identity (no schedule, or constant without warm-up)."""
    return sched is not None and not (sched.type == "constant" and sched.warmup_steps == 0)


def to_c(sched) -> Optional[LrSchedC]:
    """The device's argument, or None for the identity (the schedule-free entry points)."""
    if not active(sched):
        return None
    kind = KINDS[sched.type] or KIND_WARMUP_ONLY
    return LrSchedC(kind, int(bool(sched.staircase)), int(sched.decay_steps), int(sched.warmup_steps),
                    float(sched.decay_rate), float(sched.alpha))


# ------------------------------------------------------------------ NumPy float32
def mult_f32(sched, t) -> np.ndarray:
    """m(t) as the device computes it: float32 array for an integer array (or scalar) ``t``."""
    t = np.asarray(t, dtype=np.int64)
    g = np.maximum(t - 1, 0)
    one = np.float32(1.0)
    if not active(sched):
        return np.ones(t.shape, np.float32)
    S = int(sched.decay_steps)
    if sched.type == "cosine":
        x = np.minimum(g, S).astype(np.float32) / np.float32(S)
        a = np.float32(sched.alpha)
        m = a + (one - a) * np.float32(0.5) * (one + np.cos(_PI32 * x, dtype=np.float32))
    elif sched.type in ("exponential", "inverse_time"):
        x = (g // S).astype(np.float32) if sched.staircase else g.astype(np.float32) / np.float32(S)
        r = np.float32(sched.decay_rate)
        m = np.power(r, x, dtype=np.float32) if sched.type == "exponential" else one / (one + r * x)
    else:
        m = np.ones(t.shape, np.float32)
    W = int(sched.warmup_steps)
    if W > 0:
        m = np.where(g < W, m * ((g + 1).astype(np.float32) / np.float32(W)), m)
    return np.asarray(m, dtype=np.float32)


def lr_f32(sched, lr: float, t) -> np.ndarray:
    """lr_t = lr * m(t) in float32 (``lr`` itself, bitwise, for the identity)."""
    t = np.asarray(t, dtype=np.int64)
    if not active(sched):
        return np.full(t.shape, np.float32(lr), np.float32)
    return np.asarray(np.float32(lr) * mult_f32(sched, t), dtype=np.float32)


# ------------------------------------------------------------------ float64 (the oracle)
def mult_f64(sched, t) -> np.ndarray:
    t = np.asarray(t, dtype=np.int64)
    g = np.maximum(t - 1, 0)
    if not active(sched):
        return np.ones(t.shape, np.float64)
    S = int(sched.decay_steps)
    if sched.type == "cosine":
        x = np.minimum(g, S).astype(np.float64) / S
        a = float(sched.alpha)
        m = a + (1.0 - a) * 0.5 * (1.0 + np.cos(math.pi * x))
    elif sched.type in ("exponential", "inverse_time"):
        x = (g // S).astype(np.float64) if sched.staircase else g.astype(np.float64) / S
        # the rate is the float32 the device holds (a parameter, not a rounding of the formula)
        r = float(np.float32(sched.decay_rate))
        m = np.power(r, x) if sched.type == "exponential" else 1.0 / (1.0 + r * x)
    else:
        m = np.ones(t.shape, np.float64)
    W = int(sched.warmup_steps)
    if W > 0:
        m = np.where(g < W, m * ((g + 1).astype(np.float64) / W), m)
    return np.asarray(m, dtype=np.float64)


def lr_f64(sched, lr: float, t) -> np.ndarray:
    return float(lr) * mult_f64(sched, t)


# ------------------------------------------------------------------ torch (device tensor)
def mult_torch(sched, t: torch.Tensor) -> torch.Tensor:
    """m(t) for an int64 tensor ``t`` on its device, float32, without a host read (the
    eager program is captured into graphs too).  Call only when ``active(sched)``."""
    g = (t - 1).clamp_min(0)
    S = int(sched.decay_steps)
    if sched.type == "cosine":
        x = g.clamp_max(S).to(torch.float32) / float(S)
        a = np.float32(sched.alpha)
        c = (np.float32(1.0) - a) * np.float32(0.5)
        m = float(a) + float(c) * (1.0 + torch.cos(float(_PI32) * x))
    elif sched.type in ("exponential", "inverse_time"):
        if sched.staircase:
            x = torch.div(g, S, rounding_mode="floor").to(torch.float32)
        else:
            x = g.to(torch.float32) / float(S)
        r = float(np.float32(sched.decay_rate))
        m = torch.pow(torch.full_like(x, r), x) if sched.type == "exponential" else 1.0 / (1.0 + r * x)
    else:
        m = torch.ones_like(g, dtype=torch.float32)
    W = int(sched.warmup_steps)
    if W > 0:
        m = torch.where(g < W, m * ((g + 1).to(torch.float32) / float(W)), m)
    return m


def lr_torch(sched, lr: float, t: torch.Tensor) -> torch.Tensor:
    return float(np.float32(lr)) * mult_torch(sched, t)


# ------------------------------------------------------------------ host reporting
def lr_at(cfg, t: int) -> float:
    """The rate of 1-based step ``t`` as reported (metrics.jsonl, status.json): lr * m(t) in
    float32, Adam's bias correction excluded.  Host arithmetic only."""
    sched = getattr(cfg, "lr_schedule", None)
    if not active(sched):
        return float(cfg.effective_lr)
    return float(lr_f32(sched, cfg.effective_lr, int(t)))
