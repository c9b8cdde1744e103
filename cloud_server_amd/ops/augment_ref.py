"""The one definition of training-time augmentation: NumPy float32 (the reference) and torch.

``options.augment`` (``models.dsl.Augment``) warps every training image anew at every step:
an integer shift, a rotation by a whole number of degrees, a zoom by a whole percentage and
one erased rectangle.  The augmented image is a pure function of (seed, step, dataset row),
drawn from the counter RNG shared bit for bit between NumPy, torch and the device
(``preprocess.ops_ref.crng`` == ``crng.h`` == ``dropout_ref.crng_torch``), so it is never
stored and needs no checkpoint state: the eager model, the HIP kernel (csrc/kernels/
augment.hip) and a resumed job all form the same bytes.  Only uint8 28x28 datasets.

Draws
* ``aug_seed(cfg_seed) = smix(uint64(cfg_seed) ^ AUG_SEED_XOR)``, ``AUG_SEED_XOR =
  0x6175676D656E7421`` (the ASCII bytes of "augment!").
* Draw ``k`` (0..7) of dataset row ``row`` at step ``t`` is ``r_k = crng(aug_seed,
  t & 0xFFFFFFFF, row * 8 + k)``.  ``t`` is the number of completed training steps (the device
  counter before this step's head advances it: dropout's convention); ``row`` indexes the
  DATASET, not the batch, so world-N data parallelism draws what one process on the global
  batch draws, and a row that occurs twice in a batch gets the same image twice.

Parameters (s = ``shift``, R = ``rotate``, P = ``scale``, E = ``erase_max``)
* ``dx = r0 % (2s+1) - s``, ``dy = r1 % (2s+1) - s``      (pixels)
* ``a = r2 % (2R+1)``: the angle is ``a - R`` degrees;  ``ca = COS[a]``, ``sa = SIN[a]``
* ``z = r3 % (2P+1)``: the zoom is ``(100 + q) / 100`` with ``q = z - P``;  ``inv = INV[z]``
* ``COS[a] = float32(cos(radians(a - R)))``, ``SIN`` likewise, ``INV[z] = float32(100 /
  (100 + z - P))``: host-built tables, computed in float64 and rounded to float32 once.  The
  reference, the torch form and the kernel read the same tables (``Plan``); nothing evaluates
  a trigonometric function per pixel.

Inverse map of output pixel (x, y), fp32, no contraction, in the order written, with
``c = 13.5f``, ``u = (x - c) - dx``, ``v = (y - c) - dy``::

    sx = ((ca * u) + (sa * v)) * inv + c
    sy = ((ca * v) - (sa * u)) * inv + c

Bilinear sampling: ``x0 = floorf(sx)``, ``fx = sx - x0`` (same for y); the four taps are read
as uint8 -> float and a tap outside the image reads ``fill``::

    top = (1 - fx) * p00 + fx * p01        bot = (1 - fx) * p10 + fx * p11
    val = (1 - fy) * top + fy * bot        out = uint8(min(floorf(val + 0.5f), 255))

Erase, after the warp: gate ``(r4 >> 8) < T`` with ``T = round(erase_prob * 2^24)`` clamped to
``[0, 2^24]``; ``eh = 1 + r5 % E``, ``ew = 1 + r6 % E``, ``top = (r7 & 0xFFFF) % (H - eh + 1)``,
``left = (r7 >> 16) % (W - ew + 1)``; the pixels of that rectangle become ``fill``.

Only +, -, x and floor occur, so IEEE fp32 gives the same bytes on every side; the device
function is compiled with contraction off (a fused multiply-add rounds once where this
definition rounds twice).  With s = R = P = 0 the warp is the identity, with R = P = 0 an
integer shift with ``fill``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np
import torch

from ..preprocess.ops_ref import _smix, crng
from .dropout_ref import crng_torch

_M64 = (1 << 64) - 1
AUG_SEED_XOR = 0x6175676D656E7421
HW = 28                                   # models.dsl.INPUT_HW: the only image size in scope
MAX_ROTATE, MAX_SCALE = 45, 30            # table sizes of the kernel's argument struct
_CENTRE = np.float32(13.5)


def active(cfg) -> bool:
    """False when the config asks for no augmentation (no option, or every amount zero):
    every path then runs exactly the code it ran before the option existed."""
    a = getattr(cfg, "augment", cfg)
    return a is not None and bool(a.shift or a.rotate or a.scale or a.erase_prob > 0.0)


def aug_seed(cfg_seed: int) -> int:
    z = np.array((int(cfg_seed) & _M64) ^ AUG_SEED_XOR, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(_smix(z))


def erase_threshold(erase_prob: float) -> int:
    return min(max(int(round(float(erase_prob) * (1 << 24))), 0), 1 << 24)


class AugParamsC(C.Structure):
    """``csa::AugParams`` (csrc/kernels/augment.hip), passed to the launcher by pointer and
    read on the host; the tables travel to the kernel by value."""
    _fields_ = [("shift", C.c_int), ("rotate", C.c_int), ("scale", C.c_int), ("erase_max", C.c_int),
                ("fill", C.c_int), ("erase_T", C.c_int),
                ("cos", C.c_float * (2 * MAX_ROTATE + 1)), ("sin", C.c_float * (2 * MAX_ROTATE + 1)),
                ("inv", C.c_float * (2 * MAX_SCALE + 1))]


class Plan:
    """An ``Augment`` bound to a config seed: the seed of its draws and the float32 tables."""

    def __init__(self, aug, cfg_seed: int):
        self.aug = aug
        self.seed = aug_seed(cfg_seed)
        self.s, self.R, self.P = int(aug.shift), int(aug.rotate), int(aug.scale)
        self.E, self.fill = int(aug.erase_max), int(aug.fill)
        self.T = erase_threshold(aug.erase_prob)
        deg = np.arange(-self.R, self.R + 1, dtype=np.float64)
        self.cos = np.cos(np.radians(deg)).astype(np.float32)
        self.sin = np.sin(np.radians(deg)).astype(np.float32)
        q = np.arange(-self.P, self.P + 1, dtype=np.float64)
        self.inv = (100.0 / (100.0 + q)).astype(np.float32)
        self._torch: Dict[torch.device, tuple] = {}

    def to_c(self) -> AugParamsC:
        p = AugParamsC(self.s, self.R, self.P, self.E, self.fill, self.T)
        for dst, src in ((p.cos, self.cos), (p.sin, self.sin), (p.inv, self.inv)):
            for i, v in enumerate(src):
                dst[i] = float(v)
        return p

    def tables_torch(self, device):
        device = torch.device(device)
        if device not in self._torch:
            self._torch[device] = tuple(torch.from_numpy(t.copy()).to(device) for t in (self.cos, self.sin, self.inv))
        return self._torch[device]


def make_plan(cfg) -> Optional[Plan]:
    """The plan of a ``TrainConfig`` (None: no augmentation)."""
    return Plan(cfg.augment, cfg.seed) if active(cfg) else None


# ------------------------------------------------------------------ NumPy float32 (the reference)
def draws(plan: Plan, rows, step: int) -> np.ndarray:
    """uint64 [B, 8]: the eight draws of every row at ``step``."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    k = np.arange(8, dtype=np.uint64)[None, :]
    return crng(plan.seed, np.uint64(int(step) & 0xFFFFFFFF), rows * np.uint64(8) + k)


def erase_rects(plan: Plan, rows, step: int) -> np.ndarray:
    """int64 [B, 5]: (erased, top, left, eh, ew) of every row at ``step``."""
    r = draws(plan, rows, step).astype(np.int64)
    eh, ew = 1 + r[:, 5] % plan.E, 1 + r[:, 6] % plan.E
    top, left = (r[:, 7] & 0xFFFF) % (HW - eh + 1), (r[:, 7] >> 16) % (HW - ew + 1)
    return np.stack([((r[:, 4] >> 8) < plan.T).astype(np.int64), top, left, eh, ew], axis=1)


def augment_np(plan: Plan, images_u8: np.ndarray, rows, step: int) -> np.ndarray:
    """uint8 [B, 784]: ``images_u8`` [B, 784] (the gathered dataset rows ``rows``) augmented
    for ``step``."""
    f32, one = np.float32, np.float32(1.0)
    img = np.asarray(images_u8, dtype=np.uint8).reshape(-1, HW, HW)
    B = img.shape[0]
    r = draws(plan, rows, step).astype(np.int64)
    assert r.shape[0] == B
    n = 2 * plan.s + 1
    dx = (r[:, 0] % n - plan.s).astype(f32)[:, None, None]
    dy = (r[:, 1] % n - plan.s).astype(f32)[:, None, None]
    a = r[:, 2] % (2 * plan.R + 1)
    ca, sa = plan.cos[a][:, None, None], plan.sin[a][:, None, None]
    inv = plan.inv[r[:, 3] % (2 * plan.P + 1)][:, None, None]
    x = np.arange(HW, dtype=f32)[None, None, :]
    y = np.arange(HW, dtype=f32)[None, :, None]
    u = (x - _CENTRE) - dx
    v = (y - _CENTRE) - dy
    sx = ((ca * u) + (sa * v)) * inv + _CENTRE
    sy = ((ca * v) - (sa * u)) * inv + _CENTRE
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    fill = f32(plan.fill)
    bi = np.arange(B)[:, None, None]

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < HW) & (xx >= 0) & (xx < HW)
        p = img[bi, np.clip(yy, 0, HW - 1), np.clip(xx, 0, HW - 1)].astype(f32)
        return np.where(ok, p, fill)

    top = (one - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)
    bot = (one - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1)
    val = (one - fy) * top + fy * bot
    assert val.dtype == np.float32
    out = np.minimum(np.floor(val + f32(0.5)), f32(255.0)).astype(np.uint8)
    # erase
    eh, ew = 1 + r[:, 5] % plan.E, 1 + r[:, 6] % plan.E
    et = ((r[:, 7] & 0xFFFF) % (HW - eh + 1))[:, None, None]
    el = ((r[:, 7] >> 16) % (HW - ew + 1))[:, None, None]
    gate = ((r[:, 4] >> 8) < plan.T)[:, None, None]
    yi, xi = np.arange(HW)[None, :, None], np.arange(HW)[None, None, :]
    inside = gate & (yi >= et) & (yi < et + eh[:, None, None]) & (xi >= el) & (xi < el + ew[:, None, None])
    out = np.where(inside, np.uint8(plan.fill), out)
    return out.reshape(B, HW * HW)


# ------------------------------------------------------------------ torch (device ops only)
def augment_torch(plan: Plan, images_u8: torch.Tensor, rows: torch.Tensor, step: torch.Tensor) -> torch.Tensor:
    """``augment_np`` from device ops alone (graph-capturable, like ``keep_mask_torch``):
    uint8 [B, 784] for the gathered uint8 rows ``images_u8`` [B, 784], their int64 dataset
    rows ``rows`` [B] and the one-element int64 step tensor."""
    dev = images_u8.device
    B = images_u8.shape[0]
    cos_t, sin_t, inv_t = plan.tables_torch(dev)
    k = torch.arange(8, dtype=torch.int64, device=dev)[None, :]
    r = crng_torch(plan.seed, step.to(torch.int64).view(1, 1) & 0xFFFFFFFF, rows.to(torch.int64).view(B, 1) * 8 + k)
    n = 2 * plan.s + 1
    dx = (r[:, 0] % n - plan.s).to(torch.float32).view(B, 1, 1)
    dy = (r[:, 1] % n - plan.s).to(torch.float32).view(B, 1, 1)
    a = r[:, 2] % (2 * plan.R + 1)
    ca, sa = cos_t[a].view(B, 1, 1), sin_t[a].view(B, 1, 1)
    inv = inv_t[r[:, 3] % (2 * plan.P + 1)].view(B, 1, 1)
    x = torch.arange(HW, dtype=torch.float32, device=dev).view(1, 1, HW)
    y = torch.arange(HW, dtype=torch.float32, device=dev).view(1, HW, 1)
    c = float(_CENTRE)
    u = (x - c) - dx
    v = (y - c) - dy
    sx = ((ca * u) + (sa * v)) * inv + c
    sy = ((ca * v) - (sa * u)) * inv + c
    x0f, y0f = torch.floor(sx), torch.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    x0, y0 = x0f.to(torch.int64), y0f.to(torch.int64)
    src = images_u8.reshape(B, HW * HW).to(torch.float32)
    fill = float(plan.fill)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < HW) & (xx >= 0) & (xx < HW)
        idx = (yy.clamp(0, HW - 1) * HW + xx.clamp(0, HW - 1)).view(B, HW * HW)
        return torch.where(ok, src.gather(1, idx).view(B, HW, HW), fill)

    top = (1.0 - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)
    bot = (1.0 - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1)
    val = (1.0 - fy) * top + fy * bot
    out = torch.floor(val + 0.5).clamp_max(255.0).to(torch.uint8)
    eh, ew = 1 + r[:, 5] % plan.E, 1 + r[:, 6] % plan.E
    et = ((r[:, 7] & 0xFFFF) % (HW - eh + 1)).view(B, 1, 1)
    el = ((r[:, 7] >> 16) % (HW - ew + 1)).view(B, 1, 1)
    gate = ((r[:, 4] >> 8) < plan.T).view(B, 1, 1)
    yi = torch.arange(HW, device=dev).view(1, HW, 1)
    xi = torch.arange(HW, device=dev).view(1, 1, HW)
    inside = gate & (yi >= et) & (yi < et + eh.view(B, 1, 1)) & (xi >= el) & (xi < el + ew.view(B, 1, 1))
    out = torch.where(inside, torch.full_like(out, plan.fill), out)
    return out.view(B, HW * HW)


def check_dataset(images) -> None:
    """Augmentation is defined for uint8 [N, 784] (28x28) datasets only."""
    dt = str(getattr(images, "dtype", "")).replace("torch.", "")
    shape = tuple(getattr(images, "shape", ()))
    if dt != "uint8" or len(shape) != 2 or shape[1] != HW * HW:
        raise ValueError(f"options.augment needs a uint8 dataset of {HW}x{HW} images "
                         f"([N, {HW * HW}]); got {dt} {list(shape)}")
