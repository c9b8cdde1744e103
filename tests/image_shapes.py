"""Image-op shapes: the shape table, the image generators and plain float64 loop references.

A plain helper module (no tests, no fixtures) for ``test_image_ops_cpu`` and
``test_gpu_image_shapes``.  The loop references are written from the definitions and share no
code with ``preprocess/ops_ref.py`` or the kernels:

* NL-means: pixel p's output is ``sum_q w(p, q) v(q) / sum_q w(p, q)`` over the 21 x 21 shifts
  q - p, with ``w = exp(-d2 / h^2)`` and d2 the mean of the 49 squared differences of the 7 x 7
  patches around p and q, on the image padded by 13 with BORDER_REFLECT_101;
* erode / dilate: the min / max over the taps ``-(k // 2) .. k - 1 - k // 2`` (cv2's anchor
  ``k // 2``) that lie inside the image.
"""
from __future__ import annotations

import numpy as np

# (H, W) -> why it is here.  The three limit shapes run only on the op whose limit they are.
SHAPES = {
    (20, 36): "non-square, W > H; CLAHE with th != tw (3 x 5 tiles)",
    (36, 20): "non-square, H > W; CLAHE with th != tw (5 x 3 tiles)",
    (32, 32): "last box NL-means shape (H*W = 1024): all four per-thread pixel slots full",
    (33, 32): "first direct NL-means shape (H*W = 1056)",
    (7, 100): "extreme aspect on the box NL-means path; H below the CLAHE grid",
    (9, 8): "CLAHE with th = 2, tw = 1; filter windows larger than the image",
    (3, 50): "k/2 >= H: the reflection bounces more than once",
    (1, 17): "the n == 1 branch of reflect101, rows",
    (17, 1): "the n == 1 branch of reflect101, columns",
    (100, 64): "CLAHE padded 100 -> 104",
    (64, 128): "sep-filter limit (H*W = 8192)",
    (128, 128): "rank-filter limit (H*W = 16384)",
    (102, 102): "NL-means limit (padded 128 x 128)",
}
LIMIT_SHAPES = ((64, 128), (128, 128), (102, 102))
GENERAL_SHAPES = tuple(s for s in SHAPES if s not in LIMIT_SHAPES)

# the launchers' limits (csrc/kernels/image_ops.hip), restated
IMG_THREADS = 256
MAX_IMG_PIX = 128 * 128
SEP_MAX_PIX = MAX_IMG_PIX // 2
CLAHE_TILES = 8
NLM_TR, NLM_SR = 3, 10                     # 7 x 7 template, 21 x 21 search
ELEMENTWISE_CAP = 65536 * 256              # grid_for: elements one trip of a grid-stride loop covers


def sep_ok(H, W):
    return H * W <= SEP_MAX_PIX


def rank_ok(H, W):
    return H * W <= MAX_IMG_PIX


def clahe_ok(H, W):
    return H >= CLAHE_TILES and W >= CLAHE_TILES


def nlmeans_select(H, W, tr=NLM_TR, sr=NLM_SR):
    """csa_img_nlmeans' choice of kernel: 'box', 'direct' or 'refused'."""
    pad = tr + sr
    if H <= 0 or W <= 0 or H * W > MAX_IMG_PIX or (H + 2 * pad) * (W + 2 * pad) > MAX_IMG_PIX:
        return "refused"
    AW, AH = W + 2 * tr, H + 2 * tr
    if H * W <= 4 * IMG_THREADS and AH * AW <= 8 * IMG_THREADS and H * AW <= 8 * IMG_THREADS:
        lds = (((H + 2 * pad) * (W + 2 * pad) + 3) // 4 + AH * AW + H * AW) * 4
        if lds <= 64 * 1024:
            return "box"
    return "direct"


def random_u8(n, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W)).astype(np.uint8)


def smooth_u8(n, H, W, seed=1):
    """Digit-like images (a smooth blob plus noise) so NL-means weights are non-trivial; the
    centre lies in the middle 3/7 of each axis and the radius scales with min(H, W)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W))
    s = min(H, W) / 28.0
    for i in range(n):
        cy, cx, r = rng.uniform(8, 20) * H / 28.0, rng.uniform(8, 20) * W / 28.0, rng.uniform(4, 9) * s
        out[i] = 220 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    return np.clip(out + rng.normal(0, 12, out.shape), 0, 255).astype(np.uint8)


def reflect101(i, n):
    """The kernels' index reflection, restated: bounce until the index is inside."""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def pad_reflect101(img, r):
    """One 2-D image padded by r on every side through ``reflect101``."""
    H, W = img.shape
    ys = [reflect101(y, H) for y in range(-r, H + r)]
    xs = [reflect101(x, W) for x in range(-r, W + r)]
    return img[np.ix_(ys, xs)]


def nlmeans_loop(img, h, tr=NLM_TR, sr=NLM_SR):
    """One 2-D uint8 image -> uint8: per pixel, per shift, the (2tr+1)^2 squared-difference sum."""
    H, W = img.shape
    pad = tr + sr
    P = pad_reflect101(np.asarray(img, np.float64), pad)
    out = np.zeros((H, W), np.float64)
    area = float((2 * tr + 1) ** 2)
    for y in range(H):
        for x in range(W):
            py, px = y + pad, x + pad
            a = P[py - tr:py + tr + 1, px - tr:px + tr + 1]
            acc = wsum = 0.0
            for dy in range(-sr, sr + 1):
                for dx in range(-sr, sr + 1):
                    b = P[py + dy - tr:py + dy + tr + 1, px + dx - tr:px + dx + tr + 1]
                    d2 = float(((a - b) ** 2).sum()) / area
                    w = np.exp(-d2 / (h * h))
                    acc += w * P[py + dy, px + dx]
                    wsum += w
            out[y, x] = acc / wsum
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def window_loop(img, k, op):
    """One 2-D uint8 image -> uint8: ``op`` (min or max) over the in-image taps of the k x k
    window anchored at k // 2."""
    H, W = img.shape
    out = np.zeros((H, W), np.uint8)
    lo, hi = -(k // 2), k - 1 - k // 2
    for y in range(H):
        for x in range(W):
            vals = [img[y + dy, x + dx] for dy in range(lo, hi + 1) for dx in range(lo, hi + 1)
                    if 0 <= y + dy < H and 0 <= x + dx < W]
            out[y, x] = op(vals)
    return out
