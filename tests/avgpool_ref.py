"""Average pooling: a float64 NumPy loop reference, the kernel geometries and the networks.

A plain helper module (no tests, no fixtures) for ``test_avgpool_cpu`` and
``test_gpu_avgpool``.  The reference is written from the definition (``tf.nn.avg_pool``) and
shares no code with ``models/cnn.py``, ``models/dsl.py`` or the kernels:

* output (oy, ox) covers rows ``oy*sh - pt .. + kh`` and columns ``ox*sw - pl .. + kw``; it is
  the sum of the taps that lie inside the image, in (dy, dx) row-major order, divided by
  their number -- padding enters neither the sum nor the divisor;
* the backward gives pixel p the sum, over the windows o that contain it in (oy, ox) order,
  of ``dy[o] / n_o``; a pixel no window covers gets 0.
"""
from __future__ import annotations

import copy

import numpy as np

from cloud_server_amd.models.dsl import SAMPLE_CONFIG

U = 2.0 ** -24          # unit roundoff of fp32


def out_and_pad(size: int, k: int, s: int, padding: str):
    """TF's geometry of one axis: (output size, padding in front)."""
    if padding == "VALID":
        return (size - k) // s + 1, 0
    out = (size + s - 1) // s
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2


def geometry(H, W, kh, kw, sh, sw, padding):
    OH, pt = out_and_pad(H, kh, sh, padding)
    OW, pl = out_and_pad(W, kw, sw, padding)
    return OH, OW, pt, pl


def _window(o, s, p, k, size):
    lo = o * s - p
    return max(lo, 0), min(lo + k, size)


def avg_fwd(x: np.ndarray, kh, kw, sh, sw, padding) -> np.ndarray:
    """x: [B, H, W, C] -> float64 [B, OH, OW, C]."""
    x = np.asarray(x, dtype=np.float64)
    B, H, W, C = x.shape
    OH, OW, pt, pl = geometry(H, W, kh, kw, sh, sw, padding)
    y = np.zeros((B, OH, OW, C), np.float64)
    for oy in range(OH):
        y0, y1 = _window(oy, sh, pt, kh, H)
        for ox in range(OW):
            x0, x1 = _window(ox, sw, pl, kw, W)
            acc = np.zeros((B, C), np.float64)
            for yy in range(y0, y1):
                for xx in range(x0, x1):
                    acc = acc + x[:, yy, xx, :]
            y[:, oy, ox, :] = acc / float((y1 - y0) * (x1 - x0))
    return y


def avg_bwd(dy: np.ndarray, H, W, kh, kw, sh, sw, padding) -> np.ndarray:
    """dy: [B, OH, OW, C] -> float64 dx [B, H, W, C] (the windows visited in (oy, ox) order)."""
    dy = np.asarray(dy, dtype=np.float64)
    B, OH, OW, C = dy.shape
    assert (OH, OW) == geometry(H, W, kh, kw, sh, sw, padding)[:2]
    _, _, pt, pl = geometry(H, W, kh, kw, sh, sw, padding)
    dx = np.zeros((B, H, W, C), np.float64)
    for oy in range(OH):
        y0, y1 = _window(oy, sh, pt, kh, H)
        for ox in range(OW):
            x0, x1 = _window(ox, sw, pl, kw, W)
            share = dy[:, oy, ox, :] / float((y1 - y0) * (x1 - x0))
            for yy in range(y0, y1):
                for xx in range(x0, x1):
                    dx[:, yy, xx, :] += share
    return dx


def covered(H, W, kh, kw, sh, sw, padding) -> np.ndarray:
    """[H, W] bool: the pixels at least one window contains."""
    OH, OW, pt, pl = geometry(H, W, kh, kw, sh, sw, padding)
    m = np.zeros((H, W), bool)
    for oy in range(OH):
        y0, y1 = _window(oy, sh, pt, kh, H)
        for ox in range(OW):
            x0, x1 = _window(ox, sw, pl, kw, W)
            m[y0:y1, x0:x1] = True
    return m


def fwd_bound(n_taps: int, xmax: float) -> float:
    """|y - y64| <= 2 n u max|x|: n - 1 adds and one division (any fold order has at most
    n - 1 adds on a path)."""
    return 2.0 * n_taps * U * xmax


def bwd_bound(kh, kw, sh, sw, dymax: float) -> float:
    """|dx - dx64| <= 2 (m + 1) u max|dy|, m = ceil(kh/sh) ceil(kw/sw) windows per pixel."""
    m = -(-kh // sh) * -(-kw // sw)
    return 2.0 * (m + 1) * U * dymax


# (B, H, W, C, kh, kw, sh, sw, padding): the smallest shapes at which each index path can go wrong
GEOMETRIES = [
    (2, 7, 7, 3, 2, 2, 2, 2, "SAME"),          # odd map, edge windows of 2 and 1 taps, scalar path
    (2, 7, 7, 8, 3, 3, 2, 2, "SAME"),          # overlap, padding on both sides, float4 path
    (3, 6, 5, 4, 3, 3, 1, 1, "SAME"),          # stride 1, every pixel in up to 9 windows
    (2, 9, 8, 5, 1, 3, 2, 4, "VALID"),         # rect window, stride > kernel: uncovered pixels are 0
    (2, 5, 5, 6, 7, 7, 1, 1, "SAME"),          # window larger than the map
    (1, 5, 5, 1, 5, 5, 5, 5, "VALID"),         # global, one channel
    (3, 7, 7, 64, 7, 7, 7, 7, "VALID"),        # global, wide C, 49 taps
    (2, 14, 14, 12, 14, 14, 14, 14, "VALID"),  # global, 196 taps
    (2, 28, 28, 1, 28, 28, 28, 28, "VALID"),   # global, 784 taps
]
GAPPED = GEOMETRIES[3]
# The launchers cap their grids at 2048 workgroups of 256 threads (524288 elements, or 8192
# waves = output positions in form 2, a pass): 6 * 64 * 64 * 23 = 565248 elements on the scalar
# path (C % 4 != 0) and 24576 positions need the grid-stride loop.
GRID_STRIDE_FWD = (6, 64, 64, 23, 3, 3, 1, 1, "SAME")
GRID_STRIDE_BWD = (6, 64, 64, 23, 2, 2, 2, 2, "SAME")


def geom_id(g) -> str:
    B, H, W, C, kh, kw, sh, sw, pad = g
    return f"{B}x{H}x{W}x{C}-k{kh}x{kw}-s{sh}x{sw}-{pad}"


# ---------------------------------------------------------------- the networks
def _sample_avg():
    layers = copy.deepcopy(SAMPLE_CONFIG["net_config"]["middle_layer"])
    assert layers[2] == {"layer": "pool"}
    layers[2]["mode"] = "avg"
    return layers


AVG = {"layer": "pool", "mode": "avg"}
RELU = {"layer": "active", "active_func": "relu"}
SIGMOID = {"layer": "active", "active_func": "sigmoid"}

NETS = {
    # pair without pool, pool unit, standalone bn, two dense
    "sample_avg": _sample_avg(),
    "lenet_avg": [
        {"layer": "conv", "filter": [5, 5, 6], "padding": "SAME"}, SIGMOID, dict(AVG),
        {"layer": "conv", "filter": [5, 5, 16], "padding": "VALID"}, SIGMOID, dict(AVG),
        {"layer": "connect", "hidden": 32}, SIGMOID, {"layer": "connect", "hidden": 16}],
    "avg_overlap_same": [
        {"layer": "conv", "filter": [3, 3, 5]}, RELU,
        dict(AVG, kernel=[3, 3], stride=[2, 2], padding="SAME"), {"layer": "connect", "hidden": 16}],
    "avg_gap_rect": [
        {"layer": "conv", "filter": [3, 3, 4]}, RELU,
        dict(AVG, kernel=[1, 3], stride=[2, 4], padding="VALID"), {"layer": "connect", "hidden": 16}],
    "avg_after_norm": [
        {"layer": "conv", "filter": [3, 3, 4]}, {"layer": "norm"}, RELU, dict(AVG), {"layer": "norm"},
        {"layer": "connect", "hidden": 16}],
    # the pool reads the gathered images and has no backward launch
    "avg_first": [dict(AVG), {"layer": "conv", "filter": [3, 3, 4]}, RELU, {"layer": "connect", "hidden": 16}],
    # global average straight into the head (head_in == 12)
    "gap_head": [
        {"layer": "conv", "filter": [3, 3, 8]}, RELU, {"layer": "pool"},
        {"layer": "conv", "filter": [3, 3, 12]}, RELU, dict(AVG, kernel="global")],
}


def layers_of(name: str) -> list:
    return copy.deepcopy(NETS[name])
