"""Local response normalisation: a float64 NumPy loop reference, the kernel geometries and
the networks.

A plain helper module (no tests, no fixtures) for ``test_lrn_cpu`` and ``test_gpu_lrn``.  The
reference is written from the definition (``tf.nn.lrn``), as literal loops over the channel,
and shares no code with ``models/cnn.py``, ``models/dsl.py`` or the kernels:

    W(c) = [max(0, c - r), min(C - 1, c + r)]        (clipped to the channels, nothing padded in)
    s_c  = k + alpha * sum_{j in W(c)} x_j^2          (alpha is NOT divided by the window size)
    y_c  = x_c * s_c^(-beta)
    dx_c = dy_c * s_c^(-beta) - 2 alpha beta * x_c * sum_{j in W(c)} dy_j * y_j / s_j

The backward's window is W(c) too: it is symmetric, so {j : c in W(j)} = W(c).
"""
from __future__ import annotations

import copy

import numpy as np

from cloud_server_amd.models.dsl import SAMPLE_CONFIG

U = 2.0 ** -24          # unit roundoff of fp32


def lrn_scale(x: np.ndarray, r, k, alpha) -> np.ndarray:
    """s of x: [..., C], float64."""
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[-1]
    s = np.zeros_like(x)
    for c in range(C):
        acc = np.zeros(x.shape[:-1], np.float64)
        for j in range(max(0, c - r), min(C - 1, c + r) + 1):
            acc = acc + x[..., j] * x[..., j]
        s[..., c] = k + alpha * acc
    return s


def lrn_fwd(x: np.ndarray, r, k, alpha, beta) -> np.ndarray:
    """x: [..., C] -> float64 y of the same shape."""
    x = np.asarray(x, dtype=np.float64)
    return x * lrn_scale(x, r, k, alpha) ** (-beta)


def lrn_bwd(x: np.ndarray, dy: np.ndarray, r, k, alpha, beta) -> np.ndarray:
    """x, dy: [..., C] -> float64 dx."""
    x = np.asarray(x, dtype=np.float64)
    dy = np.asarray(dy, dtype=np.float64)
    C = x.shape[-1]
    s = lrn_scale(x, r, k, alpha)
    y = x * s ** (-beta)
    dx = np.zeros_like(x)
    for c in range(C):
        acc = np.zeros(x.shape[:-1], np.float64)
        for j in range(max(0, c - r), min(C - 1, c + r) + 1):
            acc = acc + dy[..., j] * y[..., j] / s[..., j]
        dx[..., c] = dy[..., c] * s[..., c] ** (-beta) - 2.0 * alpha * beta * x[..., c] * acc
    return dx


def kernel_bound(e32: float, ref: np.ndarray) -> float:
    """What a kernel's error against the float64 loop may be: four times the error e32 of the
    fp32 eager layer on the CPU on the same inputs (the margin the oracle tolerances give over
    fp32 eager, tests/oracle64.py), and never below 8 u max|ref| (a geometry at which the CPU
    happens to be nearly exact sets no unreachable bar)."""
    return max(4.0 * e32, 8.0 * U * float(np.abs(ref).max()))


# (B, H, W, C, r, k, alpha, beta): the smallest shapes at which each path can go wrong
GEOMETRIES = [
    (2, 3, 3, 1, 5, 1.0, 1.0, 0.5),            # C = 1: the window is the element
    (2, 3, 5, 7, 2, 1.0, 1.0, 0.5),            # odd C: scalar path, 9 rows a wave
    (2, 3, 5, 8, 1, 2.0, 1e-4, 0.75),          # C % 4 == 0: the 16-byte path; beta = 0.75
    (3, 2, 2, 20, 5, 1.0, 1.0, 0.5),           # the sample's C: 3 rows a wave, 4 idle lanes
    (2, 2, 3, 7, 9, 1.0, 0.5, 0.5),            # r >= C: every window is the whole row
    (2, 2, 2, 12, 0, 1.0, 1.0, 0.5),           # r = 0
    (2, 3, 2, 20, 12, 1.0, 0.1, 0.5),          # 2r + 1 > C > r + 1: windows wider than the row, clipped both ways
    (2, 3, 3, 64, 5, 1.0, 1.0, 0.5),           # a whole wave per row
    (2, 3, 3, 65, 5, 1.0, 1.0, 0.5),           # one past a wave: the LDS row, scalar path
    (2, 3, 3, 160, 5, 2.0, 1e-2, 1.0),         # past 128 (the gconv range); beta = 1
    (2, 3, 5, 12, 3, 1.0, 0.3, 0.6),           # a general beta: powf
    (2, 3, 5, 10, 3, 1.0, 0.3, 1.0),           # beta = 1: a reciprocal
    (3, 5, 3, 16, 4, 1.0, 0.001 / 9, 0.75),    # the CIFAR-10 tutorial's constants
]
# The launchers cap their grids at 2048 workgroups of 256 threads: 524288 elements in form 1,
# 8192 waves in form 2.  6 * 64 * 64 * 23 = 565248 elements on the scalar path, 12288 waves of
# two rows; 1 * 96 * 96 * 65 = 9216 rows of the LDS variant (a wave each) and 599040 elements.
GRID_STRIDE = [
    (6, 64, 64, 23, 2, 1.0, 1.0, 0.5),
    (1, 96, 96, 65, 2, 1.0, 1.0, 0.5),
]


def geom_id(g) -> str:
    B, H, W, C, r, k, alpha, beta = g
    return f"{B}x{H}x{W}x{C}-r{r}-k{k:g}-a{alpha:.3g}-b{beta:g}"


def inputs(g):
    """(x, dy) of a geometry: standard-normal float32, the same in every test."""
    B, H, W, C, r, k, alpha, beta = g
    rng = np.random.default_rng(H * 1000 + W * 10 + C + 7 * r)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    dy = rng.standard_normal((B, H, W, C)).astype(np.float32)
    return x, dy


# ---------------------------------------------------------------- the networks
def _lrn_sample():
    layers = copy.deepcopy(SAMPLE_CONFIG["net_config"]["middle_layer"])
    assert layers[2] == {"layer": "pool"}
    layers.insert(3, {"layer": "lrn"})
    return layers


RELU = {"layer": "active", "active_func": "relu"}
POOL32 = {"layer": "pool", "kernel": [3, 3], "stride": [2, 2]}
LRN_CIFAR = {"layer": "lrn", "depth_radius": 4, "bias": 1.0, "alpha": 0.001 / 9.0, "beta": 0.75}

NETS = {
    # the sample with lrn after the pool: pair, lrn unit, standalone bn, two dense
    "lrn_sample": _lrn_sample(),
    # TF's CIFAR-10 tutorial: conv -> pool -> norm1, conv -> norm2 -> pool
    "lrn_cifar": [
        {"layer": "conv", "filter": [5, 5, 8], "isBias": "True"}, RELU, dict(POOL32), dict(LRN_CIFAR),
        {"layer": "conv", "filter": [3, 3, 16]}, RELU, dict(LRN_CIFAR), dict(POOL32),
        {"layer": "connect", "hidden": 32}],
    # the unit reads the gathered images (C = 1) and has no backward launch
    "lrn_first": [{"layer": "lrn", "depth_radius": 2}, {"layer": "conv", "filter": [3, 3, 4]}, RELU,
                  {"layer": "connect", "hidden": 16}],
    # every window is the whole row; the head reads the unit's y and writes its dy
    "lrn_allchan_head": [
        {"layer": "pool"}, {"layer": "conv", "filter": [3, 3, 7], "stride": [2, 2]}, RELU,
        {"layer": "lrn", "depth_radius": 9, "alpha": 0.5}],
    # 160 channels: a gconv unit in front, the LDS-row form
    "lrn_wide160": [
        {"layer": "pool", "kernel": [4, 4], "stride": [4, 4]}, {"layer": "conv", "filter": [1, 1, 160]}, RELU,
        {"layer": "lrn", "depth_radius": 5, "bias": 2.0, "alpha": 1e-2, "beta": 1.0},
        {"layer": "pool", "mode": "avg", "kernel": "global"}, {"layer": "connect", "hidden": 16}],
}


def layers_of(name: str) -> list:
    return copy.deepcopy(NETS[name])


def without_lrn(layers: list) -> list:
    return [d for d in copy.deepcopy(layers) if d.get("layer") != "lrn"]
