"""Depthwise convolution: a float64 loop reference, the kernel geometries and the networks.

A plain helper module (no tests, no fixtures) for ``test_dwconv_cpu`` and ``test_gpu_dwconv``.
The reference is written from the definition and shares no code with ``models/cnn.py``,
``models/dsl.py``, ``F.conv2d`` or the kernels.  x is [B, H, W, C], w is [kh, kw, C, M] (TF's
filter layout), bias [C * M] or None, output channel c * M + q reads input channel c only:

    z[b, oh, ow, c M + q] = bias[c M + q] + sum_{di, dj} x[b, oh sh + di - pt, ow sw + dj - pl, c] w[di, dj, c, q]
    y = act(z),  dz = dy * act'(z)
    dx[b, ih, iw, c]  = sum_q sum_{windows containing (ih, iw)} dz[b, oh, ow, c M + q] w[di, dj, c, q]
    dw[di, dj, c, q]  = sum_{b, oh, ow} x[b, oh sh + di - pt, ow sw + dj - pl, c] dz[b, oh, ow, c M + q]
    dbias[c M + q]    = sum_{b, oh, ow} dz[b, oh, ow, c M + q]

over the in-image taps only.  ``dw_loops_scalar`` is the literal loop nest over
(b, oh, ow, c, q, di, dj); ``dw_loops`` is the same nest with the two channel loops (c, q)
written as one array statement each, so that the 200 KB-of-weights geometry takes seconds and
not minutes; ``test_dwconv_cpu`` holds the two equal on the small geometries.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

from cloud_server_amd.models.cnn import act_fwd, build_model
from cloud_server_amd.models.dsl import (SAMPLE_CONFIG, ActSpec, DepthwiseConvSpec, LayerPlan, TensorShape,
                                         parse_train_config)

U = 2.0 ** -24          # unit roundoff of fp32


def out_pads(size: int, k: int, s: int, pad: str):
    """(out, pad_before) of one axis, from TF's definition of SAME (even kernels pad after) and VALID."""
    if pad == "VALID":
        return (size - k) // s + 1, 0
    out = (size + s - 1) // s
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2


def _act(z: float, act, alpha: float):
    """(act(z), d act / dz) of one float64 value; ``act`` is None, "sigmoid", "relu" or "leaky_relu"."""
    if act is None:
        return z, 1.0
    if act == "sigmoid":
        s = 1.0 / (1.0 + math.exp(-z))
        return s, s * (1.0 - s)
    if act == "relu":
        return (z, 1.0) if z > 0 else (0.0, 0.0)
    assert act == "leaky_relu"
    return (z, 1.0) if z >= alpha * z else (alpha * z, alpha)      # tf.maximum(z, alpha * z)


def _act_arrays(z: np.ndarray, act, alpha: float):
    y, slope = np.empty_like(z), np.empty_like(z)
    for i, v in enumerate(z.ravel()):
        y.ravel()[i], slope.ravel()[i] = _act(float(v), act, alpha)
    return y, slope


def dw_loops_scalar(g, x, w, bias, dy=None, act=None, alpha=0.0):
    """The literal loops over (b, oh, ow, c, q, di, dj): float64 (y, dx, dw, dbias, absw, absb)."""
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    OH, pt = out_pads(H, kh, sh, pad)
    OW, pl = out_pads(W, kw, sw, pad)
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    z = np.zeros((B, OH, OW, C * M))
    for b in range(B):
        for oh in range(OH):
            for ow in range(OW):
                for c in range(C):
                    for q in range(M):
                        s = 0.0 if bias is None else float(bias[c * M + q])
                        for di in range(kh):
                            for dj in range(kw):
                                ih, iw = oh * sh + di - pt, ow * sw + dj - pl
                                if 0 <= ih < H and 0 <= iw < W:
                                    s += x[b, ih, iw, c] * w[di, dj, c, q]
                        z[b, oh, ow, c * M + q] = s
    y, slope = _act_arrays(z, act, alpha)
    if dy is None:
        return y
    dz = np.asarray(dy, dtype=np.float64) * slope
    dx, dw, db = np.zeros_like(x), np.zeros_like(w), np.zeros(C * M)
    absw, absb = np.zeros_like(w), np.zeros(C * M)
    for b in range(B):
        for oh in range(OH):
            for ow in range(OW):
                for c in range(C):
                    for q in range(M):
                        d = dz[b, oh, ow, c * M + q]
                        db[c * M + q] += d
                        absb[c * M + q] += abs(d)
                        for di in range(kh):
                            for dj in range(kw):
                                ih, iw = oh * sh + di - pt, ow * sw + dj - pl
                                if 0 <= ih < H and 0 <= iw < W:
                                    dx[b, ih, iw, c] += d * w[di, dj, c, q]
                                    dw[di, dj, c, q] += x[b, ih, iw, c] * d
                                    absw[di, dj, c, q] += abs(x[b, ih, iw, c] * d)
    return y, dx, dw, db, absw, absb


def dw_loops(g, x, w, bias, dy=None, act=None, alpha=0.0):
    """The same loops over (b, oh, ow, di, dj) with the channel loops (c, q) as one array
    statement each: float64 (y, dx, dw, dbias, absw, absb), the last two the sums of |x dz| and
    |dz| behind every dw and dbias element (the worked bound of the GPU tests)."""
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    OH, pt = out_pads(H, kh, sh, pad)
    OW, pl = out_pads(W, kw, sw, pad)
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    z = np.zeros((B, OH, OW, C, M))
    if bias is not None:
        z += np.asarray(bias, dtype=np.float64).reshape(C, M)
    for b in range(B):
        for oh in range(OH):
            for ow in range(OW):
                for di in range(kh):
                    for dj in range(kw):
                        ih, iw = oh * sh + di - pt, ow * sw + dj - pl
                        if 0 <= ih < H and 0 <= iw < W:
                            z[b, oh, ow] += x[b, ih, iw, :, None] * w[di, dj]          # all (c, q)
    z = z.reshape(B, OH, OW, C * M)
    if act is None:
        y, slope = z, np.ones_like(z)
    elif act == "sigmoid":
        y = 1.0 / (1.0 + np.exp(-z))
        slope = y * (1.0 - y)
    elif act == "relu":
        y, slope = np.where(z > 0, z, 0.0), (z > 0).astype(np.float64)
    else:
        assert act == "leaky_relu"
        own = z >= alpha * z
        y, slope = np.where(own, z, alpha * z), np.where(own, 1.0, alpha)
    if dy is None:
        return y
    dz = (np.asarray(dy, dtype=np.float64) * slope).reshape(B, OH, OW, C, M)
    dx, dw = np.zeros_like(x), np.zeros_like(w)
    absw = np.zeros_like(w)
    for b in range(B):
        for oh in range(OH):
            for ow in range(OW):
                for di in range(kh):
                    for dj in range(kw):
                        ih, iw = oh * sh + di - pt, ow * sw + dj - pl
                        if 0 <= ih < H and 0 <= iw < W:
                            d = dz[b, oh, ow]                                        # [C, M]
                            dx[b, ih, iw] += (d * w[di, dj]).sum(axis=1)             # sum over q
                            t = x[b, ih, iw, :, None] * d
                            dw[di, dj] += t
                            absw[di, dj] += np.abs(t)
    db = np.zeros(C * M)
    absb = np.zeros(C * M)
    for b in range(B):
        for oh in range(OH):
            for ow in range(OW):
                db += dz[b, oh, ow].reshape(-1)
                absb += np.abs(dz[b, oh, ow].reshape(-1))
    return y, dx, dw, db, absw, absb


def kernel_bound(e32: float, ref: np.ndarray) -> float:
    """What a kernel's error against the float64 loops may be: the project's own bound
    (``tests/gn_ref.kernel_bound``): four times the error e32 of the fp32 eager layer on the CPU
    on the same inputs, and never below 8 u max|ref|."""
    return max(4.0 * e32, 8.0 * U * float(np.abs(ref).max()))


def layer_plan(g, bias: bool, index: int = 1) -> LayerPlan:
    """The LayerPlan of a geometry, written out by hand (the map need not be square)."""
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    OH, pt = out_pads(H, kh, sh, pad)
    OW, pl = out_pads(W, kw, sw, pad)
    pb = max((OH - 1) * sh + kh - H - pt, 0) if pad == "SAME" else 0
    pr = max((OW - 1) * sw + kw - W - pl, 0) if pad == "SAME" else 0
    sp = DepthwiseConvSpec(kh, kw, M, (sh, sw), pad, "norm", bias)
    params = {"weight": (kh, kw, C, M)}
    if bias:
        params["bias"] = (C * M,)
    return LayerPlan(index, sp, TensorShape(C, (H, W)), TensorShape(C * M, (OH, OW)), (pt, pb, pl, pr), params)


def eager(g, x, w, bias, dy, dtype=torch.float32, act=None, alpha=0.0, det=False):
    """The eager layer (``DigitNet._layer``, then ``act_fwd``) on the CPU in ``dtype`` with w and
    bias as the layer's parameters: (y, dx, dw, dbias) by autograd, as float64 arrays (dbias is
    None without a bias).  In float32 its error against the loops is the e32 of ``kernel_bound``."""
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    cfg = copy.deepcopy(SAMPLE_CONFIG)
    ent = {"layer": "depthwise", "filter": [kh, kw, M]}
    if bias is not None:
        ent["isBias"] = "True"
    cfg["net_config"]["middle_layer"] = [{"layer": "conv", "filter": [1, 1, C]}, ent]
    m = build_model(parse_train_config(cfg)).to(dtype)
    m.deterministic = det
    lp = layer_plan(g, bias is not None)
    with torch.no_grad():
        m.p("layers.1.weight").copy_(torch.from_numpy(w))
        if bias is not None:
            m.p("layers.1.bias").copy_(torch.from_numpy(bias))
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = m._layer(lp, xt, True)
    if act is not None:
        y = act_fwd(y, ActSpec(act, alpha))
    assert y.dtype == dtype and tuple(y.shape) == (B,) + lp.out_shape.hw + (C * M,)
    dx, dflat = torch.autograd.grad(y, [xt, m.flat], torch.from_numpy(dy).to(dtype))
    gv = m.state.views(dflat)
    out = [y, dx, gv["layers.1.weight"], gv["layers.1.bias"] if bias is not None else None]
    return tuple(None if t is None else t.detach().double().numpy() for t in out)


# (B, H, W, C, M, kh, kw, sh, sw, padding): each chosen for one way to go wrong
GEOMETRIES = [
    (2, 5, 5, 3, 1, 3, 3, 1, 1, "SAME"),         # the plain case
    (2, 7, 6, 4, 2, 3, 3, 2, 2, "SAME"),         # non-square map, multiplier 2, odd and even extents under stride 2
    (1, 6, 6, 1, 3, 2, 2, 1, 1, "SAME"),         # even kernel (pads after), C = 1, M = 3: the c M + q order
    (2, 9, 8, 5, 1, 5, 3, 2, 1, "VALID"),        # rectangular kernel, mixed strides
    (2, 4, 4, 2, 1, 1, 1, 3, 3, "SAME"),         # stride larger than the kernel: input pixels with gradient exactly 0
    (2, 2, 2, 3, 1, 5, 5, 1, 1, "SAME"),         # kernel larger than the map
    (3, 5, 5, 70, 1, 3, 3, 1, 1, "SAME"),        # channels beyond one wave
    (2, 3, 3, 130, 2, 3, 3, 1, 1, "SAME"),       # C M = 260
    (2, 14, 14, 20, 1, 3, 3, 1, 1, "SAME"),      # the sample's map
    (1, 7, 7, 256, 4, 7, 7, 1, 1, "SAME"),       # 200 KB of weights: the form that does not stage them in LDS
]
# 39200 pixels: at 32 pixels a row the split form would want 1225 slab rows; the cap is 256, so
# every workgroup's range is 153 or 154 pixels
ROW_CAP = [(50, 28, 28, 8, 1, 3, 3, 1, 1, "SAME")]
# run a second time on buffers shifted by one float: the scalar path
SHIFTED = [GEOMETRIES[0], GEOMETRIES[1], GEOMETRIES[6], GEOMETRIES[7], GEOMETRIES[8]]


def geom_id(g) -> str:
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    return f"{B}x{H}x{W}x{C}-M{M}-k{kh}x{kw}-s{sh}x{sw}-{pad}"


def has_bias(g) -> bool:
    """Every other geometry carries a bias (the rest run the null-bias calls)."""
    return (GEOMETRIES + ROW_CAP).index(g) % 2 == 0


def inputs(g):
    """(x, w, bias or None, dy) of a geometry, float32, the same in every test."""
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    OH, OW = out_pads(H, kh, sh, pad)[0], out_pads(W, kw, sw, pad)[0]
    rng = np.random.default_rng(B * 1000003 + H * 10007 + W * 1009 + C * 101 + M * 11 + kh * 7 + kw * 3 + sh)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((kh, kw, C, M)) / math.sqrt(kh * kw)).astype(np.float32)
    bias = (0.3 * rng.standard_normal(C * M)).astype(np.float32) if has_bias(g) else None
    dy = rng.standard_normal((B, OH, OW, C * M)).astype(np.float32)
    return x, w, bias, dy


# ---------------------------------------------------------------- the networks
RELU = {"layer": "active", "active_func": "relu"}
SIGMOID = {"layer": "active", "active_func": "sigmoid"}


def _separable() -> list:
    """The sample with a 3x3 depthwise + 1x1 conv in place of its second conv."""
    layers = copy.deepcopy(SAMPLE_CONFIG["net_config"]["middle_layer"])
    assert layers[1] == {"layer": "conv", "filter": [2, 2, 20]}
    layers[1:2] = [{"layer": "depthwise", "filter": [3, 3, 1]}, {"layer": "conv", "filter": [1, 1, 20]}]
    return layers


NETS = {
    # the unit reads the gathered images: no input gradient, but weight and bias gradients
    "dw_first": [{"layer": "depthwise", "filter": [3, 3, 2], "isBias": "True"}, RELU, {"layer": "pool"},
                 {"layer": "connect", "hidden": 16}],
    "dw_act_pool": [{"layer": "conv", "filter": [3, 3, 4]}, RELU, {"layer": "depthwise", "filter": [3, 3, 1]}, RELU,
                    {"layer": "pool"}, {"layer": "connect", "hidden": 16}],
    "dw_separable": _separable(),
    # a norm behind the layer has no conv producer: a standalone bn unit with the activation
    "dw_norm_act": [{"layer": "conv", "filter": [3, 3, 4], "stride": [2, 2]},
                    {"layer": "depthwise", "filter": [3, 3, 2], "stride": [2, 2]}, {"layer": "norm"}, SIGMOID,
                    {"layer": "connect", "hidden": 16}],
    "dw_pair": [{"layer": "conv", "filter": [2, 2, 10]}, {"layer": "conv", "filter": [2, 2, 20]}, {"layer": "pool"},
                {"layer": "depthwise", "filter": [3, 3, 1], "isBias": "True"}, RELU, {"layer": "connect", "hidden": 16}],
    # maximum(z, -0.1 z) is not invertible from y: the activation stays pending
    "dw_leaky_neg": [{"layer": "conv", "filter": [3, 3, 4], "stride": [2, 2]}, {"layer": "depthwise", "filter": [3, 3, 1]},
                     {"layer": "active", "active_func": "leaky_relu", "param": [-0.1]},
                     {"layer": "connect", "hidden": 16}],
    # directly before the head
    "dw_head": [{"layer": "conv", "filter": [3, 3, 4], "stride": [2, 2]}, RELU, {"layer": "pool"},
                {"layer": "depthwise", "filter": [3, 3, 2], "stride": [2, 2], "padding": "VALID", "isBias": "True"},
                SIGMOID],
}
KINDS = {
    "dw_first": ["dw", "pool", "dense"],
    "dw_act_pool": ["conv", "dw", "pool", "dense"],
    "dw_separable": ["conv", "dw", "conv", "dense", "dense"],
    "dw_norm_act": ["conv", "dw", "bn", "dense"],
    "dw_pair": ["conv", "conv", "dw", "dense"],
    "dw_leaky_neg": ["conv", "dw", "dense"],
    "dw_head": ["conv", "dw"],
}
# the activation that rides in each dw unit's launches
ACTS = {"dw_first": "relu", "dw_act_pool": "relu", "dw_separable": None, "dw_norm_act": None, "dw_pair": "relu",
        "dw_leaky_neg": None, "dw_head": "sigmoid"}


def layers_of(name: str) -> list:
    return copy.deepcopy(NETS[name])
