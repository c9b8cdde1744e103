"""The geometry grid without a GPU: the conv / pool geometry itself, and the fp64 oracle.

The fp64 oracle and the eager engine share ``dsl.same_pads`` and ``models/cnn.py``, so a
geometry mistake there is invisible to every test that compares the two.  Here conv2d and
max-pool are written again as plain NumPy float64 loops from TensorFlow's definition (SAME:
out = ceil(in / s), total pad = max((out - 1) s + k - in, 0), ``total // 2`` before and the
rest after; VALID: out = (in - k) // s + 1, no pad; pool padding is -inf; the pool gradient
goes to the first maximum in row-major window order) and compared with ``cnn.py`` in float64
on every conv and pool layer of ``geometry_nets``, to 1e-12 of the layer's largest output.

Then three steps of the eager CPU engine against ``Oracle64`` on every network, as
``test_oracle64_cpu`` does for the step tests' networks — all in one process, the strided 1x1
conv of ``unit_stride_mixed`` included (torch 2.10.0+rocm7.0: the mkldnn backward of such a
conv corrupts the heap; ``cnn.py`` subsamples instead).
"""
import numpy as np
import pytest
import torch

import geometry_nets as G
import oracle64 as X

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.cnn import build_model
from cloud_server_amd.models.dsl import ConvSpec, PoolSpec
from cloud_server_amd.runtime.engine import TrainEngine

RTOL = 1e-12
LR = X.LRS["AdagradOptimizer"]


# ---- TensorFlow's geometry, written out ------------------------------------------------
def tf_axis(size: int, k: int, s: int, padding: str):
    """(out, pad before, pad after) of one axis."""
    if padding == "VALID":
        return (size - k) // s + 1, 0, 0
    out = (size + s - 1) // s
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


def np_conv2d(x: np.ndarray, w: np.ndarray, b, stride, padding: str) -> np.ndarray:
    """x [B, H, W, Cin], w [kh, kw, Cin, Cout] -> [B, OH, OW, Cout]; zero padding."""
    B, H, W, _ = x.shape
    kh, kw, _, cout = w.shape
    (oh, pt, _), (ow, pl, _) = tf_axis(H, kh, stride[0], padding), tf_axis(W, kw, stride[1], padding)
    y = np.zeros((B, oh, ow, cout), np.float64)
    for n in range(B):
        for oy in range(oh):
            for ox in range(ow):
                acc = np.zeros(cout, np.float64)
                for i in range(kh):
                    yy = oy * stride[0] - pt + i
                    if yy < 0 or yy >= H:
                        continue
                    for j in range(kw):
                        xx = ox * stride[1] - pl + j
                        if 0 <= xx < W:
                            acc += x[n, yy, xx] @ w[i, j]
                y[n, oy, ox] = acc
    return y if b is None else y + b


def np_max_pool(x: np.ndarray, kernel, stride, padding: str, dy=None):
    """[B, H, W, C] -> [B, OH, OW, C] (padding is -inf); with ``dy`` also the input gradient:
    every window sends its dy to its FIRST maximum in row-major window order."""
    B, H, W, C = x.shape
    (kh, kw), (sh, sw) = kernel, stride
    (oh, pt, _), (ow, pl, _) = tf_axis(H, kh, sh, padding), tf_axis(W, kw, sw, padding)
    y = np.full((B, oh, ow, C), -np.inf)
    dx = np.zeros_like(x) if dy is not None else None
    for n in range(B):
        for oy in range(oh):
            for ox in range(ow):
                for c in range(C):
                    best, at = -np.inf, None
                    for i in range(kh):
                        yy = oy * sh - pt + i
                        if yy < 0 or yy >= H:
                            continue
                        for j in range(kw):
                            xx = ox * sw - pl + j
                            if 0 <= xx < W and x[n, yy, xx, c] > best:
                                best, at = x[n, yy, xx, c], (yy, xx)
                    y[n, oy, ox, c] = best
                    if dx is not None:
                        dx[n, at[0], at[1], c] += dy[n, oy, ox, c]
    return y, dx


# ---- every conv and pool layer of the table ---------------------------------------------
def _geometry_layers():
    out = []
    for name, layers in G.NETS.items():
        plan = X.make_cfg(layers, batch=2).plan()
        out += [(name, lp.index) for lp in plan.layers if isinstance(lp.spec, (ConvSpec, PoolSpec))]
    return out


@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


@pytest.fixture(scope="module")
def traced(dataset):
    """Per network: the fp64 model and the input of every layer for two images."""
    cache = {}

    def get(name):
        if name not in cache:
            cfg = X.make_cfg(G.NETS[name], batch=2)
            m = build_model(cfg, "cpu").train().double()
            h = (torch.from_numpy(np.ascontiguousarray(dataset.images[:2])).double() / 255.0).reshape(2, 28, 28, 1)
            ins = []
            with torch.no_grad():
                for lp in m.plan.layers:
                    ins.append(h)
                    h = m._layer(lp, h, True)
            cache[name] = (m, ins)
        return cache[name]
    return get


def _close(got: np.ndarray, want: np.ndarray, what: str) -> None:
    assert got.shape == want.shape, f"{what}: shape {got.shape}, the definition gives {want.shape}"
    scale = np.abs(want[np.isfinite(want)]).max()
    err = np.abs(got - want).max()
    assert err <= RTOL * scale, f"{what}: err {err:.3e} of max {scale:.3e}"


@pytest.mark.parametrize("name,index", _geometry_layers(), ids=lambda v: str(v))
def test_layer_matches_loop_reference(name, index, traced):
    m, ins = traced(name)
    lp = m.plan.layers[index]
    sp = lp.spec
    x = ins[index]
    what = f"{name} {lp.name}"
    if isinstance(sp, ConvSpec):
        with torch.no_grad():
            got = m._layer(lp, x, True).numpy()
        w = m.p(f"{lp.name}.weight").detach().numpy()
        b = m.p(f"{lp.name}.bias").detach().numpy() if sp.bias else None
        want = np_conv2d(x.numpy(), w, b, sp.stride, sp.padding)
        assert want.shape[1:3] == tuple(lp.out_shape.hw), what
        _close(got, want, what)
        return
    # pool: the traced input, then small integers (ties in almost every window) with a
    # different upstream gradient for every output
    rng = np.random.default_rng(index)
    tied = rng.integers(0, 3, size=tuple(x.shape)).astype(np.float64)
    for label, inp in (("traced", x.numpy()), ("ties", tied)):
        t = torch.from_numpy(inp).requires_grad_(True)
        y = m._layer(lp, t, True)
        dy = rng.standard_normal(tuple(y.shape))
        (dx,) = torch.autograd.grad((y * torch.from_numpy(dy)).sum(), t)
        want_y, want_dx = np_max_pool(inp, sp.kernel, sp.stride, sp.padding, dy)
        assert want_y.shape[1:3] == tuple(lp.out_shape.hw), what
        _close(y.detach().numpy(), want_y, f"{what} ({label})")
        _close(dx.numpy(), want_dx, f"{what} ({label}) backward")


def test_strided_1x1_conv_is_a_subsampled_conv():
    """The strided 1x1 conv of ``cnn.py`` (a subsample, then stride 1) against the loop
    reference, values and gradients, for every stride of the reported crash and two more."""
    rng = np.random.default_rng(0)
    for stride in ((2, 1), (1, 2), (2, 2), (3, 1), (2, 3)):
        for padding in ("SAME", "VALID"):
            layers = [G.conv(3, 3, 3), G.conv(1, 1, 5, stride=stride, valid=padding == "VALID", bias=True), G.FC]
            m = build_model(X.make_cfg(layers, batch=2), "cpu").train().double()
            lp = m.plan.layers[1]
            x = torch.from_numpy(rng.standard_normal((2, 28, 28, 3))).requires_grad_(True)
            y = m._layer(lp, x, True)
            dy = rng.standard_normal(tuple(y.shape))
            dx, dflat = torch.autograd.grad((y * torch.from_numpy(dy)).sum(), [x, m.flat])
            w = m.p(f"{lp.name}.weight").detach().numpy()
            want = np_conv2d(x.detach().numpy(), w, m.p(f"{lp.name}.bias").detach().numpy(), stride, padding)
            _close(y.detach().numpy(), want, f"1x1 stride {stride} {padding}")
            # dx: only the sampled pixels receive a gradient, dy @ w^T each
            want_dx = np.zeros((2, 28, 28, 3))
            want_dx[:, ::stride[0], ::stride[1]] = dy @ w[0, 0].T
            _close(dx.numpy(), want_dx, f"1x1 stride {stride} {padding} dx")
            want_dw = np.einsum("bhwi,bhwo->io", x.detach().numpy()[:, ::stride[0], ::stride[1]], dy)
            got_dw = m.state.view(f"{lp.name}.weight", dflat).numpy()[0, 0]
            _close(got_dw, want_dw, f"1x1 stride {stride} {padding} dw")


# ---- the oracle against the eager engine -------------------------------------------------
@pytest.mark.parametrize("name", list(G.NETS))
def test_oracle_matches_eager_cpu(name, dataset):
    cfg = X.make_cfg(G.NETS[name], "AdagradOptimizer", LR)
    eng = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    recs = X.run_trajectory(eng, X.Oracle64(cfg, dataset), 3)
    X.check(recs, X.tolerances(name, LR), name)
