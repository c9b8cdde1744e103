"""Depthwise convolution on the GPU: ``csa_dw_fwd`` / ``csa_dw_bwd`` / ``csa_dw_bwd_params``
(depthwise_conv.hip) against the float64 loop reference (tests/dwconv_ref.py) in every form, the
lowered ``dw`` unit against the eager program and the fp64 oracle, deterministic mode, the
forward-only programs (serving, validation), packed jobs, world-1 data parallelism and resume.

Kernel bound (the project's own, ``dwconv_ref.kernel_bound``): with e32 the error of the fp32 eager
layer on the CPU against the float64 loops on the same inputs, a kernel's error against the
float64 loops is at most ``max(4 e32, 8 u max|ref|)``, u = 2^-24, for y, dx, dw and dbias.  For
dw and dbias, sums of B OH OW terms in an order that is not torch's, ``_check_sum`` also prints
the worked worst case of the kernel's own order."""
import copy
import math
import os
import socket

import numpy as np
import pytest
import torch

import dwconv_ref as R
import oracle64 as X

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, DepthwiseConvSpec, parse_train_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = -123.0
ADAGRAD = "AdagradOptimizer"
ALL_GEOMS = R.GEOMETRIES + R.ROW_CAP
CASES = [(g, 8) for g in ALL_GEOMS] + [(g, 9) for g in R.SHIFTED]
ACT_IDS = {None: 0, "sigmoid": 1, "relu": 2, "leaky_relu": 3}
# each fused activation once (the backward reads y only: the leaky alpha is not negative)
ACT_CASES = [((2, 7, 6, 4, 2, 3, 3, 2, 2, "SAME"), "sigmoid", 0.0), ((2, 5, 5, 3, 1, 3, 3, 1, 1, "SAME"), "relu", 0.0),
             ((2, 9, 8, 5, 1, 5, 3, 2, 1, "VALID"), "leaky_relu", 0.2), ((2, 14, 14, 20, 1, 3, 3, 1, 1, "SAME"), "leaky_relu", 0.0)]


def _case_id(c) -> str:
    return R.geom_id(c[0]) + ("-plus1float" if c[1] == 9 else "")


# ----------------------------------------------------------------------- 1. the kernels
def _guarded(shape, off):
    """A tensor of ``shape`` that starts ``off`` floats into a sentinel-filled buffer (off = 8:
    16-byte aligned; off = 9: one float further, every element on the scalar path)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * off + 8,), FILL, device=DEV)
    return buf, buf[off:off + n].view(shape)


def _guards_intact(buf, off, n):
    return bool((buf[:off] == FILL).all()) and bool((buf[off + n:] == FILL).all())


def _dims(g):
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    OH, pt = R.out_pads(H, kh, sh, pad)
    OW, pl = R.out_pads(W, kw, sw, pad)
    return OH, OW, pt, pl


def _geom(K, g):
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    OH, OW, pt, pl = _dims(g)
    return K.ints([B, H, W, C, kh, kw, sh, sw, pt, pl, OH, OW, M])


def _fwd_forms(lib, g):
    """Every forward form the geometry has: 0, 2, and 1 when the weights fit its LDS budget."""
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    return [0, 2] + ([1] if kh * kw * C * M <= lib.csa_dw_lds_floats() else [])


def _depth(lib, K, g, form):
    """d, the additions on the longest path of a backward form's summation order, as the header
    comment of depthwise_conv.hip states it."""
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    OH, OW, _, _ = _dims(g)
    P, L = B * OH * OW, (kh * kw + 1) * C * M
    if form == 2:
        return math.ceil(P / 16) + 16
    Rr = lib.csa_dw_slab_rows(_geom(K, g))
    S = max(256 // L, 1)
    return math.ceil(math.ceil(P / Rr) / S) + S + Rr


@pytest.fixture(scope="module")
def references():
    """(geometry, act, alpha) -> (x, w, bias, dy, refs, e32s, mags) with refs = float64
    (y, dx, dw, dbias) of the loops, e32s the fp32 eager layer's errors against them on the CPU and
    mags = (max sum|x dz|, max sum|dz|) over the dw and dbias elements: computed once, shared,
    never changed."""
    cache = {}

    def get(g, act=None, alpha=0.0):
        key = (g, act, alpha)
        if key not in cache:
            x, w, bias, dy = R.inputs(g)
            y, dx, dw, db, absw, absb = R.dw_loops(g, x, w, bias, dy, act, alpha)
            refs = (y, dx, dw, db)
            got = R.eager(g, x, w, bias, dy, torch.float32, act, alpha)
            if got[3] is None:               # (no bias in the eager layer: dbias = sum dz, from dy alone)
                e_db = 0.0
            else:
                e_db = float(np.abs(got[3] - db).max())
            e32s = tuple(float(np.abs(a - r).max()) for a, r in zip(got[:3], refs[:3])) + (e_db,)
            cache[key] = (x, w, bias, dy, refs, e32s, (float(absw.max()), float(absb.max())))
        return cache[key]
    return get


def _check(label, name, got, ref, e32):
    bound = R.kernel_bound(e32, ref)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{label} {name}: e32 {e32:.3e} bound {bound:.3e} err {err:.3e} (max|ref| {np.abs(ref).max():.3e})")
    assert err <= bound, f"{label} {name}: err {err:.3e} > bound {bound:.3e}"


def _check_sum(label, name, got, ref, e32, mag, d):
    """dw and dbias: the project's bound, as for y and dx.  The issue allowed the worked worst
    case of the kernel's own summation order in its place, should torch's order happen to be the
    more accurate one; on an MI355X that never showed (every serial sum in the kernels is
    compensated: err was 0.03 to 0.2 of the project's bound at every geometry and form), so the
    project's bound is what is asserted.  The worked figure is still printed next to it: every
    term x dz is one rounding off and a sum whose longest path has d additions adds at most
    d u sum|x dz|, so |err| <= (d + 1) u max_out sum|x dz|, d from the header comment of
    depthwise_conv.hip (``_depth``)."""
    project = R.kernel_bound(e32, ref)
    worked = (d + 1) * R.U * mag
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{label} {name}: err {err:.3e} project bound {project:.3e} (e32 {e32:.3e}) worked bound {worked:.3e} "
          f"(d {d}, sum|terms| {mag:.3e})")
    assert err <= project, f"{label} {name}: err {err:.3e} > bound {project:.3e}"


def _run_case(K, lib, g, form, off, ref, act=None, alpha=0.0, label=""):
    """Forward (twice) and backward (dx, dx again, null dx) of one geometry in one form at one
    alignment: guards, inputs, equal bits, every element written, the bounds.  A forward form 1
    whose weights do not fit is refused; the backward then reads the y of form 2."""
    x, w, bias, dy, refs, e32s, mags = ref
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    OH, OW, _, _ = _dims(g)
    CM, taps = C * M, kh * kw
    geom, st = _geom(K, g), K.stream()
    aid = ACT_IDS[act]
    assert lib.csa_dw_ok(geom) == 1
    bufs = {}
    for name, arr in (("x", x), ("w", w), ("b", bias), ("g", dy)):
        if arr is None:
            bufs[name] = (None, None)
            continue
        bufs[name] = _guarded(arr.shape, off)
        bufs[name][1].copy_(torch.from_numpy(arr))
    (xbuf, xd), (wbuf, wd), (bbuf, bd), (gbuf, gd) = (bufs[k] for k in ("x", "w", "b", "g"))
    ybuf, yd = _guarded(dy.shape, off)
    ffwd = form
    if form not in _fwd_forms(lib, g):
        assert lib.csa_dw_fwd(K.ptr(xd), K.ptr(wd), K.ptr(bd), K.ptr(yd), geom, aid, alpha, form, st) != 0
        torch.cuda.synchronize()
        assert bool((ybuf == FILL).all())
        ffwd = 2
    outs = []
    for _ in range(2):
        ybuf.fill_(FILL)
        assert lib.csa_dw_fwd(K.ptr(xd), K.ptr(wd), K.ptr(bd), K.ptr(yd), geom, aid, alpha, ffwd, st) == 0
        torch.cuda.synchronize()
        assert _guards_intact(ybuf, off, yd.numel())
        assert bool((yd != FILL).all())                         # every element written
        outs.append(yd.cpu().clone())
    assert torch.equal(outs[0], outs[1])                        # no atomics: equal bits
    _check(label, "y", outs[0].numpy(), refs[0], e32s[0])
    # backward
    fb = lib.csa_dw_bwd_form(geom) if form == 0 else form
    assert fb in (1, 2)
    rows = lib.csa_dw_slab_rows(geom)
    assert 1 <= rows <= lib.csa_dw_max_rows()
    L = (taps + 1) * CM
    dxbuf, dxd = _guarded(x.shape, off)
    sbuf, sd = _guarded((rows, L), off)
    wgbuf, wgd = _guarded(w.shape, off)
    bgbuf, bgd = _guarded((CM,), off)
    want_db = bias is not None
    back = []
    for dx in (dxd, dxd, None):
        for b in (dxbuf, sbuf, wgbuf, bgbuf):
            b.fill_(FILL)
        assert lib.csa_dw_bwd(K.ptr(xd), K.ptr(wd), K.ptr(yd), K.ptr(gd), K.ptr(dx), K.ptr(sd), K.ptr(wgd),
                              K.ptr(bgd) if want_db else None, geom, aid, alpha, form, st) == 0
        if fb == 1:
            torch.cuda.synchronize()
            assert bool((sd != FILL).all())                     # every slab row stored whole
            assert bool((wgbuf == FILL).all()) and bool((bgbuf == FILL).all())
            assert lib.csa_dw_bwd_params(K.ptr(sd), rows, geom, K.ptr(wgd), K.ptr(bgd) if want_db else None, st) == 0
        torch.cuda.synchronize()
        for buf, t in ((dxbuf, dxd), (xbuf, xd), (wbuf, wd), (gbuf, gd), (ybuf, yd), (sbuf, sd), (wgbuf, wgd),
                       (bgbuf, bgd)):
            assert _guards_intact(buf, off, t.numel())
        if fb == 2:
            assert bool((sbuf == FILL).all())                   # the owner form has no slab
        assert bool((wgd != FILL).all())
        assert bool((bgd != FILL).all()) if want_db else bool((bgbuf == FILL).all())
        if dx is None:
            assert bool((dxbuf == FILL).all())                  # a first unit: nothing for the input
        else:
            assert bool((dxd != FILL).all())
        back.append((dxd.cpu().clone(), wgd.cpu().clone(), bgd.cpu().clone()))
    assert torch.equal(back[0][0], back[1][0])
    for k in (1, 2):
        assert torch.equal(back[0][k], back[1][k]) and torch.equal(back[0][k], back[2][k])
    for t, arr in ((xd, x), (wd, w), (gd, dy)):
        assert torch.equal(t.cpu(), torch.from_numpy(arr))
    assert torch.equal(yd.cpu(), outs[0])
    _check(label, "dx", back[0][0].numpy(), refs[1], e32s[1])
    d = _depth(lib, K, g, fb)
    _check_sum(label, "dw", back[0][1].numpy(), refs[2], e32s[2], mags[0], d)
    if want_db:
        _check_sum(label, "dbias", back[0][2].numpy(), refs[3], e32s[3], mags[1], d)
    return outs[0], back[0][0]


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernels_match_loop_reference(case, form, references):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    g, off = case
    y, dx = _run_case(K, lib, g, form, off, references(g), label=f"{_case_id(case)} form {form}")
    if g == (2, 4, 4, 2, 1, 1, 1, 3, 3, "SAME"):
        # stride 3, kernel 1: only rows and columns 0 and 3 are in a window; the rest get exactly 0
        seen = np.zeros((4, 4), dtype=bool)
        seen[np.ix_([0, 3], [0, 3])] = True
        dxn = dx.numpy()
        assert not dxn[:, ~seen].any() and dxn[:, seen].all()


@pytest.mark.parametrize("off", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("ac", ACT_CASES, ids=lambda a: f"{R.geom_id(a[0])}-{a[1]}{a[2]:g}")
def test_fused_activations_match_loop_reference(ac, off, references):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    g, act, alpha = ac
    for form in (1, 2):
        _run_case(K, lib, g, form, off, references(g, act, alpha), act, alpha,
                  label=f"{R.geom_id(g)} {act} form {form} off {off}")


def test_automatic_forms():
    """Which forms form = 0 picks, and that every geometry of the list is accepted."""
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    assert lib.csa_dw_lds_floats() == 8192 and lib.csa_dw_max_rows() == 256
    for g in ALL_GEOMS:
        geom = _geom(K, g)
        B, H, W, C, M, kh, kw, sh, sw, pad = g
        assert lib.csa_dw_ok(geom) == 1, g
        assert lib.csa_dw_form(geom) == (1 if M > 1 and kh * kw * C * M <= 1024 else 2), g
        assert lib.csa_dw_bwd_form(geom) == (1 if (kh * kw + 1) * C * M <= 8192 else 2), g
    big = (1, 7, 7, 256, 4, 7, 7, 1, 1, "SAME")               # 200 KB of weights: accepted, never staged
    assert lib.csa_dw_form(_geom(K, big)) == 2 and lib.csa_dw_bwd_form(_geom(K, big)) == 2
    # the measured choice (profiles/r20_notes.md): LDS weights only with a multiplier and few weights
    assert lib.csa_dw_form(_geom(K, (50, 14, 14, 20, 1, 3, 3, 1, 1, "SAME"))) == 2
    assert lib.csa_dw_form(_geom(K, (50, 14, 14, 20, 2, 5, 5, 1, 1, "SAME"))) == 1
    assert lib.csa_dw_form(_geom(K, (50, 14, 14, 64, 2, 5, 5, 1, 1, "SAME"))) == 2
    # the row cap binds: 39200 pixels would be 1225 rows of 32
    g = R.ROW_CAP[0]
    assert g[0] * g[1] * g[2] // 32 > lib.csa_dw_max_rows() == lib.csa_dw_slab_rows(_geom(K, g))
    assert lib.csa_dw_slab_rows(_geom(K, (2, 5, 5, 3, 1, 3, 3, 1, 1, "SAME"))) == 1
    assert lib.csa_dw_slab_rows(_geom(K, (2, 14, 14, 20, 1, 3, 3, 1, 1, "SAME"))) == 12


def test_launchers_refuse_without_launching():
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    g = (2, 5, 5, 4, 1, 3, 3, 1, 1, "SAME")
    good = [2, 5, 5, 4, 3, 3, 1, 1, 1, 1, 5, 5, 1]
    gi = K.ints(good)
    st = K.stream()
    xbuf, xd = _guarded((2, 5, 5, 4), 8)
    xd.zero_()
    wd = torch.ones(3, 3, 4, 1, device=DEV)
    bd = torch.ones(4, device=DEV)
    ybuf, yd = _guarded((2, 5, 5, 4), 8)
    dxbuf, dxd = _guarded((2, 5, 5, 4), 8)
    rows = lib.csa_dw_slab_rows(gi)
    sbuf, sd = _guarded((rows, 40), 8)
    wgbuf, wgd = _guarded((3, 3, 4, 1), 8)
    bgbuf, bgd = _guarded((4,), 8)
    nan, inf = float("nan"), float("inf")

    def fwd(x=xd, w=wd, b=bd, y=yd, geom=gi, act=0, alpha=0.0, form=0):
        return lib.csa_dw_fwd(K.ptr(x), K.ptr(w), K.ptr(b), K.ptr(y), geom, act, alpha, form, st)

    def bwd(x=xd, w=wd, y=xd, dy=xd, dx=dxd, slab=sd, dw=wgd, db=bgd, geom=gi, act=0, alpha=0.0, form=0):
        return lib.csa_dw_bwd(K.ptr(x), K.ptr(w), K.ptr(y), K.ptr(dy), K.ptr(dx), K.ptr(slab), K.ptr(dw), K.ptr(db),
                              geom, act, alpha, form, st)

    def params(slab=sd, r=rows, geom=gi, dw=wgd, db=bgd):
        return lib.csa_dw_bwd_params(K.ptr(slab), r, geom, K.ptr(dw), K.ptr(db), st)

    bads = []
    for k in range(13):
        if k not in (8, 9):
            bads += [good[:k] + [0] + good[k + 1:], good[:k] + [-good[k]] + good[k + 1:]]
    bads += [good[:8] + [-1] + good[9:], good[:9] + [-1] + good[10:],          # negative pads
             good[:8] + [3] + good[9:], good[:9] + [3] + good[10:],            # pads of a whole kernel
             [1 << 10, 1 << 11, 1 << 10, 1, 1, 1, 1, 1, 0, 0, 1 << 11, 1 << 10, 1],   # 2^31 elements
             [1, 4, 4, 1 << 20, 1, 1, 1, 1, 0, 0, 4, 4, 1 << 11],              # C M = 2^31
             [1, 300, 300, 1, 300, 300, 1, 1, 149, 149, 300, 300, 1]]          # 90000 taps
    for bad in bads:
        b = K.ints(bad)
        assert lib.csa_dw_ok(b) == 0 and lib.csa_dw_form(b) == 0 and lib.csa_dw_bwd_form(b) == 0, bad
        assert lib.csa_dw_slab_rows(b) == 0 and params(geom=b) != 0, bad
        for form in (0, 1, 2):
            assert fwd(geom=b, form=form) != 0 and bwd(geom=b, form=form) != 0, bad
    assert lib.csa_dw_ok(gi) == 1 and lib.csa_dw_ok(None) == 0
    for act in (-1, 4):
        assert fwd(act=act) != 0 and bwd(act=act) != 0
    for alpha in (nan, inf, -inf):                          # (it multiplies every element)
        assert fwd(act=3, alpha=alpha) != 0 and bwd(act=3, alpha=alpha) != 0, alpha
    assert bwd(act=3, alpha=-0.1) != 0                       # not invertible from y: lowered elsewhere
    for form in (-1, 3):
        assert fwd(form=form) != 0 and bwd(form=form) != 0
    # weights beyond forward form 1's LDS budget: that form is refused, the geometry is not
    big = K.ints([1, 7, 7, 256, 7, 7, 1, 1, 3, 3, 7, 7, 4])
    assert lib.csa_dw_ok(big) == 1 and fwd(geom=big, form=1) != 0
    # null pointers (a null bias, dx and db are the calls without them; the slab goes with
    # form 1 and dw with form 2)
    for kw in ({"x": None}, {"w": None}, {"y": None}, {"geom": None}):
        assert fwd(**kw) != 0, kw
    for kw in ({"x": None}, {"w": None}, {"y": None}, {"dy": None}, {"geom": None}, {"slab": None, "form": 1},
               {"dw": None, "form": 2}):
        assert bwd(**kw) != 0, kw
    for kw in ({"slab": None}, {"dw": None}, {"geom": None}, {"r": rows + 1}, {"r": 0}):
        assert params(**kw) != 0, kw
    torch.cuda.synchronize()
    for buf in (ybuf, dxbuf, sbuf, wgbuf, bgbuf):
        assert bool((buf == FILL).all())
    assert _guards_intact(xbuf, 8, xd.numel()) and not bool(xd.any())
    assert fwd() == 0 and bwd() == 0 and params() == 0      # (the good calls do launch)
    assert fwd(b=None) == 0 and bwd(dx=None, db=None, form=2, slab=None) == 0
    torch.cuda.synchronize()
    assert bool((yd != FILL).all()) and bool((wgd != FILL).all())


# ----------------------------------------------------------------------- 2. the lowering, one step vs eager
def _cfg(layers, **kw):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c["optimizer_name"] = kw.pop("optimizer", "GradientDescentOptimizer")
    c["learning_rate"] = kw.pop("lr", 0.5)
    c["loss_name"] = kw.pop("loss", "entropy")
    c["options"] = dict(batch_size=kw.pop("batch", 50), **kw)
    return parse_train_config(c)


def _check_lowering(name, prog):
    """A ``dw`` unit per layer, forward-only programs included; a slab only in training programs
    of the split form and never a zero region; the activation behind the layer is the unit's
    when its backward can be formed from y."""
    units = prog.units
    assert [u.kind for u in units] == R.KINDS[name], [u.kind for u in units]
    at = [k for k, u in enumerate(units) if u.kind == "dw"]
    assert len(at) == 1 == sum(isinstance(lp.spec, DepthwiseConvSpec) for lp in prog.e.model.plan.layers)
    u = units[at[0]]
    lp = u.layer
    assert isinstance(lp.spec, DepthwiseConvSpec) and u.pool is None and u.norm is None
    assert (u.act.func if u.act is not None else None) == R.ACTS[name]
    assert tuple(u.y.shape) == (prog.B,) + tuple(lp.out_shape.hw) + (lp.out_shape.c,)
    if prog.forward_only:
        assert u.dw_slab is None and u.dy is None and u.dw_form == 0
    else:
        row = (lp.spec.kh * lp.spec.kw + 1) * lp.out_shape.c
        assert u.dw_form == (1 if row <= 8192 else 2)
        if u.dw_form == 1:
            assert u.dw_slab.shape[1] == row and 1 <= u.dw_slab.shape[0] <= 256
            assert not any(r.data_ptr() == u.dw_slab.data_ptr() for r in prog.zero_regions + prog.zero_early)
    nxt = units[at[0] + 1].in_tf if at[0] + 1 < len(units) else prog.head_tf
    if name == "dw_leaky_neg":
        assert u.act is None and nxt.act is not None and nxt.act.alpha == -0.1 and nxt.norm is None
    elif name == "dw_separable":
        assert nxt.norm is None and nxt.act is None and units[2].pool is not None and units[3].in_tf.has_bn
        if not prog.forward_only and not prog.e.ctx.enabled:
            assert units[3].fused and units[4].fused
    else:
        assert nxt.norm is None and nxt.act is None
    if name == "dw_first":
        assert tuple(units[0].x.shape) == (prog.B, 28, 28, 1)
    if name == "dw_pair":
        assert prog.pair is not None and units[1].pool is not None      # conv conv pool: the pair
    if name == "dw_norm_act":
        assert units[2].norm is not None and units[2].act.func == "sigmoid"
    if name == "dw_head":
        assert prog.forward_only or prog.dlast is u.dy


def _run_one(cfg, backend, ds, name=None):
    from cloud_server_amd.runtime.engine import TrainEngine
    eng = TrainEngine(cfg, ds, device="cuda", backend=backend, use_graph=False)
    assert eng.backend == backend and not eng.fallback_reason, eng.fallback_reason
    if backend == "hip":
        _check_lowering(name, eng.program)
    w0 = eng.flat.clone()
    eng.step()
    torch.cuda.synchronize()
    return eng, w0, eng.flat.clone()


@pytest.mark.parametrize("name", list(R.NETS))
def test_lowering_and_step_match_torch(name):
    """Each network lowers to the expected unit kinds with an empty ``fallback_reason``; one step
    with the procedure and bound of test_hip_step.py::test_step_matches_torch."""
    ds = synthetic_mnist(400, seed=3)
    cfg = _cfg(R.layers_of(name), lr=0.5)
    eh, w0h, w1h = _run_one(cfg, "hip", ds, name)
    et, w0t, w1t = _run_one(cfg, "torch", ds)
    assert torch.equal(w0h, w0t)
    gh = (w0h - w1h) / cfg.effective_lr
    gt = (w0t - w1t) / cfg.effective_lr
    gmax = gt.abs().max().item()
    for k in eh.model.state.shapes:
        a, b = eh.model.state.view(k, gh), et.model.state.view(k, gt)
        scale = b.abs().max().item() + 1e-6
        err = (a - b).abs().max().item()
        print(f"{name} grad {k}: err {err:.3e} scale {scale:.3e}")
        assert err <= 2e-3 * scale + 1e-6 + 1e-5 * gmax, f"{name} grad {k}: err {err:.3e} scale {scale:.3e}"
    mh, mt = eh.metrics_since(0), et.metrics_since(0)
    assert abs(mh["loss"] - mt["loss"]) < 1e-4 * max(1, abs(mt["loss"]))
    assert mh["accuracy"] == mt["accuracy"]


def test_without_the_layer_the_plan_is_what_it_was():
    from cloud_server_amd.runtime.engine import TrainEngine
    eng = TrainEngine(_cfg(SAMPLE_CONFIG["net_config"]["middle_layer"]), synthetic_mnist(200, seed=3), device="cuda",
                      backend="hip", use_graph=False)
    assert eng.backend == "hip", eng.fallback_reason
    assert [u.kind for u in eng.program.units] == ["conv", "conv", "dense", "dense"]
    assert all(u.dw_slab is None and u.dw_form == 0 for u in eng.program.units) and eng.program.pair is not None


# ----------------------------------------------------------------------- 3. three steps vs the oracle
@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


ORACLE_GRID = [(n, b) for n in R.NETS for b in (50, 7)]


@pytest.mark.parametrize("name,batch", ORACLE_GRID, ids=[f"{n}-b{b}" for n, b in ORACLE_GRID])
def test_matches_fp64_oracle(name, batch, dataset):
    """The test_gpu_geometry.py procedure: three steps, each recomputed in fp64 from the
    engine's own state, health words 0, ``oracle64`` tolerances unchanged."""
    from cloud_server_amd.runtime.engine import TrainEngine
    cfg = X.make_cfg(R.layers_of(name), ADAGRAD, X.LRS[ADAGRAD], "entropy", batch)
    eng = TrainEngine(cfg, dataset, device="cuda", backend="hip", use_graph=False)
    assert eng.backend == "hip" and not eng.fallback_reason, eng.fallback_reason
    _check_lowering(name, eng.program)
    recs = X.run_trajectory(eng, X.Oracle64(cfg, dataset), 3)
    torch.cuda.synchronize()
    assert all(int(w.item()) == 0 for w in eng.health_words())
    X.check(recs, X.tolerances(name, X.LRS[ADAGRAD]), f"{name}-b{batch}")


# ----------------------------------------------------------------------- 4. deterministic mode
@pytest.mark.parametrize("name", ["dw_separable", "dw_first"])
def test_deterministic_graph_eager_and_group_are_bitwise_equal(name, monkeypatch):
    from cloud_server_amd.runtime.engine import TrainEngine
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    monkeypatch.setenv("CSA_GRAPH_STEPS", "8")
    ds = synthetic_mnist(600, seed=7)
    cfg = _cfg(R.layers_of(name), optimizer=ADAGRAD, lr=0.01)
    try:
        runs = []
        for mode in ("graph", "graph", "eager", "group"):
            eng = TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=mode != "eager")
            assert eng.backend == "hip" and eng.program.det, eng.fallback_reason
            _check_lowering(name, eng.program)
            if mode == "group":
                eng.step()
                eng.run_steps(11)
                assert eng.graph_k is not None
            else:
                for _ in range(12):
                    eng.step()
            eng.sync_device()
            assert int(eng.dstep.item()) == 12
            runs.append((eng.flat.clone(), eng.slots.clone()))
        for i in range(1, len(runs)):
            assert torch.equal(runs[0][0], runs[i][0]), f"{name} run {i}: parameters differ"
            assert torch.equal(runs[0][1], runs[i][1]), f"{name} run {i}: optimizer slots differ"
    finally:
        torch.use_deterministic_algorithms(False)


def test_the_unit_has_no_atomics_two_production_runs_are_equal():
    """Production mode: the unit's own launches, run twice on the step's buffers, give equal
    bits for y, the input gradient and the stored weight and bias gradients (other units of a
    production program may use atomics, so the unit is compared, not the trajectory)."""
    from cloud_server_amd.ops import fused as K
    from cloud_server_amd.runtime.engine import TrainEngine
    cfg = _cfg(R.layers_of("dw_pair"), optimizer=ADAGRAD, lr=0.01)
    eng = TrainEngine(cfg, synthetic_mnist(600, seed=7), device="cuda", backend="hip", use_graph=False)
    assert eng.backend == "hip" and not eng.program.det, eng.fallback_reason
    eng.step()
    eng.sync_device()
    prog = eng.program
    k = [u.kind for u in prog.units].index("dw")
    u, prev = prog.units[k], prog.units[k - 1]
    u.dy.copy_(torch.randn_like(u.dy))
    names = [f"{u.layer.name}.weight", f"{u.layer.name}.bias"]
    runs = []
    for _ in range(2):
        u.y.fill_(FILL)
        prev.dy.fill_(FILL)
        for n in names:
            prog.gviews[n].fill_(FILL)
        prog._standalone_fwd(u, K.stream())
        prog._standalone_bwd(u, prev, K.stream())
        torch.cuda.synchronize()
        runs.append([t.clone() for t in (u.y, prev.dy, prog.gviews[names[0]], prog.gviews[names[1]])])
    for a, b in zip(*runs):
        assert torch.equal(a, b) and bool((a != FILL).all())         # stored, never added


# ----------------------------------------------------------------------- 5. forward-only programs
@pytest.mark.parametrize("name", ["dw_separable", "dw_head"])
def test_serving_and_validation(name):
    """The checks of test_gpu_gn.py::test_serving_and_validation; validation leaves the training
    state bit for bit unchanged and the forward-only programs keep no slab."""
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.validation import HipValidator, TorchValidator
    from cloud_server_amd.serve.hip_infer import HipPredictor
    train, test = synthetic_mnist(1280, seed=0).split(0.8)
    c = _cfg(R.layers_of(name), optimizer="AdamOptimizer", lr=1e-3)
    eng = TrainEngine(c, train, device=DEV, backend="hip")
    assert eng.backend == "hip", eng.fallback_reason
    for _ in range(10):
        eng.step()
    eng.sync_device()
    dw = [u for u in eng.program.units if u.kind == "dw"]
    before = (eng.flat.clone(), eng.slots.clone(), [u.dw_slab.clone() for u in dw if u.dw_slab is not None])
    val = eng.validator(test, 64, True)
    assert isinstance(val, HipValidator) and val.program.forward_only
    _check_lowering(name, val.program)
    res = eng.validate(test, 64, True)
    tv = TorchValidator(eng, test, 64, predictions=True)
    tv.issue()
    want = tv.wait()[1]
    assert res.n == want.n == len(test)
    assert res.confusion == want.confusion
    # the training program's own forward-only pass
    idx = eng.stream.rows.index_select(0, eng.stream.cursor).view(-1)
    xb, _ = eng.data.batch(idx)
    eng.model.eval()
    with torch.no_grad():
        zt = eng.model(xb).cpu().numpy()
    eng.model.train()
    logits = torch.zeros(50, 10, device=DEV)
    eng.program.predict_logits_into(logits)
    torch.cuda.synchronize()
    scale = float(np.abs(zt).max())
    assert np.abs(logits.cpu().numpy() - zt).max() <= 2e-3 * scale + 1e-6 + 1e-5 * scale
    assert torch.equal(before[0], eng.flat) and torch.equal(before[1], eng.slots)
    assert all(torch.equal(a, u.dw_slab) for a, u in zip(before[2], [u for u in dw if u.dw_slab is not None]))
    # serving: 256 images through the HIP predictor
    state = eng.model.export_state()
    pred = HipPredictor(c, state, torch.device(DEV), buckets=(256,), preps=("mnist",))
    for bk in pred._buckets.values():
        _check_lowering(name, bk.program)
    x8 = np.ascontiguousarray(test.images[:256].reshape(256, 784))
    got = pred.logits_u8(x8, "mnist")
    cls = pred.predict_u8(x8, "mnist")
    eng.model.eval()
    with torch.no_grad():
        zs = eng.model(torch.from_numpy(x8).to(DEV).float().div_(255.0)).cpu().numpy()
    eng.model.train()
    scale = float(np.abs(zs).max())
    err = np.abs(got - zs).max()
    print(f"{name}: served logits err {err:.3e}, scale {scale:.3e}")
    assert err <= 2e-3 * scale + 1e-6 + 1e-5 * scale
    assert np.array_equal(np.asarray(cls).reshape(-1), zs.argmax(1))


# ----------------------------------------------------------------------- 6. packed jobs, world-1 data parallelism
def test_packed_jobs_with_dw_match_solo_runs():
    """Two jobs with the layer as branches of one graph (the packed launch profile,
    ``TrainEngine(packed=True)``) end where the same jobs trained alone end."""
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.multijob import PackedJobs
    names = ("dw_act_pool", "dw_separable")

    def eng(seed, packed):
        cfg = _cfg(R.layers_of(names[seed]), optimizer=ADAGRAD, lr=0.01, seed=seed)
        return TrainEngine(cfg, synthetic_mnist(600, seed=seed), device="cuda", backend="hip",
                           use_graph=packed, packed=packed)

    packed = [eng(s, True) for s in (0, 1)]
    assert all(e.backend == "hip" and e.program.packed for e in packed)
    for s, e in zip((0, 1), packed):
        _check_lowering(names[s], e.program)
    pack = PackedJobs(packed)
    for _ in range(4):
        pack.step()
    pack.sync_device()
    for s, e in zip((0, 1), packed):
        solo = eng(s, False)
        for _ in range(4):
            solo.step()
        solo.sync_device()
        assert e.host_step == 4 and int(e.dstep.item()) == 4
        d = (e.flat - solo.flat).abs().max().item()
        print(f"{names[s]}: packed vs solo {d:.3e}")
        assert d < 3e-3             # test_gpu_gn.py's: atomics elsewhere, run-to-run fp32 order


@pytest.fixture(scope="module")
def pg():
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from cloud_server_amd.parallel.dist import rccl_env_defaults
    rccl_env_defaults()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.mark.parametrize("strategy", ["allreduce", "ps"])
def test_world1_data_parallel_programs_match_single_gpu(pg, monkeypatch, strategy):
    """One process group of one rank whose context reports data parallelism as enabled (the
    pattern of test_gpu_dp_overlap.py): the dw unit's weight and bias gradients land in the flat
    gradient before the exchange, the flat optimizer updates them."""
    from cloud_server_amd.parallel.dist import DistContext
    from cloud_server_amd.runtime.engine import TrainEngine

    class _DPContext(DistContext):
        @property
        def enabled(self) -> bool:
            return True

    monkeypatch.setenv("CSA_XGMI", "0")
    cfg = _cfg(R.layers_of("dw_separable"), optimizer=ADAGRAD, lr=1e-3)
    ds = synthetic_mnist(2000, seed=0)
    ctx = _DPContext(rank=0, world=1, local_rank=0, backend="nccl", device=torch.device("cuda", 0))
    a = TrainEngine(cfg, ds, device="cuda:0", ctx=ctx, backend="hip", strategy=strategy)
    assert a.backend == "hip", a.fallback_reason
    _check_lowering("dw_separable", a.program)
    b = TrainEngine(cfg, ds, device="cuda:0", backend="hip")
    for _ in range(4):
        a.step(); b.step()
    a.run_steps(8); b.run_steps(8)
    a.sync_device(); b.sync_device()
    assert a.host_step == b.host_step == 12 and int(a.dstep.item()) == 12
    torch.testing.assert_close(a.flat, b.flat, rtol=2e-3, atol=2e-5)


# ----------------------------------------------------------------------- 7. resume
def test_resume_is_exact_on_the_hip_backend(monkeypatch):
    """Three steps, a checkpoint, a fresh engine restored from it and three more steps: the same
    bits as six steps in one engine (deterministic mode; the slab holds nothing a resume needs)."""
    from cloud_server_amd.runtime import checkpoint as ckpt
    from cloud_server_amd.runtime.engine import TrainEngine
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    ds = synthetic_mnist(600, seed=7)
    cfg = _cfg(R.layers_of("dw_separable"), optimizer="AdamOptimizer", lr=1e-3)

    def make():
        eng = TrainEngine(cfg, ds, device="cuda:0", backend="hip", use_graph=True)
        assert eng.backend == "hip" and eng.program.det, eng.fallback_reason
        return eng

    try:
        a = make()
        for _ in range(6):
            a.step()
        a.sync_device()
        b = make()
        for _ in range(3):
            b.step()
        b.sync_device()
        obj = ckpt.engine_state(b)
        c = make()
        ckpt.restore_engine(c, obj)
        for _ in range(3):
            c.step()
        c.sync_device()
        assert int(c.dstep.item()) == 6
        assert torch.equal(a.flat, c.flat) and torch.equal(a.slots, c.slots)
    finally:
        torch.use_deterministic_algorithms(False)
