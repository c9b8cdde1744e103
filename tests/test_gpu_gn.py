"""Layer / group / instance normalisation on the GPU: ``csa_gn_fwd`` / ``csa_gn_bwd`` /
``csa_gn_bwd_params`` (group_norm.hip) against the float64 loop reference (tests/gn_ref.py) in
every form, the lowered ``gn`` unit against the eager program and the fp64 oracle, deterministic
mode, the forward-only programs (serving, validation), packed jobs and world-1 data parallelism.

Kernel bound (the project's own, ``gn_ref.kernel_bound``): with e32 the error of the fp32 eager
layer on the CPU against the float64 loops on the same inputs, a kernel's error against the
float64 loops is at most ``max(4 e32, 8 u max|ref|)``, u = 2^-24, for y, dx, dscale and doffset."""
import copy
import os
import socket

import numpy as np
import pytest
import torch

import gn_ref as R
import oracle64 as X

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, GroupNormSpec, parse_train_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = -123.0
ADAGRAD = "AdagradOptimizer"
ALL_GEOMS = R.GEOMETRIES + R.GRID_STRIDE
CASES = [(g, False) for g in ALL_GEOMS] + [(g, True) for g in R.SHIFTED]
ACT_IDS = {None: 0, "sigmoid": 1, "relu": 2, "leaky_relu": 3}
# each fused activation once (the leaky alpha is negative: not invertible from y)
ACT_CASES = [((2, 3, 3, 20, 4), "sigmoid", 0.0), ((2, 2, 3, 8, 2), "relu", 0.0), ((3, 3, 5, 7, 1), "leaky_relu", -0.1),
             ((2, 14, 14, 20, 1), "leaky_relu", 0.2)]


def _case_id(c) -> str:
    return R.geom_id(c[0]) + ("-shifted" if c[1] else "")


# ----------------------------------------------------------------------- 1. the kernels
def _guarded(shape, off):
    """A tensor of ``shape`` that starts ``off`` floats into a sentinel-filled buffer (off = 8:
    16-byte aligned; off = 9: one float further, every element on the scalar path)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * off + 8,), FILL, device=DEV)
    return buf, buf[off:off + n].view(shape)


def _guards_intact(buf, off, n):
    return bool((buf[:off] == FILL).all()) and bool((buf[off + n:] == FILL).all())


def _geom(K, g):
    B, H, W, C, G = g
    return K.ints([B, H * W, C, G])


def _forms(lib, g):
    """Every form the geometry has: 0, and each named form whose register budget holds a group."""
    B, H, W, C, G = g
    m = H * W * C // G
    return [0] + [f for f in (1, 2, 3) if m <= lib.csa_gn_form_max(f)]


@pytest.fixture(scope="module")
def references():
    """(geometry, shifted, act, alpha) -> (x, dy, scale, offset, refs, e32s) with refs = float64
    (y, dx, dscale, doffset, mean [B, G], rstd [B, G]) of the loops and e32s the fp32 eager layer's errors against them on
    the CPU: computed once, shared, never changed."""
    cache = {}

    def get(g, shifted=False, act=None, alpha=0.0):
        key = (g, shifted, act, alpha)
        if key not in cache:
            x, dy, sc, of = R.inputs(g, shifted)
            y, mean, rstd, dx, dsc, dof = R.gn_loops(x, sc, of, g[4], R.EPS, dy, act, alpha)
            refs = (y, dx, dsc, dof, mean, rstd)
            got = R.eager(g, x, dy, sc, of, torch.float32, act, alpha)
            e32s = tuple(float(np.abs(a - r).max()) for a, r in zip(got, refs))
            cache[key] = (x, dy, sc, of, refs, e32s)
        return cache[key]
    return get


def _check(label, name, got, ref, e32):
    bound = R.kernel_bound(e32, ref)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{label} {name}: e32 {e32:.3e} bound {bound:.3e} err {err:.3e} (max|ref| {np.abs(ref).max():.3e})")
    assert err <= bound, f"{label} {name}: err {err:.3e} > bound {bound:.3e}"


def _check_stat(label, kept, x, mean64, rstd64):
    """The kept {mean, rstd} per (b, g) against the loops.  The eager layer exposes neither, so
    the bounds are worked out, worst case.  A sum in any form is at most 98 serial adds in a
    thread (form 3 at 100352 elements; 16 in forms 1 and 2), 6 tree levels and 16 waves: 120
    roundings.  The mean is mean0 + sum(x - mean0) / m: one rounding of the result at |mean| and
    the second sum's error at the size of the deviations, 4 u max|x| + 128 u / min rstd.  The
    variance is a sum of squares of deviations that are each one rounding off, about the
    corrected mean: 123 u of itself whatever the offset of x, so rstd, its root's reciprocal, is
    within 64 u of itself."""
    B, G = mean64.shape
    got = kept.numpy().astype(np.float64).reshape(B, G, 2)
    e_mean = float(np.abs(got[..., 0] - mean64).max())
    b_mean = 4.0 * R.U * float(np.abs(x).max()) + 128.0 * R.U / float(rstd64.min())
    e_rstd = float(np.abs(got[..., 1] / rstd64 - 1.0).max())
    print(f"{label} stat: mean err {e_mean:.3e} bound {b_mean:.3e}, rstd rel err {e_rstd:.3e} bound {64 * R.U:.3e}")
    assert e_mean <= b_mean and e_rstd <= 64.0 * R.U, label


def _run_case(K, lib, g, form, off, ref, act=None, alpha=0.0, label=""):
    """Forward (statistics kept, kept again, not kept) and backward (dx, dx again, null dx) of one
    geometry in one form at one alignment: guards, inputs, equal bits, every element written,
    the bound."""
    x, dy, sc, of, refs, e32s = ref
    B, H, W, C, G = g
    geom, st = _geom(K, g), K.stream()
    aid = ACT_IDS[act]
    assert lib.csa_gn_ok(geom) == 1 and form in _forms(lib, g)
    xbuf, xd = _guarded(x.shape, off)
    xd.copy_(torch.from_numpy(x))
    gbuf, gd = _guarded(x.shape, off)
    gd.copy_(torch.from_numpy(dy))
    scd, ofd = torch.from_numpy(sc).to(DEV), torch.from_numpy(of).to(DEV)
    ybuf, yd = _guarded(x.shape, off)
    sbuf, sd = _guarded((B, G, 2), 8)
    outs = []
    for stat in (sd, sd, None):
        ybuf.fill_(FILL)
        sbuf.fill_(FILL)
        assert lib.csa_gn_fwd(K.ptr(xd), K.ptr(scd), K.ptr(ofd), K.ptr(yd), K.ptr(stat), geom, R.EPS, aid, alpha,
                              form, st) == 0
        torch.cuda.synchronize()
        assert _guards_intact(ybuf, off, yd.numel()) and _guards_intact(xbuf, off, xd.numel())
        assert _guards_intact(sbuf, 8, sd.numel())
        assert bool((yd != FILL).all())                         # every element written
        if stat is None:
            assert bool((sbuf == FILL).all())                   # a forward-only program keeps nothing
        else:
            assert bool((sd != FILL).all())
            kept = sd.cpu().clone()
        outs.append(yd.cpu().clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])     # no atomics: equal bits
    assert torch.equal(xd.cpu(), torch.from_numpy(x))
    _check(label, "y", outs[0].numpy(), refs[0], e32s[0])
    _check_stat(label, kept, x, refs[4], refs[5])
    # backward: what it reads is what the forward of the same form kept
    sd.copy_(kept)
    dxbuf, dxd = _guarded(x.shape, off)
    lbuf, ld = _guarded((B, 2, C), 8)
    pbuf, pd = _guarded((2, C), 8)
    back = []
    for dx in (dxd, dxd, None):
        for b in (dxbuf, lbuf, pbuf):
            b.fill_(FILL)
        assert lib.csa_gn_bwd(K.ptr(xd), K.ptr(scd), K.ptr(ofd), K.ptr(sd), K.ptr(gd), K.ptr(dx), K.ptr(ld), geom,
                              aid, alpha, form, st) == 0
        assert lib.csa_gn_bwd_params(K.ptr(ld), B, C, K.ptr(pd[0]), K.ptr(pd[1]), st) == 0
        torch.cuda.synchronize()
        for buf, t, o in ((dxbuf, dxd, off), (xbuf, xd, off), (gbuf, gd, off), (lbuf, ld, 8), (pbuf, pd, 8),
                          (sbuf, sd, 8)):
            assert _guards_intact(buf, o, t.numel())
        assert bool((ld != FILL).all()) and bool((pd != FILL).all())
        if dx is None:
            assert bool((dxbuf == FILL).all())                  # a first unit: nothing for the input
        else:
            assert bool((dxd != FILL).all())
        back.append((dxd.cpu().clone(), pd.cpu().clone()))
    assert torch.equal(back[0][0], back[1][0])
    assert torch.equal(back[0][1], back[1][1]) and torch.equal(back[0][1], back[2][1])
    assert torch.equal(xd.cpu(), torch.from_numpy(x)) and torch.equal(gd.cpu(), torch.from_numpy(dy))
    assert torch.equal(sd.cpu(), kept)
    _check(label, "dx", back[0][0].numpy(), refs[1], e32s[1])
    _check(label, "dscale", back[0][1][0].numpy(), refs[2], e32s[2])
    _check(label, "doffset", back[0][1][1].numpy(), refs[3], e32s[3])
    return outs[0], back[0][0]


@pytest.mark.parametrize("off", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernels_match_loop_reference(case, form, off, references):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    g, shifted = case
    if form not in _forms(lib, g):
        # not a case of this geometry: the form's register budget does not hold a group, and the
        # launchers say so (the refusal is what is tested here)
        x = torch.zeros(g[:4], device=DEV)
        p = torch.ones(g[3], device=DEV)
        y = torch.full_like(x, FILL)
        assert lib.csa_gn_fwd(K.ptr(x), K.ptr(p), K.ptr(p), K.ptr(y), None, _geom(K, g), R.EPS, 0, 0.0, form,
                              K.stream()) != 0
        torch.cuda.synchronize()
        assert bool((y == FILL).all())
        return
    y, dx = _run_case(K, lib, g, form, off, references(g, shifted), label=f"{_case_id(case)} form {form} off {off}")
    if g == (2, 1, 1, 1, 1):                                    # m = 1: y = offset and dx = 0, exactly
        of = torch.from_numpy(R.inputs(g)[3])
        assert torch.equal(y.view(2, 1), of.view(1, 1).expand(2, 1)) and not bool(dx.any())


@pytest.mark.parametrize("off", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("ac", ACT_CASES, ids=lambda a: f"{R.geom_id(a[0])}-{a[1]}{a[2]:g}")
def test_fused_activations_match_loop_reference(ac, off, references):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    g, act, alpha = ac
    for form in _forms(lib, g)[1:]:
        _run_case(K, lib, g, form, off, references(g, False, act, alpha), act, alpha,
                  label=f"{R.geom_id(g)} {act} form {form} off {off}")


def test_automatic_form():
    """The register-resident forms and the streaming form are all known to run: the shapes that
    take each, and the thresholds between them."""
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    m1, m2 = lib.csa_gn_form_max(1), lib.csa_gn_form_max(2)
    assert (m1, m2) == (1024, 4096) and lib.csa_gn_max_blocks() == 2048
    form = lambda *g: lib.csa_gn_form(K.ints(list(g)))
    assert form(50, 196, 20, 20) == 1 and form(50, 1, 512, 1) == 2 and form(50, 196, 20, 4) == 2
    assert form(50, 1, 32, 1) == 1 and form(50, 1, 32, 8) == 1
    assert form(50, 196, 20, 1) == 3                 # the sample's layer norm streams (profiles/r19_notes.md)
    assert form(1, 784, 128, 1) == 3                 # 100352 elements: only streaming takes them
    # the thresholds, and that every automatic choice is a form the group fits
    a1 = max(m for m in range(1, m2 + 2) if form(1, 1, m, 1) == 1)
    a2 = max(m for m in range(1, m2 + 2) if form(1, 1, m, 1) <= 2)
    assert (a1, a2) == (256, 2048) and a1 <= m1 and a2 <= m2
    assert form(1, 1, a1 + 1, 1) == 2 and form(1, 1, a2 + 1, 1) == 3
    assert form(1, 1, 6, 4) == 0 and form(0, 1, 4, 1) == 0
    B, H, W, C, G = R.GRID_STRIDE[0]
    assert B * G > lib.csa_gn_max_blocks()           # more groups than one grid-stride trip covers


def test_launchers_refuse_without_launching():
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    g = (2, 2, 3, 8, 2)
    B, H, W, C, G = g
    good = _geom(K, g)
    st = K.stream()
    xbuf, xd = _guarded(g[:4], 8)
    xd.zero_()
    p = torch.ones(C, device=DEV)
    ybuf, yd = _guarded(g[:4], 8)
    dxbuf, dxd = _guarded(g[:4], 8)
    sbuf, sd = _guarded((B, G, 2), 8)
    lbuf, ld = _guarded((B, 2, C), 8)
    pbuf, pd = _guarded((2, C), 8)
    nan, inf = float("nan"), float("inf")

    def fwd(x=xd, sc=p, of=p, y=yd, stat=sd, geom=good, eps=R.EPS, act=0, alpha=0.0, form=0):
        return lib.csa_gn_fwd(K.ptr(x), K.ptr(sc), K.ptr(of), K.ptr(y), K.ptr(stat), geom, eps, act, alpha, form, st)

    def bwd(x=xd, sc=p, of=p, stat=sd, dy=xd, dx=dxd, slab=ld, geom=good, act=0, alpha=0.0, form=0):
        return lib.csa_gn_bwd(K.ptr(x), K.ptr(sc), K.ptr(of), K.ptr(stat), K.ptr(dy), K.ptr(dx), K.ptr(slab), geom,
                              act, alpha, form, st)

    for bad in ([0, 6, 8, 2], [2, 0, 8, 2], [2, 6, 0, 2], [2, 6, 8, 0], [-2, 6, 8, 2], [2, -6, 8, 2], [2, 6, -8, 2],
                [2, 6, 8, -2], [2, 6, 8, 3], [2, 6, 7, 2],
                [1 << 10, 1 << 11, 1 << 10, 1],            # 2^31 elements: beyond the 2^30 index range
                [(1 << 30) + 1, 1, 1, 1]):
        gi = K.ints(bad)
        assert lib.csa_gn_ok(gi) == 0 and lib.csa_gn_form(gi) == 0, bad
        for form in (0, 1, 2, 3):
            assert fwd(geom=gi, form=form) != 0 and bwd(geom=gi, form=form) != 0, bad
    assert lib.csa_gn_ok(good) == 1 and lib.csa_gn_ok(None) == 0
    for eps in (0.0, -1e-6, nan, inf, -inf):
        assert fwd(eps=eps) != 0, eps
    for act in (-1, 4):
        assert fwd(act=act) != 0 and bwd(act=act) != 0
    for alpha in (nan, inf, -inf):                          # (it multiplies every element)
        assert fwd(act=3, alpha=alpha) != 0 and bwd(act=3, alpha=alpha) != 0, alpha
    for form in (-1, 4):
        assert fwd(form=form) != 0 and bwd(form=form) != 0
    # a group beyond a form's register budget: that form is refused
    big = K.ints([1, 1, lib.csa_gn_form_max(2) + 4, 1])
    assert lib.csa_gn_ok(big) == 1
    for form in (1, 2):
        assert fwd(geom=big, form=form) != 0 and bwd(geom=big, form=form) != 0
    # null pointers (a null stat is the forward-only call, a null dx the first unit's)
    for kw in ({"x": None}, {"sc": None}, {"of": None}, {"y": None}, {"geom": None}):
        assert fwd(**kw) != 0, kw
    for kw in ({"x": None}, {"sc": None}, {"of": None}, {"stat": None}, {"dy": None}, {"slab": None}, {"geom": None}):
        assert bwd(**kw) != 0, kw
    for args in ((None, B, C, pd[0], pd[1]), (ld, B, C, None, pd[1]), (ld, B, C, pd[0], None), (ld, 0, C, pd[0], pd[1]),
                 (ld, B, 0, pd[0], pd[1]), (ld, -1, C, pd[0], pd[1]), (ld, 1 << 16, 1 << 15, pd[0], pd[1])):
        s, b, c, d0, d1 = args
        assert lib.csa_gn_bwd_params(K.ptr(s), b, c, K.ptr(d0), K.ptr(d1), st) != 0, args[1:3]
    torch.cuda.synchronize()
    for buf in (ybuf, dxbuf, sbuf, lbuf, pbuf):
        assert bool((buf == FILL).all())
    assert _guards_intact(xbuf, 8, xd.numel()) and not bool(xd.any())
    assert fwd() == 0 and bwd(stat=sd) == 0                 # (the good call does launch)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------- 2. one step vs eager
def _cfg(layers, **kw):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c["optimizer_name"] = kw.pop("optimizer", "GradientDescentOptimizer")
    c["learning_rate"] = kw.pop("lr", 0.5)
    c["loss_name"] = kw.pop("loss", "entropy")
    c["options"] = dict(batch_size=kw.pop("batch", 50), **kw)
    return parse_train_config(c)


KINDS = {
    "gn_sample_layer": ["conv", "conv", "gn", "dense", "dense"],
    "gn_sample_group": ["conv", "conv", "gn", "dense", "dense"],
    "gn_instance": ["conv", "gn", "conv", "dense"],
    "gn_dense": ["conv", "dense", "gn", "dense", "gn"],
    "gn_first": ["gn", "conv", "dense"],
    "gn_wide160": ["pool", "gconv", "gn", "pool", "dense"],
    "gn_leaky_neg": ["conv", "gn", "dense"],
}
# the activation that rides in each gn unit's launches, in unit order
ACTS = {
    "gn_sample_layer": ["sigmoid"], "gn_sample_group": ["sigmoid"], "gn_instance": [None],
    "gn_dense": ["relu", "sigmoid"], "gn_first": [None], "gn_wide160": ["relu"], "gn_leaky_neg": ["leaky_relu"],
}


def _check_lowering(name, prog):
    """A ``gn`` unit per layer, forward-only programs included; statistics and slab only in
    training programs; the activation behind the norm is the unit's, not a transform; the
    sample still forms the pair and fuses both dense units."""
    units = prog.units
    at = [k for k, u in enumerate(units) if u.kind == "gn"]
    want = sum(isinstance(lp.spec, GroupNormSpec) for lp in prog.e.model.plan.layers)
    assert len(at) == want and want >= 1, [u.kind for u in units]
    assert [u.kind for u in units] == KINDS[name]
    assert [u.act.func if u.act is not None else None for u in units if u.kind == "gn"] == ACTS[name]
    for k in at:
        u = units[k]
        G, C = u.layer.spec.groups, u.layer.in_shape.c
        assert isinstance(u.layer.spec, GroupNormSpec) and u.y.shape == u.x.shape and u.norm is None
        if prog.forward_only:
            assert u.gn_stat is None and u.gn_slab is None and u.dy is None
        else:
            assert tuple(u.gn_stat.shape) == (prog.B, G, 2) and tuple(u.gn_slab.shape) == (prog.B, 2, C)
            assert not any(r.data_ptr() in (u.gn_stat.data_ptr(), u.gn_slab.data_ptr())
                           for r in prog.zero_regions + prog.zero_early)
        # the consumer behind reads a plain tensor
        nxt = units[k + 1].in_tf if k + 1 < len(units) else prog.head_tf
        assert nxt.norm is None and nxt.act is None
    if name.startswith("gn_sample"):
        assert prog.pair is not None and units[1].pool is not None      # conv conv pool: the pair
        if not prog.forward_only and not prog.e.ctx.enabled:
            assert units[3].fused and units[4].fused
    if name == "gn_first":
        assert tuple(units[0].x.shape) == (prog.B, 28, 28, 1)
    if name == "gn_dense":
        assert units[2].x.dim() == 2 and units[-1].kind == "gn" and (prog.forward_only or prog.dlast is units[-1].dy)
    if name == "gn_leaky_neg":
        assert units[1].act.alpha == -0.1 and units[0].act is None


def _run_one(cfg, backend, ds, name=None):
    from cloud_server_amd.runtime.engine import TrainEngine
    eng = TrainEngine(cfg, ds, device="cuda", backend=backend, use_graph=False)
    assert eng.backend == backend, eng.fallback_reason
    if backend == "hip":
        _check_lowering(name, eng.program)
    w0 = eng.flat.clone()
    eng.step()
    torch.cuda.synchronize()
    return eng, w0, eng.flat.clone()


@pytest.mark.parametrize("name", list(R.NETS))
@pytest.mark.parametrize("loss", ["entropy", "mse"])
def test_step_matches_torch(name, loss):
    """The procedure and bound of test_hip_step.py::test_step_matches_torch."""
    ds = synthetic_mnist(400, seed=3)
    cfg = _cfg(R.layers_of(name), loss=loss, lr=0.5)
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
        print(f"{name}/{loss} grad {k}: err {err:.3e} scale {scale:.3e}")
        assert err <= 2e-3 * scale + 1e-6 + 1e-5 * gmax, f"{name}/{loss} grad {k}: err {err:.3e} scale {scale:.3e}"
    mh, mt = eh.metrics_since(0), et.metrics_since(0)
    assert abs(mh["loss"] - mt["loss"]) < 1e-4 * max(1, abs(mt["loss"]))
    assert mh["accuracy"] == mt["accuracy"]


def test_without_a_mode_the_plan_is_what_it_was():
    """A config without the option lowers to no gn unit: the sample's program is the pair, the
    bn transform and two dense units, as before."""
    from cloud_server_amd.runtime.engine import TrainEngine
    eng = TrainEngine(_cfg(SAMPLE_CONFIG["net_config"]["middle_layer"]), synthetic_mnist(200, seed=3), device="cuda",
                      backend="hip", use_graph=False)
    assert eng.backend == "hip", eng.fallback_reason
    assert [u.kind for u in eng.program.units] == ["conv", "conv", "dense", "dense"]
    assert all(u.gn_stat is None and u.gn_slab is None for u in eng.program.units) and eng.program.pair is not None
    assert eng.program.units[2].in_tf.has_bn


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
    assert eng.backend == "hip", eng.fallback_reason
    _check_lowering(name, eng.program)
    recs = X.run_trajectory(eng, X.Oracle64(cfg, dataset), 3)
    torch.cuda.synchronize()
    assert all(int(w.item()) == 0 for w in eng.health_words())
    X.check(recs, X.tolerances(name, X.LRS[ADAGRAD]), f"{name}-b{batch}")


# ----------------------------------------------------------------------- 4. deterministic mode
@pytest.mark.parametrize("name", ["gn_sample_layer", "gn_dense"])
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


# ----------------------------------------------------------------------- 5. forward-only programs
@pytest.mark.parametrize("name", ["gn_sample_layer", "gn_dense"])
def test_serving_and_validation(name):
    """The checks of test_gpu_lrn.py::test_serving_and_validation; validation leaves the training
    state bit for bit unchanged."""
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
    gn = [u for u in eng.program.units if u.kind == "gn"]
    before = (eng.flat.clone(), eng.slots.clone(), [u.gn_stat.clone() for u in gn], [u.gn_slab.clone() for u in gn])
    # the validation sweep: a forward-only program holding the gn unit
    val = eng.validator(test, 64, True)
    assert isinstance(val, HipValidator) and val.program.forward_only
    _check_lowering(name, val.program)
    res = eng.validate(test, 64, True)
    tv = TorchValidator(eng, test, 64, predictions=True)
    tv.issue()
    want = tv.wait()[1]
    assert res.n == want.n == len(test)
    assert res.confusion == want.confusion
    # the training program's own forward-only pass (it leaves the step's kept statistics alone)
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
    assert all(torch.equal(a, u.gn_stat) for a, u in zip(before[2], gn))
    assert all(torch.equal(a, u.gn_slab) for a, u in zip(before[3], gn))
    # serving: 256 images through the HIP predictor
    state = eng.model.export_state()
    assert not any(k.startswith("buffers.") for k in state)
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


# ----------------------------------------------------------------------- 6. packed jobs
def test_packed_jobs_with_gn_match_solo_runs():
    """Two jobs with the layer as branches of one graph (the packed launch profile) end where
    the same jobs trained alone end."""
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.multijob import PackedJobs
    names = ("gn_instance", "gn_sample_layer")

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
        assert d < 3e-3             # test_gpu_dropout.py: atomics, run-to-run fp32 order


# ----------------------------------------------------------------------- 7. world-1 data parallelism
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


@pytest.mark.parametrize("strategy", ["allreduce", "allreduce:hf"])
def test_world1_data_parallel_programs_match_single_gpu(pg, monkeypatch, strategy):
    """One process group of one rank whose context reports data parallelism as enabled (the
    pattern of test_gpu_dp_overlap.py): the gn unit's parameter gradients land in the flat
    gradient before the exchange, the flat optimizer updates them."""
    from cloud_server_amd.parallel.dist import DistContext
    from cloud_server_amd.runtime.engine import TrainEngine

    class _DPContext(DistContext):
        @property
        def enabled(self) -> bool:
            return True

    monkeypatch.setenv("CSA_XGMI", "0")
    cfg = _cfg(R.layers_of("gn_sample_layer"), optimizer=ADAGRAD, lr=1e-3)
    ds = synthetic_mnist(2000, seed=0)
    ctx = _DPContext(rank=0, world=1, local_rank=0, backend="nccl", device=torch.device("cuda", 0))
    a = TrainEngine(cfg, ds, device="cuda:0", ctx=ctx, backend="hip", strategy=strategy)
    assert a.backend == "hip", a.fallback_reason
    _check_lowering("gn_sample_layer", a.program)
    assert a.program.dp_hf == strategy.endswith(":hf")
    b = TrainEngine(cfg, ds, device="cuda:0", backend="hip")
    for _ in range(4):
        a.step(); b.step()
    a.run_steps(8); b.run_steps(8)
    a.sync_device(); b.sync_device()
    assert a.host_step == b.host_step == 12 and int(a.dstep.item()) == 12
    torch.testing.assert_close(a.flat, b.flat, rtol=2e-3, atol=2e-5)
