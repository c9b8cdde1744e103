"""Local response normalisation on the GPU: ``csa_lrn_fwd`` / ``csa_lrn_bwd`` (lrn.hip) against
the float64 loop reference (tests/lrn_ref.py) in every form, the lowered ``lrn`` unit against
the eager program and the fp64 oracle, deterministic mode, the forward-only programs (serving,
validation) and packed jobs.

Kernel bound (measured against the reference, never against the kernel: the device's powf /
sqrtf errors are not documented): with e32 the error of the fp32 eager layer on the CPU against
the float64 loop on the same inputs, a kernel's error against the float64 loop is at most
``max(4 e32, 8 u max|ref|)``, u = 2^-24, forward and backward (``lrn_ref.kernel_bound``)."""
import copy

import numpy as np
import pytest
import torch

import lrn_ref as R
import oracle64 as X

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.cnn import build_model
from cloud_server_amd.models.dsl import (SAMPLE_CONFIG, LayerPlan, LrnSpec, TensorShape, parse_train_config)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = -123.0
ADAGRAD = "AdagradOptimizer"
ALL_GEOMS = R.GEOMETRIES + R.GRID_STRIDE


# ----------------------------------------------------------------------- 1. the kernels
def _guarded(shape, off):
    """A tensor of ``shape`` that starts ``off`` floats into a sentinel-filled buffer (off = 8:
    16-byte aligned, the float4 path when C % 4 == 0; off = 9: one float further, every
    element on the scalar path)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * off + 8,), FILL, device=DEV)
    return buf, buf[off:off + n].view(shape)


def _guards_intact(buf, off, n):
    return bool((buf[:off] == FILL).all()) and bool((buf[off + n:] == FILL).all())


def _args(K, g):
    B, H, W, C, r, k, alpha, beta = g
    return K.ints([B * H * W, C, r]), (float(k), float(alpha), float(beta))


@pytest.fixture(scope="module")
def references():
    """geometry -> (x, dy, y64, dx64, e32 forward, e32 backward): computed once, shared, never
    changed.  e32: the fp32 eager layer on the CPU against the float64 loop."""
    cache = {}
    model = build_model(parse_train_config(SAMPLE_CONFIG))

    def get(g):
        if g not in cache:
            B, H, W, C, r, k, alpha, beta = g
            x, dy = R.inputs(g)
            y64, dx64 = R.lrn_fwd(x, r, k, alpha, beta), R.lrn_bwd(x, dy, r, k, alpha, beta)
            lp = LayerPlan(0, LrnSpec(r, k, alpha, beta), TensorShape(C, (H, W)), TensorShape(C, (H, W)))
            xt = torch.from_numpy(x).requires_grad_(True)
            y32 = model._layer(lp, xt, True)
            (dx32,) = torch.autograd.grad(y32, xt, torch.from_numpy(dy))
            e_f = float(np.abs(y32.detach().numpy().astype(np.float64) - y64).max())
            e_b = float(np.abs(dx32.numpy().astype(np.float64) - dx64).max())
            cache[g] = (x, dy, y64, dx64, e_f, e_b)
        return cache[g]
    return get


def _forms(lib, g):
    """Every form the geometry has (form 2 stops at csa_lrn_row_max channels)."""
    return [0, 1, 2] if g[3] <= lib.csa_lrn_row_max() else [0, 1]


@pytest.mark.parametrize("off", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("g", ALL_GEOMS, ids=R.geom_id)
def test_forward_matches_loop_reference(g, form, off, references):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    assert form in _forms(lib, g)
    x, _, y64, _, e32, _ = references(g)
    geom, consts = _args(K, g)
    assert lib.csa_lrn_ok(geom, *consts) == 1
    xbuf, xd = _guarded(x.shape, off)
    xd.copy_(torch.from_numpy(x))
    ybuf, yd = _guarded(x.shape, off)
    kbuf, kd = _guarded(x.shape, off)
    outs = []
    for keep in (kd, kd, None):
        ybuf.fill_(FILL)
        kbuf.fill_(FILL)
        assert lib.csa_lrn_fwd(K.ptr(xd), K.ptr(yd), K.ptr(keep), geom, *consts, form, K.stream()) == 0
        torch.cuda.synchronize()
        assert _guards_intact(ybuf, off, yd.numel()) and _guards_intact(xbuf, off, xd.numel())
        assert _guards_intact(kbuf, off, kd.numel())
        if keep is None:
            assert bool((kbuf == FILL).all())              # a forward-only program keeps nothing
        else:
            assert bool((kd != FILL).all())
        outs.append(yd.cpu().clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])     # no atomics: equal bits
    assert torch.equal(xd.cpu(), torch.from_numpy(x))
    bound = R.kernel_bound(e32, y64)
    err = np.abs(outs[0].numpy().astype(np.float64) - y64).max()
    print(f"{R.geom_id(g)} form {form} off {off}: e32 {e32:.3e} bound {bound:.3e} err {err:.3e} "
          f"(max|y| {np.abs(y64).max():.3e})")
    assert err <= bound


@pytest.mark.parametrize("off", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("g", ALL_GEOMS, ids=R.geom_id)
def test_backward_matches_loop_reference(g, form, off, references):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    assert form in _forms(lib, g)
    x, dy, _, dx64, _, e32 = references(g)
    geom, consts = _args(K, g)
    xbuf, xd = _guarded(x.shape, off)
    xd.copy_(torch.from_numpy(x))
    gbuf, gd = _guarded(x.shape, off)
    gd.copy_(torch.from_numpy(dy))
    ybuf, yd = _guarded(x.shape, off)
    kbuf, kd = _guarded(x.shape, off)
    # what the backward reads is what the forward of the same form kept
    assert lib.csa_lrn_fwd(K.ptr(xd), K.ptr(yd), K.ptr(kd), geom, *consts, form, K.stream()) == 0
    torch.cuda.synchronize()
    kept = kd.cpu().clone()
    dxbuf, dxd = _guarded(x.shape, off)
    outs = []
    for _ in range(2):
        dxbuf.fill_(FILL)                                  # (every element must be written)
        assert lib.csa_lrn_bwd(K.ptr(xd), K.ptr(kd), K.ptr(gd), K.ptr(dxd), geom, *consts, form, K.stream()) == 0
        torch.cuda.synchronize()
        for buf, t in ((dxbuf, dxd), (xbuf, xd), (gbuf, gd), (kbuf, kd)):
            assert _guards_intact(buf, off, t.numel())
        assert bool((dxd != FILL).all())
        outs.append(dxd.cpu().clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(xd.cpu(), torch.from_numpy(x)) and torch.equal(gd.cpu(), torch.from_numpy(dy))
    assert torch.equal(kd.cpu(), kept)
    bound = R.kernel_bound(e32, dx64)
    err = np.abs(outs[0].numpy().astype(np.float64) - dx64).max()
    print(f"{R.geom_id(g)} form {form} off {off}: e32 {e32:.3e} bound {bound:.3e} err {err:.3e} "
          f"(max|dx| {np.abs(dx64).max():.3e})")
    assert err <= bound


def test_launchers_refuse_without_launching():
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    good = (2, 3, 5, 8, 2, 1.0, 1.0, 0.5)
    geom, consts = _args(K, good)
    shape = good[:4]
    xbuf, xd = _guarded(shape, 8)
    xd.zero_()
    kbuf, kd = _guarded(shape, 8)
    kd.fill_(1.0)
    ybuf, yd = _guarded(shape, 8)
    dxbuf, dxd = _guarded(shape, 8)
    st = K.stream()
    nan, inf = float("nan"), float("inf")
    refused = [([0, 8, 2], consts), ([30, 0, 2], consts), ([-30, 8, 2], consts), ([30, -8, 2], consts),
               ([30, 8, -1], consts),
               ([1 << 20, 1 << 11, 1], consts),            # 2^31 elements: beyond the 2^30 index range
               ([(1 << 30) + 1, 1, 0], consts)]
    for bad in ((0.0, 1.0, 0.5), (-1.0, 1.0, 0.5), (nan, 1.0, 0.5), (inf, 1.0, 0.5), (1.0, -1e-3, 0.5),
                (1.0, nan, 0.5), (1.0, inf, 0.5), (1.0, 1.0, 0.0), (1.0, 1.0, -0.5), (1.0, 1.0, nan), (1.0, 1.0, inf)):
        refused.append(([30, 8, 2], bad))
    for gi, cs in refused:
        gi = K.ints(gi)
        assert lib.csa_lrn_ok(gi, *cs) == 0, (list(gi), cs)
        for form in (0, 1, 2):
            assert lib.csa_lrn_fwd(K.ptr(xd), K.ptr(yd), K.ptr(kd), gi, *cs, form, st) != 0, (list(gi), cs)
            assert lib.csa_lrn_bwd(K.ptr(xd), K.ptr(kd), K.ptr(yd), K.ptr(dxd), gi, *cs, form, st) != 0, (list(gi), cs)
    assert lib.csa_lrn_ok(geom, *consts) == 1
    assert lib.csa_lrn_ok(None, *consts) == 0
    for form in (-1, 3):
        assert lib.csa_lrn_fwd(K.ptr(xd), K.ptr(yd), K.ptr(kd), geom, *consts, form, st) != 0
        assert lib.csa_lrn_bwd(K.ptr(xd), K.ptr(kd), K.ptr(yd), K.ptr(dxd), geom, *consts, form, st) != 0
    # a row wider than form 2 takes: form 2 is refused (form 0 picks form 1)
    wide = K.ints([1, lib.csa_lrn_row_max() + 1, 2])
    assert lib.csa_lrn_ok(wide, *consts) == 1
    assert lib.csa_lrn_fwd(K.ptr(xd), K.ptr(yd), K.ptr(kd), wide, *consts, 2, st) != 0
    assert lib.csa_lrn_bwd(K.ptr(xd), K.ptr(kd), K.ptr(yd), K.ptr(dxd), wide, *consts, 2, st) != 0
    assert lib.csa_lrn_row_taps(lib.csa_lrn_row_max() + 1) == 2 ** 31 - 1
    assert lib.csa_lrn_row_taps(20) >= 1 and lib.csa_lrn_row_taps(160) >= 1
    # null pointers (a null ``keep`` is the forward-only call, refused by the backward only)
    assert lib.csa_lrn_fwd(None, K.ptr(yd), K.ptr(kd), geom, *consts, 0, st) != 0
    assert lib.csa_lrn_fwd(K.ptr(xd), None, K.ptr(kd), geom, *consts, 0, st) != 0
    assert lib.csa_lrn_fwd(K.ptr(xd), K.ptr(yd), K.ptr(kd), None, *consts, 0, st) != 0
    assert lib.csa_lrn_bwd(None, K.ptr(kd), K.ptr(yd), K.ptr(dxd), geom, *consts, 0, st) != 0
    assert lib.csa_lrn_bwd(K.ptr(xd), None, K.ptr(yd), K.ptr(dxd), geom, *consts, 0, st) != 0
    assert lib.csa_lrn_bwd(K.ptr(xd), K.ptr(kd), None, K.ptr(dxd), geom, *consts, 0, st) != 0
    assert lib.csa_lrn_bwd(K.ptr(xd), K.ptr(kd), K.ptr(yd), None, geom, *consts, 0, st) != 0
    assert lib.csa_lrn_bwd(K.ptr(xd), K.ptr(kd), K.ptr(yd), K.ptr(dxd), None, *consts, 0, st) != 0
    torch.cuda.synchronize()
    assert bool((ybuf == FILL).all()) and bool((dxbuf == FILL).all())
    assert bool((kd == 1.0).all()) and _guards_intact(kbuf, 8, kd.numel())


def test_a_row_wider_than_form_two_runs_in_form_one(references):
    """C = csa_lrn_row_max() + 4: form 0 is form 1 and agrees with the loop reference."""
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    g = (1, 1, 3, lib.csa_lrn_row_max() + 4, 3, 1.0, 0.01, 0.75)
    x, _, y64, _, e32, _ = references(g)
    geom, consts = _args(K, g)
    xd = torch.from_numpy(x).to(DEV)
    y0, y1 = torch.zeros_like(xd), torch.zeros_like(xd)
    assert lib.csa_lrn_fwd(K.ptr(xd), K.ptr(y0), None, geom, *consts, 0, K.stream()) == 0
    assert lib.csa_lrn_fwd(K.ptr(xd), K.ptr(y1), None, geom, *consts, 1, K.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    assert np.abs(y0.cpu().numpy().astype(np.float64) - y64).max() <= R.kernel_bound(e32, y64)


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
    "lrn_sample": ["conv", "conv", "lrn", "bn", "dense", "dense"],
    # (deterministic mode keeps the overlapping 3 x 3 / 2 pool out of the conv unit)
    "lrn_cifar": ["conv", "lrn", "conv", "lrn", "pool", "dense"],
    "lrn_first": ["lrn", "conv", "dense"],
    "lrn_allchan_head": ["pool", "conv", "lrn"],
    # the 160-channel conv is an implicit-GEMM unit; its relu is materialised in front of the lrn
    "lrn_wide160": ["pool", "gconv", "bn", "lrn", "pool", "dense"],
}
KINDS_DET = dict(KINDS, lrn_cifar=["conv", "pool", "lrn", "conv", "lrn", "pool", "dense"])


def _check_lowering(name, prog):
    """An ``lrn`` unit per lrn layer, forward-only programs included; the kept tensor only in
    training programs; a conv in front keeps its own act / pool; the sample with an lrn after
    the pool still forms the pair; a norm after an lrn is a standalone bn unit."""
    units = prog.units
    at = [k for k, u in enumerate(units) if u.kind == "lrn"]
    want = sum(isinstance(lp.spec, LrnSpec) for lp in prog.e.model.plan.layers)
    assert len(at) == want and want >= 1, [u.kind for u in units]
    for k in at:
        u = units[k]
        assert isinstance(u.layer.spec, LrnSpec) and u.y.shape == u.x.shape and u.y.dim() == 4
        if prog.forward_only:
            assert u.lrn_s is None and u.dy is None
        else:
            assert u.lrn_s is not None and u.lrn_s.shape == u.x.shape
    assert [u.kind for u in units] == (KINDS_DET if prog.det else KINDS)[name]
    if name == "lrn_sample":
        assert prog.pair is not None and units[1].pool is not None     # conv conv pool lrn: the pair
        assert units[3].norm is not None                                # the norm after the lrn: standalone
    if name == "lrn_cifar" and not prog.det:
        assert units[0].pool is not None and units[0].act is not None and units[2].pool is None
    if name == "lrn_allchan_head":
        assert units[-1].kind == "lrn" and prog.dlast is units[-1].dy
    if name == "lrn_first":
        assert tuple(units[0].x.shape) == (prog.B, 28, 28, 1)


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


def test_without_an_lrn_entry_the_plan_is_what_it_was():
    """A config without the layer lowers to no lrn unit: the sample's program is the pair,
    the bn transform and two dense units, as before."""
    from cloud_server_amd.runtime.engine import TrainEngine
    eng = TrainEngine(_cfg(SAMPLE_CONFIG["net_config"]["middle_layer"]), synthetic_mnist(200, seed=3), device="cuda",
                      backend="hip", use_graph=False)
    assert eng.backend == "hip", eng.fallback_reason
    assert [u.kind for u in eng.program.units] == ["conv", "conv", "dense", "dense"]
    assert all(u.lrn_s is None for u in eng.program.units) and eng.program.pair is not None


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
@pytest.mark.parametrize("name", ["lrn_sample", "lrn_cifar"])
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
@pytest.mark.parametrize("name", ["lrn_allchan_head", "lrn_cifar"])
def test_serving_and_validation(name):
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.validation import HipValidator, TorchValidator
    from cloud_server_amd.serve.hip_infer import HipPredictor
    train, test = synthetic_mnist(1280, seed=0).split(0.8)
    c = _cfg(R.layers_of(name), optimizer="AdamOptimizer", lr=1e-3)
    eng = TrainEngine(c, train, device=DEV, backend="hip")
    assert eng.backend == "hip", eng.fallback_reason
    for _ in range(10):
        eng.step()
    torch.cuda.synchronize()
    # the validation sweep: a forward-only program holding the lrn unit
    val = eng.validator(test, 64, True)
    assert isinstance(val, HipValidator) and val.program.forward_only
    _check_lowering(name, val.program)
    assert all(u.dy is None for u in val.program.units)
    res = eng.validate(test, 64, True)
    tv = TorchValidator(eng, test, 64, predictions=True)
    tv.issue()
    want = tv.wait()[1]
    assert res.n == want.n == len(test)
    assert res.confusion == want.confusion
    # the training program's own forward-only pass (it leaves the step's kept tensor alone)
    kept = [u.lrn_s.clone() for u in eng.program.units if u.kind == "lrn"]
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
    assert all(torch.equal(a, u.lrn_s) for a, u in zip(kept, [u for u in eng.program.units if u.kind == "lrn"]))
    # serving: 256 images through the HIP predictor
    pred = HipPredictor(c, eng.model.export_state(), torch.device(DEV), buckets=(256,), preps=("mnist",))
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
def test_packed_jobs_with_lrn_match_solo_runs():
    """Two jobs with lrn layers as branches of one graph (the packed launch profile) end where
    the same jobs trained alone end."""
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.multijob import PackedJobs
    names = ("lrn_cifar", "lrn_sample")

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
        torch.cuda.synchronize()
        assert e.host_step == 4 and int(e.dstep.item()) == 4
        d = (e.flat - solo.flat).abs().max().item()
        print(f"{names[s]}: packed vs solo {d:.3e}")
        assert d < 3e-3             # test_gpu_dropout.py: atomics, run-to-run fp32 order
