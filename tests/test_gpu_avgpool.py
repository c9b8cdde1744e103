"""Average and global pooling on the GPU: ``csa_avgpool_fwd`` / ``csa_avgpool_bwd``
(avg_pool.hip) against the float64 loop reference (tests/avgpool_ref.py) in both forward
forms, the lowered ``pool`` unit against the eager program and the fp64 oracle, deterministic
mode, the forward-only programs (serving, validation) and packed jobs.

Kernel bounds (derived, u = 2^-24): forward ``|y - y64| <= 2 n u max|x|`` for a window of n taps
(n - 1 adds and one division; any fold order has at most n - 1 adds on a path), backward
``|dx - dx64| <= 2 (m + 1) u max|dy|`` with m = ceil(kh/sh) ceil(kw/sw) windows per pixel."""
import copy

import numpy as np
import pytest
import torch

import avgpool_ref as R
import oracle64 as X

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, AvgPoolSpec, parse_train_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = -123.0
ADAGRAD = "AdagradOptimizer"


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


def _ints(K, g):
    B, H, W, C, kh, kw, sh, sw, pad = g
    OH, OW, pt, pl = R.geometry(H, W, kh, kw, sh, sw, pad)
    return K.ints([B, H, W, C, kh, kw, sh, sw, pt, pl, OH, OW]), (B, OH, OW, C)


@pytest.fixture(scope="module")
def references():
    """geometry -> (x, dy, y64, dx64): computed once, shared, never changed."""
    cache = {}

    def get(g):
        if g not in cache:
            B, H, W, C, kh, kw, sh, sw, pad = g
            rng = np.random.default_rng(H * 1000 + W * 10 + C)
            x = rng.standard_normal((B, H, W, C)).astype(np.float32)
            OH, OW, _, _ = R.geometry(H, W, kh, kw, sh, sw, pad)
            dy = rng.standard_normal((B, OH, OW, C)).astype(np.float32)
            cache[g] = (x, dy, R.avg_fwd(x, kh, kw, sh, sw, pad), R.avg_bwd(dy, H, W, kh, kw, sh, sw, pad))
        return cache[g]
    return get


@pytest.mark.parametrize("off", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("g", R.GEOMETRIES + [R.GRID_STRIDE_FWD], ids=R.geom_id)
def test_forward_matches_loop_reference(g, form, off, references):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    B, H, W, C, kh, kw, sh, sw, pad = g
    x, _, y64, _ = references(g)
    geom, oshape = _ints(K, g)
    assert lib.csa_avgpool_ok(geom) == 1
    xbuf, xd = _guarded(x.shape, off)
    xd.copy_(torch.from_numpy(x))
    ybuf, yd = _guarded(oshape, off)
    outs = []
    for _ in range(2):
        ybuf.fill_(FILL)
        assert lib.csa_avgpool_fwd(K.ptr(xd), K.ptr(yd), geom, form, K.stream()) == 0
        torch.cuda.synchronize()
        assert _guards_intact(ybuf, off, yd.numel()) and _guards_intact(xbuf, off, xd.numel())
        outs.append(yd.cpu().clone())
    assert torch.equal(outs[0], outs[1])                  # no atomics: equal bits
    assert torch.equal(xd.cpu(), torch.from_numpy(x))
    bound = R.fwd_bound(min(kh, H) * min(kw, W), float(np.abs(x).max()))
    err = np.abs(outs[0].numpy().astype(np.float64) - y64).max()
    print(f"{R.geom_id(g)} form {form} off {off}: err {err:.3e} <= {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("off", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("g", R.GEOMETRIES + [R.GRID_STRIDE_BWD], ids=R.geom_id)
def test_backward_matches_loop_reference(g, off, references):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    B, H, W, C, kh, kw, sh, sw, pad = g
    _, dy, _, dx64 = references(g)
    geom, oshape = _ints(K, g)
    gbuf, gd = _guarded(oshape, off)
    gd.copy_(torch.from_numpy(dy))
    dxbuf, dxd = _guarded((B, H, W, C), off)
    outs = []
    for _ in range(2):
        dxbuf.fill_(FILL)                                  # (every input element must be written)
        assert lib.csa_avgpool_bwd(K.ptr(gd), K.ptr(dxd), geom, K.stream()) == 0
        torch.cuda.synchronize()
        assert _guards_intact(dxbuf, off, dxd.numel()) and _guards_intact(gbuf, off, gd.numel())
        outs.append(dxd.cpu().clone())
    assert torch.equal(outs[0], outs[1])
    dx = outs[0].numpy()
    bound = R.bwd_bound(kh, kw, sh, sw, float(np.abs(dy).max()))
    err = np.abs(dx.astype(np.float64) - dx64).max()
    print(f"{R.geom_id(g)} off {off}: err {err:.3e} <= {bound:.3e}")
    assert err <= bound
    hole = ~R.covered(H, W, kh, kw, sh, sw, pad)
    assert hole.any() == (g == R.GAPPED)
    assert (dx[:, hole, :] == 0).all()                     # uncovered pixels: exactly 0


def test_launchers_refuse_without_launching():
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    good = (2, 7, 7, 4, 3, 3, 2, 2, "SAME")
    geom, oshape = _ints(K, good)
    xbuf, xd = _guarded(good[:4], 8)
    xd.zero_()
    ybuf, yd = _guarded(oshape, 8)
    dxbuf, dxd = _guarded(good[:4], 8)
    vals = list(geom)
    refused = []
    for i, v in ((4, 0), (5, 0), (6, 0), (7, 0), (0, 0), (3, 0), (10, 0), (8, 3), (9, 3), (8, -1), (10, 5), (11, 5)):
        bad = list(vals)
        bad[i] = v
        refused.append(bad)
    refused.append([1 << 20, 64, 64, 1, 2, 2, 2, 2, 0, 0, 32, 32])      # 2^32 elements: beyond the 2^30 index range
    refused.append([5, 1 << 14, 1 << 14, 1, 1, 1, 1, 1, 0, 0, 1 << 14, 1 << 14])
    st = K.stream()
    for bad in refused:
        gi = K.ints(bad)
        assert lib.csa_avgpool_ok(gi) == 0, bad
        for form in (0, 1, 2):
            assert lib.csa_avgpool_fwd(K.ptr(xd), K.ptr(yd), gi, form, st) != 0, bad
        assert lib.csa_avgpool_bwd(K.ptr(yd), K.ptr(dxd), gi, st) != 0, bad
    assert lib.csa_avgpool_ok(geom) == 1
    for form in (-1, 3):
        assert lib.csa_avgpool_fwd(K.ptr(xd), K.ptr(yd), geom, form, st) != 0
    assert lib.csa_avgpool_fwd(None, K.ptr(yd), geom, 0, st) != 0
    assert lib.csa_avgpool_fwd(K.ptr(xd), None, geom, 0, st) != 0
    assert lib.csa_avgpool_fwd(K.ptr(xd), K.ptr(yd), None, 0, st) != 0
    assert lib.csa_avgpool_bwd(None, K.ptr(dxd), geom, st) != 0
    assert lib.csa_avgpool_bwd(K.ptr(yd), None, geom, st) != 0
    assert lib.csa_avgpool_bwd(K.ptr(yd), K.ptr(dxd), None, st) != 0
    torch.cuda.synchronize()
    assert bool((ybuf == FILL).all()) and bool((dxbuf == FILL).all())
    assert lib.csa_avgpool_wave_taps() >= 1


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
    "sample_avg": ["conv", "conv", "pool", "bn", "dense", "dense"],
    "avg_first": ["pool", "conv", "dense"],
    # norm + relu materialised in front of the pool; the norm after it has no conv producer
    "avg_after_norm": ["conv", "bn", "pool", "bn", "dense"],
}


def _check_lowering(name, prog):
    """A ``pool`` unit per average pool, without an argmax; the conv in front of it fused no
    pool; the sample with ``mode: avg`` still forms the pair (in its no-pool form)."""
    units = prog.units
    avg = [k for k, u in enumerate(units) if u.kind == "pool" and isinstance(u.layer.spec, AvgPoolSpec)]
    want = sum(isinstance(lp.spec, AvgPoolSpec) for lp in prog.e.model.plan.layers)
    assert len(avg) == want and want >= 1, [u.kind for u in units]
    for k in avg:
        assert units[k].argmax is None
        if k and units[k - 1].kind == "conv":
            assert units[k - 1].pool is None
    if name in KINDS:
        assert [u.kind for u in units] == KINDS[name]
    if name == "sample_avg":
        assert prog.pair is not None
    if name == "gap_head":
        assert units[0].kind == "conv" and units[0].pool is not None      # the max pool still fuses
        assert units[-1].kind == "pool" and tuple(units[-1].layer.spec.kernel) == (14, 14)
        assert tuple(units[-1].y.shape[1:]) == (1, 1, 12)


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


# ----------------------------------------------------------------------- 3. three steps vs the oracle
@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


ORACLE_GRID = [(n, 50) for n in R.NETS] + [("lenet_avg", 7), ("gap_head", 7)]


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
@pytest.mark.parametrize("name", ["lenet_avg", "gap_head"])
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
@pytest.mark.parametrize("name", ["gap_head", "lenet_avg"])
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
    # the validation sweep: a forward-only program holding the pool unit
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
def test_packed_jobs_with_average_pool_match_solo_runs():
    """Two jobs with an average pool as branches of one graph (the packed launch profile)
    end where the same jobs trained alone end."""
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.multijob import PackedJobs
    names = ("lenet_avg", "sample_avg")

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
