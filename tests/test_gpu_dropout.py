"""Dropout on the GPU: ``csa_drop_fwd`` / ``csa_drop_bwd`` (dropout.hip) against the NumPy
mask definition (ops/dropout_ref.py), the lowered ``drop`` unit against the eager program
tensor by tensor, masks advancing with the device step counter under multi-step graphs,
dropout-free evaluation / validation / serving, and deterministic mode."""
import copy

import numpy as np
import pytest
import torch

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config
from cloud_server_amd.ops import dropout_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACT_IDS = {"none": 0, "sigmoid": 1, "relu": 2, "leaky_relu": 3}
FILL = -123.0


# ----------------------------------------------------------------------- 1. the kernels
def _act64(x, act, alpha):
    x = x.astype(np.float64)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if act == "relu":
        return np.maximum(x, 0.0)
    if act == "leaky_relu":
        return np.maximum(x, np.float64(np.float32(alpha)) * x)
    return x


def _dact64(x, act, alpha):
    x = x.astype(np.float64)
    if act == "sigmoid":
        y = 1.0 / (1.0 + np.exp(-x))
        return y * (1.0 - y)
    if act == "relu":
        return (x > 0).astype(np.float64)
    if act == "leaky_relu":
        return np.where(x >= 0, 1.0, np.float64(np.float32(alpha)))
    return np.ones_like(x)


def _guarded(n, off):
    """An n-element view ``off`` floats into a sentinel-filled buffer (off = 8: 16-byte
    aligned, the float4 body; off = 3: misaligned, every element on the scalar path)."""
    buf = torch.full((n + 2 * off + 8,), FILL, device=DEV)
    return buf, buf[off:off + n]


def _guards_intact(buf, off, n):
    return bool((buf[:off] == FILL).all()) and bool((buf[off + n:] == FILL).all())


KERNEL_SHAPES = [(n, n, 1, 0, 8) for n in (1, 3, 4, 5, 1023, 1025, 4103)] + [(4100, 100, 2, 1, 8), (1025, 205, 1, 0, 3)]


@pytest.mark.parametrize("act", ["none", "relu", "sigmoid", "leaky_relu"])
@pytest.mark.parametrize("n,F,row_mul,row_add,off", KERNEL_SHAPES)
def test_drop_kernels_match_numpy(n, F, row_mul, row_add, off, act):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    keep_prob, alpha = (0.5 if n % 2 else 0.75), 0.2
    seed = D.drop_seed(3, n % 7)
    T, s = D.keep_threshold(keep_prob), D.keep_scale(keep_prob)
    s32 = np.float32(s)
    step_fwd, step_other = (2 ** 32 + 9 if n == 4103 else 7), 11       # (only the low 32 bits count)
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    dy = rng.standard_normal(n).astype(np.float32)
    mask = D.keep_mask(seed, step_fwd, n // F, F, keep_prob, row_mul, row_add).reshape(-1)
    assert not np.array_equal(mask, D.keep_mask(seed, step_other, n // F, F, keep_prob, row_mul, row_add).reshape(-1)) \
        or n < 8

    xbuf, xd = _guarded(n, off)
    xd.copy_(torch.from_numpy(x))
    gbuf, gd = _guarded(n, off)
    gd.copy_(torch.from_numpy(dy))
    ybuf, yd = _guarded(n, off)
    dxbuf, dxd = _guarded(n, off)
    dstep = torch.tensor([step_fwd], dtype=torch.int64, device=DEV)
    used = torch.tensor([-5], dtype=torch.int64, device=DEV)
    a_id = ACT_IDS[act]

    def fwd(train):
        rc = lib.csa_drop_fwd(K.ptr(xd), K.ptr(yd), n, F, row_mul, row_add, seed, K.ptr(dstep), K.ptr(used),
                              T, s, a_id, alpha, train, K.stream())
        assert rc == 0
        torch.cuda.synchronize()

    # train = 0: act(x), no draw, the recorded step untouched
    fwd(0)
    assert int(used.item()) == -5 and _guards_intact(ybuf, off, n)
    a64 = _act64(x, act, alpha)
    if act in ("none", "relu"):
        assert torch.equal(yd.cpu(), torch.from_numpy(a64.astype(np.float32)))
    else:
        np.testing.assert_allclose(yd.cpu().numpy().astype(np.float64), a64, rtol=1e-6, atol=1e-7)
    # train = 1: the mask of *dstep, which the forward records
    ybuf.fill_(FILL)
    fwd(1)
    assert int(used.item()) == step_fwd and _guards_intact(ybuf, off, n)
    y = yd.cpu().numpy()
    if act in ("none", "relu"):
        # one fp32 multiply, no contraction: bit-exact
        want = np.where(mask, a64.astype(np.float32) * s32, np.float32(0)).astype(np.float32)
        assert torch.equal(yd.cpu(), torch.from_numpy(want))
    else:
        # the fp32 rounding of one exp and two multiplies
        np.testing.assert_allclose(y.astype(np.float64), np.where(mask, a64 * np.float64(s32), 0.0),
                                   rtol=1e-6, atol=1e-7)
    assert (y[~mask] == 0).all()
    # the backward redraws the forward's mask from the recorded step, whatever dstep is now
    dstep.fill_(step_other)
    rc = lib.csa_drop_bwd(K.ptr(xd), K.ptr(gd), K.ptr(dxd), n, F, row_mul, row_add, seed, K.ptr(used),
                          T, s, a_id, alpha, K.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert _guards_intact(dxbuf, off, n) and _guards_intact(xbuf, off, n) and _guards_intact(gbuf, off, n)
    dx = dxd.cpu().numpy()
    assert (dx[~mask] == 0).all()
    if act in ("none", "relu"):
        want = np.where(mask & ((x > 0) | (act == "none")), dy * s32, np.float32(0)).astype(np.float32)
        assert torch.equal(dxd.cpu(), torch.from_numpy(want))
    else:
        # dx = (dy * s) * act'(x) in fp32.  leaky: two multiplies.  sigmoid: y (1 - y) from an
        # fp32 y with an absolute error up to one ulp of [0.5, 1) = 2^-24 * 2, which the
        # subtraction passes on unscaled: |err| <= |dy| s 2^-23 on top of the multiplies'
        # relative rounding
        want = np.where(mask, dy.astype(np.float64) * np.float64(s32) * _dact64(x, act, alpha), 0.0)
        atol = 1e-7 + (2.0 ** -23) * float(np.abs(dy).max()) * s
        np.testing.assert_allclose(dx.astype(np.float64), want, rtol=1e-6, atol=atol)


def test_drop_launchers_reject_bad_arguments():
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    x = torch.zeros(16, device=DEV)
    y = torch.zeros(16, device=DEV)
    w = torch.zeros(1, dtype=torch.int64, device=DEV)
    ok = (K.ptr(x), K.ptr(y), 16, 4, 1, 0, 1, K.ptr(w), K.ptr(w), 1 << 23, 2.0, 0, 0.0, 1, K.stream())
    assert lib.csa_drop_fwd(*ok) == 0
    for i, bad in ((2, 0), (3, 5), (4, 0), (5, 1), (9, 0), (9, (1 << 24) + 1)):
        args = list(ok)
        args[i] = bad
        assert lib.csa_drop_fwd(*args) < 0, (i, bad)
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


def _case_a(h1, h2):
    return SAMPLE_CONFIG["net_config"]["middle_layer"][:5] + [
        {"layer": "connect", "hidden": h1},
        {"layer": "active", "active_func": "relu"},
        {"layer": "dropout", "keep_prob": 0.5},
        {"layer": "connect", "hidden": h2}]


CASES = {
    # the sample's layers with ``active relu, dropout 0.5`` between the two connects.  The
    # horizontally fused program takes dense layers whose width is a multiple of 128
    # (HipProgram._plan_hfuse), so the fast-program assertions need 128 / 128; 64 / 32 run
    # the same lowering on the fused (not horizontally fused) program
    "a": (_case_a(128, 128), 50),
    "a_64_32": (_case_a(64, 32), 50),
    # a dropout on a spatial tensor (7 * 13 * 13 * 3 = 3549 elements: the scalar tail) and a
    # dropout as the last unit (the head reads a drop unit's output)
    "b": ([{"layer": "conv", "filter": [3, 3, 3], "padding": "VALID"},
           {"layer": "active"},
           {"layer": "pool"},
           {"layer": "dropout", "keep_prob": 0.75},
           {"layer": "connect", "hidden": 32},
           {"layer": "dropout", "keep_prob": 0.8}], 7),
    "c": ([{"layer": "dropout", "keep_prob": 0.9}, {"layer": "connect", "hidden": 64}], 50),
    # a norm in the pending group: a bn unit, then a plain drop unit
    "d": ([{"layer": "connect", "hidden": 64},
           {"layer": "norm"},
           {"layer": "active", "active_func": "relu"},
           {"layer": "dropout", "keep_prob": 0.5},
           {"layer": "connect", "hidden": 32}], 50),
}


def _check_lowering(name, prog):
    kinds = [u.kind for u in prog.units]
    drops = [u for u in prog.units if u.kind == "drop"]
    dense = [u for u in prog.units if u.kind == "dense"]
    if name in ("a", "a_64_32"):
        assert kinds == ["conv", "conv", "dense", "drop", "dense"], kinds
        assert prog.pair is not None
        assert drops[0].act is not None and drops[0].act.func == "relu"
        assert [u.fused for u in dense] == [True, True]
        assert dense[1].in_tf.act is None and dense[1].in_tf.norm is None
        assert prog.hfuse == (name == "a")
    elif name == "b":
        assert kinds == ["conv", "drop", "dense", "drop"], kinds
        assert drops[0].x.numel() == 7 * 13 * 13 * 3 and drops[0].act is None
        assert not prog.head_row
    elif name == "c":
        assert kinds == ["drop", "dense"], kinds
    elif name == "d":
        assert kinds == ["dense", "bn", "drop", "dense"], kinds
        assert drops[0].act is None and prog.units[1].act is not None


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


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("loss", ["entropy", "mse"])
def test_step_matches_torch(name, loss):
    ds = synthetic_mnist(400, seed=3)
    layers, batch = CASES[name]
    cfg = _cfg(layers, loss=loss, lr=0.5, batch=batch)
    eh, w0h, w1h = _run_one(cfg, "hip", ds, name)
    et, w0t, w1t = _run_one(cfg, "torch", ds)
    assert torch.equal(w0h, w0t)
    # the drop units' outputs carry exactly the NumPy mask of step 0
    for u in eh.program.units:
        if u.kind == "drop":
            assert int(u.used_step.item()) == 0
            kp = u.layer.spec.keep_prob
            mask = D.keep_mask(D.drop_seed(cfg.seed, u.layer.index), 0, batch, u.x[0].numel(), kp)
            y = u.y.reshape(batch, -1).cpu().numpy()
            assert (y[~mask] == 0).all() and (y[mask] != 0).any()
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


# ----------------------------------------------------------------------- 3. steps advance the mask
def test_mask_advances_under_multi_step_graphs(monkeypatch):
    from cloud_server_amd.runtime.engine import TrainEngine
    ds = synthetic_mnist(700, seed=29)
    cfg = _cfg(CASES["a"][0], optimizer="AdagradOptimizer", lr=0.01)
    monkeypatch.setenv("CSA_GRAPH_STEPS", "4")
    a = TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=True)
    b = TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=False)
    t = TrainEngine(cfg, ds, device="cuda", backend="torch", use_graph=False)
    assert a.program.hfuse
    a.step()
    a.prepare_group_graph()
    assert a.graph_k is not None
    a.run_steps(5)
    for _ in range(6):
        b.step()
        t.step()
    torch.cuda.synchronize()
    assert a.host_step == 6 and int(a.dstep.item()) == 6
    drops = [u for u in a.program.units if u.kind == "drop"]
    assert len(drops) == 1
    for u in drops:
        assert int(u.used_step.item()) == 5
        seed, F = D.drop_seed(cfg.seed, u.layer.index), u.x[0].numel()
        # y = relu(x) * mask * s: zero wherever step 5's mask drops, and its nonzero elements
        # (those kept with x > 0) do not fit the masks of the neighbouring steps
        nz = (u.y != 0).cpu().numpy()
        assert 0.05 < nz.mean() < 0.6
        assert not nz[~D.keep_mask(seed, 5, 50, F, 0.5)].any()
        for other in (4, 6):
            outside = nz[~D.keep_mask(seed, other, 50, F, 0.5)].sum() / nz.sum()
            assert 0.4 < outside < 0.6, (other, outside)
    d_ab = (a.flat - b.flat).abs().max().item()
    d_at = (a.flat - t.flat).abs().max().item()
    d_bt = (b.flat - t.flat).abs().max().item()
    print(f"graph vs eager hip {d_ab:.3e}, graph vs torch {d_at:.3e}, eager hip vs torch {d_bt:.3e}")
    assert d_ab < 3e-3          # atomics: run-to-run fp32 order (test_graph_replay_matches_eager)
    assert d_at < 2e-3 and d_bt < 2e-3      # test_optimizers_match_torch


# ----------------------------------------------------------------------- 4. evaluation, serving
def _bound(ref):
    """The project's HIP-vs-reference tolerance (tests/test_gpu_serving.py ``_close``)."""
    return 1e-4 + 1e-4 * float(np.abs(ref).max())


def _state(eng):
    return ([eng.flat.clone(), eng.slots.clone(), eng.stream.cursor.clone(), eng.dstep.clone(),
             eng.ring_loss.clone(), eng.ring_correct.clone()] + [x.clone() for x in eng.model.buffers()]
            + [u.used_step.clone() for u in eng.program.units if u.kind == "drop"])


def test_evaluation_validation_and_serving_are_dropout_free():
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.validation import HipValidator, TorchValidator
    from cloud_server_amd.serve.hip_infer import HipPredictor
    train, test = synthetic_mnist(1000, seed=0).split(0.8)
    c = _cfg(CASES["a"][0], optimizer="AdamOptimizer", lr=1e-3)
    eng = TrainEngine(c, train, device=DEV, backend="hip")
    assert eng.backend == "hip", eng.fallback_reason
    for _ in range(10):
        eng.step()
    torch.cuda.synchronize()
    # evaluate(): the same accuracy as the torch engine holding the same parameters
    ref = TrainEngine(c, train, device=DEV, backend="torch", use_graph=False)
    ref.flat.copy_(eng.flat)
    for (_, x), (_, y) in zip(ref.model.named_buffers(), eng.model.named_buffers()):
        x.copy_(y)
    assert eng.evaluate(test) == ref.evaluate(test)
    assert eng.model.training and ref.model.training
    # the validation sweep: a forward-only program without drop units, equal to the eager
    # validator, training state untouched bit for bit
    before = _state(eng)
    val = eng.validator(test, 64, True)
    assert isinstance(val, HipValidator) and val.program.forward_only
    assert all(u.kind != "drop" for u in val.program.units)
    assert [u.kind for u in val.program.units] == ["conv", "conv", "dense", "dense"]
    assert val.program.units[3].in_tf.act is not None      # the activation: a consumer transform again
    res = eng.validate(test, 64, True)
    tv = TorchValidator(eng, test, 64, predictions=True)
    tv.issue()
    want = tv.wait()[1]
    z = tv.logits().double().cpu().numpy()
    lb = _bound(np.asarray([want.loss]))
    print(f"loss {res.loss:.6f} vs {want.loss:.6f}, acc {res.accuracy:.4f} vs {want.accuracy:.4f}")
    assert res.n == want.n == len(test)
    assert abs(res.loss - want.loss) <= lb, (res.loss, want.loss, lb)
    top = np.sort(z, axis=1)
    sure = (top[:, -1] - top[:, -2]) > 2 * _bound(z)
    same = res.predictions == want.predictions
    assert same[sure].all() and same.mean() >= 0.99
    eng.check_health()
    after = _state(eng)
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
    # the training program's own predict: train = 0 launches, act(x) without a draw
    idx = eng.stream.rows.index_select(0, eng.stream.cursor).view(-1)      # (the cursor stays)
    xb, _ = eng.data.batch(idx)
    eng.model.eval()
    with torch.no_grad():
        zt = eng.model(xb).cpu().numpy()
    eng.model.train()
    logits = torch.zeros(50, 10, device=DEV)
    eng.program.predict_logits_into(logits)
    torch.cuda.synchronize()
    assert np.abs(logits.cpu().numpy() - zt).max() <= _bound(zt)
    assert all(torch.equal(x, y) for x, y in zip(before[-1:], _state(eng)[-1:]))     # used_step untouched
    # serving: no drop unit in any bucket, logits of the eval-mode model
    pred = HipPredictor(c, eng.model.export_state(), torch.device(DEV), buckets=(16,), preps=("mnist",))
    for bk in pred._buckets.values():
        assert all(u.kind != "drop" for u in bk.program.units)
    x8 = test.images[:16].reshape(16, 784)
    got = pred.logits_u8(np.ascontiguousarray(x8), "mnist")
    eng.model.eval()
    with torch.no_grad():
        zs = eng.model(torch.from_numpy(x8).to(DEV).float().div_(255.0)).cpu().numpy()
    eng.model.train()
    assert np.abs(got - zs).max() <= _bound(zs)


def test_packed_jobs_with_dropout_match_solo_runs():
    """Two jobs with a dropout layer as branches of one graph (the packed launch profile):
    each draws its own seed's masks and ends where the same job trained alone ends."""
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.multijob import PackedJobs

    def eng(seed, packed):
        cfg = _cfg(CASES["a"][0], optimizer="AdagradOptimizer", lr=0.01, seed=seed)
        return TrainEngine(cfg, synthetic_mnist(600, seed=seed), device="cuda", backend="hip",
                           use_graph=packed, packed=packed)

    packed = [eng(s, True) for s in (0, 1)]
    assert all(e.backend == "hip" and e.program.packed for e in packed)
    pack = PackedJobs(packed)
    for _ in range(4):
        pack.step()
    pack.sync_device()
    masks = []
    for s, e in zip((0, 1), packed):
        solo = eng(s, False)
        for _ in range(4):
            solo.step()
        torch.cuda.synchronize()
        assert e.host_step == 4 and int(e.dstep.item()) == 4
        d = (e.flat - solo.flat).abs().max().item()
        print(f"seed {s}: packed vs solo {d:.3e}")
        assert d < 3e-3             # atomics: run-to-run fp32 order (test_graph_replay_matches_eager)
        (u,) = [u for u in e.program.units if u.kind == "drop"]
        assert int(u.used_step.item()) == 3
        nz = (u.y != 0).cpu().numpy()
        assert nz.any() and not nz[~D.keep_mask(D.drop_seed(s, u.layer.index), 3, 50, u.x[0].numel(), 0.5)].any()
        masks.append(nz)
    assert 0.1 < (masks[0] != masks[1]).mean() < 0.6


# ----------------------------------------------------------------------- 5. deterministic mode
def test_deterministic_graph_equals_eager(monkeypatch):
    from cloud_server_amd.runtime.engine import TrainEngine
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    ds = synthetic_mnist(400, seed=5)
    cfg = _cfg(CASES["a"][0], optimizer="AdagradOptimizer", lr=0.01)
    outs = []
    for graph in (True, False):
        eng = TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=graph)
        assert eng.backend == "hip" and eng.program.det
        assert any(u.kind == "drop" for u in eng.program.units)
        for _ in range(4):
            eng.step()
        torch.cuda.synchronize()
        outs.append([eng.flat.clone(), eng.slots.clone()] + [x.clone() for x in eng.model.buffers()])
    assert all(torch.equal(x, y) for x, y in zip(*outs))
