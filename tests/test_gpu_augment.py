"""Training-time augmentation on the GPU: ``csa_augment_batch`` (augment.hip) against the
NumPy float32 definition (ops/augment_ref.py) byte for byte, the lowered step against the
eager program, images advancing with the device step counter under multi-step graphs,
augmentation-free evaluation / validation / serving, deterministic mode, packed jobs, and the
option absent or all zero."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config
from cloud_server_amd.ops import augment_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, SENTINEL = 64, 0xA5

# the five parameter sets of the byte-parity tests (as in test_augment_cpu.py)
SETS = {
    "shift": {"shift": 3},
    "rotate": {"rotate": 20},
    "scale": {"scale": 15},
    "erase": {"erase_prob": 0.6, "erase_max": 9, "fill": 77},
    "all": {"shift": 8, "rotate": 45, "scale": 30, "erase_prob": 0.5, "erase_max": 14, "fill": 255},
}
AUG = {"shift": 2, "rotate": 10, "scale": 10, "erase_prob": 0.25}
STRONG = {"shift": 8, "rotate": 45, "scale": 30, "erase_prob": 1, "erase_max": 14}
SAMPLE = SAMPLE_CONFIG["net_config"]["middle_layer"]


def _cfg(layers, aug=None, **kw):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c["optimizer_name"] = kw.pop("optimizer", "GradientDescentOptimizer")
    c["learning_rate"] = kw.pop("lr", 0.5)
    c["loss_name"] = kw.pop("loss", "entropy")
    c["options"] = dict(batch_size=kw.pop("batch", 50), **kw)
    if aug is not None:
        c["options"]["augment"] = aug
    return parse_train_config(c)


def _plan(aug, seed=0):
    return A.Plan(_cfg(SAMPLE, aug).augment, seed)


@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


def _ref(plan, ds, rows, step):
    rows = np.asarray(rows)
    return torch.from_numpy(A.augment_np(plan, ds.images[rows], rows, step))


def _step_rows(eng, k):
    """The dataset rows of step ``k`` (< the row table's half: no refill yet)."""
    return eng.stream.rows[k].cpu().numpy()


# ----------------------------------------------------------------------- 1. the kernel
def _row_table(B, n):
    """[4, B] rows in [0, n): every line holds the first and the last dataset row (B = 1: lines
    1 and 3 hold them in turn) and, from B = 3 on, one row twice."""
    t = np.random.default_rng(B).integers(0, n, size=(4, B)).astype(np.int64)
    if B == 1:
        t[:, 0] = [5, 0, 6, n - 1]
    elif B == 3:
        t[:] = [n - 1, 0, n - 1]
    else:
        t[:, 0], t[:, 1], t[:, 3] = 0, n - 1, t[:, 2]
    return t


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("B", [1, 3, 50])
def test_kernel_matches_numpy_bytes(B, name, dataset):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    plan = _plan(SETS[name], seed=11)
    pc = plan.to_c()
    n = len(dataset)
    images = torch.from_numpy(dataset.images).to(DEV)
    table = _row_table(B, n)
    rows = torch.from_numpy(table).to(DEV)
    cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    buf = torch.full((GUARD + B * 784 + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + B * 784].view(B, 784)
    # a nonzero cursor, the last line of the table, and line 0
    for t, cur in ((0, 1), (7, 3), ((1 << 32) + 9, 0)):
        cursor.fill_(cur)
        step.fill_(t)
        buf.fill_(SENTINEL)
        rc = lib.csa_augment_batch(K.ptr(images), K.ptr(rows), K.ptr(cursor), B, 28, 28, ctypes.byref(pc),
                                   plan.seed, K.ptr(step), K.ptr(out), K.stream())
        assert rc == 0
        torch.cuda.synchronize()
        want = _ref(plan, dataset, table[cur], t)
        got = out.cpu()
        assert torch.equal(got, want), (name, B, t, int((got != want).sum()))
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + B * 784:] == SENTINEL).all())
        assert int(cursor.item()) == cur and int(step.item()) == t
    # (the last launch: line 0, step 2^32 + 9, which is step 9)
    assert torch.equal(_ref(plan, dataset, table[0], 9), got)
    if B >= 3:
        i, j = (0, 2) if B == 3 else (2, 3)
        assert table[0][i] == table[0][j] and torch.equal(got[i], got[j])  # a row twice: its image twice


def test_launcher_rejects_bad_arguments(dataset):
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    plan = _plan(SETS["all"])
    images = torch.from_numpy(dataset.images[:8].copy()).to(DEV)
    rows = torch.zeros(1, 4, dtype=torch.int64, device=DEV)
    w = torch.zeros(1, dtype=torch.int64, device=DEV)
    buf = torch.zeros(4 * 784 + 8, dtype=torch.uint8, device=DEV)
    pc = plan.to_c()

    def call(args):
        return lib.csa_augment_batch(*args)

    ok = [K.ptr(images), K.ptr(rows), K.ptr(w), 4, 28, 28, ctypes.byref(pc), plan.seed, K.ptr(w), K.ptr(buf),
          K.stream()]
    assert call(ok) == 0
    for i, bad in ((0, None), (1, None), (2, None), (3, 0), (3, -4), (4, 27), (5, 29), (4, 32), (6, None), (8, None),
                   (9, None), (9, K.ptr(buf) + 2), (0, K.ptr(images) + 1)):
        args = list(ok)
        args[i] = bad
        assert call(args) < 0, (i, bad)
    for field, bad in (("shift", 9), ("shift", -1), ("rotate", 46), ("rotate", -1), ("scale", 31), ("scale", -1),
                       ("erase_max", 0), ("erase_max", 15), ("fill", 256), ("fill", -1), ("erase_T", (1 << 24) + 1),
                       ("erase_T", -1)):
        p = plan.to_c()
        setattr(p, field, bad)
        args = list(ok)
        args[6] = ctypes.byref(p)
        assert call(args) < 0, (field, bad)
    torch.cuda.synchronize()
    assert not buf[4 * 784:].any()


# ----------------------------------------------------------------------- 2. one step vs eager
LOWERINGS = {
    # the sample config: the fused conv pair, the staged batch, the horizontally fused program
    "sample": (SAMPLE, 50),
    # test_gpu_dropout's case b without its dropouts: a raw single first conv, batch 7
    "raw_conv": ([{"layer": "conv", "filter": [3, 3, 3], "padding": "VALID"},
                  {"layer": "active"},
                  {"layer": "pool"},
                  {"layer": "connect", "hidden": 32}], 7),
    # a dense first layer: the float gather
    "dense_first": ([{"layer": "connect", "hidden": 64}], 50),
}


def _check_lowering(name, prog):
    kinds = [u.kind for u in prog.units]
    assert prog.aug is not None and prog.aug_img is not None
    if name == "sample":
        assert prog.pair is not None and prog.staged and prog.hfuse, (prog.pair, prog.staged, prog.hfuse)
    elif name == "raw_conv":
        assert kinds == ["conv", "dense"] and prog.pair is None and prog.units[0].x is None, kinds
    else:
        assert kinds == ["dense"] and prog.x_dense_in is not None, kinds


def _run_one(cfg, backend, ds, name=None):
    from cloud_server_amd.runtime.engine import TrainEngine
    eng = TrainEngine(cfg, ds, device="cuda", backend=backend, use_graph=False)
    assert eng.backend == backend, eng.fallback_reason
    if backend == "hip":
        _check_lowering(name, eng.program)
    w0 = eng.flat.clone()
    rows = _step_rows(eng, 0)
    eng.step()
    torch.cuda.synchronize()
    return eng, w0, eng.flat.clone(), rows


@pytest.mark.parametrize("name", list(LOWERINGS))
@pytest.mark.parametrize("loss", ["entropy", "mse"])
def test_step_matches_torch(name, loss, dataset):
    layers, batch = LOWERINGS[name]
    cfg = _cfg(layers, AUG, loss=loss, lr=0.5, batch=batch)
    eh, w0h, w1h, rows_h = _run_one(cfg, "hip", dataset, name)
    et, w0t, w1t, rows_t = _run_one(cfg, "torch", dataset)
    assert torch.equal(w0h, w0t) and np.array_equal(rows_h, rows_t)
    # both programs trained on exactly the reference's bytes for step 0's rows
    want = _ref(A.Plan(cfg.augment, cfg.seed), dataset, rows_h, 0)
    assert torch.equal(eh.program.aug_img.cpu(), want)
    assert torch.equal(et.program.aug_img.cpu(), want)
    assert (want != torch.from_numpy(dataset.images[rows_h])).float().mean() > 0.05
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
    print(f"{name}/{loss} loss {mh['loss']:.6f} vs {mt['loss']:.6f}")
    assert abs(mh["loss"] - mt["loss"]) < 1e-4 * max(1, abs(mt["loss"]))
    assert mh["accuracy"] == mt["accuracy"]


# ----------------------------------------------------------------------- 3. steps advance the images
def test_images_advance_under_multi_step_graphs(monkeypatch):
    from cloud_server_amd.runtime.engine import TrainEngine
    ds = synthetic_mnist(700, seed=29)
    cfg = _cfg(SAMPLE, AUG, optimizer="AdagradOptimizer", lr=0.01)
    monkeypatch.setenv("CSA_GRAPH_STEPS", "4")
    a = TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=True)
    b = TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=False)
    t = TrainEngine(cfg, ds, device="cuda", backend="torch", use_graph=False)
    assert a.program.hfuse and a.program.aug is not None
    a.step()
    a.prepare_group_graph()
    assert a.graph_k is not None
    a.run_steps(5)
    for _ in range(6):
        b.step()
        t.step()
    torch.cuda.synchronize()
    assert a.host_step == 6 and int(a.dstep.item()) == 6
    plan = A.Plan(cfg.augment, cfg.seed)
    got = a.program.aug_img.cpu()
    assert torch.equal(got, _ref(plan, ds, _step_rows(a, 5), 5))
    assert not torch.equal(got, _ref(plan, ds, _step_rows(a, 4), 4))
    assert not torch.equal(got, _ref(plan, ds, _step_rows(a, 5), 4))           # same rows, the step before
    assert torch.equal(b.program.aug_img.cpu(), got) and torch.equal(t.program.aug_img.cpu(), got)
    d_ab = (a.flat - b.flat).abs().max().item()
    d_at = (a.flat - t.flat).abs().max().item()
    d_bt = (b.flat - t.flat).abs().max().item()
    print(f"graph vs eager hip {d_ab:.3e}, graph vs torch {d_at:.3e}, eager hip vs torch {d_bt:.3e}")
    assert d_ab < 3e-3          # (test_gpu_dropout.test_mask_advances_under_multi_step_graphs)
    assert d_at < 2e-3 and d_bt < 2e-3


# ----------------------------------------------------------------------- 4. evaluation, serving
def _bound(ref):
    """The project's HIP-vs-reference tolerance (tests/test_gpu_dropout.py ``_bound``)."""
    return 1e-4 + 1e-4 * float(np.abs(ref).max())


def _state(eng):
    return ([eng.flat.clone(), eng.slots.clone(), eng.stream.cursor.clone(), eng.dstep.clone(),
             eng.ring_loss.clone(), eng.ring_correct.clone()] + [x.clone() for x in eng.model.buffers()]
            + [eng.program.aug_img.clone()])


def test_evaluation_validation_and_serving_see_unaugmented_images():
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.validation import HipValidator, TorchValidator
    from cloud_server_amd.serve.hip_infer import HipPredictor
    train, test = synthetic_mnist(1000, seed=0).split(0.8)
    c = _cfg(SAMPLE, STRONG, optimizer="AdamOptimizer", lr=1e-3)
    eng = TrainEngine(c, train, device=DEV, backend="hip")
    assert eng.backend == "hip", eng.fallback_reason
    for _ in range(10):
        eng.step()
    torch.cuda.synchronize()
    assert eng.program.aug_img.any()
    # evaluate(): the same accuracy as the torch engine holding the same parameters
    ref = TrainEngine(c, train, device=DEV, backend="torch", use_graph=False)
    ref.flat.copy_(eng.flat)
    for (_, x), (_, y) in zip(ref.model.named_buffers(), eng.model.named_buffers()):
        x.copy_(y)
    assert eng.evaluate(test) == ref.evaluate(test)
    # the validation sweep: a forward-only program without augmentation, equal to the eager
    # validator (which reads the stored images), training state untouched bit for bit
    before = _state(eng)
    val = eng.validator(test, 64, True)
    assert isinstance(val, HipValidator) and val.program.forward_only
    assert val.program.aug is None and val.program.aug_img is None
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
    # the training program's own predict reads the stored rows of the cursor's batch
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
    assert all(torch.equal(x, y) for x, y in zip(before, _state(eng)))       # aug_img untouched too
    # serving: the logits of the eval-mode model on the posted bytes
    pred = HipPredictor(c, eng.model.export_state(), torch.device(DEV), buckets=(16,), preps=("mnist",))
    for bk in pred._buckets.values():
        assert bk.program.aug is None
    x8 = test.images[:16].reshape(16, 784)
    got = pred.logits_u8(np.ascontiguousarray(x8), "mnist")
    eng.model.eval()
    with torch.no_grad():
        zs = eng.model(torch.from_numpy(x8).to(DEV).float().div_(255.0)).cpu().numpy()
    eng.model.train()
    assert np.abs(got - zs).max() <= _bound(zs)


# ----------------------------------------------------------------------- 5. deterministic mode
def _det_run(cfg, ds, graph, steps):
    from cloud_server_amd.runtime.engine import TrainEngine
    eng = TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=graph)
    assert eng.backend == "hip" and eng.program.det
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    return eng, [eng.flat.clone(), eng.slots.clone()] + [x.clone() for x in eng.model.buffers()]


def test_deterministic_graph_equals_eager(monkeypatch):
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    ds = synthetic_mnist(400, seed=5)
    cfg = _cfg(SAMPLE, AUG, optimizer="AdagradOptimizer", lr=0.01)
    outs = []
    for graph in (True, False):
        eng, out = _det_run(cfg, ds, graph, 4)
        assert eng.program.aug is not None
        outs.append(out + [eng.program.aug_img.clone()])
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    assert torch.equal(outs[0][-1].cpu(), _ref(A.Plan(cfg.augment, cfg.seed), ds, _step_rows(eng, 3), 3))


# ----------------------------------------------------------------------- 6. packed jobs
def test_packed_jobs_with_augment_match_solo_runs():
    """Two augmenting jobs as branches of one graph (the packed launch profile): each draws
    its own seed's images and ends where the same job trained alone ends."""
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.multijob import PackedJobs
    ds = synthetic_mnist(600, seed=7)

    def eng(seed, packed):
        cfg = _cfg(SAMPLE, AUG, optimizer="AdagradOptimizer", lr=0.01, seed=seed)
        return TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=packed, packed=packed)

    packed = [eng(s, True) for s in (0, 1)]
    assert all(e.backend == "hip" and e.program.packed and e.program.aug is not None for e in packed)
    pack = PackedJobs(packed)
    for _ in range(4):
        pack.step()
    pack.sync_device()
    imgs = []
    for s, e in zip((0, 1), packed):
        solo = eng(s, False)
        for _ in range(4):
            solo.step()
        torch.cuda.synchronize()
        assert e.host_step == 4 and int(e.dstep.item()) == 4
        d = (e.flat - solo.flat).abs().max().item()
        print(f"seed {s}: packed vs solo {d:.3e}")
        assert d < 3e-3             # atomics: run-to-run fp32 order (test_graph_replay_matches_eager)
        got = e.program.aug_img.cpu()
        assert torch.equal(got, _ref(A.Plan(e.cfg.augment, s), ds, _step_rows(e, 3), 3))
        assert torch.equal(got, solo.program.aug_img.cpu())
        imgs.append(got)
    assert not torch.equal(imgs[0], imgs[1])


# ----------------------------------------------------------------------- 7. absent or all zero
def test_absent_and_all_zero_are_the_same_program(monkeypatch):
    from cloud_server_amd.runtime.hip_program import HipProgram
    calls = []
    launch = HipProgram._augment
    monkeypatch.setattr(HipProgram, "_augment", lambda self, st: (calls.append(1), launch(self, st))[1])
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    ds = synthetic_mnist(400, seed=5)
    outs = []
    for aug in (None, {"shift": 0, "rotate": 0, "scale": 0, "erase_prob": 0, "erase_max": 3, "fill": 9}):
        cfg = _cfg(SAMPLE, aug, optimizer="AdagradOptimizer", lr=0.01)
        eng, out = _det_run(cfg, ds, False, 3)
        p = eng.program
        assert eng.aug is None and p.aug is None and p.aug_img is None
        assert not hasattr(p, "aug_rows") and not hasattr(p, "aug_cur") and not hasattr(p, "aug_c")
        assert all(x is y for x, y in zip(p._train_src(), p._batch_src()))
        assert p._train_src(table=True)[0] is eng.data.images
        outs.append(out)
    assert not calls                                                     # no augmentation launch
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    # and with the option the launch is issued once a step
    eng, _ = _det_run(_cfg(SAMPLE, AUG, optimizer="AdagradOptimizer", lr=0.01), ds, False, 3)
    assert len(calls) == 3 and eng.program.aug_img is not None
