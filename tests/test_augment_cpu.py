"""options.augment on the CPU: parsing, the definition (ops/augment_ref.py: NumPy float32 is
the reference), the torch form against it byte for byte, exact resume on the eager engine,
and gloo data parallelism against one process on the global batch."""
import copy
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_distributed import CFG as DCFG, _init, _port

from cloud_server_amd.data.datasets import ArrayDataset, synthetic_mnist
from cloud_server_amd.models.dsl import Augment, ConfigError, SAMPLE_CONFIG, TrainConfig, parse_train_config
from cloud_server_amd.ops import augment_ref as A
from cloud_server_amd.runtime import checkpoint as ckpt
from cloud_server_amd.runtime.engine import TrainEngine

_ABSENT = object()

# the five parameter sets of the byte-parity tests (here and in test_gpu_augment.py)
SETS = {
    "shift": {"shift": 3},
    "rotate": {"rotate": 20},
    "scale": {"scale": 15},
    "erase": {"erase_prob": 0.6, "erase_max": 9, "fill": 77},
    "all": {"shift": 8, "rotate": 45, "scale": 30, "erase_prob": 0.5, "erase_max": 14, "fill": 255},
}


def _cfg(aug=_ABSENT, **options):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["options"] = dict(options)
    if aug is not _ABSENT:
        c["options"]["augment"] = aug
    return c


def _plan(aug: dict, seed: int = 0) -> A.Plan:
    return A.Plan(parse_train_config(_cfg(aug)).augment, seed)


@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


# ------------------------------------------------------------------------------ parsing
def test_defaults():
    assert parse_train_config(_cfg()).augment == Augment()
    assert Augment() == Augment(0, 0, 0, 0.0, 8, 0) and not A.active(Augment())
    assert not A.active(parse_train_config(_cfg()))
    a = parse_train_config(_cfg({"shift": 2})).augment
    assert a == Augment(shift=2, rotate=0, scale=0, erase_prob=0.0, erase_max=8, fill=0) and A.active(a)
    with pytest.raises(Exception):
        a.shift = 3                                                    # frozen


def test_string_numbers_and_round_trip():
    raw = {"shift": "2", "rotate": "10", "scale": 10.0, "erase_prob": "0.25", "erase_max": "6", "fill": "255"}
    cfg = parse_train_config(_cfg(raw))
    assert cfg.augment == Augment(2, 10, 10, 0.25, 6, 255)
    assert all(isinstance(getattr(cfg.augment, k), int) for k in ("shift", "rotate", "scale", "erase_max", "fill"))
    assert cfg.to_json()["options"]["augment"] == raw                  # round-trips through raw
    assert parse_train_config(json.dumps(cfg.to_json())).augment == cfg.augment


@pytest.mark.parametrize("key,lo,hi", [("shift", 0, 8), ("rotate", 0, 45), ("scale", 0, 30), ("erase_max", 1, 14),
                                       ("fill", 0, 255)])
def test_integer_range_edges(key, lo, hi):
    for v in (lo, hi):
        a = parse_train_config(_cfg({"erase_prob": 0.5, key: v})).augment
        assert getattr(a, key) == v
    for v in (lo - 1, hi + 1, 1.5, "x", True, None):
        with pytest.raises(ConfigError):
            parse_train_config(_cfg({"erase_prob": 0.5, key: v}))


def test_erase_prob_range_edges():
    assert parse_train_config(_cfg({"erase_prob": 1})).augment.erase_prob == 1.0
    assert parse_train_config(_cfg({"shift": 1, "erase_prob": 0})).augment.erase_prob == 0.0
    for v in (-0.01, 1.01, "often", float("nan"), None, True):
        with pytest.raises(ConfigError):
            parse_train_config(_cfg({"shift": 1, "erase_prob": v}))
    assert A.erase_threshold(0.0) == 0 and A.erase_threshold(1.0) == 1 << 24 and A.erase_threshold(0.25) == 1 << 22


@pytest.mark.parametrize("bad", [{"shift": 1, "shear": 2}, "shift", ["shift"], None, 3])
def test_unknown_key_and_non_objects_raise(bad):
    with pytest.raises(ConfigError):
        parse_train_config(_cfg(bad))


@pytest.mark.parametrize("aug", [{}, {"shift": 0, "rotate": "0", "scale": 0.0, "erase_prob": 0},
                                 {"erase_max": 3, "fill": 200}])
def test_all_zero_equals_absent(aug, dataset):
    cfg = parse_train_config(_cfg(aug))
    assert cfg.augment == Augment() == parse_train_config(_cfg()).augment
    assert not A.active(cfg) and A.make_plan(cfg) is None
    eng = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    assert eng.aug is None and eng.program.aug_img is None


def test_api_rejects_a_bad_augment(tmp_path):
    from fastapi.testclient import TestClient
    from cloud_server_amd.api.app import create_app
    from cloud_server_amd.config import Settings
    s = Settings(storage_root=str(tmp_path / "store"), db_path=str(tmp_path / "db.sqlite3"),
                 executor="inline", train_backend="torch")
    pw = "Str0ng-pass-42"
    with TestClient(create_app(s, executor="inline", ngpu=0, inference_device="cpu")) as c:
        r = c.post("/rest-auth/registration/", json={"username": "al", "email": "al@x.org", "password1": pw,
                                                       "password2": pw})
        assert r.status_code == 201, r.text
        key = c.post("/rest-auth/login/", json={"username": "al", "password": pw}).json()["key"]
        cfg = {"iter": 5, "learning_rate": 0.1, "net_config": {"middle_layer": [{"layer": "connect", "hidden": 8}]},
               "options": {"augment": {"rotate": 90}}}
        r = c.post("/construct/construction/m/file/", json=cfg, headers={"Authorization": "Token " + key})
        assert r.status_code == 400, r.text
        assert "augment" in r.text


def test_argument_struct_mirrors_the_plan():
    p = _plan(SETS["all"], seed=5)
    c = p.to_c()
    assert ctypes.sizeof(A.AugParamsC) == 4 * (6 + 91 + 91 + 61)
    assert (c.shift, c.rotate, c.scale, c.erase_max, c.fill, c.erase_T) == (8, 45, 30, 14, 255, 1 << 23)
    assert np.array_equal(np.array(c.cos[:]), p.cos) and np.array_equal(np.array(c.inv[:]), p.inv)
    assert p.cos.dtype == p.sin.dtype == p.inv.dtype == np.float32
    assert p.cos[45] == 1.0 and p.sin[45] == 0.0 and p.inv[30] == 1.0          # angle 0, zoom 1
    assert p.sin[0] == np.float32(np.sin(np.radians(-45.0))) and p.inv[0] == np.float32(100.0 / 70.0)
    assert p.seed == A.aug_seed(5) != A.aug_seed(6)


def test_unsupported_dataset_is_refused_at_construction():
    cfg = parse_train_config(_cfg({"shift": 1}))
    ds = synthetic_mnist(64, seed=0)
    bad = ArrayDataset(ds.images.astype(np.float32) / 255.0, ds.labels)
    with pytest.raises(ValueError, match="uint8"):
        TrainEngine(cfg, bad, device="cpu", backend="torch")


# ------------------------------------------------------------------------------ definition
ROWS = np.array([0, 133, 7, 42, 7, 399, 250, 1], dtype=np.int64)       # first, last, one row twice


def test_identity_parameters_return_the_input(dataset):
    # (the warp alone: an erase whose gate never opens keeps the plan active)
    p = A.Plan(Augment(0, 0, 0, 0.0, 8, 0), 0)
    rows = np.arange(134)
    for step in (0, 5):
        assert np.array_equal(A.augment_np(p, dataset.images[rows], rows, step), dataset.images[rows])


@pytest.mark.parametrize("fill", [0, 255])
def test_shift_only_is_an_integer_shift_with_fill(fill, dataset):
    p = _plan({"shift": 8, "fill": fill})
    rows = np.arange(134)
    src = dataset.images[rows].reshape(-1, 28, 28)
    out = A.augment_np(p, dataset.images[rows], rows, 3).reshape(-1, 28, 28)
    r = A.draws(p, rows, 3).astype(np.int64)
    dx, dy = r[:, 0] % 17 - 8, r[:, 1] % 17 - 8
    assert dx.min() == -8 and dx.max() == 8 and len(set(dy)) > 8
    for b in range(len(rows)):
        want = np.full((28, 28), fill, np.uint8)
        ys, xs = np.arange(28) - dy[b], np.arange(28) - dx[b]           # out[y, x] = src[y - dy, x - dx]
        oky, okx = (ys >= 0) & (ys < 28), (xs >= 0) & (xs < 28)
        want[np.ix_(oky, okx)] = src[b][np.ix_(ys[oky], xs[okx])]
        assert np.array_equal(out[b], want), b


def test_erase_always_and_never(dataset):
    rows = np.arange(134)
    src = dataset.images[rows]
    p = _plan({"erase_prob": 1, "erase_max": 14, "fill": 255})
    out = A.augment_np(p, src, rows, 2).reshape(-1, 28, 28)
    rect = A.erase_rects(p, rows, 2)
    assert rect[:, 0].all()
    seen_h = set()
    for b, (_, top, left, eh, ew) in enumerate(rect):
        assert 1 <= eh <= 14 and 1 <= ew <= 14 and 0 <= top and top + eh <= 28 and 0 <= left and left + ew <= 28
        want = src[b].reshape(28, 28).copy()
        want[top:top + eh, left:left + ew] = 255
        assert np.array_equal(out[b], want), b
        seen_h.add(int(eh))
    assert {1, 14} <= seen_h or len(seen_h) >= 10
    # erase_prob 0 with another amount set: never
    p0 = _plan({"shift": 1, "erase_prob": 0, "fill": 255})
    assert not A.erase_rects(p0, rows, 2)[:, 0].any()
    assert np.array_equal(A.augment_np(p0, src, rows, 2),
                          A.augment_np(_plan({"shift": 1, "fill": 255, "erase_max": 2}), src, rows, 2))


def test_output_depends_on_seed_step_and_row_only(dataset):
    p = _plan(SETS["all"], seed=3)
    src = dataset.images[ROWS]
    out = A.augment_np(p, src, ROWS, 9)
    perm = np.array([5, 0, 3, 7, 1, 2, 6, 4])
    assert np.array_equal(A.augment_np(p, src[perm], ROWS[perm], 9), out[perm])       # batch position: no
    assert np.array_equal(out[2], out[4]) and ROWS[2] == ROWS[4]                      # a repeated row
    assert np.array_equal(A.augment_np(p, src[:1], ROWS[:1], 9), out[:1])             # batch size: no
    assert np.array_equal(A.augment_np(p, src, ROWS, (1 << 32) + 9), out)             # step mod 2^32
    assert not np.array_equal(A.augment_np(p, src, ROWS, 10), out)
    assert not np.array_equal(A.augment_np(_plan(SETS["all"], seed=4), src, ROWS, 9), out)
    assert not np.array_equal(A.augment_np(p, src, ROWS + np.array([1, 0, 0, 0, 0, 0, 0, 0]), 9)[0], out[0])


# ------------------------------------------------------------------------------ torch form
@pytest.mark.parametrize("name", list(SETS))
def test_torch_form_matches_numpy_bytes(name, dataset):
    p = _plan(SETS[name], seed=11)
    rows = np.concatenate([ROWS, np.arange(100, 142)])
    src = dataset.images[rows]
    for step in (0, 7, (1 << 32) + 9):
        want = A.augment_np(p, src, rows, step)
        got = A.augment_torch(p, torch.from_numpy(src), torch.from_numpy(rows),
                              torch.tensor([step], dtype=torch.int64))
        assert got.dtype == torch.uint8 and got.shape == (len(rows), 784)
        assert np.array_equal(got.numpy(), want), (name, step, int((got.numpy() != want).sum()))
        if name != "erase":
            assert (want != src).mean() > 0.05                           # and the warp did act


# ------------------------------------------------------------------------------ engine
AUG = {"shift": 2, "rotate": 10, "scale": 10, "erase_prob": 0.25}


def test_resume_is_exact_and_the_program_trains_on_the_reference_images(dataset):
    cfg = parse_train_config(_cfg(AUG, seed=2))
    a = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    plan = A.Plan(cfg.augment, cfg.seed)
    for k in range(6):
        rows = a.stream.rows[int(a.stream.cursor.item())].numpy().copy()          # step k's dataset rows
        a.step()
        want = A.augment_np(plan, dataset.images[rows], rows, k)
        assert np.array_equal(a.program.aug_img.numpy(), want), k
        assert (want != dataset.images[rows]).any()
    b = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    for _ in range(3):
        b.step()
    obj = ckpt.engine_state(b)
    assert not any("aug" in str(k).lower() for k in obj)                          # no augmentation state
    c = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    ckpt.restore_engine(c, obj)
    for _ in range(3):
        c.step()
    assert int(c.dstep.item()) == 6
    assert torch.equal(a.flat, c.flat) and torch.equal(a.slots, c.slots)
    assert torch.equal(a.program.aug_img, c.program.aug_img)
    # and augmentation did change the run
    ref = TrainEngine(parse_train_config(_cfg(seed=2)), dataset, device="cpu", backend="torch")
    for _ in range(6):
        ref.step()
    assert not torch.equal(ref.flat, a.flat)


# ------------------------------------------------------------------------------ data parallel (gloo)
def _dcfg(batch, **opts) -> TrainConfig:
    return parse_train_config(dict(DCFG, options=dict(DCFG["options"], batch_size=batch, augment=AUG, **opts)))


def _train(rank, world, port, steps, out):
    from cloud_server_amd.parallel.dist import shutdown
    ctx = _init(rank, world, port)
    eng = TrainEngine(_dcfg(8), synthetic_mnist(256, seed=1), device="cpu", ctx=ctx, strategy="allreduce")
    for _ in range(steps):
        eng.step()
    out[rank] = eng.flat.clone()
    shutdown(ctx)


def test_dp_equals_single_process_big_batch():
    out = mp.Manager().dict()
    mp.spawn(_train, args=(2, _port(), 6, out), nprocs=2, join=True)
    out = dict(out)
    torch.testing.assert_close(out[0], out[1], rtol=0, atol=0)
    eng = TrainEngine(_dcfg(16), synthetic_mnist(256, seed=1), device="cpu")
    for _ in range(6):
        eng.step()
    n = eng.flat.numel()
    torch.testing.assert_close(out[0][:n], eng.flat, rtol=2e-4, atol=2e-5)     # (test_distributed's tolerance)
    # and the augmentation did act: the run on the stored images ends elsewhere
    ref = TrainEngine(parse_train_config(dict(DCFG, options=dict(DCFG["options"], batch_size=16))),
                      synthetic_mnist(256, seed=1), device="cpu")
    for _ in range(6):
        ref.step()
    assert (ref.flat - eng.flat).abs().max() > 1e-4
