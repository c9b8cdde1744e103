"""Learning-rate schedules (``options.lr_schedule``) without a GPU: parsing, the definition
(NumPy float32 against float64), the eager engine's trajectory against a schedule-aware fp64
oracle, resume, data parallelism on gloo and reporting.

A tree without the feature ignores the option silently: from step 2 on the eager update is
then at least 2 x off (the trajectory tests below fail there)."""
import copy
import dataclasses
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import oracle64 as X
import oracle64_sched as XS
from test_distributed import CFG as DCFG, _init, _port

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import ConfigError, LrSchedule, SAMPLE_CONFIG, parse_train_config
from cloud_server_amd.ops import lr_schedule as L
from cloud_server_amd.runtime import checkpoint as ckpt
from cloud_server_amd.runtime.engine import TrainEngine

T = np.arange(1, 65)


_ABSENT = object()


def _cfg(sched=_ABSENT, **options):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["options"] = dict(options)
    if sched is not _ABSENT:
        c["options"]["lr_schedule"] = sched
    return c


# ------------------------------------------------------------------------------ parsing
def test_defaults():
    assert parse_train_config(_cfg()).lr_schedule == LrSchedule()
    s = parse_train_config(_cfg({})).lr_schedule
    assert s == LrSchedule("constant", 1, 1.0, False, 0.0, 0) and not L.active(s) and L.to_c(s) is None
    s = parse_train_config(_cfg({"type": "cosine", "decay_steps": 10})).lr_schedule
    assert (s.type, s.decay_steps, s.alpha, s.warmup_steps, s.staircase) == ("cosine", 10, 0.0, 0, False)
    s = parse_train_config(_cfg({"warmup_steps": 3})).lr_schedule
    assert s.type == "constant" and s.warmup_steps == 3 and L.active(s)


def test_string_numbers_and_round_trip():
    raw = {"type": "exponential", "decay_steps": "7", "decay_rate": "0.5", "staircase": "true",
           "warmup_steps": "2"}
    cfg = parse_train_config(_cfg(raw))
    assert cfg.lr_schedule == LrSchedule("exponential", 7, 0.5, True, 0.0, 2)
    assert cfg.to_json()["options"]["lr_schedule"] == raw              # round-trips through raw
    assert parse_train_config(json.dumps(cfg.to_json())).lr_schedule == cfg.lr_schedule
    c = L.to_c(cfg.lr_schedule)
    assert (c.kind, c.staircase, c.decay_steps, c.warmup_steps, c.rate, c.alpha) == (1, 1, 7, 2, 0.5, 0.0)
    import ctypes
    assert ctypes.sizeof(L.LrSchedC) == 24


BAD = [
    {"type": "step"},                                                   # unknown type
    {"type": "cosine", "decay_steps": 4, "gamma": 0.1},                 # unknown key
    {"type": "exponential", "decay_rate": 0.5},                         # decay_steps required
    {"type": "exponential", "decay_steps": 4},                          # decay_rate required
    {"type": "inverse_time", "decay_steps": 4},
    {"type": "cosine"},
    {"type": "exponential", "decay_steps": 0, "decay_rate": 0.5},       # out of range
    {"type": "exponential", "decay_steps": 2.5, "decay_rate": 0.5},
    {"type": "exponential", "decay_steps": 4, "decay_rate": 0.0},
    {"type": "exponential", "decay_steps": 4, "decay_rate": 1.5},
    {"type": "inverse_time", "decay_steps": 4, "decay_rate": -0.1},
    {"type": "cosine", "decay_steps": 4, "alpha": 1.5},
    {"type": "cosine", "decay_steps": 4, "alpha": -0.1},
    {"type": "cosine", "decay_steps": 4, "warmup_steps": -1},
    {"type": "cosine", "decay_steps": "many"},
    {"type": "exponential", "decay_steps": 4, "decay_rate": 0.5, "staircase": "maybe"},
    "cosine",                                                           # not an object
    ["cosine"],
    None,
]


@pytest.mark.parametrize("bad", BAD, ids=[json.dumps(b)[:48] for b in BAD])
def test_invalid_schedules_raise(bad):
    with pytest.raises(ConfigError):
        parse_train_config(_cfg(bad))


def test_compat_adagrad_goes_with_constant_only():
    with pytest.raises(ConfigError):
        parse_train_config(_cfg({"type": "cosine", "decay_steps": 4}, compat_adagrad=True))
    cfg = parse_train_config(_cfg({"type": "constant"}, compat_adagrad=True))
    assert cfg.effective_lr == 1e-4 and L.lr_at(cfg, 9) == 1e-4


def test_api_rejects_a_bad_schedule(tmp_path):
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
               "options": {"lr_schedule": {"type": "cosine", "decay_steps": 0}}}
        r = c.post("/construct/construction/m/file/", json=cfg, headers={"Authorization": "Token " + key})
        assert r.status_code == 400, r.text
        assert "lr_schedule" in r.text


# ------------------------------------------------------------------------------ definition
def _schedules():
    out = []
    for S in (1, 3, 7):
        for W in (0, 1, 5):
            for stair in (False, True):
                out.append(LrSchedule("exponential", S, 0.5, stair, 0.0, W))
                out.append(LrSchedule("inverse_time", S, 0.5, stair, 0.0, W))
            out.append(LrSchedule("cosine", S, 1.0, False, 0.0, W))
            out.append(LrSchedule("cosine", S, 1.0, False, 0.25, W))
    return out


SCHEDULES = _schedules()


def _sid(s):
    return f"{s.type}-S{s.decay_steps}-W{s.warmup_steps}" + ("-stair" if s.staircase else "") + \
        (f"-a{s.alpha}" if s.alpha else "")


@pytest.mark.parametrize("s", SCHEDULES, ids=_sid)
def test_float32_form_matches_float64(s):
    """A handful of fp32 roundings plus NumPy's float32 pow / cos (a few ulp); the rounding of
    the quotient x is amplified by |x ln r| <= 21 ln 2 = 14.6 where it is inexact (S = 3, 7;
    S = 1 has an exact x): 14.6 * 6e-8 + ~1e-6 < 5e-6."""
    lr = 0.01
    a, b = L.lr_f32(s, lr, T), L.lr_f64(s, lr, T)
    assert a.dtype == np.float32 and b.dtype == np.float64
    err = np.abs(a.astype(np.float64) - b)
    print(_sid(s), "worst relative error", (err[b > 0] / b[b > 0]).max())
    assert (b >= 0).all() and (err <= 5e-6 * b).all()          # (cosine's floor 0 is exact in both)
    for t in (1, 2, 17, 64):
        assert L.lr_at(SimpleNamespace(lr_schedule=s, effective_lr=lr), t) == float(a[t - 1])


@pytest.mark.parametrize("s", [s for s in SCHEDULES if s.staircase and s.warmup_steps == 0], ids=_sid)
def test_staircase_plateaus_and_edges(s):
    """Bitwise equal inside a stair, a change exactly at g = kS (S = 3, 7: where the floor of
    a float quotient picks the wrong stair)."""
    v = L.lr_f32(s, 0.01, T)
    for t in T[1:]:
        g = t - 1
        same = v[t - 1] == v[t - 2]
        assert same == (g % s.decay_steps != 0), (t, v[t - 2], v[t - 1])
        if not same:
            assert v[t - 1] < v[t - 2]


@pytest.mark.parametrize("s", SCHEDULES, ids=_sid)
def test_decay_never_increases_after_warmup(s):
    v = L.lr_f32(s, 0.01, T)
    after = v[s.warmup_steps:]
    assert (np.diff(after.astype(np.float64)) <= 0).all()
    W = s.warmup_steps
    if W:                                                     # the warm-up: m * float(g + 1) / float(W), g < W
        m, base = L.mult_f32(s, T), L.mult_f32(dataclasses.replace(s, warmup_steps=0), T)
        ramp = np.arange(1, W + 1).astype(np.float32) / np.float32(W)
        assert (m[:W] == base[:W] * ramp).all() and (m[W:] == base[W:]).all()
    if s.type == "cosine":
        lr32 = np.float32(0.01)
        tail = v[max(s.decay_steps, s.warmup_steps):]          # g >= S (and past the warm-up)
        assert (tail == lr32 * np.float32(s.alpha)).all() if s.alpha else (tail == 0).all()


def test_constant_is_lr_bitwise():
    for s in (None, LrSchedule()):
        v = L.lr_f32(s, 0.0123, T)
        assert (v == np.float32(0.0123)).all()
    cfg = parse_train_config(_cfg({"type": "constant"}))
    assert L.lr_at(cfg, 5) == cfg.effective_lr                 # the Python float itself
    eng = TrainEngine(cfg, synthetic_mnist(100, seed=3), device="cpu", backend="torch")
    assert eng.lr_sched is None and eng.lr_sched_c is None


def test_torch_form_matches_numpy():
    for s in SCHEDULES:
        got = L.lr_torch(s, 0.01, torch.from_numpy(T)).numpy()
        ref = L.lr_f64(s, 0.01, T)
        assert got.dtype == np.float32
        assert (np.abs(got - ref) <= 5e-6 * ref + 1e-12).all(), _sid(s)
        if s.staircase and s.warmup_steps == 0:
            g = T - 1
            assert ((got[1:] == got[:-1]) == (g[1:] % s.decay_steps != 0)).all(), _sid(s)


# ------------------------------------------------------------------------------ eager trajectory
@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


@pytest.mark.parametrize("sched", [XS.STAIR_HALF, XS.COSINE_WARM], ids=["stair_half", "cosine_warm"])
@pytest.mark.parametrize("opt", list(X.LRS), ids=lambda o: X.SHORT[o])
def test_eager_trajectory_follows_the_schedule(opt, sched, dataset):
    cfg = XS.make_cfg(XS.SAMPLE128, opt, X.LRS[opt], sched)
    eng = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    XS.run_trajectory(eng, XS.SchedOracle64(cfg, dataset, decisions=False), 4, "sample",
                      f"{X.SHORT[opt]}-{sched['type']}", max_borderline=1)


# ------------------------------------------------------------------------------ resume
@pytest.mark.parametrize("opt", ["AdagradOptimizer", "AdamOptimizer"], ids=lambda o: X.SHORT[o])
def test_resume_is_exact(opt, dataset):
    cfg = XS.make_cfg(XS.SAMPLE128, opt, X.LRS[opt], {"type": "exponential", "decay_steps": 2, "decay_rate": 0.5,
                                                      "warmup_steps": 2})
    a = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    for _ in range(6):
        a.step()
    b = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    for _ in range(3):
        b.step()
    obj = ckpt.engine_state(b)
    assert not any("lr" in str(k).lower() and "sched" in str(k).lower() for k in obj)    # no schedule state
    c = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    ckpt.restore_engine(c, obj)
    for _ in range(3):
        c.step()
    assert int(c.dstep.item()) == 6
    assert torch.equal(a.flat, c.flat) and torch.equal(a.slots, c.slots)


# ------------------------------------------------------------------------------ data parallel (gloo)
DSCHED = {"type": "exponential", "decay_steps": 2, "decay_rate": 0.5, "staircase": True, "warmup_steps": 2}


def _dcfg(batch, **opts):
    return parse_train_config(dict(DCFG, options=dict(DCFG["options"], batch_size=batch, lr_schedule=DSCHED, **opts)))


def _train(rank, world, port, strategy, steps, out):
    from cloud_server_amd.parallel.dist import shutdown
    ctx = _init(rank, world, port)
    eng = TrainEngine(_dcfg(8), synthetic_mnist(256, seed=1), device="cpu", ctx=ctx, strategy=strategy)
    for _ in range(steps):
        eng.step()
    out[rank] = eng.flat.clone()
    shutdown(ctx)


def _train_async(rank, world, port, steps, out):
    from cloud_server_amd.parallel.dist import shutdown
    ctx = _init(rank, world, port)
    eng = TrainEngine(_dcfg(16, staleness=1), synthetic_mnist(512, seed=1), device="cpu", ctx=ctx,
                      strategy="async_ps")
    for _ in range(steps):
        eng.step()
    eng.finish_async()
    out[rank] = (eng.aps.applied, list(eng.aps.lr_used), eng.flat.clone())
    shutdown(ctx)


def _spawn(fn, world, *args):
    out = mp.Manager().dict()
    mp.spawn(fn, args=(world, _port(), *args, out), nprocs=world, join=True)
    return dict(out)


@pytest.mark.parametrize("strategy", ["allreduce", "ps"])
def test_dp_equals_single_process_big_batch(strategy):
    out = _spawn(_train, 2, strategy, 6)
    torch.testing.assert_close(out[0], out[1], rtol=0, atol=0)
    eng = TrainEngine(_dcfg(16), synthetic_mnist(256, seed=1), device="cpu")
    for _ in range(6):
        eng.step()
    n = eng.flat.numel()
    torch.testing.assert_close(out[0][:n], eng.flat, rtol=2e-4, atol=2e-5)     # (test_distributed's tolerance)
    # and the schedule did act: the constant-rate run ends elsewhere
    ref = TrainEngine(parse_train_config(dict(DCFG, options=dict(DCFG["options"], batch_size=16))),
                      synthetic_mnist(256, seed=1), device="cpu")
    for _ in range(6):
        ref.step()
    assert (ref.flat - eng.flat).abs().max() > 1e-3


def test_async_ps_applies_the_rate_by_apply_count():
    steps, world = 6, 2
    out = _spawn(_train_async, world, steps)
    cfg = _dcfg(16, staleness=1)
    want = [L.lr_at(cfg, n) for n in range(1, world * steps + 1)]
    assert len(set(want)) > 3
    for r in range(world):
        applied, used, flat = out[r]
        assert applied == world * steps
        assert used == want, (r, used, want)
        torch.testing.assert_close(flat, out[0][2], rtol=0, atol=0)


# ------------------------------------------------------------------------------ reporting
def test_metrics_and_status_carry_lr(tmp_path):
    from cloud_server_amd.runtime.trainer import METRICS, RESULT, STATUS, run_job
    job = {"iter": 12, "learning_rate": 0.05, "ratio": 0.8, "loss_name": "entropy",
           "optimizer_name": "AdamOptimizer",
           "options": {"log_every": 3, "batch_size": 16,
                       "lr_schedule": {"type": "inverse_time", "decay_steps": 4, "decay_rate": 1.0,
                                       "warmup_steps": 2}},
           "net_config": {"middle_layer": [{"layer": "connect", "hidden": 16}]}}
    mdir = str(tmp_path / "m")
    os.makedirs(mdir)
    out = run_job(mdir, job, device="cpu", backend="torch", data=synthetic_mnist(200, seed=0).split(0.8))
    assert out["state"] == "done"
    cfg = parse_train_config(job)
    rows = [json.loads(l) for l in open(os.path.join(mdir, METRICS))]
    assert [r["step"] for r in rows] == [0, 3, 6, 9, 12][:len(rows)] and len(rows) >= 4
    for r in rows:
        assert r["lr"] == L.lr_at(cfg, r["step"] + 1), r
    assert len({r["lr"] for r in rows}) == len(rows)
    st = json.load(open(os.path.join(mdir, STATUS)))
    assert st["lr"] == L.lr_at(cfg, st["step"]) and st["step"] == 12
    assert all("lr" not in l for l in open(os.path.join(mdir, RESULT)))      # result.txt contract unchanged
