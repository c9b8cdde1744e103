"""The dropout layer on the CPU: DSL, the one mask definition (NumPy == torch), the eager
model, exact resume, and world-2 data parallelism drawing the mask of one big batch.

The reference feeds ``keep_prob`` 0.5 / 1.0 and never applies it (construct_distribute.py:
364-417); here ``{"layer": "dropout"}`` is a real layer whose mask is a pure function of
(seed, layer, step, element): ops/dropout_ref.py."""
import copy
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, ConfigError, parse_layer, parse_train_config
from cloud_server_amd.preprocess import ops_ref


def _cfg(layers, **opts):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = layers
    c["options"] = dict(opts)
    return parse_train_config(c)


# ---------------------------------------------------------------- 1. parse
def test_parse_dropout_layer():
    from cloud_server_amd.models.dsl import DropoutSpec
    sp = parse_layer({"layer": "dropout"}, 0)
    assert isinstance(sp, DropoutSpec) and sp.keep_prob == 0.5 and sp.kind == "dropout"
    assert parse_layer({"layer": "dropout", "keep_prob": "0.8"}, 0).keep_prob == 0.8
    assert parse_layer({"layer": "dropout", "keep_prob": 1}, 0).keep_prob == 1.0
    for bad in (0, -1, 1.5, "x"):
        with pytest.raises(ConfigError):
            parse_layer({"layer": "dropout", "keep_prob": bad}, 0)
    base = SAMPLE_CONFIG["net_config"]["middle_layer"]
    with_drop = ([{"layer": "dropout", "keep_prob": 0.9}] + base[:3] + [{"layer": "dropout"}] + base[3:6]
                 + [{"layer": "dropout", "keep_prob": "0.25"}] + base[6:])
    a, b = _cfg(base), _cfg(with_drop)
    assert [s.kind for s in b.layers].count("dropout") == 3 and b.layers[0].kind == "dropout"
    pa, pb = a.plan(), b.plan()
    assert [lp.spec.kind for lp in pb.layers].count("dropout") == 3
    for lp in pb.layers:
        if lp.spec.kind == "dropout":
            assert lp.in_shape == lp.out_shape and not lp.params
    assert pa.num_params() == pb.num_params() and pa.flops_per_sample() == pb.flops_per_sample()
    assert pa.head_in == pb.head_in
    assert list(pa.param_shapes().values()) == list(pb.param_shapes().values())
    # the flat-buffer layout of a config without the layer is what it was
    from cloud_server_amd.models.cnn import build_model
    ma, mb = build_model(a), build_model(b)
    assert list(ma.state.offsets.values()) == list(mb.state.offsets.values())
    assert torch.equal(ma.flat, mb.flat)


def test_api_lists_and_accepts_dropout(tmp_path):
    from fastapi.testclient import TestClient
    from cloud_server_amd.api.app import create_app
    from cloud_server_amd.config import Settings
    s = Settings(storage_root=str(tmp_path / "store"), db_path=str(tmp_path / "db.sqlite3"),
                 executor="inline", train_backend="torch")
    with TestClient(create_app(s, executor="inline", ngpu=0, inference_device="cpu")) as c:
        layers = [{"layer": "connect", "hidden": 32}, {"layer": "dropout", "keep_prob": "0.8"}]
        body = {"iter": 5, "learning_rate": 0.1, "ratio": 0.8, "net_config": {"middle_layer": layers}}
        r = c.post("/generation/generate/", json=body)
        assert r.status_code == 200, r.text
        out = r.json()
        assert out["params"] == 784 * 32 + 32 + 32 * 10 + 10
        assert out["layers"][1]["spec"] == {"keep_prob": 0.8, "kind": "dropout"} and out["layers"][1]["out"] == [32]
        layers[1]["keep_prob"] = 1.5
        assert c.post("/generation/generate/", json=body).status_code == 400
        assert "dropout" in c.get("/generation/options/next/", params={"layer": "connect"}).json()["options"]
        assert "dropout" in c.get("/generation/options/next/", params={"layer": "conv"}).json()["options"]


# ---------------------------------------------------------------- 2. RNG
def test_crng_torch_equals_numpy():
    from cloud_server_amd.ops import dropout_ref as D
    j = np.arange(70000)
    jt = torch.from_numpy(j)
    for seed in (0, 1, 12345, 2 ** 63 + 77):
        for layer in (0, 5, 19):
            ds = D.drop_seed(seed, layer)
            with np.errstate(over="ignore"):
                want = int(ops_ref._smix(np.array((seed ^ ((layer + 1) << 32)) & (2 ** 64 - 1), dtype=np.uint64)))
            assert ds == want
            for step in (0, 1, 7, 1000, 2 ** 32 - 1):
                ref = ops_ref.crng(ds, np.uint64(step), j)
                got = D.crng_torch(ds, torch.tensor([step], dtype=torch.int64), jt)
                assert got.dtype == torch.int64
                assert np.array_equal(got.numpy().astype(np.uint64), ref), (seed, layer, step)


def test_threshold_and_scale():
    from cloud_server_amd.ops import dropout_ref as D
    assert D.keep_threshold(0.5) == 1 << 23 and D.keep_threshold(1.0) == 1 << 24
    assert D.keep_threshold(1e-9) == 1
    assert D.keep_scale(0.5) == 2.0 and D.keep_scale(0.75) == float(np.float32(1 / 0.75))
    assert D.keep_mask(D.drop_seed(0, 0), 0, 5, 7, 1.0).all()
    # world-N ranks draw the rows b * N + rank of the one-process mask
    full = D.keep_mask(77, 3, 12, 9, 0.5)
    for rank in range(3):
        assert np.array_equal(D.keep_mask(77, 3, 4, 9, 0.5, world=3, rank=rank), full[rank::3])


# ---------------------------------------------------------------- 3. DigitNet
def _net(layers, seed=0):
    from cloud_server_amd.models.cnn import build_model
    m = build_model(_cfg(layers, seed=seed))
    m.train()
    return m


def test_digitnet_applies_the_numpy_mask():
    from cloud_server_amd.ops import dropout_ref as D
    m = _net([{"layer": "connect", "hidden": 512}, {"layer": "dropout", "keep_prob": 0.5}])
    fc, drop = m.plan.layers
    x = torch.rand(50, 784, generator=torch.Generator().manual_seed(1))
    h = m._layer(fc, x, True).detach()
    y = m._layer(drop, h, True)
    mask = torch.from_numpy(D.keep_mask(D.drop_seed(0, drop.index), 0, 50, 512, 0.5))
    assert torch.equal(y, h * mask.float() * 2.0)
    # the whole forward: logits of the masked hidden tensor
    assert torch.equal(m(x), y @ m.p("head.weight") + m.p("head.bias"))
    # autograd: dx = dy * mask * s
    hg = h.clone().requires_grad_(True)
    dy = torch.randn(50, 512, generator=torch.Generator().manual_seed(2))
    m._layer(drop, hg, True).backward(dy)
    assert torch.equal(hg.grad, dy * mask.float() * 2.0)
    # eval mode: the identity
    m.eval()
    assert m._layer(drop, h, False) is h
    assert torch.equal(m(x), h @ m.p("head.weight") + m.p("head.bias"))


def test_masks_differ_between_steps_and_layers():
    m = _net([{"layer": "connect", "hidden": 512}, {"layer": "dropout"}, {"layer": "dropout"}])
    _, d1, d2 = m.plan.layers
    ones = torch.ones(50, 512)
    k1s0 = m._layer(d1, ones, True) != 0
    k2s0 = m._layer(d2, ones, True) != 0
    m.drop_step = torch.ones(1, dtype=torch.int64)
    k1s1 = m._layer(d1, ones, True) != 0
    for a, b in ((k1s0, k1s1), (k1s0, k2s0)):
        frac = (a != b).float().mean().item()
        assert 0.4 <= frac <= 0.6, frac


@pytest.mark.parametrize("keep_prob", [0.25, 0.5, 0.8])
@pytest.mark.parametrize("B,F", [(50, 512), (7, 507), (50, 64)])      # n = 25600, 3549, 3200
def test_kept_fraction_within_six_sigma(keep_prob, B, F):
    from cloud_server_amd.ops import dropout_ref as D
    n = B * F
    sigma = (keep_prob * (1 - keep_prob) / n) ** 0.5
    for seed in (0, 3):
        for layer in (0, 3, 7):
            for step in (0, 5):
                ds = D.drop_seed(seed, layer)
                ref = D.keep_mask(ds, step, B, F, keep_prob)
                got = D.keep_mask_torch(ds, torch.tensor([step]), B, F, keep_prob)
                assert np.array_equal(got.numpy(), ref)
                assert abs(ref.mean() - keep_prob) <= 6 * sigma, (seed, layer, step, ref.mean())


# ---------------------------------------------------------------- 4. CPU TrainEngine
DROP_JOB = {"iter": 6, "learning_rate": 0.05, "ratio": 0.8, "loss_name": "entropy",
            "optimizer_name": "AdamOptimizer",
            "options": {"log_every": 3, "ckpt_every": 3, "batch_size": 16},
            "net_config": {"middle_layer": [{"layer": "conv", "filter": [3, 3, 4]},
                                            {"layer": "active", "active_func": "relu"},
                                            {"layer": "pool"},
                                            {"layer": "dropout", "keep_prob": 0.75},
                                            {"layer": "connect", "hidden": 16},
                                            {"layer": "active", "active_func": "relu"},
                                            {"layer": "dropout"}]}}


def test_resume_with_dropout_is_exact(tmp_path):
    """Checkpoint at step 3, resume, run to step 6: bitwise the 6 straight steps (the mask
    depends on the checkpointed step counter alone), and two runs from one seed are equal."""
    from cloud_server_amd.runtime import checkpoint as ckpt
    from cloud_server_amd.runtime.trainer import run_job
    data = synthetic_mnist(400, seed=0).split(0.8)
    dirs = [str(tmp_path / n) for n in "abc"]
    for d in dirs:
        os.makedirs(d)
    a, b, c = dirs
    run_job(a, dict(DROP_JOB), device="cpu", backend="torch", data=data)
    run_job(b, dict(DROP_JOB, iter=3), device="cpu", backend="torch", data=data)
    assert ckpt.latest(b)[0] == 3
    run_job(b, dict(DROP_JOB), device="cpu", backend="torch", data=data)
    run_job(c, dict(DROP_JOB), device="cpu", backend="torch", data=data)
    o = [ckpt.load(ckpt.latest(d)[1]) for d in dirs]
    assert [x["host_step"] for x in o] == [6, 6, 6]
    for other in o[1:]:
        for k in o[0]["model"]:
            assert torch.equal(o[0]["model"][k], other["model"][k]), k
        assert torch.equal(o[0]["slots"], other["slots"])


def test_engine_hands_the_step_counter_to_the_model():
    """The eager program draws the mask of ``dstep``: dropping changes training, and a run
    whose model keeps drawing step 0's mask differs from the real one after two steps."""
    from cloud_server_amd.runtime.engine import TrainEngine
    cfg = parse_train_config(DROP_JOB)
    ds = synthetic_mnist(200, seed=2)
    eng = TrainEngine(cfg, ds, device="cpu", backend="torch")
    assert eng.model.drop_step is eng.dstep and (eng.model.drop_world, eng.model.drop_rank) == (1, 0)
    frozen = TrainEngine(cfg, ds, device="cpu", backend="torch")
    frozen.model.drop_step = torch.zeros(1, dtype=torch.int64)
    plain = TrainEngine(parse_train_config(dict(DROP_JOB, net_config={"middle_layer": [
        l for l in DROP_JOB["net_config"]["middle_layer"] if l["layer"] != "dropout"]})), ds, device="cpu",
        backend="torch")
    eng.step(); frozen.step(); plain.step()
    assert torch.equal(eng.flat, frozen.flat) and not torch.equal(eng.flat, plain.flat)
    eng.step(); frozen.step()
    assert not torch.equal(eng.flat, frozen.flat)
    # evaluation is dropout-free: the same logits as the model without the layers
    plain.flat.copy_(eng.flat)
    assert eng.evaluate(ds) == plain.evaluate(ds)


# ---------------------------------------------------------------- 5. gloo, world 2
DP_CFG = {"iter": 12, "learning_rate": 0.05, "ratio": 0.8, "loss_name": "entropy",
          "optimizer_name": "AdagradOptimizer",
          "options": {"log_every": 4, "ckpt_every": 4, "batch_size": 8},
          "net_config": {"middle_layer": [{"layer": "conv", "filter": [3, 3, 4], "isBias": "True"},
                                          {"layer": "active", "active_func": "relu"},
                                          {"layer": "pool"},
                                          {"layer": "dropout", "keep_prob": 0.8},
                                          {"layer": "connect", "hidden": 24},
                                          {"layer": "active", "active_func": "sigmoid"},
                                          {"layer": "dropout"}]}}


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _train_dp(rank, world, port, steps, out):
    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from cloud_server_amd.parallel.dist import init_distributed, shutdown
    from cloud_server_amd.runtime.engine import TrainEngine
    ctx = init_distributed("cpu", timeout_s=120)
    eng = TrainEngine(parse_train_config(DP_CFG), synthetic_mnist(256, seed=1), device="cpu", ctx=ctx,
                      strategy="allreduce")
    for _ in range(steps):
        eng.step()
    out[rank] = eng.flat.clone()
    shutdown(ctx)


def test_world2_draws_the_mask_of_one_big_batch():
    from cloud_server_amd.runtime.engine import TrainEngine
    out = mp.Manager().dict()
    mp.spawn(_train_dp, args=(2, _port(), 4, out), nprocs=2, join=True)
    out = dict(out)
    torch.testing.assert_close(out[0], out[1], rtol=0, atol=0)          # replicas identical
    cfg = parse_train_config(dict(DP_CFG, options=dict(DP_CFG["options"], batch_size=16)))
    eng = TrainEngine(cfg, synthetic_mnist(256, seed=1), device="cpu")
    for _ in range(4):
        eng.step()
    n = eng.flat.numel()
    torch.testing.assert_close(out[0][:n], eng.flat, rtol=2e-4, atol=2e-5)
