"""Local response normalisation on the CPU: the DSL entry ``{"layer": "lrn"}``, shape
inference, the eager model against the float64 loop reference (tests/lrn_ref.py), the networks
against the fp64 oracle at its unchanged tolerances, deterministic mode, the API.

The reference has no ``tf.nn.lrn``; before this layer the entry was an unknown name and was
silently skipped, so a config with it planned (and trained) the network without it."""
import copy

import numpy as np
import pytest
import torch

import lrn_ref as R
import oracle64 as X

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.cnn import build_model
from cloud_server_amd.models.dsl import (SAMPLE_CONFIG, ConfigError, LayerPlan, LrnSpec, TensorShape, parse_layer,
                                         parse_train_config, spec_to_dict)
from cloud_server_amd.runtime.engine import TrainEngine

ALL_GEOMS = R.GEOMETRIES + R.GRID_STRIDE


def _cfg(layers, **opts):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c["options"] = dict(opts)
    return parse_train_config(c)


# ---------------------------------------------------------------- 1. parsing
def test_parse_defaults_are_tensorflows():
    sp = parse_layer({"layer": "lrn"}, 0)
    assert type(sp) is LrnSpec
    assert (sp.depth_radius, sp.bias, sp.alpha, sp.beta, sp.kind) == (5, 1.0, 1.0, 0.5, "lrn")
    assert sp == LrnSpec()
    assert spec_to_dict(sp) == {"depth_radius": 5, "bias": 1.0, "alpha": 1.0, "beta": 0.5, "kind": "lrn"}
    sp = parse_layer({"layer": "lrn", "depth_radius": 4, "bias": 2, "alpha": 0.001 / 9, "beta": 0.75}, 3)
    assert sp == LrnSpec(4, 2.0, 0.001 / 9, 0.75)
    assert parse_layer({"layer": "lrn", "depth_radius": 0, "alpha": 0}, 0) == LrnSpec(0, 1.0, 0.0, 0.5)
    assert parse_layer({"layer": "lrn", "depth_radius": 2 ** 15 - 1}, 0).depth_radius == 2 ** 15 - 1


def test_parse_numbers_as_strings():
    sp = parse_layer({"layer": "lrn", "depth_radius": "3", "bias": "2.0", "alpha": "1e-4", "beta": "0.75"}, 0)
    assert sp == LrnSpec(3, 2.0, 1e-4, 0.75)
    assert type(sp.depth_radius) is int
    assert parse_layer({"layer": "lrn", "depth_radius": 3.0}, 0).depth_radius == 3


@pytest.mark.parametrize("bad", [
    {"depth_radius": -1}, {"depth_radius": 2 ** 15}, {"depth_radius": 2.5}, {"depth_radius": "2.5"},
    {"depth_radius": "two"}, {"depth_radius": True}, {"depth_radius": None}, {"depth_radius": float("nan")},
    {"depth_radius": float("inf")}, {"depth_radius": [2]},
    {"bias": 0}, {"bias": -1.0}, {"bias": float("inf")}, {"bias": float("nan")}, {"bias": "k"}, {"bias": None},
    {"bias": True},
    {"alpha": -1e-9}, {"alpha": float("inf")}, {"alpha": float("nan")}, {"alpha": "a"}, {"alpha": [1.0]},
    {"beta": 0}, {"beta": -0.5}, {"beta": float("inf")}, {"beta": float("nan")}, {"beta": "b"}, {"beta": False},
], ids=lambda d: "{}={!r}".format(*next(iter(d.items()))))
def test_parse_refusals(bad):
    with pytest.raises(ConfigError):
        parse_layer(dict({"layer": "lrn"}, **bad), 0)
    with pytest.raises(ConfigError):
        _cfg([{"layer": "conv", "filter": [3, 3, 4]}, dict({"layer": "lrn"}, **bad)])


# ---------------------------------------------------------------- 2. shape inference
def test_shape_preserving_and_without_parameters():
    conv = {"layer": "conv", "filter": [3, 3, 6], "stride": [2, 2]}
    plan = _cfg([conv, {"layer": "lrn", "depth_radius": 9}]).plan()
    lp = plan.layers[1]
    assert type(lp.spec) is LrnSpec and lp.in_shape == lp.out_shape == TensorShape(6, (14, 14))
    assert lp.params == {} and lp.pads == (0, 0, 0, 0) and plan.head_in == 6 * 14 * 14
    assert plan.num_params() == _cfg([conv]).plan().num_params()
    assert plan.flops_per_sample() == _cfg([conv]).plan().flops_per_sample()
    # first layer: the 28 x 28 x 1 input
    p = _cfg([{"layer": "lrn"}, conv]).plan()
    assert p.layers[0].in_shape == p.layers[0].out_shape == TensorShape(1, (28, 28))


def test_after_connect_is_an_error():
    for front in ([{"layer": "connect", "hidden": 8}],
                  [{"layer": "conv", "filter": [3, 3, 4]}, {"layer": "connect", "hidden": 8}, {"layer": "active"}]):
        with pytest.raises(ConfigError, match="lrn after a connect"):
            _cfg(front + [{"layer": "lrn"}])


def test_an_lrn_entry_plans_one_more_layer():
    """The old silent skip: the entry was an unknown name and the job trained the network
    without it."""
    for name in R.NETS:
        layers = R.layers_of(name)
        n_lrn = sum(d["layer"] == "lrn" for d in layers)
        with_, without = _cfg(layers), _cfg(R.without_lrn(layers))
        assert n_lrn >= 1 and len(with_.plan().layers) == len(without.plan().layers) + n_lrn
        assert sum(type(sp) is LrnSpec for sp in with_.layers) == n_lrn
        # (the names carry the layer index; the shapes, in order, are the same)
        assert list(with_.plan().param_shapes().values()) == list(without.plan().param_shapes().values())
    assert len(_cfg(R.layers_of("lrn_sample")).plan().layers) == \
        len(_cfg(SAMPLE_CONFIG["net_config"]["middle_layer"]).plan().layers) + 1


def test_lrn_trains_another_network_than_the_one_without_it():
    ds = synthetic_mnist(100, seed=1)
    outs = []
    for layers in (R.layers_of("lrn_sample"), SAMPLE_CONFIG["net_config"]["middle_layer"]):
        eng = TrainEngine(_cfg(layers, batch_size=16), ds, device="cpu", backend="torch")
        eng.step()
        outs.append(eng.flat.clone())
    assert not torch.equal(outs[0], outs[1])


def test_networks_have_the_shapes_they_are_named_for():
    p = _cfg(R.layers_of("lrn_allchan_head")).plan()
    assert type(p.layers[-1].spec) is LrnSpec and p.layers[-1].out_shape == TensorShape(7, (7, 7))
    assert p.head_in == 7 * 7 * 7 and p.layers[-1].spec.depth_radius >= 7
    p = _cfg(R.layers_of("lrn_wide160")).plan()
    assert p.layers[3].in_shape == TensorShape(160, (7, 7)) and p.head_in == 16
    p = _cfg(R.layers_of("lrn_first")).plan()
    assert type(p.layers[0].spec) is LrnSpec and p.layers[0].in_shape == TensorShape(1, (28, 28))
    p = _cfg(R.layers_of("lrn_cifar")).plan()
    assert [lp.out_shape.hw for lp in p.layers[:8]] == [(28, 28)] * 2 + [(14, 14)] * 5 + [(7, 7)]
    assert [lp.out_shape.c for lp in p.layers[:8]] == [8] * 4 + [16] * 4


# ---------------------------------------------------------------- 3. DigitNet against the loop reference
@pytest.fixture(scope="module")
def any_model():
    return build_model(_cfg([{"layer": "connect", "hidden": 8}]))


@pytest.fixture(scope="module")
def references():
    """geometry -> (x, dy, y64, dx64): computed once, shared, never changed."""
    out = {}
    for g in ALL_GEOMS:
        B, H, W, C, r, k, alpha, beta = g
        x, dy = R.inputs(g)
        out[g] = (x, dy, R.lrn_fwd(x, r, k, alpha, beta), R.lrn_bwd(x, dy, r, k, alpha, beta))
    return out


def _layer_plan(g):
    B, H, W, C, r, k, alpha, beta = g
    return LayerPlan(0, LrnSpec(r, k, alpha, beta), TensorShape(C, (H, W)), TensorShape(C, (H, W)))


@pytest.mark.parametrize("det", [False, True], ids=["normal", "deterministic"])
@pytest.mark.parametrize("g", ALL_GEOMS, ids=R.geom_id)
def test_digitnet_matches_loop_reference(g, det, any_model, references):
    x, dy, y64, dx64 = references[g]
    lp = _layer_plan(g)
    any_model.deterministic = det
    try:
        xt = torch.from_numpy(x).double().requires_grad_(True)
        y = any_model._layer(lp, xt, True)
        assert y.dtype == torch.float64 and tuple(y.shape) == y64.shape
        (dx,) = torch.autograd.grad(y, xt, torch.from_numpy(dy).double())
        ey = np.abs(y.detach().numpy() - y64).max() / np.abs(y64).max()
        ex = np.abs(dx.numpy() - dx64).max() / np.abs(dx64).max()
        print(f"{R.geom_id(g)} det={det}: fp64 forward {ey:.2e}, backward {ex:.2e}")
        assert ey <= 1e-14 and ex <= 1e-13
        # fp32: e32 is the yardstick of the kernels' bound (tests/test_gpu_lrn.py); here it only
        # has to be an fp32 rounding error (the issue measured 0.5-1.1e-7 of the maximum)
        x32 = torch.from_numpy(x).requires_grad_(True)
        y32 = any_model._layer(lp, x32, True)
        assert y32.dtype == torch.float32
        (dx32,) = torch.autograd.grad(y32, x32, torch.from_numpy(dy))
        e32y = np.abs(y32.detach().numpy().astype(np.float64) - y64).max() / np.abs(y64).max()
        e32x = np.abs(dx32.numpy().astype(np.float64) - dx64).max() / np.abs(dx64).max()
        print(f"  fp32 forward {e32y:.2e}, backward {e32x:.2e} of the maximum")
        assert e32y <= 16 * R.U and e32x <= 16 * R.U
    finally:
        any_model.deterministic = False


def test_normal_and_deterministic_mode_are_one_form(any_model, references):
    g = R.GEOMETRIES[3]
    x = torch.from_numpy(references[g][0])
    outs = []
    for det in (False, True):
        any_model.deterministic = det
        outs.append(any_model._layer(_layer_plan(g), x, True))
    any_model.deterministic = False
    assert torch.equal(outs[0], outs[1])


def test_alpha_is_not_divided_by_the_window():
    """``F.local_response_norm`` divides alpha by the window size and counts padded taps: with
    alpha * (2 r + 1) it is the layer, edges included."""
    g = R.GEOMETRIES[3]
    B, H, W, C, r, k, alpha, beta = g
    x = torch.from_numpy(R.inputs(g)[0]).double()
    want = torch.nn.functional.local_response_norm(x.permute(0, 3, 1, 2), 2 * r + 1, alpha * (2 * r + 1), beta, k)
    got = torch.from_numpy(R.lrn_fwd(x.numpy(), r, k, alpha, beta))
    assert (want.permute(0, 2, 3, 1) - got).abs().max().item() <= 1e-14


# ---------------------------------------------------------------- 4. the networks against the oracle
@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


@pytest.mark.parametrize("batch", [50, 7])
@pytest.mark.parametrize("name", list(R.NETS))
def test_networks_match_fp64_oracle_cpu(name, batch, dataset):
    opt = "AdagradOptimizer"
    cfg = X.make_cfg(R.layers_of(name), opt, X.LRS[opt], "entropy", batch)
    assert LrnSpec in [type(lp.spec) for lp in cfg.plan().layers]
    eng = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    recs = X.run_trajectory(eng, X.Oracle64(cfg, dataset), 3)
    X.check(recs, X.tolerances(name, X.LRS[opt]), f"{name}-b{batch}-cpu")


# ---------------------------------------------------------------- 5. deterministic eager program
def test_deterministic_eager_program(monkeypatch):
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    try:
        runs = []
        for _ in range(2):
            cfg = X.make_cfg(R.layers_of("lrn_cifar"), batch=16)
            eng = TrainEngine(cfg, synthetic_mnist(200, seed=1), device="cpu")
            assert eng.deterministic and eng.backend == "torch" and eng.model.deterministic
            assert torch.are_deterministic_algorithms_enabled()
            for _ in range(3):
                eng.step()                   # (raises if an op has no deterministic form)
            runs.append((eng.flat.clone(), eng.slots.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    finally:
        torch.use_deterministic_algorithms(False)


# ---------------------------------------------------------------- 6. API
def test_api_lrn(tmp_path):
    from fastapi.testclient import TestClient
    from cloud_server_amd.api.app import create_app
    from cloud_server_amd.config import Settings
    s = Settings(storage_root=str(tmp_path / "store"), db_path=str(tmp_path / "db.sqlite3"),
                 executor="inline", train_backend="torch")
    with TestClient(create_app(s, executor="inline", ngpu=0, inference_device="cpu")) as c:
        layers = [{"layer": "conv", "filter": [3, 3, 6], "stride": [2, 2]},
                  {"layer": "lrn", "depth_radius": "4", "alpha": "0.5", "beta": 0.75},
                  {"layer": "lrn"}]
        body = {"iter": 5, "learning_rate": 0.1, "ratio": 0.8, "net_config": {"middle_layer": layers}}
        r = c.post("/generation/generate/", json=body)
        assert r.status_code == 200, r.text
        out = r.json()
        assert len(out["layers"]) == 3
        assert out["layers"][1]["spec"] == {"depth_radius": 4, "bias": 1.0, "alpha": 0.5, "beta": 0.75, "kind": "lrn"}
        assert out["layers"][2]["spec"] == {"depth_radius": 5, "bias": 1.0, "alpha": 1.0, "beta": 0.5, "kind": "lrn"}
        assert out["layers"][1]["out"] == out["layers"][2]["out"] == [6, 14, 14]
        assert out["params"] == 3 * 3 * 6 + 6 * 14 * 14 * 10 + 10
        for bad in ({"depth_radius": -1}, {"depth_radius": 1.5}, {"bias": 0}, {"alpha": -1}, {"beta": 0},
                    {"beta": "x"}, {"depth_radius": 40000}):
            layers[2] = dict({"layer": "lrn"}, **bad)
            r = c.post("/generation/generate/", json=body)
            assert r.status_code == 400, (bad, r.text)
        layers[2] = {"layer": "lrn"}
        layers.insert(2, {"layer": "connect", "hidden": 8})
        assert c.post("/generation/generate/", json=body).status_code == 400
        for prev in ("conv", "pool", "norm", "active", "lrn", ""):
            assert "lrn" in c.get("/generation/options/next/", params={"layer": prev}).json()["options"]
        assert "lrn" not in c.get("/generation/options/next/", params={"layer": "connect"}).json()["options"]
