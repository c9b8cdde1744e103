"""Average and global pooling on the CPU: the DSL (``mode``, ``kernel: "global"``), shape
inference, the eager model against the float64 loop reference (tests/avgpool_ref.py), the
networks against the fp64 oracle at its unchanged tolerances, deterministic mode, the API.

The reference only ever builds ``tf.nn.max_pool`` (construct_distribute.py:121-130); a
``pool`` entry without ``mode`` is that max pool, field for field."""
import copy

import numpy as np
import pytest
import torch

import avgpool_ref as R
import oracle64 as X

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.cnn import build_model
from cloud_server_amd.models.dsl import (SAMPLE_CONFIG, AvgPoolSpec, ConfigError, ConvSpec, LayerPlan, PoolSpec,
                                         TensorShape, parse_layer, parse_train_config, plan_network, same_pads,
                                         spec_to_dict, valid_out)
from cloud_server_amd.runtime.engine import TrainEngine

ALL_GEOMS = R.GEOMETRIES + [R.GRID_STRIDE_FWD, R.GRID_STRIDE_BWD]


def _cfg(layers, **opts):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c["options"] = dict(opts)
    return parse_train_config(c)


# ---------------------------------------------------------------- 1. parsing
def test_parse_mode_and_default():
    assert parse_layer({"layer": "pool"}, 0) == PoolSpec()
    assert type(parse_layer({"layer": "pool"}, 0)) is PoolSpec
    assert parse_layer({"layer": "pool", "mode": "max"}, 0) == PoolSpec()
    assert parse_layer({"layer": "pool", "mode": "max", "kernel": [3, 3], "padding": "valid"}, 0) == \
        PoolSpec((3, 3), (2, 2), "VALID")
    sp = parse_layer({"layer": "pool", "mode": "avg"}, 0)
    assert type(sp) is AvgPoolSpec and not isinstance(sp, PoolSpec)
    assert (sp.kernel, sp.stride, sp.padding) == ((2, 2), (2, 2), "SAME")
    sp = parse_layer({"layer": "pool", "mode": "avg", "kernel": [1, 3], "stride": [2, 4], "padding": "VALID"}, 0)
    assert (sp.kernel, sp.stride, sp.padding) == ((1, 3), (2, 4), "VALID")
    # PoolSpec itself is what it was
    assert [f for f in PoolSpec.__dataclass_fields__] == ["kernel", "stride", "padding", "kind"]
    assert spec_to_dict(PoolSpec()) == {"kernel": (2, 2), "stride": (2, 2), "padding": "SAME", "kind": "pool"}


@pytest.mark.parametrize("bad", ["mean", "AVG", "", None, 1, ["avg"]])
def test_parse_bad_mode(bad):
    with pytest.raises(ConfigError):
        parse_layer({"layer": "pool", "mode": bad}, 0)


def test_parse_numbers_as_strings():
    sp = parse_layer({"layer": "pool", "mode": "avg", "kernel": ["3", "2"], "stride": "2"}, 0)
    assert (sp.kernel, sp.stride) == ((3, 2), (2, 2))
    assert parse_layer({"layer": "pool", "mode": "avg", "kernel": "3"}, 0).kernel == (3, 3)
    with pytest.raises(ConfigError):
        parse_layer({"layer": "pool", "mode": "avg", "kernel": "three"}, 0)
    with pytest.raises(ConfigError):
        parse_layer({"layer": "pool", "mode": "avg", "kernel": [0, 2]}, 0)


@pytest.mark.parametrize("mode,cls", [(None, PoolSpec), ("max", PoolSpec), ("avg", AvgPoolSpec)])
def test_parse_global(mode, cls):
    d = {"layer": "pool", "kernel": "global"}
    if mode is not None:
        d["mode"] = mode
    assert type(parse_layer(d, 0)) is cls
    for extra in ({"stride": [2, 2]}, {"padding": "VALID"}, {"padding": "SAME"}, {"stride": 1, "padding": "SAME"}):
        with pytest.raises(ConfigError):
            parse_layer(dict(d, **extra), 0)
    conv = {"layer": "conv", "filter": [3, 3, 6], "stride": [2, 2]}
    plan = _cfg([conv, d]).plan()
    lp = plan.layers[1]
    # the concrete window: the whole 14 x 14 map, stride = window, VALID, 1 x 1 x C out
    assert type(lp.spec) is cls
    assert (tuple(lp.spec.kernel), tuple(lp.spec.stride), lp.spec.padding) == ((14, 14), (14, 14), "VALID")
    assert lp.pads == (0, 0, 0, 0) and lp.out_shape == TensorShape(6, (1, 1)) and plan.head_in == 6
    want = {"kernel": (14, 14), "stride": (14, 14), "padding": "VALID", "kind": "pool"}
    if cls is AvgPoolSpec:
        want["mode"] = "avg"
    assert spec_to_dict(lp.spec) == want
    with pytest.raises(ConfigError, match="after a connect"):
        _cfg([{"layer": "connect", "hidden": 8}, d])


# ---------------------------------------------------------------- 2. shape inference
def _plans(g):
    """The LayerPlans of a max and an average pool of geometry ``g`` (an H x W x C map made
    from a square input by one VALID conv)."""
    B, H, W, C, kh, kw, sh, sw, pad = g
    side = max(H, W)
    conv = ConvSpec(side - H + 1, side - W + 1, C, padding="VALID")
    out = []
    for cls in (PoolSpec, AvgPoolSpec):
        plan = plan_network([conv, cls((kh, kw), (sh, sw), pad)], in_hw=side)
        assert plan.layers[1].in_shape == TensorShape(C, (H, W))
        out.append(plan)
    return out


@pytest.mark.parametrize("g", ALL_GEOMS, ids=R.geom_id)
def test_shape_inference_is_the_max_pools(g):
    B, H, W, C, kh, kw, sh, sw, pad = g
    pm, pa = _plans(g)
    lm, la = pm.layers[1], pa.layers[1]
    assert type(la.spec) is AvgPoolSpec and type(lm.spec) is PoolSpec
    assert (la.in_shape, la.out_shape, la.pads, la.params) == (lm.in_shape, lm.out_shape, lm.pads, lm.params)
    assert pa.head_in == pm.head_in and pa.num_params() == pm.num_params()
    OH, OW, pt, pl = R.geometry(H, W, kh, kw, sh, sw, pad)
    assert la.out_shape == TensorShape(C, (OH, OW)) and (la.pads[0], la.pads[2]) == (pt, pl)
    if (kh, kw) == (H, W):
        assert la.out_shape.hw == (1, 1) and pa.head_in == C


def test_shape_errors_are_the_max_pools():
    for mode in ("max", "avg"):
        with pytest.raises(ConfigError, match="after a connect"):
            _cfg([{"layer": "connect", "hidden": 8}, {"layer": "pool", "mode": mode}])
        with pytest.raises(ConfigError, match="larger than"):
            _cfg([{"layer": "pool", "mode": mode, "kernel": [29, 29], "padding": "VALID"}])


# ---------------------------------------------------------------- 3. DigitNet against the loop reference
@pytest.fixture(scope="module")
def any_model():
    return build_model(_cfg([{"layer": "connect", "hidden": 8}]))


@pytest.fixture(scope="module")
def references():
    """geometry -> (x, dy, y64, dx64): computed once, shared, never changed."""
    out = {}
    for g in ALL_GEOMS:
        B, H, W, C, kh, kw, sh, sw, pad = g
        rng = np.random.default_rng(H * 1000 + W * 10 + C)
        x = rng.standard_normal((B, H, W, C)).astype(np.float32)
        OH, OW, _, _ = R.geometry(H, W, kh, kw, sh, sw, pad)
        dy = rng.standard_normal((B, OH, OW, C)).astype(np.float32)
        out[g] = (x, dy, R.avg_fwd(x, kh, kw, sh, sw, pad), R.avg_bwd(dy, H, W, kh, kw, sh, sw, pad))
    return out


def _layer_plan(g):
    B, H, W, C, kh, kw, sh, sw, pad = g
    if pad == "SAME":
        (oh, pt, pb), (ow, pl, pr) = same_pads(H, kh, sh), same_pads(W, kw, sw)
    else:
        oh, ow, pt, pb, pl, pr = valid_out(H, kh, sh), valid_out(W, kw, sw), 0, 0, 0, 0
    return LayerPlan(0, AvgPoolSpec((kh, kw), (sh, sw), pad), TensorShape(C, (H, W)), TensorShape(C, (oh, ow)),
                     (pt, pb, pl, pr))


@pytest.mark.parametrize("det", [False, True], ids=["pool2d", "gather"])
@pytest.mark.parametrize("g", ALL_GEOMS, ids=R.geom_id)
def test_digitnet_matches_loop_reference(g, det, any_model, references):
    B, H, W, C, kh, kw, sh, sw, pad = g
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
        assert ey <= 1e-12 and ex <= 1e-12
        if g == R.GAPPED:
            hole = ~R.covered(H, W, kh, kw, sh, sw, pad)
            assert hole.any() and (dx.numpy()[:, hole, :] == 0).all()
        # fp32: n - 1 adds and one division
        y32 = any_model._layer(lp, torch.from_numpy(x), True)
        assert y32.dtype == torch.float32
        bound = R.fwd_bound(min(kh, H) * min(kw, W), float(np.abs(x).max()))
        e32 = np.abs(y32.numpy().astype(np.float64) - y64).max()
        print(f"  fp32 forward {e32:.2e} <= {bound:.2e}")
        assert e32 <= bound
    finally:
        any_model.deterministic = False


# ---------------------------------------------------------------- 4. the networks against the oracle
@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


@pytest.mark.parametrize("name", list(R.NETS))
def test_networks_match_fp64_oracle_cpu(name, dataset):
    opt = "AdagradOptimizer"
    cfg = X.make_cfg(R.layers_of(name), opt, X.LRS[opt])
    kinds = [type(lp.spec) for lp in cfg.plan().layers]
    assert AvgPoolSpec in kinds
    eng = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    recs = X.run_trajectory(eng, X.Oracle64(cfg, dataset), 3)
    X.check(recs, X.tolerances(name, X.LRS[opt]), f"{name}-cpu")


def test_networks_have_the_shapes_they_are_named_for():
    p = _cfg(R.layers_of("gap_head")).plan()
    assert p.head_in == 12 and p.layers[-1].out_shape == TensorShape(12, (1, 1))
    assert tuple(p.layers[-1].spec.kernel) == (14, 14)
    p = _cfg(R.layers_of("lenet_avg")).plan()
    assert [lp.out_shape.hw for lp in p.layers[:6]] == [(28, 28)] * 2 + [(14, 14)] + [(10, 10)] * 2 + [(5, 5)]
    p = _cfg(R.layers_of("avg_first")).plan()
    assert type(p.layers[0].spec) is AvgPoolSpec and p.layers[0].in_shape == TensorShape(1, (28, 28))
    # the sample with mode: avg has the sample's shapes and parameters
    a, b = _cfg(R.layers_of("sample_avg")).plan(), _cfg(SAMPLE_CONFIG["net_config"]["middle_layer"]).plan()
    assert a.param_shapes() == b.param_shapes() and type(a.layers[2].spec) is AvgPoolSpec
    assert type(b.layers[2].spec) is PoolSpec


def test_average_pool_is_not_a_max_pool():
    """``mode: avg`` trains something else than the max pool it used to fall back to."""
    ds = synthetic_mnist(100, seed=1)
    outs = []
    for layers in (R.layers_of("sample_avg"), SAMPLE_CONFIG["net_config"]["middle_layer"]):
        eng = TrainEngine(_cfg(layers, batch_size=16), ds, device="cpu", backend="torch")
        eng.step()
        outs.append(eng.flat.clone())
    assert not torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- 5. deterministic eager program
def test_deterministic_eager_program(monkeypatch):
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    try:
        runs = []
        for _ in range(2):
            # an overlapping SAME pool and a global one
            cfg = X.make_cfg(R.layers_of("avg_overlap_same")[:3] + [dict(R.AVG, kernel="global")], batch=16)
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
def test_api_average_pool(tmp_path):
    from fastapi.testclient import TestClient
    from cloud_server_amd.api.app import create_app
    from cloud_server_amd.config import Settings
    s = Settings(storage_root=str(tmp_path / "store"), db_path=str(tmp_path / "db.sqlite3"),
                 executor="inline", train_backend="torch")
    with TestClient(create_app(s, executor="inline", ngpu=0, inference_device="cpu")) as c:
        layers = [{"layer": "conv", "filter": [3, 3, 6], "stride": [2, 2]},
                  {"layer": "pool", "mode": "avg", "kernel": "3", "stride": ["2", "2"]},
                  {"layer": "pool", "mode": "avg", "kernel": "global"}]
        body = {"iter": 5, "learning_rate": 0.1, "ratio": 0.8, "net_config": {"middle_layer": layers}}
        r = c.post("/generation/generate/", json=body)
        assert r.status_code == 200, r.text
        out = r.json()
        assert out["layers"][1]["spec"] == {"kernel": [3, 3], "stride": [2, 2], "padding": "SAME", "kind": "pool",
                                            "mode": "avg"}
        assert out["layers"][1]["out"] == [6, 7, 7]
        assert out["layers"][2]["spec"] == {"kernel": [7, 7], "stride": [7, 7], "padding": "VALID", "kind": "pool",
                                            "mode": "avg"}
        assert out["layers"][2]["out"] == [6, 1, 1]
        assert out["params"] == 3 * 3 * 6 + 6 * 10 + 10
        for bad in ({"mode": "median"}, {"kernel": "global", "stride": [1, 1]}, {"kernel": "global", "padding": "SAME"}):
            layers[2] = dict({"layer": "pool", "mode": "avg"}, **bad)
            r = c.post("/generation/generate/", json=body)
            assert r.status_code == 400, (bad, r.text)
        o = c.post("/construct/options/", json={"option": "pooling_method"})
        assert o.status_code == 200, o.text
        assert o.json()["options"] == ["Max", "Average"] and o.json()["default"] == "Max"
        assert o.json()["tokens"] == {"Max": "max", "Average": "avg"}
        assert c.get("/generation/options/list/").json()["pooling_method"]["options"] == ["Max", "Average"]
