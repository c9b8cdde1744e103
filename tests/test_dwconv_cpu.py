"""Depthwise convolution on the CPU: the ``depthwise`` entry, shape inference, the initialisers,
the eager model against the float64 loop reference (tests/dwconv_ref.py), the networks against
the fp64 oracle at its unchanged tolerances, resume, the API.

Before this layer ``{"layer": "depthwise"}`` was an unknown layer name: ``parse_layer`` returned
None, the entry was skipped and the job trained another network than the one written."""
import copy
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dwconv_ref as R
import oracle64 as X

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.cnn import build_model
from cloud_server_amd.models.dsl import (SAMPLE_CONFIG, ConfigError, ConvSpec, DepthwiseConvSpec, TensorShape,
                                         parse_layer, parse_train_config, plan_network, same_pads, spec_to_dict,
                                         valid_out)
from cloud_server_amd.models.options import get_options
from cloud_server_amd.runtime.engine import TrainEngine

ALL_GEOMS = R.GEOMETRIES + R.ROW_CAP
CONV = {"layer": "conv", "filter": [3, 3, 8]}


def _cfg(layers, **opts):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c["options"] = dict(opts)
    return parse_train_config(c)


# ---------------------------------------------------------------- 1. parsing
def test_entry_parses_to_a_depthwise_spec():
    """The test that fails without the feature: the entry parsed to nothing."""
    sp = parse_layer({"layer": "depthwise", "filter": [3, 3, 2]}, 0)
    assert type(sp) is DepthwiseConvSpec and not isinstance(sp, ConvSpec)
    assert sp == DepthwiseConvSpec(3, 3, 2, (1, 1), "SAME", "norm", False, 0.1, 0.1) and sp.kind == "depthwise"
    sp = parse_layer({"layer": "depthwise", "filter": [5, 3, 1], "stride": [2, 1], "padding": "valid", "init": "xavier",
                      "stddev_norm": 0.5, "isBias": "True", "bias_constant": 0.25}, 3)
    assert sp == DepthwiseConvSpec(5, 3, 1, (2, 1), "VALID", "xavier", True, 0.25, 0.5)
    assert len(_cfg([{"layer": "depthwise", "filter": [3, 3, 1]}]).layers) == 1


def test_parse_numbers_as_strings_and_conv_quirks():
    sp = parse_layer({"layer": "depthwise", "filter": ["3", "2", "4"], "stride": ["2", "1"], "stddev_norm": "0.2",
                      "bias_constant": "0.3", "isBias": "yes"}, 0)
    assert sp == DepthwiseConvSpec(3, 2, 4, (2, 1), "SAME", "norm", True, 0.3, 0.2)
    assert all(type(v) is int for v in (sp.kh, sp.kw, sp.mult) + tuple(sp.stride))
    assert parse_layer({"layer": "depthwise", "filter": [3, 3, 1], "stride": 2}, 0).stride == (2, 2)
    # the reference's string compare: only "False" (and a JSON false) switch the bias off
    for v, want in (("False", False), (False, False), ("false", True), ("True", True), (True, True), (0, True)):
        assert parse_layer({"layer": "depthwise", "filter": [3, 3, 1], "isBias": v}, 0).bias is want, v
    # key for key what a conv entry parses to
    d = {"filter": [3, 3, 2], "stride": [2, 2], "padding": "VALID", "init": "zero", "isBias": "x", "bias_constant": 1}
    a, b = parse_layer(dict(d, layer="depthwise"), 0), parse_layer(dict(d, layer="conv"), 0)
    assert (a.kh, a.kw, a.mult, a.stride, a.padding, a.init, a.bias, a.bias_constant, a.stddev) == \
        (b.kh, b.kw, b.cout, b.stride, b.padding, b.init, b.bias, b.bias_constant, b.stddev)


BAD = [
    {}, {"filter": [3, 3]}, {"filter": 3}, {"filter": [3, 3, 1, 1]}, {"filter": "3x3"}, {"filter": [3, "a", 1]},
    {"filter": [0, 3, 1]}, {"filter": [3, -1, 1]}, {"filter": [3, 3, 0]}, {"filter": [3, 3, -2]},
    {"filter": [3, 3, 1], "stride": [0, 1]}, {"filter": [3, 3, 1], "stride": [1, -1]}, {"filter": [3, 3, 1], "stride": "a"},
    {"filter": [3, 3, 1], "padding": "FULL"}, {"filter": [3, 3, 1], "init": "he"},
    {"filter": [3, 3, 1], "stddev_norm": "wide"},
]


@pytest.mark.parametrize("bad", BAD, ids=[str(b)[:40] for b in BAD])
def test_parse_refusals_name_the_layer(bad):
    with pytest.raises(ConfigError) as e:
        parse_layer(dict({"layer": "depthwise"}, **bad), 4)
    assert "middle_layer[4]" in str(e.value)
    if "stride\": \"a" not in str(bad) and "stddev" not in str(bad) and "'a'" not in str(bad):
        assert "depthwise" in str(e.value)


def test_plan_time_refusals_name_the_layer():
    with pytest.raises(ConfigError, match=r"layer 1: depthwise after a connect"):
        _cfg([{"layer": "connect", "hidden": 8}, {"layer": "depthwise", "filter": [3, 3, 1]}])
    with pytest.raises(ConfigError, match=r"layer 1: depthwise kernel larger than its 7x7 input"):
        _cfg([{"layer": "pool", "kernel": [4, 4], "stride": [4, 4]},
              {"layer": "depthwise", "filter": [8, 3, 1], "padding": "VALID"}])
    # the same kernel under SAME is fine: larger than the map
    assert _cfg([{"layer": "pool", "kernel": [4, 4], "stride": [4, 4]},
                 {"layer": "depthwise", "filter": [8, 3, 1]}]).plan().layers[1].out_shape == TensorShape(1, (7, 7))


# ---------------------------------------------------------------- 2. shapes, parameters, flops, the catalogue
@pytest.mark.parametrize("g", ALL_GEOMS, ids=R.geom_id)
def test_plan_shapes_pads_and_parameters(g):
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    lp = R.layer_plan(g, R.has_bias(g))
    # the hand-written plan of the reference module is what ConvSpec's arithmetic gives
    if pad == "SAME":
        (oh, pt, pb), (ow, pl, pr) = same_pads(H, kh, sh), same_pads(W, kw, sw)
    else:
        oh, ow, pt, pb, pl, pr = valid_out(H, kh, sh), valid_out(W, kw, sw), 0, 0, 0, 0
    assert lp.out_shape == TensorShape(C * M, (oh, ow)) and lp.pads == (pt, pb, pl, pr)
    if H == W:
        # plan_network on a square map of the same size: the same plan, and a dense conv's pads
        sp = lp.spec
        p = plan_network([sp], in_hw=H, in_c=C).layers[0]
        assert (p.in_shape, p.out_shape, p.pads, p.params) == (lp.in_shape, lp.out_shape, lp.pads, lp.params)
        cv = plan_network([ConvSpec(kh, kw, C * M, (sh, sw), pad)], in_hw=H, in_c=C).layers[0]
        assert (cv.out_shape, cv.pads) == (p.out_shape, p.pads)
        assert p.params["weight"] == (kh, kw, C, M) and p.params.get("bias") == ((C * M,) if sp.bias else None)


def test_param_shapes_flops_and_order():
    layers = [CONV, {"layer": "depthwise", "filter": [5, 3, 2], "stride": [2, 2], "isBias": "True"},
              {"layer": "conv", "filter": [1, 1, 4]}]
    plan = _cfg(layers).plan()
    lp = plan.layers[1]
    assert lp.in_shape == TensorShape(8, (28, 28)) and lp.out_shape == TensorShape(16, (14, 14))
    shapes = plan.param_shapes()
    assert list(shapes)[:4] == ["layers.0.weight", "layers.1.weight", "layers.1.bias", "layers.2.weight"]
    assert shapes["layers.1.weight"] == (5, 3, 8, 2) and shapes["layers.1.bias"] == (16,)
    assert shapes["layers.2.weight"] == (1, 1, 16, 4)
    without = _cfg([CONV, {"layer": "conv", "filter": [1, 1, 4], "stride": [2, 2]}]).plan()
    own = 2 * 14 * 14 * 16 * 5 * 3
    assert plan.flops_per_sample() - own == (without.flops_per_sample() - 2 * 14 * 14 * 4 * 8) + 2 * 14 * 14 * 4 * 16
    assert own == 2 * lp.out_shape.hw[0] * lp.out_shape.hw[1] * 8 * 2 * 5 * 3
    assert plan.num_params() == 3 * 3 * 8 + 5 * 3 * 8 * 2 + 16 + 16 * 4 + 14 * 14 * 4 * 10 + 10


def test_catalogue_entry():
    o = get_options("convolution_method")
    assert o["options"] == ["Standard", "Depthwise"] and o["default"] == "Standard"
    assert o["tokens"] == {"Standard": "conv", "Depthwise": "depthwise"}


def test_networks_have_the_shapes_they_are_named_for():
    p = _cfg(R.layers_of("dw_separable")).plan()
    assert type(p.layers[1].spec) is DepthwiseConvSpec and p.layers[1].out_shape == TensorShape(10, (28, 28))
    assert p.layers[2].out_shape == TensorShape(20, (28, 28)) and p.head_in == 512
    p = _cfg(R.layers_of("dw_first")).plan()
    assert p.layers[0].in_shape == TensorShape(1, (28, 28)) and p.layers[0].out_shape == TensorShape(2, (28, 28))
    p = _cfg(R.layers_of("dw_head")).plan()
    assert p.layers[3].out_shape == TensorShape(8, (3, 3)) and p.head_in == 72
    p = _cfg(R.layers_of("dw_leaky_neg")).plan()
    assert p.layers[2].spec.alpha == -0.1
    for name in R.NETS:
        assert DepthwiseConvSpec in [type(lp.spec) for lp in _cfg(R.layers_of(name)).plan().layers], name


# ---------------------------------------------------------------- 3. the initialisers
def _init(entry, seed=0):
    m = build_model(_cfg([{"layer": "conv", "filter": [2, 2, 6]}, entry, {"layer": "connect", "hidden": 8}], seed=seed))
    return m


def test_init_params_three_initialisers():
    base = {"layer": "depthwise", "filter": [3, 5, 2], "isBias": "True", "bias_constant": 0.25}
    z = _init(dict(base, init="zero"))
    assert z.p("layers.1.weight").shape == (3, 5, 6, 2) and not z.p("layers.1.weight").any()
    assert torch.equal(z.p("layers.1.bias"), torch.full((12,), 0.25))
    n = _init(dict(base, init="norm", stddev_norm=0.3)).p("layers.1.weight")
    x = _init(dict(base, init="xavier", stddev_norm=0.3)).p("layers.1.weight")
    # truncated normal at two sigma; xavier keeps the reference's formula on this shape:
    # sigma / (kw * C * M), so the same draws scaled
    assert 0.15 < n.std().item() < 0.35 and n.abs().max().item() <= 2 * 0.3 + 1e-6
    sx = 0.3 / (5 * 6 * 2)
    assert x.abs().max().item() <= 2 * sx + 1e-9
    torch.testing.assert_close(x, n * (sx / 0.3), rtol=1e-5, atol=0)
    # the same shape as a conv weight draws the same numbers, in DSL order
    c = _init({"layer": "conv", "filter": [3, 5, 2], "init": "norm", "stddev_norm": 0.3, "isBias": "True",
               "bias_constant": 0.25})
    d = _init(dict(base, init="norm", stddev_norm=0.3))
    assert c.p("layers.1.weight").shape == (3, 5, 6, 2)
    assert torch.equal(c.p("layers.1.weight"), d.p("layers.1.weight"))
    assert torch.equal(c.p("layers.0.weight"), d.p("layers.0.weight"))


PARENT = "61168ce"      # the commit the hash below was taken from (sha256 of the initial flat buffer)
SAMPLE_INIT_SHA256 = "699386e7cf1e2f712b8e262c5dd798980fe510e37588eea9fba9c39cebfba0e2"


def test_a_config_without_the_layer_initialises_as_before():
    a = build_model(parse_train_config(SAMPLE_CONFIG))
    b = build_model(parse_train_config(copy.deepcopy(SAMPLE_CONFIG)))
    assert torch.equal(a.state.buffer, b.state.buffer)
    assert [type(s).__name__ for s in parse_train_config(SAMPLE_CONFIG).layers] == \
        ["ConvSpec", "ConvSpec", "PoolSpec", "NormSpec", "ActSpec", "DenseSpec", "DenseSpec"]
    assert a.state.numel == 2276416
    assert hashlib.sha256(a.state.buffer.detach().numpy().tobytes()).hexdigest() == SAMPLE_INIT_SHA256, PARENT


# ---------------------------------------------------------------- 4. the eager layer against the loops
@pytest.fixture(scope="module")
def references():
    """geometry -> (x, w, bias, dy, y, dx, dw, dbias) with the float64 loops' results: computed
    once, shared, never changed."""
    out = {}
    for g in ALL_GEOMS:
        x, w, bias, dy = R.inputs(g)
        out[g] = (x, w, bias, dy) + R.dw_loops(g, x, w, bias, dy)[:4]
    return out


def _loop_count(g):
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    return B * R.out_pads(H, kh, sh, pad)[0] * R.out_pads(W, kw, sw, pad)[0] * C * M * kh * kw


@pytest.mark.parametrize("g", [g for g in ALL_GEOMS if _loop_count(g) <= 40000], ids=R.geom_id)
@pytest.mark.parametrize("act,alpha", [(None, 0.0), ("sigmoid", 0.0), ("relu", 0.0), ("leaky_relu", 0.2)])
def test_the_two_loop_references_agree(g, act, alpha):
    """The literal seven-deep loop nest and the one with the channel loops as array statements."""
    x, w, bias, dy = R.inputs(g)
    a = R.dw_loops_scalar(g, x, w, bias, dy, act, alpha)
    b = R.dw_loops(g, x, w, bias, dy, act, alpha)
    for name, u, v in zip(("y", "dx", "dw", "dbias", "absw", "absb"), a, b):
        assert u.shape == v.shape, name
        assert np.abs(u - v).max() <= 1e-13 * max(1.0, np.abs(u).max()), name


def test_channel_order_is_tfs():
    """C = 1, M = 3: output channel q is the map filtered with w[:, :, 0, q]; C = 2, M = 2: output
    channels (0, 1) read input channel 0 and (2, 3) input channel 1."""
    g = (1, 4, 4, 2, 2, 1, 1, 1, 1, "SAME")
    x = np.arange(32, dtype=np.float32).reshape(1, 4, 4, 2)
    w = np.array([1.0, 10.0, 100.0, 1000.0], dtype=np.float32).reshape(1, 1, 2, 2)
    y = R.dw_loops(g, x, w, None)
    want = np.stack([x[..., 0], 10 * x[..., 0], 100 * x[..., 1], 1000 * x[..., 1]], axis=-1)
    assert np.array_equal(y, want)
    got = R.eager(g, x, w, None, np.ones_like(want, dtype=np.float32), torch.float64)[0]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("g", ALL_GEOMS, ids=R.geom_id)
def test_digitnet_matches_loop_reference(g, references):
    """fp64: y, dx, dw and dbias by autograd agree with the loops to rounding (1e-12 of the
    reference's largest magnitude).  fp32: every output is a sum of n products of fp32 numbers,
    n <= kh kw for y, <= M kh kw for dx and B OH OW for dw and dbias, so its error is at most
    (n + 1) u sum|terms| <= (n + 1) u n max|term|; asserted with the sum's own length."""
    B, H, W, C, M, kh, kw, sh, sw, pad = g
    x, w, bias, dy, *ref = references[g]
    got = R.eager(g, x, w, bias, dy, torch.float64)
    for name, a, r in zip(("y", "dx", "dw", "dbias"), got, ref):
        if a is None:
            assert name == "dbias" and bias is None
            continue
        err = float(np.abs(a - r).max()) / max(float(np.abs(r).max()), 1e-300)
        print(f"{R.geom_id(g)} fp64 {name}: {err:.2e}")
        assert err <= 1e-12, name
    got32 = R.eager(g, x, w, bias, dy, torch.float32)
    npix = B * ref[0].shape[1] * ref[0].shape[2]
    xm, wm, dm = (float(np.abs(t).max()) for t in (x, w, dy))
    terms = {"y": (kh * kw + 1, xm * wm + (0.0 if bias is None else float(np.abs(bias).max()))),
             "dx": (M * kh * kw, dm * wm), "dw": (npix, xm * dm), "dbias": (npix, dm)}
    for name, a, r in zip(("y", "dx", "dw", "dbias"), got32, ref):
        if a is None:
            continue
        n, t = terms[name]
        e32 = float(np.abs(a - r).max())
        bound = (n + 1) * R.U * n * t
        print(f"  fp32 {name}: {e32:.2e} abs, bound {bound:.2e}; kernel bound {R.kernel_bound(e32, r):.2e}")
        assert e32 <= bound, name
    if g == (2, 4, 4, 2, 1, 1, 1, 3, 3, "SAME"):
        # stride 3, kernel 1: only rows and columns 0 and 3 are read; the rest get exactly 0
        dx = got32[1]
        seen = np.zeros((4, 4), dtype=bool)
        seen[np.ix_([0, 3], [0, 3])] = True
        assert not dx[:, ~seen].any() and dx[:, seen].all() and not ref[1][:, ~seen].any()


def test_normal_and_deterministic_mode_are_one_form(references):
    """The CPU backward of the grouped conv is order-stable: two runs and the deterministic
    switch give equal bits, so the layer has one form."""
    g = (2, 14, 14, 20, 1, 3, 3, 1, 1, "SAME")
    x, w, bias, dy, *_ = references[g]
    outs = [R.eager(g, x, w, bias, dy, torch.float32, det=det) for det in (False, True, False)]
    for a, b, c in zip(*outs):
        assert (a is None and b is None) or (np.array_equal(a, b) and np.array_equal(a, c))
    torch.use_deterministic_algorithms(True)
    try:
        d = R.eager(g, x, w, bias, dy, torch.float32, det=True)
    finally:
        torch.use_deterministic_algorithms(False)
    for a, b in zip(outs[0], d):
        assert (a is None and b is None) or np.array_equal(a, b)


def test_strided_one_by_one_subsamples_first():
    """The conv branch's workaround (a strided 1x1 kernel in this torch build's mkldnn backward):
    forward and backward run and agree with the loops for every stride pair."""
    for sh, sw in ((2, 1), (1, 2), (2, 2), (3, 3)):
        g = (2, 6, 5, 3, 2, 1, 1, sh, sw, "SAME")
        rng = np.random.default_rng(sh * 10 + sw)
        x = rng.standard_normal((2, 6, 5, 3)).astype(np.float32)
        w = rng.standard_normal((1, 1, 3, 2)).astype(np.float32)
        oh, ow = R.out_pads(6, 1, sh, "SAME")[0], R.out_pads(5, 1, sw, "SAME")[0]
        dy = rng.standard_normal((2, oh, ow, 6)).astype(np.float32)
        ref = R.dw_loops(g, x, w, None, dy)
        got = R.eager(g, x, w, None, dy, torch.float64)
        for a, r in zip(got[:3], ref[:3]):
            assert np.abs(a - r).max() <= 1e-12


def test_matches_torch_grouped_conv_on_a_symmetric_case():
    """An independent spelling: torch's grouped conv on an odd kernel, stride 1 (symmetric pads)."""
    g = (2, 5, 5, 3, 1, 3, 3, 1, 1, "SAME")
    x, w, bias, dy = R.inputs(g)
    y = R.dw_loops(g, x, w, bias)
    tw = torch.from_numpy(w).double().permute(2, 3, 0, 1).reshape(3, 1, 3, 3)
    want = F.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), tw, torch.from_numpy(bias).double(), padding=1,
                    groups=3).permute(0, 2, 3, 1).numpy()
    assert np.abs(y - want).max() <= 1e-13


# ---------------------------------------------------------------- 5. the networks against the oracle
@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


@pytest.mark.parametrize("batch", [50, 7])
@pytest.mark.parametrize("name", list(R.NETS))
def test_networks_match_fp64_oracle_cpu(name, batch, dataset):
    opt = "AdagradOptimizer"
    cfg = X.make_cfg(R.layers_of(name), opt, X.LRS[opt], "entropy", batch)
    assert DepthwiseConvSpec in [type(lp.spec) for lp in cfg.plan().layers]
    eng = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    recs = X.run_trajectory(eng, X.Oracle64(cfg, dataset), 3)
    X.check(recs, X.tolerances(name, X.LRS[opt]), f"{name}-b{batch}-cpu")


def test_the_layer_trains():
    """The weights move, and the entry changes the network: before, it was skipped."""
    cfg = _cfg(R.layers_of("dw_head"), batch_size=16)
    eng = TrainEngine(cfg, synthetic_mnist(64, seed=1), device="cpu", backend="torch")
    w0 = eng.model.p("layers.3.weight").detach().clone()
    b0 = eng.model.p("layers.3.bias").detach().clone()
    for _ in range(3):
        eng.step()
    assert not torch.equal(w0, eng.model.p("layers.3.weight")) and not torch.equal(b0, eng.model.p("layers.3.bias"))


# ---------------------------------------------------------------- 6. resume
DW_JOB = {"iter": 6, "learning_rate": 0.05, "ratio": 0.8, "loss_name": "entropy", "optimizer_name": "AdamOptimizer",
          "options": {"log_every": 3, "ckpt_every": 3, "batch_size": 16},
          "net_config": {"middle_layer": R.layers_of("dw_head")}}


def test_resume_is_exact(tmp_path):
    from cloud_server_amd.runtime import checkpoint as ckpt
    from cloud_server_amd.runtime.trainer import run_job
    data = synthetic_mnist(400, seed=0).split(0.8)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(a)
    os.makedirs(b)
    run_job(a, copy.deepcopy(DW_JOB), device="cpu", backend="torch", data=data)
    run_job(b, dict(copy.deepcopy(DW_JOB), iter=3), device="cpu", backend="torch", data=data)
    assert ckpt.latest(b)[0] == 3
    run_job(b, copy.deepcopy(DW_JOB), device="cpu", backend="torch", data=data)
    oa, ob = (ckpt.load(ckpt.latest(d)[1]) for d in (a, b))
    assert oa["host_step"] == ob["host_step"] == 6
    assert tuple(oa["model"]["layers.3.weight"].shape) == (3, 3, 4, 2) and "layers.3.bias" in oa["model"]
    for k in oa["model"]:
        assert torch.equal(oa["model"][k], ob["model"][k]), k
    assert torch.equal(oa["slots"], ob["slots"])


# ---------------------------------------------------------------- 7. API
def test_api_depthwise(tmp_path):
    from fastapi.testclient import TestClient
    from cloud_server_amd.api.app import create_app
    from cloud_server_amd.config import Settings
    s = Settings(storage_root=str(tmp_path / "store"), db_path=str(tmp_path / "db.sqlite3"),
                 executor="inline", train_backend="torch")
    pw = "Str0ng-pass-42"
    with TestClient(create_app(s, executor="inline", ngpu=0, inference_device="cpu")) as c:
        layers = [{"layer": "conv", "filter": [3, 3, 6], "stride": [2, 2]},
                  {"layer": "depthwise", "filter": ["3", "3", "2"], "stride": [2, 2], "isBias": "True"},
                  {"layer": "conv", "filter": [1, 1, 4]}]
        body = {"iter": 2, "learning_rate": 0.1, "ratio": 0.8, "net_config": {"middle_layer": layers},
                "options": {"batch_size": 8, "log_every": 1}}
        r = c.post("/generation/generate/", json=body)
        assert r.status_code == 200, r.text
        out = r.json()
        assert len(out["layers"]) == 3
        assert out["layers"][1]["spec"] == spec_to_dict(DepthwiseConvSpec(3, 3, 2, (2, 2), "SAME", "norm", True)) | \
            {"stride": [2, 2]}
        assert out["layers"][1]["out"] == [12, 7, 7] and out["layers"][2]["out"] == [4, 7, 7]
        assert out["params"] == 3 * 3 * 6 + 3 * 3 * 6 * 2 + 12 + 12 * 4 + 4 * 7 * 7 * 10 + 10
        assert out["flops_per_sample"] == 2 * (14 * 14 * 6 * 9 + 7 * 7 * 12 * 9 + 7 * 7 * 4 * 12 + 196 * 10)
        for bad in ({}, {"filter": [3, 3]}, {"filter": [3, 3, 0]}, {"filter": [3, 3, 1], "stride": [0, 1]},
                    {"filter": [3, 3, 1], "padding": "FULL"}, {"filter": [3, 3, 1], "init": "he"},
                    {"filter": [15, 15, 1], "padding": "VALID"}):
            layers[1] = dict({"layer": "depthwise"}, **bad)
            r = c.post("/generation/generate/", json=body)
            assert r.status_code == 400 and "depthwise" in r.text, (bad, r.text)
        layers[1] = {"layer": "connect", "hidden": 8}
        layers[2] = {"layer": "depthwise", "filter": [3, 3, 1]}
        r = c.post("/generation/generate/", json=body)
        assert r.status_code == 400 and "depthwise" in r.text
        # the catalogue and the layer menu
        assert c.get("/generation/options/list/").json()["convolution_method"]["options"] == ["Standard", "Depthwise"]
        assert c.post("/construct/options/", json={"option": "convolution_method"}).json()["tokens"]["Depthwise"] == \
            "depthwise"
        for prev in ("conv", "pool", "norm", "active", "depthwise", ""):
            assert "depthwise" in c.get("/generation/options/next/", params={"layer": prev}).json()["options"]
        assert "depthwise" not in c.get("/generation/options/next/", params={"layer": "connect"}).json()["options"]
        # construction stores the config as written and hands it back
        r = c.post("/rest-auth/registration/", json={"username": "al", "email": "al@x.org", "password1": pw,
                                                       "password2": pw})
        assert r.status_code == 201, r.text
        h = {"Authorization": "Token " + c.post("/rest-auth/login/", json={"username": "al", "password": pw}).json()["key"]}
        layers[1] = {"layer": "depthwise", "filter": [3, 3, 2], "stride": [2, 2], "isBias": "True"}
        layers[2] = {"layer": "conv", "filter": [1, 1, 4]}
        layers[1] = dict(layers[1], filter=[3, 3, 0])
        r = c.post("/construct/construction/dwm/file/", json=body, headers=h)
        assert r.status_code == 400 and "depthwise" in r.text, r.text
        layers[1] = dict(layers[1], filter=[3, 3, 2])
        r = c.post("/construct/construction/dwm/file/", json=body, headers=h)
        assert r.status_code == 200 and r.json()["params"] == out["params"], r.text
        back = c.get("/construct/detail/dwm/", headers=h).json()
        assert back["net_config"]["middle_layer"] == layers
        assert parse_train_config(back).layers[1] == DepthwiseConvSpec(3, 3, 2, (2, 2), "SAME", "norm", True)
