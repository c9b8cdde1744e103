"""Layer / group / instance normalisation on the CPU: the ``mode`` of a ``norm`` entry, shape
inference, the eager model against the float64 loop reference (tests/gn_ref.py), the networks
against the fp64 oracle at its unchanged tolerances, data parallelism without ``sync_bn``,
resume, the API.

Before this layer ``{"layer": "norm", "mode": "layer"}`` parsed to a ``NormSpec``: the stray key
was ignored and the job trained BatchNorm."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gn_ref as R
import oracle64 as X
import test_distributed as TD

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.cnn import build_model
from cloud_server_amd.models.dsl import (SAMPLE_CONFIG, ConfigError, GroupNormSpec, NormSpec, TensorShape, parse_layer,
                                         parse_train_config, spec_to_dict)
from cloud_server_amd.models.options import get_options
from cloud_server_amd.runtime.engine import TrainEngine

ALL_GEOMS = R.GEOMETRIES + R.GRID_STRIDE
CONV = {"layer": "conv", "filter": [3, 3, 8]}


def _cfg(layers, **opts):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c["options"] = dict(opts)
    return parse_train_config(c)


# ---------------------------------------------------------------- 1. parsing
def test_mode_parses_to_a_group_norm_spec():
    """The test that fails without the feature: the key was ignored and gave a NormSpec."""
    sp = parse_layer({"layer": "norm", "mode": "layer"}, 0)
    assert type(sp) is GroupNormSpec and not isinstance(sp, NormSpec)
    assert (sp.groups, sp.epsilon, sp.mode, sp.kind) == (None, 1e-6, "layer", "norm")
    sp = parse_layer({"layer": "norm", "mode": "instance", "epsilon": 1e-5}, 0)
    assert sp == GroupNormSpec(None, 1e-5, "instance")
    sp = parse_layer({"layer": "norm", "mode": "group", "groups": 4}, 2)
    assert sp == GroupNormSpec(4, 1e-6, "group")


def test_parse_numbers_as_strings():
    sp = parse_layer({"layer": "norm", "mode": "group", "groups": "4", "epsilon": "1e-5"}, 0)
    assert sp == GroupNormSpec(4, 1e-5, "group") and type(sp.groups) is int
    assert parse_layer({"layer": "norm", "mode": "group", "groups": 2.0}, 0).groups == 2


def test_batch_norm_entries_parse_as_before():
    for d in ({"layer": "norm"}, {"layer": "norm", "mode": "batch"}):
        sp = parse_layer(d, 0)
        assert type(sp) is NormSpec and sp == NormSpec(1e-3)
    assert parse_layer({"layer": "norm", "epsilon": "1e-2"}, 0) == NormSpec(1e-2)
    # stray keys are ignored, as before
    assert parse_layer({"layer": "norm", "groups": 3, "momentum": 0.9}, 0) == NormSpec(1e-3)
    assert parse_layer({"layer": "norm", "mode": "batch", "groups": 3}, 0) == NormSpec(1e-3)
    assert spec_to_dict(parse_layer({"layer": "norm"}, 0)) == {"epsilon": 1e-3, "kind": "norm"}


@pytest.mark.parametrize("bad", [
    {"mode": "Layer"}, {"mode": "rms"}, {"mode": ""}, {"mode": 1}, {"mode": None}, {"mode": True}, {"mode": ["layer"]},
    {"mode": "layer", "groups": 1}, {"mode": "instance", "groups": 8},
    {"mode": "group"},
    {"mode": "group", "groups": 0}, {"mode": "group", "groups": -2}, {"mode": "group", "groups": 2.5},
    {"mode": "group", "groups": "2.5"}, {"mode": "group", "groups": "two"}, {"mode": "group", "groups": None},
    {"mode": "group", "groups": True}, {"mode": "group", "groups": float("nan")},
    {"mode": "group", "groups": float("inf")}, {"mode": "group", "groups": [2]},
    {"mode": "layer", "epsilon": 0}, {"mode": "layer", "epsilon": -1e-6}, {"mode": "layer", "epsilon": float("inf")},
    {"mode": "layer", "epsilon": float("nan")}, {"mode": "layer", "epsilon": "e"}, {"mode": "layer", "epsilon": None},
    {"mode": "layer", "epsilon": True}, {"mode": "group", "groups": 2, "epsilon": False},
], ids=lambda d: ",".join(f"{k}={v!r}" for k, v in d.items()))
def test_parse_refusals(bad):
    with pytest.raises(ConfigError):
        parse_layer(dict({"layer": "norm"}, **bad), 0)
    with pytest.raises(ConfigError):
        _cfg([CONV, dict({"layer": "norm"}, **bad)])


# ---------------------------------------------------------------- 2. shapes, parameters, the catalogue
def test_shapes_parameters_and_concrete_groups():
    plan = _cfg([CONV, {"layer": "norm", "mode": "layer"}, {"layer": "norm", "mode": "instance"},
                 {"layer": "norm", "mode": "group", "groups": 4}, {"layer": "connect", "hidden": 12},
                 {"layer": "norm", "mode": "layer"}, {"layer": "norm", "mode": "group", "groups": 3}]).plan()
    assert [lp.spec.groups for lp in plan.layers if type(lp.spec) is GroupNormSpec] == [1, 8, 4, 1, 3]
    for lp in plan.layers[1:4]:
        assert lp.in_shape == lp.out_shape == TensorShape(8, (28, 28))
        assert lp.params == {"scale": (8,), "offset": (8,)}
    for lp in plan.layers[5:]:
        assert lp.in_shape == lp.out_shape == TensorShape(12, None)
        assert lp.params == {"scale": (12,), "offset": (12,)}
    # the same parameters as BatchNorm in the same places
    bn = _cfg([CONV, {"layer": "norm"}, {"layer": "norm"}, {"layer": "norm"}, {"layer": "connect", "hidden": 12},
               {"layer": "norm"}, {"layer": "norm"}]).plan()
    assert plan.param_shapes() == bn.param_shapes()
    # the parsed spec keeps what was written: only the plan holds the concrete count
    assert _cfg([CONV, {"layer": "norm", "mode": "instance"}]).layers[1].groups is None


def test_a_spec_built_in_code_is_valid_or_refused():
    from cloud_server_amd.models.dsl import plan_network
    assert GroupNormSpec() == GroupNormSpec(None, 1e-6, "layer")        # the default is a valid layer norm
    assert plan_network([GroupNormSpec()]).layers[0].spec.groups == 1
    for bad in (GroupNormSpec(None, 1e-6, "group"), GroupNormSpec(0, 1e-6, "group"), GroupNormSpec(2.0, 1e-6, "group")):
        with pytest.raises(ConfigError, match="layer 0.*needs groups"):
            plan_network([bad])


def test_plan_time_refusals_name_the_layer():
    with pytest.raises(ConfigError, match="layer 1.*does not divide"):
        _cfg([CONV, {"layer": "norm", "mode": "group", "groups": 3}])
    with pytest.raises(ConfigError, match="layer 2.*does not divide"):
        _cfg([CONV, {"layer": "connect", "hidden": 10}, {"layer": "norm", "mode": "group", "groups": 4}])
    with pytest.raises(ConfigError, match="layer 2.*instance norm after a connect"):
        _cfg([CONV, {"layer": "connect", "hidden": 10}, {"layer": "norm", "mode": "instance"}])
    # first layer: one channel
    assert _cfg([{"layer": "norm", "mode": "instance"}, CONV]).plan().layers[0].spec.groups == 1
    with pytest.raises(ConfigError):
        _cfg([{"layer": "norm", "mode": "group", "groups": 2}, CONV])


def test_model_has_no_running_buffers_and_unit_parameters():
    model = build_model(_cfg(R.layers_of("gn_dense")))
    assert list(model.named_buffers()) == []
    assert not any(k.startswith("buffers.") for k in model.export_state())
    for lp in model.plan.layers:
        if type(lp.spec) is GroupNormSpec:
            assert torch.equal(model.p(f"{lp.name}.scale"), torch.ones(lp.in_shape.c))
            assert torch.equal(model.p(f"{lp.name}.offset"), torch.zeros(lp.in_shape.c))
    assert len(list(build_model(_cfg(SAMPLE_CONFIG["net_config"]["middle_layer"])).named_buffers())) == 2


def test_catalogue_entry():
    o = get_options("normalization_method")
    assert o["options"] == ["Batch", "Layer", "Group", "Instance"] and o["default"] == "Batch"
    assert o["tokens"] == {"Batch": "batch", "Layer": "layer", "Group": "group", "Instance": "instance"}
    for tok in o["tokens"].values():
        d = {"layer": "norm", "mode": tok}
        if tok == "group":
            d["groups"] = 2
        assert parse_layer(d, 0) is not None


def test_networks_have_the_shapes_they_are_named_for():
    for name in ("gn_sample_layer", "gn_sample_group"):
        p = _cfg(R.layers_of(name)).plan()
        assert type(p.layers[3].spec) is GroupNormSpec and p.layers[3].in_shape == TensorShape(20, (14, 14))
    assert _cfg(R.layers_of("gn_sample_group")).plan().layers[3].spec.groups == 4
    p = _cfg(R.layers_of("gn_instance")).plan()
    assert p.layers[3].spec.groups == 8 and p.layers[3].in_shape == TensorShape(8, (14, 14))
    p = _cfg(R.layers_of("gn_dense")).plan()
    assert [lp.spec.groups for lp in p.layers if type(lp.spec) is GroupNormSpec] == [1, 8] and p.head_in == 32
    p = _cfg(R.layers_of("gn_first")).plan()
    assert type(p.layers[0].spec) is GroupNormSpec and p.layers[0].in_shape == TensorShape(1, (28, 28))
    p = _cfg(R.layers_of("gn_wide160")).plan()
    assert p.layers[2].in_shape == TensorShape(160, (7, 7)) and p.layers[2].spec.groups == 32
    p = _cfg(R.layers_of("gn_leaky_neg")).plan()
    assert p.layers[1].in_shape == TensorShape(4, (14, 14)) and p.layers[2].spec.alpha == -0.1


# ---------------------------------------------------------------- 3. DigitNet against the loop reference
@pytest.fixture(scope="module")
def references():
    """(geometry, shifted) -> (x, dy, scale, offset, y64, dx64, dscale64, doffset64), and
    ("rstd", (geometry, shifted)) -> the loops' rstd [B, G]: computed once, shared, never changed."""
    out = {}
    for g in ALL_GEOMS:
        for shifted in ((False, True) if g in R.SHIFTED else (False,)):
            x, dy, sc, of = R.inputs(g, shifted)
            y, _, rstd, dx, dsc, dof = R.gn_loops(x, sc, of, g[4], R.EPS, dy)
            out[g, shifted] = (x, dy, sc, of, y, dx, dsc, dof)
            out["rstd", (g, shifted)] = rstd
    return out


CASES = [(g, False) for g in ALL_GEOMS] + [(g, True) for g in R.SHIFTED]


def _case_id(c) -> str:
    return R.geom_id(c[0]) + ("-shifted" if c[1] else "")


def _rel(got, ref):
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-300)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_digitnet_matches_loop_reference(case, references):
    """fp64: forward, dx, dscale and doffset by autograd within 1e-12 of the loops (of the
    reference's largest magnitude), at every geometry and on the shifted set alike.

    fp32: the issue words this half as "inside ``kernel_bound``", but that bound is
    ``max(4 e32, ...)`` with e32 this very error, so it holds whatever the layer computes.
    What is asserted instead is worked out from the arithmetic.  The one step that loses more
    than a few roundings is the centring: ``x - mean`` with a mean rounded to fp32 (and summed in
    fp32) is off by about ``2 u max|x|``, which ``rstd`` turns into ``2 u kappa`` of xhat, with
    ``kappa = 1 + max|x| max rstd`` the condition number of the centring (4 to 9 on the
    standard-normal sets, about 310 on the shifted set, 3161 at two elements a group).  The
    roundings of rstd, the scale and the products about double that, and y, dx, dscale and
    doffset are xhat times quantities of the reference's own size: e32 <= 4 u kappa max(|ref|, 1).
    (The eager layer sits at 0.69 of it at most.)"""
    g, shifted = case
    x, dy, sc, of, *ref = references[case]
    rstd = references["rstd", case]
    got = R.eager(g, x, dy, sc, of, torch.float64)
    for name, a, r in zip(("y", "dx", "dscale", "doffset"), got, ref):
        err = _rel(a, r) if np.abs(r).max() > 0 else float(np.abs(a).max())
        print(f"{_case_id(case)} fp64 {name}: {err:.2e}")
        assert err <= 1e-12, name
    got32 = R.eager(g, x, dy, sc, of, torch.float32)
    kappa = 1.0 + float(np.abs(x).max()) * float(rstd.max())
    for name, a, r in zip(("y", "dx", "dscale", "doffset"), got32, ref):
        e32 = float(np.abs(a - r).max())
        bound = 4.0 * R.U * kappa * max(float(np.abs(r).max()), 1.0)
        print(f"  fp32 {name}: {e32:.2e} abs, bound {bound:.2e} (kappa {kappa:.1f}); kernel bound "
              f"{R.kernel_bound(e32, r):.2e}")
        assert e32 <= bound, name
    if g[:4] == (2, 1, 1, 1):            # m = 1: y = offset and dx = 0, exactly
        assert np.array_equal(got32[0].reshape(2, 1), np.broadcast_to(of.astype(np.float64), (2, 1)))
        assert not got32[1].any() and not got[1].any()


def test_normal_and_deterministic_mode_are_one_form(references):
    g = (2, 3, 3, 20, 4)
    x, dy, sc, of, *_ = references[g, False]
    outs = [R.eager(g, x, dy, sc, of, torch.float32, det=det) for det in (False, True)]
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_layer_mode_on_a_flat_input_is_layer_norm():
    g = (3, 1, 1, 32, 1)
    x, dy, sc, of = R.inputs(g)
    model = build_model(_cfg([{"layer": "connect", "hidden": 32}, {"layer": "norm", "mode": "layer"}])).double()
    with torch.no_grad():
        model.p("layers.1.scale").copy_(torch.from_numpy(sc))
        model.p("layers.1.offset").copy_(torch.from_numpy(of))
    lp = model.plan.layers[1]
    assert lp.spec == GroupNormSpec(1, R.EPS, "layer") and lp.in_shape == TensorShape(32, None)
    xt = torch.from_numpy(x).double().view(3, 32)
    got = model._layer(lp, xt, True)
    want = F.layer_norm(xt, (32,), torch.from_numpy(sc).double(), torch.from_numpy(of).double(), R.EPS)
    assert (got - want).abs().max().item() <= 1e-13


def test_instance_mode_is_instance_norm():
    g = (2, 5, 5, 6, 6)
    x, dy, sc, of = R.inputs(g)
    got = R.eager(g, x, dy, sc, of, torch.float64)[0]
    want = F.instance_norm(torch.from_numpy(x).double().permute(0, 3, 1, 2), weight=torch.from_numpy(sc).double(),
                           bias=torch.from_numpy(of).double(), eps=R.EPS).permute(0, 2, 3, 1)
    assert np.abs(got - want.numpy()).max() <= 1e-13


def test_training_and_eval_are_the_same_arithmetic():
    model = build_model(_cfg(R.layers_of("gn_dense")))
    x = torch.from_numpy(synthetic_mnist(16, seed=5).images[:7]).float().div(255.0)
    model.train()
    a = model(x)
    model.eval()
    assert torch.equal(a, model(x))


# ---------------------------------------------------------------- 4. the networks against the oracle
@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


@pytest.mark.parametrize("batch", [50, 7])
@pytest.mark.parametrize("name", list(R.NETS))
def test_networks_match_fp64_oracle_cpu(name, batch, dataset):
    opt = "AdagradOptimizer"
    cfg = X.make_cfg(R.layers_of(name), opt, X.LRS[opt], "entropy", batch)
    assert GroupNormSpec in [type(lp.spec) for lp in cfg.plan().layers]
    eng = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    recs = X.run_trajectory(eng, X.Oracle64(cfg, dataset), 3)
    X.check(recs, X.tolerances(name, X.LRS[opt]), f"{name}-b{batch}-cpu")


# ---------------------------------------------------------------- 5. data parallelism without sync_bn
DP_CFG = dict(TD.CFG, net_config={"middle_layer": R.layers_of("gn_sample_layer")},
              options=dict(TD.CFG["options"], batch_size=25))


def _train_gn(rank, world, port, steps, out):
    from cloud_server_amd.parallel.dist import shutdown
    ctx = TD._init(rank, world, port)
    cfg = parse_train_config(DP_CFG)
    assert not cfg.sync_bn
    eng = TrainEngine(cfg, synthetic_mnist(256, seed=1), device="cpu", ctx=ctx, strategy="allreduce")
    for _ in range(steps):
        eng.step()
    out[rank] = eng.flat.clone()
    shutdown(ctx)


def test_two_ranks_equal_one_process_on_the_global_batch_without_sync_bn():
    """Every sample is normalised on its own: a world-2 run at batch 25 is one process at
    batch 50, with no statistic exchanged (the comparison of test_distributed.py::
    test_allreduce_dp_equals_single_process_big_batch)."""
    out = TD._spawn(_train_gn, 2, 6)
    torch.testing.assert_close(out[0], out[1], rtol=0, atol=0)
    cfg = parse_train_config(dict(DP_CFG, options=dict(DP_CFG["options"], batch_size=50)))
    eng = TrainEngine(cfg, synthetic_mnist(256, seed=1), device="cpu")
    n = eng.flat.numel()
    for _ in range(6):
        eng.step()
    torch.testing.assert_close(out[0][:n], eng.flat, rtol=2e-4, atol=2e-5)


# ---------------------------------------------------------------- 6. resume
GN_JOB = {"iter": 6, "learning_rate": 0.05, "ratio": 0.8, "loss_name": "entropy", "optimizer_name": "AdamOptimizer",
          "options": {"log_every": 3, "ckpt_every": 3, "batch_size": 16},
          "net_config": {"middle_layer": R.layers_of("gn_dense")}}


def test_resume_is_exact_and_the_checkpoint_holds_no_buffer(tmp_path):
    from cloud_server_amd.runtime import checkpoint as ckpt
    from cloud_server_amd.runtime.trainer import run_job
    data = synthetic_mnist(400, seed=0).split(0.8)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(a)
    os.makedirs(b)
    run_job(a, copy.deepcopy(GN_JOB), device="cpu", backend="torch", data=data)
    run_job(b, dict(copy.deepcopy(GN_JOB), iter=3), device="cpu", backend="torch", data=data)
    assert ckpt.latest(b)[0] == 3
    run_job(b, copy.deepcopy(GN_JOB), device="cpu", backend="torch", data=data)
    oa, ob = (ckpt.load(ckpt.latest(d)[1]) for d in (a, b))
    assert oa["host_step"] == ob["host_step"] == 6
    assert not any(k.startswith("buffers.") for k in oa["model"])
    assert "layers.4.scale" in oa["model"] and "layers.7.offset" in oa["model"]
    for k in oa["model"]:
        assert torch.equal(oa["model"][k], ob["model"][k]), k
    assert torch.equal(oa["slots"], ob["slots"])


# ---------------------------------------------------------------- 7. API
def test_api_group_norm(tmp_path):
    from fastapi.testclient import TestClient
    from cloud_server_amd.api.app import create_app
    from cloud_server_amd.config import Settings
    s = Settings(storage_root=str(tmp_path / "store"), db_path=str(tmp_path / "db.sqlite3"),
                 executor="inline", train_backend="torch")
    with TestClient(create_app(s, executor="inline", ngpu=0, inference_device="cpu")) as c:
        layers = [{"layer": "conv", "filter": [3, 3, 6], "stride": [2, 2]},
                  {"layer": "norm", "mode": "instance"},
                  {"layer": "norm", "mode": "group", "groups": "3", "epsilon": "1e-5"},
                  {"layer": "norm", "mode": "layer"},
                  {"layer": "norm"}]
        body = {"iter": 5, "learning_rate": 0.1, "ratio": 0.8, "net_config": {"middle_layer": layers}}
        r = c.post("/generation/generate/", json=body)
        assert r.status_code == 200, r.text
        out = r.json()
        assert out["layers"][1]["spec"] == {"groups": 6, "epsilon": 1e-6, "mode": "instance", "kind": "norm"}
        assert out["layers"][2]["spec"] == {"groups": 3, "epsilon": 1e-5, "mode": "group", "kind": "norm"}
        assert out["layers"][3]["spec"] == {"groups": 1, "epsilon": 1e-6, "mode": "layer", "kind": "norm"}
        assert out["layers"][4]["spec"] == {"epsilon": 1e-3, "kind": "norm"}
        assert all(l["out"] == [6, 14, 14] for l in out["layers"])
        assert out["params"] == 3 * 3 * 6 + 4 * 12 + 6 * 14 * 14 * 10 + 10
        for bad in ({"mode": "rms"}, {"mode": "group"}, {"mode": "group", "groups": 4}, {"mode": "group", "groups": 0},
                    {"mode": "layer", "groups": 1}, {"mode": "layer", "epsilon": 0}, {"mode": "group", "groups": True}):
            layers[1] = dict({"layer": "norm"}, **bad)
            r = c.post("/generation/generate/", json=body)
            assert r.status_code == 400, (bad, r.text)
        layers[1] = {"layer": "connect", "hidden": 8}
        layers[2] = {"layer": "norm", "mode": "instance"}
        assert c.post("/generation/generate/", json=body).status_code == 400
