"""The VALU pair forward's lane mapping (GPU only): conv B runs one 16-lane row per
(output-channel pair, block of 16 units), the BatchNorm statistics are row reductions of the
registers, and bands wider than one row fold their row sums through LDS.

Every case runs one eager step of a fresh engine and recomputes conv A -> act -> conv B ->
act -> pool with torch in fp64 and in fp32 from the parameters and batch indices taken before
the step.  ``y`` / ``argmax`` are NaN / 0xFF-filled before the step.  The statistic slab is
read right after the forward launch (the step's end zeroes it again).

Bounds: an error of the kernel against fp64 may be 4 x the error of torch's own fp32 result
against fp64 (floor 1e-6 for ``y``), the convention of test_pair_c1_reuse / test_hip_trajectory.

The slab in the atomic mode: the workgroups ADD into ``nslab`` rows that the end of the
previous step left zero, so a NaN fill cannot be survived by any correct kernel there; the
test asserts the rows are zero before the step and that their sum is the fp64 sum (every
contribution exactly once).  The NaN fill is applied in deterministic mode, where every
workgroup stores an exclusive row: all ``prod_rows`` rows must be overwritten.

Geometries (the smallest at which the mapping can go wrong):
  sample           14 units per band: a partial row; C2 = 20 (10 rows of 16 rows); also batch 1
  pair_relu_valid  3x3 instantiation, VALID conv B, 13 units, C2 = 8, C1 = 6, activations
  pair_nopool      28 units per row of a 2-row band: several rows per channel, one position
  nopool_norm      the same family with a BatchNorm consumer: the LDS fold of the row sums
  odd_pool         2x2 VALID conv A, SAME conv B (27 x 27), pool: partial windows at the
                   bottom / right edge and a ragged last band
  chan_limit       C1 = 16 with the largest C2 the VALU family admits for 2x2 kernels
  sample packed    two pooled rows per band (28 units: two rows per channel)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_hip_step import CASES, _cfg

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.ops import fused as FK
from cloud_server_amd.runtime.engine import TrainEngine
from cloud_server_amd.runtime.hip_program import _act_id, _alpha

pytestmark = pytest.mark.gpu

CHAN_LIMIT_C2 = 28      # 64 + 64 C2 weights <= 2048 and C2 % 4 == 0 (test_channel_limit_is_the_family_limit)

NETS = dict(CASES)
NETS["nopool_norm"] = [
    {"layer": "conv", "filter": [2, 2, 4]},
    {"layer": "conv", "filter": [3, 3, 8]},
    {"layer": "active", "active_func": "relu"},
    {"layer": "norm"},
    {"layer": "connect", "hidden": 16},
]
NETS["odd_pool"] = [
    {"layer": "conv", "filter": [2, 2, 6], "padding": "VALID", "isBias": "True"},
    {"layer": "active", "active_func": "relu"},
    {"layer": "conv", "filter": [2, 2, 8], "isBias": "True"},
    {"layer": "active", "active_func": "leaky_relu", "param": [0.1]},
    {"layer": "pool"},
    {"layer": "norm"},
    {"layer": "connect", "hidden": 16},
]
NETS["chan_limit"] = [
    {"layer": "conv", "filter": [2, 2, 16]},
    {"layer": "conv", "filter": [2, 2, CHAN_LIMIT_C2], "isBias": "True"},
    {"layer": "pool"},
    {"layer": "norm"},
    {"layer": "active"},
    {"layer": "connect", "hidden": 16},
]

# (net, batch, packed)
RUNS = [("sample", 3, False), ("sample", 1, False), ("pair_relu_valid", 3, False), ("pair_nopool", 3, False),
        ("nopool_norm", 3, False), ("odd_pool", 3, False), ("chan_limit", 3, False), ("sample", 3, True)]
IDS = [f"{n}-B{b}{'-packed' if p else ''}" for n, b, p in RUNS]


@functools.lru_cache(maxsize=None)
def _ds():
    return synthetic_mnist(200, seed=3)


def _engine(name, batch, packed):
    eng = TrainEngine(_cfg(NETS[name], batch=batch), _ds(), device="cuda", backend="hip", use_graph=False,
                      packed=packed)
    assert eng.backend == "hip", eng.fallback_reason
    p = eng.program
    assert p.pair is not None, f"{name}: no fused conv pair"
    assert p.lib.csa_conv_pair_valu_ok(FK.ints(p.pair)), f"{name}: not the VALU pair family"
    assert p.packed == packed
    return eng


def _act(x, aid, alpha):
    if aid == 1:
        return torch.sigmoid(x)
    if aid == 2:
        return torch.relu(x)
    if aid == 3:
        return torch.maximum(x, alpha * x)
    return x


def _reference(eng, w0, idx, dtype):
    """(pooled y [B, PH, PW, C2], window values [B, PH, PW, C2, 4] with -inf outside conv B's
    output) — for a pair without pool: (y [B, H2, W2, C2], None)."""
    p = eng.program
    (B, H, W, C0, KAh, KAw, PTA, PLA, C1, H1, W1, KBh, KBw, PTB, PLB, C2, H2, W2, pool, PH, PW) = p.pair[:21]
    ua, ub = p.units[0], p.units[1]
    view = eng.model.state.view

    def conv(x, u, kh, kw, pt, pl, hin, win, hout, wout):
        w = view(f"{u.layer.name}.weight", w0).to(dtype).permute(3, 2, 0, 1)          # HWIO -> OIHW
        b = view(f"{u.layer.name}.bias", w0).to(dtype) if u.layer.spec.bias else None
        x = F.pad(x, (pl, wout + kw - 1 - win - pl, pt, hout + kh - 1 - hin - pt))
        return _act(F.conv2d(x, w, b), _act_id(u.act), _alpha(u.act))

    x = eng.data.images.index_select(0, idx).view(B, H, W, C0).to(dtype).mul(1.0 / 255.0).permute(0, 3, 1, 2)
    c1 = conv(x, ua, KAh, KAw, PTA, PLA, H, W, H1, W1)
    z = conv(c1, ub, KBh, KBw, PTB, PLB, H1, W1, H2, W2)
    assert tuple(z.shape) == (B, C2, H2, W2)
    if not pool:
        return z.permute(0, 2, 3, 1).contiguous(), None
    z = F.pad(z, (0, 2 * PW - W2, 0, 2 * PH - H2), value=float("-inf"))
    win = z.view(B, C2, PH, 2, PW, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, PH, PW, C2, 4)   # q = 2 dy + dx
    return win.max(dim=4).values.contiguous(), win


def _step(name, batch, packed, det_fill=False):
    """One step of a fresh engine: kernel outputs, the slab as the forward launch left it and
    the references, on the CPU."""
    eng = _engine(name, batch, packed)
    p = eng.program
    ub = p.units[1]
    nt = p.units[2].in_tf if len(p.units) > 2 else p.head_tf
    slab = nt.slab if nt.has_bn else None
    idx = eng.stream.rows.index_select(0, eng.stream.cursor).view(-1).clone()
    w0 = eng.flat.clone()
    ub.y.fill_(float("nan"))
    if ub.argmax is not None:
        ub.argmax.fill_(0xFF)
    out = {"pool": bool(p.pair[18]), "det": bool(p.det)}
    if slab is not None:
        if det_fill:
            assert p.det
            slab.fill_(float("nan"))
        else:
            assert not p.det and (slab == 0).all(), "the atomic slab rows start the step zeroed"
        fwd = p.lib.csa_conv_pair_fwd

        def spy(*args):
            rc = fwd(*args)
            out["slab"] = slab.clone()
            return rc

        p.lib.csa_conv_pair_fwd = spy
    try:
        eng.step()
    finally:
        if slab is not None:
            p.lib.csa_conv_pair_fwd = fwd
    torch.cuda.synchronize()
    out["y"] = ub.y.clone()
    out["argmax"] = ub.argmax.clone() if ub.argmax is not None else None
    out["rows"] = (nt.prod_rows if p.det else int(p.lib.csa_conv_fwd_nslab(None, None))) if slab is not None else 0
    out["y64"], out["win64"] = _reference(eng, w0, idx, torch.float64)
    out["y32"], _ = _reference(eng, w0, idx, torch.float32)
    return out


@functools.lru_cache(maxsize=None)
def _atomic(name, batch, packed):
    return _step(name, batch, packed)


def _tol(o):
    err32 = (o["y32"].double() - o["y64"]).abs().max().item()
    return max(4 * err32, 1e-6), err32


def _check_y(o, tag):
    bound, err32 = _tol(o)
    assert not torch.isnan(o["y"]).any(), f"{tag}: outputs not written"
    err = (o["y"].double() - o["y64"]).abs().max().item()
    print(f"{tag}: y max err {err:.3e}, torch fp32 err {err32:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{tag}: y err {err:.3e} > {bound:.3e}"


def _check_argmax(o, tag):
    if not o["pool"]:
        assert o["argmax"] is None
        return
    bound, _ = _tol(o)
    am, win = o["argmax"].long(), o["win64"]
    assert (am < 4).all(), f"{tag}: argmax not written or outside the window"
    got = win.gather(4, am.unsqueeze(4)).squeeze(4)
    assert torch.isfinite(got).all(), f"{tag}: argmax names a position outside conv B's output"
    top = win.max(dim=4)
    gap = (top.values - got).max().item()
    print(f"{tag}: argmax value short of the window maximum by at most {gap:.3e} (bound {bound:.3e})")
    assert gap <= bound, f"{tag}: argmax value {gap:.3e} below the maximum"
    second = win.topk(2, dim=4).values[..., 1]
    clear = (top.values - second) > bound
    assert (am[clear] == top.indices[clear]).all(), f"{tag}: argmax position differs where the maximum is clear"
    # ties in fp64 are rare; where the kernel's own values tie the first position wins (checked
    # through exact-position equality above whenever the fp64 gap is clear)


def _check_stats(o, tag):
    if "slab" not in o:
        return
    slab = o["slab"]
    rows = o["rows"]
    assert slab.shape[0] >= rows >= 1
    read = slab[:rows]
    assert not torch.isnan(read).any(), f"{tag}: a slab row the consumer reads was not written"
    got = read.double().sum(dim=0)                              # [2, C2]
    y64, y32 = o["y64"], o["y32"]
    want = torch.stack([y64.sum(dim=(0, 1, 2)), (y64 * y64).sum(dim=(0, 1, 2))])
    t32 = torch.stack([y32.sum(dim=(0, 1, 2)), (y32 * y32).sum(dim=(0, 1, 2))]).double()
    for k, what in enumerate(("sum", "sum of squares")):
        err32 = (t32[k] - want[k]).abs().max().item()
        err = (got[k] - want[k]).abs().max().item()
        print(f"{tag}: {what} max err {err:.3e}, torch fp32 err {err32:.3e}, bound {4 * err32:.3e}")
        assert err <= 4 * err32, f"{tag}: {what} err {err:.3e} > {4 * err32:.3e}"


@pytest.mark.parametrize("name,batch,packed", RUNS, ids=IDS)
def test_outputs_match_fp64(name, batch, packed):
    """``y`` within the bound of fp64 and none of the NaN fill left."""
    _check_y(_atomic(name, batch, packed), f"{name} B={batch} packed={packed}")


@pytest.mark.parametrize("name,batch,packed", RUNS, ids=IDS)
def test_argmax_names_the_window_maximum(name, batch, packed):
    """Every window: the fp64 value at the named position is within the bound of the window's
    fp64 maximum and lies inside conv B's output; exact position where the top two differ by
    more than the bound."""
    _check_argmax(_atomic(name, batch, packed), f"{name} B={batch} packed={packed}")


@pytest.mark.parametrize("name,batch,packed", RUNS, ids=IDS)
def test_statistics_match_fp64(name, batch, packed):
    """The slab rows summed per channel are the fp64 sum and sum of squares of the pooled
    output within 4 x the error of torch's fp32 sums."""
    o = _atomic(name, batch, packed)
    if name != "pair_nopool":
        assert "slab" in o, f"{name}: no statistic slab"
    _check_stats(o, f"{name} B={batch} packed={packed}")


DET_RUNS = [r for r in RUNS if not r[2]]


@pytest.mark.parametrize("name,batch,packed", DET_RUNS, ids=[i for i, r in zip(IDS, RUNS) if not r[2]])
def test_deterministic_mode_is_bitwise_reproducible(monkeypatch, name, batch, packed):
    """Two fresh engines with the same seed: ``y``, ``argmax`` and the slab (one exclusive
    row per workgroup, every one overwriting its NaN fill) are bitwise equal, and correct."""
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    a, b = _step(name, batch, packed, det_fill=True), _step(name, batch, packed, det_fill=True)
    tag = f"{name} B={batch} det"
    assert a["det"] and b["det"]
    _check_y(a, tag)
    _check_argmax(a, tag)
    _check_stats(a, tag)
    assert torch.equal(a["y"], b["y"])
    if a["argmax"] is not None:
        assert torch.equal(a["argmax"], b["argmax"])
    if "slab" in a:
        assert torch.equal(a["slab"], b["slab"])


def test_channel_limit_is_the_family_limit():
    """chan_limit's C2 is the largest the VALU family admits with C1 = 16 and 2x2 kernels."""
    p = _engine("chan_limit", 3, False).program
    assert p.pair[8] == 16 and p.pair[15] == CHAN_LIMIT_C2
    for c2 in range(CHAN_LIMIT_C2 + 2, 66, 2):
        g = list(p.pair)
        g[15] = c2
        ok = p.lib.csa_conv_pair_ok(FK.ints(g)) and p.lib.csa_conv_pair_valu_ok(FK.ints(g))
        assert not ok, f"C2 = {c2} is admitted too"
