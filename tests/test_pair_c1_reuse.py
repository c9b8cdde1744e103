"""The pair backward loads the conv-A tiles the VALU pair forward stored (GPU only).

``program.pair_c1`` holds, per (image, band) workgroup of the pair launches, the band's
post-activation c1 tile in the order of the forward's LDS tile (``csa_conv_pair_c1_bands``:
first c1 row, rows, columns, stride; tile column 0 is image column ``-PLB``; zero outside
the image).  The backward's prologue copies it into LDS instead of recomputing conv A;
``CSA_PAIR_C1=0`` restores the recompute.

Geometries (``test_hip_step.CASES``): ``sample`` (2x2 SAME + pool), ``pair_relu_valid``
(VALID conv B, act A decides act'), ``pair_nopool`` (another band height).  Batch 3, eager.
"""
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from test_hip_step import CASES, _cfg

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.ops import fused as FK
from cloud_server_amd.runtime.engine import TrainEngine
from cloud_server_amd.runtime.hip_program import HipProgram, _act_id, _alpha

pytestmark = pytest.mark.gpu

GEOMS = ["sample", "pair_relu_valid", "pair_nopool"]


@functools.lru_cache(maxsize=None)
def _ds():
    return synthetic_mnist(200, seed=3)


class _env:
    """CSA_PAIR_C1 for the engines built inside (the knob is read when a program allocates)."""

    def __init__(self, c1):
        self.c1 = c1

    def __enter__(self):
        self.prev = os.environ.get("CSA_PAIR_C1")
        os.environ["CSA_PAIR_C1"] = self.c1

    def __exit__(self, *exc):
        if self.prev is None:
            del os.environ["CSA_PAIR_C1"]
        else:
            os.environ["CSA_PAIR_C1"] = self.prev


def _engine(name, backend="hip", c1="1", batch=3, graph=False, **kw):
    with _env(c1):
        eng = TrainEngine(_cfg(CASES[name], batch=batch, **kw), _ds(), device="cuda", backend=backend,
                          use_graph=graph)
    assert eng.backend == backend, eng.fallback_reason
    return eng


@functools.lru_cache(maxsize=None)
def _grads(name, batch, mode):
    """One SGD step's implied gradients per parameter; mode: "on" | "off" | "torch"."""
    eng = _engine(name, "torch" if mode == "torch" else "hip", "0" if mode == "off" else "1", batch)
    if mode != "torch":
        assert (eng.program.pair_c1 is not None) == (mode == "on")
    w0 = eng.flat.clone()
    eng.step()
    torch.cuda.synchronize()
    g = (w0 - eng.flat) / eng.cfg.effective_lr
    return {k: eng.model.state.view(k, g).clone() for k in eng.model.state.shapes}


def _act64(x, aid, alpha):
    if aid == 1:
        return torch.sigmoid(x)
    if aid == 2:
        return torch.relu(x)
    if aid == 3:
        return torch.maximum(x, alpha * x)
    return x


def _conv_a(eng, w0, idx, dtype):
    """conv A + act A of the batch ``idx`` with the parameters ``w0``: [B, H1, W1, C1]."""
    p = eng.program
    (B, H, W, C0, KAh, KAw, PTA, PLA, C1, H1, W1) = p.pair[:11]
    ua = p.units[0]
    x = eng.data.images.index_select(0, idx).view(B, H, W, C0).to(dtype).mul(1.0 / 255.0).permute(0, 3, 1, 2)
    w = eng.model.state.view(f"{ua.layer.name}.weight", w0).to(dtype).permute(3, 2, 0, 1)       # HWIO -> OIHW
    b = eng.model.state.view(f"{ua.layer.name}.bias", w0).to(dtype) if ua.layer.spec.bias else None
    x = F.pad(x, (PLA, W1 + KAw - 1 - W - PLA, PTA, H1 + KAh - 1 - H - PTA))
    y = _act64(F.conv2d(x, w, b), _act_id(ua.act), _alpha(ua.act))
    assert tuple(y.shape) == (B, C1, H1, W1)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("name", GEOMS)
def test_buffer_holds_c1(name):
    """Every element the backward reads was written by this step's forward (none of the NaN
    fill survives), is conv A + act A of the step's batch inside the image — within 4 x the
    error of torch's own fp32 conv against the fp64 result, floor 1e-6 — and 0 outside."""
    eng = _engine(name)
    p = eng.program
    assert p.pair_c1 is not None
    (B, H, W, C0, KAh, KAw, PTA, PLA, C1, H1, W1, KBh, KBw, PTB, PLB) = p.pair[:15]
    nb = int(p.lib.csa_conv_pair_grid(FK.ints(p.pair))) // B
    bands = (C.c_int * (4 * nb))()
    assert p.lib.csa_conv_pair_c1_bands(FK.ints(p.pair), bands, nb) == nb
    stride = bands[3]
    assert p.pair_c1.numel() == B * nb * stride
    idx = eng.stream.rows.index_select(0, eng.stream.cursor).view(-1).clone()
    w0 = eng.flat.clone()
    p.pair_c1.fill_(float("nan"))
    eng.step()
    torch.cuda.synchronize()
    buf = p.pair_c1.view(B, nb, stride)
    ref64 = _conv_a(eng, w0, idx, torch.float64)
    err32 = (_conv_a(eng, w0, idx, torch.float32).double() - ref64).abs().max().item()
    bound = max(4 * err32, 1e-6)
    worst = 0.0
    for band in range(nb):
        y0, T1H, T1W = bands[4 * band], bands[4 * band + 1], bands[4 * band + 2]
        assert T1H * T1W * C1 <= stride
        tile = buf[:, band, :T1H * T1W * C1].view(B, T1H, T1W, C1)
        assert not torch.isnan(tile).any(), f"{name} band {band}: unwritten elements"
        want = torch.zeros(B, T1H, T1W, C1, dtype=torch.float64, device=tile.device)
        ya, yb = max(0, y0), min(H1, y0 + T1H)
        xa, xb = max(0, -PLB), min(W1, T1W - PLB)
        want[:, ya - y0:yb - y0, xa + PLB:xb + PLB] = ref64[:, ya:yb, xa:xb]
        inside = torch.zeros(T1H, T1W, dtype=torch.bool, device=tile.device)
        inside[ya - y0:yb - y0, xa + PLB:xb + PLB] = True
        assert (tile[:, ~inside] == 0).all(), f"{name} band {band}: padding not zero"
        worst = max(worst, (tile.double() - want).abs().max().item())
    print(f"{name}: c1 max err {worst:.3e}, torch fp32 err {err32:.3e}, bound {bound:.3e}")
    assert worst <= bound, f"{name}: c1 err {worst:.3e} > {bound:.3e}"


@pytest.mark.parametrize("name,batch", [(n, 3) for n in GEOMS] + [("sample", 1)])
def test_gradients_on_off_torch(name, batch):
    """One step with the stored tiles and one with the recompute, each against the torch
    backend and against each other, under test_step_matches_torch's per-parameter bound."""
    on, off, ref = _grads(name, batch, "on"), _grads(name, batch, "off"), _grads(name, batch, "torch")
    gmax = max(v.abs().max().item() for v in ref.values())
    for what, a, b in (("on/torch", on, ref), ("off/torch", off, ref), ("on/off", on, off)):
        for k in ref:
            scale = b[k].abs().max().item() + 1e-6
            err = (a[k] - b[k]).abs().max().item()
            assert err <= 2e-3 * scale + 1e-6 + 1e-5 * gmax, \
                f"{name} B={batch} {what} grad {k}: err {err:.3e} scale {scale:.3e}"


def test_right_path_taken(monkeypatch):
    """Only a training program of the VALU family in the atomic mode stores and loads c1."""
    from cloud_server_amd.serve.hip_infer import ServeState, _FwdEngine
    eng = _engine("sample")
    assert eng.program.pair is not None and eng.program.pair_c1 is not None
    assert _engine("sample", c1="0").program.pair_c1 is None
    mf = _engine("pair_mfma")
    assert mf.program.pair is not None and mf.program.pair_c1 is None
    st = ServeState(eng.cfg, eng.model.export_state(), eng.device)
    fo = HipProgram(_FwdEngine(st, 4), forward_only=True)
    assert fo.forward_only and fo.pair is not None and fo.pair_c1 is None
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    det = _engine("sample")
    assert det.program.det and det.program.pair is not None and det.program.pair_c1 is None


def test_graph_replay_with_c1_matches_eager_recompute():
    """20 graph-replayed steps loading the stored tiles against 20 eager steps recomputing
    them: parameters within test_graph_replay_matches_eager's 3e-3."""
    kw = dict(optimizer="AdagradOptimizer", lr=0.01)
    a = _engine("sample", graph=True, **kw)
    b = _engine("sample", c1="0", graph=False, **kw)
    assert a.program.pair_c1 is not None and b.program.pair_c1 is None
    a.step()
    a.run_steps(19)
    for _ in range(20):
        b.step()
    a.sync_device()
    torch.cuda.synchronize()
    assert a.host_step == b.host_step == 20
    assert (a.flat - b.flat).abs().max().item() < 3e-3
