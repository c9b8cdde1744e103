"""The dense update launches called directly, against an fp64 computation done here (GPU only).

Three launch forms share ``csrc/kernels/dense_update.h``: the fused backward (input gradient,
weight gradient and optimizer update in one launch; ``csa_dense_bwd_update`` and, storing the
gradients whole, ``csa_dense_bwd_grad_head``), the narrow input gradient alone
(``csa_dense_bwd_dgrad`` when a row group is split into column blocks) and the deferred
weight-gradient + update segments launched on their own (``csa_dense_update_defer`` +
``csa_dense_update_flush``), with and without the head epilogue.  What a call must produce, with
scale = 1:

    dW     = Xw^T @ dY                                  [K][N]
    db     = sum_m dY                                   [N]
    W, b, slots after one optimizer step (``ops.optim_ref.step_ref`` on fp64 copies), or in
    gradient mode dW and db stored whole
    dX, slab   as in test_dense_dgrad.py (g = dY @ W_old^T, transform backward, BN statistics)
    dWh    = act(hy)^T @ dl   [N][10],   dbh = sum_m dl,   ring entry (step - 1) % ring =
             {sum hrl / ldiv, sum hrc}                  (head epilogue; stored, or applied to
             the head's parameters in place)

Slots start from random values with accumulators and second moments >= 0.1, so the update is a
smooth function of the gradient (from zero slots Adam's first step is +-lr whatever the
gradient's size).  Inputs keep |z| >= 0.02 as in test_dense_dgrad.py.  The forward BatchNorm
statistics always arrive as ONE folded row: a workgroup folds several rows with LDS atomics in
free order, and every printed hash below must be reproducible.

Shapes are the smallest at which each path can go wrong:

    wide    K = 2036 (128 row groups, the fewest on the 16-wave path, the last one partial),
            N in {16, 48, 272, 512}, M in {1, 17, 50, 64}
    narrow  K = 36 (3 row groups, the last partial; 43 bias columns per block > 4 waves),
            N = 144 (2 column blocks, the second 16 wide), 256, 640 (5 blocks: the clamp of the
            hand-off loop), 1152 (9 blocks: its second pass)
    flush   N in {128, 256}, K = 36 (43 dWh rows per block: the direct global loop) and 256
            (8 rows: the staged path)

Every weight-updating case runs SGD, Adagrad, Adam and the gradient mode; every case that
forms dX runs (no transform; sigmoid + BatchNorm C = 20 with the table; leaky + BatchNorm
C = 3 without it) in atomic and in deterministic mode, where a second call must reproduce the
first bit for bit.  Every output lives inside a larger buffer whose other elements must keep
their fill value; the arrival tickets must be zero again after every call.

Each call prints a hash of the raw bytes of every output that does not depend on atomic order
(everything but the slab in atomic mode): equal hashes from two builds of the library mean
bitwise equal results.

Bounds.  Errors are relative to the largest magnitude of the case's reference array.  The
same inputs ran through the parent's library (one ``du_body`` for every form) on an MI355X;
the bound is 4 x the parent's worst figure per quantity, the PARENT_* constants
(profiles/r11_notes.md).  The arithmetic is meant to be the parent's, so anything near 4 x is
a changed kernel, not noise.
"""
import ctypes as C
import hashlib

import pytest
import torch

from cloud_server_amd.ops import fused as FK
from cloud_server_amd.ops.optim_ref import step_ref
from test_dense_dgrad import COUNT, EPS, _inputs, _reference

pytestmark = pytest.mark.gpu

# worst error of the parent's library against fp64 over every case below, MI355X
PARENT_DX = 2.4472e-07        # wide K=2036 N=512 M=64, sigmoid + BatchNorm C=20, SGD
PARENT_SLAB = 4.8632e-07      # wide K=2036 N=272 M=50, leaky + BatchNorm C=3, gradient mode
PARENT_W = 2.1428e-06         # wide K=2036 N=512 M=64, Adagrad
PARENT_SLOTS = 4.1456e-07     # wide K=2036 N=16 M=50, Adagrad
PARENT_BIAS = 7.3682e-07      # wide K=2036 N=16 M=64, Adam (the bias and its slots)
PARENT_DW = 3.2177e-07        # wide K=2036 N=16 M=64 (gradient mode: dW and db stored whole)
PARENT_DWH = 2.9051e-07       # flush K=256 N=256 M=50, SGD (head epilogue, store mode: dWh and dbh)
PARENT_HW = 8.2600e-07        # flush K=36 N=256 M=64, Adam (head in place: its W, b and their slots)
PARENT = lambda: dict(dX=PARENT_DX, slab=PARENT_SLAB, W=PARENT_W, slots=PARENT_SLOTS, bias=PARENT_BIAS,
                      dW=PARENT_DW, dWh=PARENT_DWH, hW=PARENT_HW)

MS = (1, 17, 50, 64)
WIDE_K, WIDE_NS = 2036, (16, 48, 272, 512)
NARROW_K, NARROW_NS = 36, (144, 256, 640, 1152)
TRANSFORMS = ((0, 0.0, 0, False), (1, 0.0, 20, True), (3, 0.2, 3, False))   # act, alpha, C, table
OPTS = (0, 1, 2, "grad")                        # SGD, Adagrad, Adam, gradient mode
LR, STEP, RING, LDIV, NC = 0.05, 3, 4, 50.0, 10
GUARD, FILL = 64, -777.0


def _lib():
    lib = FK.load()
    assert lib is not None
    return lib


class Out:
    """An output buffer between two guard regions, holding ``init`` (or zeros of ``shape``)."""

    def __init__(self, init=None, shape=None, dtype=torch.float32):
        if init is None:
            init = torch.zeros(shape, dtype=dtype, device="cuda")
        self.n = init.numel()
        self.buf = torch.full((2 * GUARD + self.n,), FILL, dtype=init.dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(init.shape)
        self.t.copy_(init)

    def intact(self):
        return bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.n:] == FILL).all())


def _hash(outs):
    h = hashlib.sha1()
    for o in outs:
        h.update(o.buf.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:12]


class Worst:
    def __init__(self):
        self.w = {}

    def add(self, q, got, ref, tag):
        e = float((got.double() - ref.reshape(got.shape)).abs().max() / ref.abs().max())
        if e > self.w.get(q, (-1.0, ""))[0]:
            self.w[q] = (e, tag)

    def finish(self, what):
        print(f"du-err {what} " + " ".join(f"{q} {e:.4e} ({tag})" for q, (e, tag) in sorted(self.w.items())))
        bounds = PARENT()
        assert all(bounds[q] is not None for q in self.w), "bounds not measured"
        bad = [f"{q} {e:.3e} > {4 * bounds[q]:.3e} ({tag})" for q, (e, tag) in self.w.items() if not e <= 4 * bounds[q]]
        assert not bad, "; ".join(bad)


def _rand(gen, *s):
    return torch.randn(*s, generator=gen, device="cuda", dtype=torch.float64)


def _slots(opt, like, gen):
    """Random optimizer slots of a parameter: accumulators and second moments >= 0.1."""
    pos = lambda: (0.1 + torch.rand(like.shape, generator=gen, device="cuda", dtype=torch.float64)).float()
    if opt == 1:
        return [pos()]
    if opt == 2:
        return [(0.5 * _rand(gen, *like.shape)).float(), pos()]
    return []


def _stepped(opt, w0, g64, s0):
    """fp64 parameter and slots after one optimizer step from fp32 ``w0`` / ``s0``."""
    w = w0.double().flatten().clone()
    s = torch.stack([t.double().flatten() for t in s0]) if s0 else w.new_zeros(0, w.numel())
    step_ref(opt, w, g64.flatten(), s, LR, STEP)
    return w, s


class Params:
    """W [K][N] and bias [N] with their slots in guarded buffers, and what one step must leave."""

    def __init__(self, opt, W0, b0, gw, gb, gen):
        self.opt, self.grad = (0, True) if opt == "grad" else (opt, False)
        sw, sb = _slots(self.opt, W0, gen), _slots(self.opt, b0, gen)
        self.W, self.b = Out(W0), Out(b0)
        self.sw, self.sb = [Out(t) for t in sw], [Out(t) for t in sb]
        self.gW, self.gb = (Out(shape=W0.shape), Out(shape=b0.shape)) if self.grad else (None, None)
        self.W0, self.gw, self.gb64 = W0, gw, gb
        if not self.grad:
            self.ref_w, self.ref_b = _stepped(self.opt, W0, gw, sw), _stepped(self.opt, b0, gb, sb)

    def outs(self):
        return [o for o in (self.W, self.b, *self.sw, *self.sb, self.gW, self.gb) if o is not None]

    def slot_ptrs(self):
        p = lambda l, k: FK.ptr(l[k].t) if k < len(l) else None
        return p(self.sw, 0), p(self.sw, 1), p(self.sb, 0), p(self.sb, 1)

    def check(self, worst, tag):
        assert all(o.intact() for o in self.outs()), f"{tag}: wrote outside a parameter buffer"
        if self.grad:
            assert torch.equal(self.W.t, self.W0), f"{tag}: gradient mode changed W"
            worst.add("dW", self.gW.t, self.gw, tag)
            worst.add("dW", self.gb.t, self.gb64, tag)
            return
        worst.add("W", self.W.t, self.ref_w[0], tag)
        worst.add("bias", self.b.t, self.ref_b[0], tag)
        for k, (o, ob) in enumerate(zip(self.sw, self.sb)):
            worst.add("slots", o.t, self.ref_w[1][k], tag)
            worst.add("bias", ob.t, self.ref_b[1][k], tag)


def _shape_inputs(M, K, N, gen):
    """Per BatchNorm width: test_dense_dgrad's operands plus Xw, the bias and the fp64 gradients."""
    ins = {}
    for C_ in sorted({t[2] for t in TRANSFORMS}):
        d = _inputs(M, K, N, C_, gen)
        d["xw"] = _rand(gen, M, K).float()
        d["bias"] = (0.1 * _rand(gen, N)).float()
        d["gw"] = d["xw"].double().t() @ d["dY"].double()
        d["gb"] = d["dY"].double().sum(0)
        ins[C_] = d
    return ins


def _bn_args(d, C_, use_tab):
    if not C_:
        return (None, 0, 0, 0.0, 0.0, None, None), None
    return ((FK.ptr(d["slab"][1]), 1, C_, COUNT, EPS, FK.ptr(d["scale"]), FK.ptr(d["offset"])),
            FK.ptr(d["tab"]) if use_tab else None)


class Workspace:
    """The partial hand-off's workspace, sized by the library; tickets start at zero."""

    def __init__(self, lib, K, N, cs):
        ws = (C.c_longlong * 2)()
        assert lib.csa_dense_bwd_update_ws(K, N, ws) == cs, "not the expected launch form"
        self.part = Out(shape=(max(int(ws[0]), 1),))
        self.cnt = Out(shape=(max(int(ws[1]), 1),), dtype=torch.int32)
        self.on = cs > 1

    def ptrs(self):
        return (FK.ptr(self.part.t), FK.ptr(self.cnt.t)) if self.on else (None, None)

    def check(self, tag):
        assert self.part.intact() and self.cnt.intact(), f"{tag}: wrote outside the workspace"
        assert not bool(self.cnt.t.any()), f"{tag}: arrival tickets not back at zero"


def _fused(lib, d, p, wsp, M, K, N, tr, rows, step):
    """One fused backward launch; returns the guarded dX and slab (None without BatchNorm)."""
    act, alpha, C_, use_tab = tr
    dX = Out(shape=(M, K))
    slab = Out(shape=(rows, 2, C_)) if C_ else None
    bn, tab = _bn_args(d, C_, use_tab)
    common = (M, K, N, FK.ptr(d["x"]), act, alpha, *bn, FK.ptr(slab.t) if slab else None, FK.ptr(d["xw"]))
    if p.grad:
        rc = lib.csa_dense_bwd_grad_head(FK.ptr(d["dY"]), FK.ptr(p.W.t), FK.ptr(dX.t), *common, 1.0, tab, *wsp.ptrs(),
                                         FK.ptr(p.gW.t), FK.ptr(p.gb.t), None, None, None, None, None, None, None,
                                         None, 1, 1.0, 0, 0.0, FK.ptr(step), FK.stream())
    else:
        rc = lib.csa_dense_bwd_update(FK.ptr(d["dY"]), FK.ptr(p.W.t), FK.ptr(p.b.t), FK.ptr(dX.t), *common, p.opt, LR,
                                      FK.ptr(step), *p.slot_ptrs(), 1.0, tab, *wsp.ptrs(), FK.stream())
    assert rc == 0, rc
    return dX, slab


def _check_dx(worst, dX, slab, ref, tot, tag):
    assert dX.intact() and (slab is None or slab.intact()), f"{tag}: wrote outside dX or the slab"
    worst.add("dX", dX.t, ref, tag)
    if slab is not None:
        worst.add("slab", slab.t.double().sum(0), tot, tag)


def _fused_case(what, K, N, M, cs):
    lib = _lib()
    assert lib.csa_dense_bwd_update_ok(M, K, N, 20) == 1
    gen = torch.Generator(device="cuda").manual_seed(K * 1000 + N * 7 + M)
    ins = _shape_inputs(M, K, N, gen)
    wsp = Workspace(lib, K, N, cs)
    step = torch.tensor([STEP], dtype=torch.int64, device="cuda")
    worst = Worst()
    prev_det = int(lib.csa_deterministic())
    try:
        for det in (0, 1):
            lib.csa_set_deterministic(det)
            rows = int(lib.csa_dense_bwd_update_slabs(K))
            for tr in TRANSFORMS:
                d = ins[tr[2]]
                ref, tot = _reference(d, tr[2], tr[3], tr[0], tr[1], 1)
                for opt in OPTS:
                    tag = f"K{K}-N{N}-M{M}-det{det}-act{tr[0]}-C{tr[2]}-opt{opt}"
                    hashes = []
                    for rep in range(2 if det else 1):
                        pgen = torch.Generator(device="cuda").manual_seed(N + M + 17 * OPTS.index(opt))
                        p = Params(opt, d["W"], d["bias"], d["gw"], d["gb"], pgen)
                        dX, slab = _fused(lib, d, p, wsp, M, K, N, tr, rows, step)
                        wsp.check(tag)
                        hashes.append(_hash([dX, *p.outs()] + ([slab] if det and slab else [])))
                    _check_dx(worst, dX, slab, ref, tot, tag)
                    p.check(worst, tag)
                    assert len(set(hashes)) == 1, f"{tag}: two deterministic calls differ"
                    print(f"du-hash {what} {tag} {hashes[0]}")
    finally:
        lib.csa_set_deterministic(prev_det)
    worst.finish(f"{what} K={K} N={N} M={M}")


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", WIDE_NS)
def test_wide_update(N, M):
    _fused_case("wide", WIDE_K, N, M, 1)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NARROW_NS)
def test_narrow_update(N, M):
    _fused_case("narrow", NARROW_K, N, M, (N + 127) // 128)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NARROW_NS)
def test_narrow_dgrad(N, M):
    """The input gradient alone on the narrow shapes; two calls share one workspace."""
    lib, K = _lib(), NARROW_K
    gen = torch.Generator(device="cuda").manual_seed(K * 1000 + N * 7 + M)
    ins = _shape_inputs(M, K, N, gen)
    wsp = Workspace(lib, K, N, (N + 127) // 128)
    worst = Worst()
    prev_det = int(lib.csa_deterministic())
    try:
        for det in (0, 1):
            lib.csa_set_deterministic(det)
            rows = int(lib.csa_dense_bwd_update_slabs(K))
            for act, alpha, C_, use_tab in TRANSFORMS:
                d = ins[C_]
                tag = f"K{K}-N{N}-M{M}-det{det}-act{act}-C{C_}"
                ref, tot = _reference(d, C_, use_tab, act, alpha, 1)
                bn, tab = _bn_args(d, C_, use_tab)
                got = []
                for rep in range(2):
                    dX = Out(shape=(M, K))
                    slab = Out(shape=(rows, 2, C_)) if C_ else None
                    rc = lib.csa_dense_bwd_dgrad(FK.ptr(d["dY"]), FK.ptr(d["W"]), FK.ptr(dX.t), M, K, N, FK.ptr(d["x"]),
                                                 act, alpha, *bn, FK.ptr(slab.t) if slab else None, tab, *wsp.ptrs(),
                                                 FK.stream())
                    assert rc == 0, rc
                    wsp.check(tag)
                    _check_dx(worst, dX, slab, ref, tot, tag)
                    got.append((dX, slab))
                assert torch.equal(got[0][0].buf, got[1][0].buf), f"{tag}: dX differs between two calls"
                assert not (det and slab) or torch.equal(got[0][1].buf, got[1][1].buf), f"{tag}: slab differs"
                print(f"du-hash dgrad {tag} {_hash([dX] + ([slab] if det and slab else []))}")
    finally:
        lib.csa_set_deterministic(prev_det)
    worst.finish(f"dgrad K={K} N={N} M={M}")


def _act64(v, act, alpha):
    if act == 1:
        return torch.sigmoid(v)
    return torch.where(v >= 0, v, alpha * v) if act == 3 else v


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", (128, 256))
@pytest.mark.parametrize("K", (36, 256))
def test_deferred_flush(K, N, M):
    """Deferred segments launched on their own: no head, head stored, head applied in place."""
    lib = _lib()
    gen = torch.Generator(device="cuda").manual_seed(K * 1000 + N * 7 + M)
    dY, xw = _rand(gen, M, N).float(), _rand(gen, M, K).float()
    W0, b0 = (_rand(gen, K, N) / N ** 0.5).float(), (0.1 * _rand(gen, N)).float()
    gw, gb = xw.double().t() @ dY.double(), dY.double().sum(0)
    # the head: this layer's output hy, the scaled dlogits, the per-row loss and hit
    hy = (torch.where(_rand(gen, M, N) < 0, -1.0, 1.0) * (0.02 + _rand(gen, M, N).abs())).float()
    dl = (_rand(gen, M, NC) / M).float()
    hrl = (0.1 + torch.rand(M, generator=gen, device="cuda")).float()
    hrc = (torch.rand(M, generator=gen, device="cuda") < 0.5).int()
    hW0, hb0 = (_rand(gen, N, NC) / N ** 0.5).float(), (0.1 * _rand(gen, NC)).float()
    step = torch.tensor([STEP], dtype=torch.int64, device="cuda")
    pos = (STEP - 1) % RING
    worst = Worst()
    assert lib.csa_dense_update_pending() == 0
    try:
        for head, hact, halpha in ((None, 0, 0.0), ("store", 1, 0.0), ("inplace", 3, 0.2)):
            gwh = _act64(hy.double(), hact, halpha).t() @ dl.double()
            gbh = dl.double().sum(0)
            for opt in OPTS:
                if opt == "grad" and head != "store":       # gradient mode once, as data parallel runs it
                    continue
                tag = f"K{K}-N{N}-M{M}-head{head}-opt{opt}"
                pgen = torch.Generator(device="cuda").manual_seed(N + M + 17 * OPTS.index(opt))
                p = Params(opt, W0, b0, gw, gb, pgen)
                hp = Params(p.opt, hW0, hb0, gwh, gbh, pgen)          # the head's parameters (in place)
                hgw, hgb = Out(shape=(N, NC)), Out(shape=(NC,))
                hgw.t.fill_(FILL), hgb.t.fill_(FILL)
                rl = Out(torch.full((RING,), FILL, device="cuda"))
                rc_ = Out(torch.full((RING,), int(FILL), dtype=torch.int32, device="cuda"))
                hargs = ((FK.ptr(hy), FK.ptr(dl), FK.ptr(hgw.t), FK.ptr(hgb.t), FK.ptr(hrl), FK.ptr(hrc), FK.ptr(rl.t),
                          FK.ptr(rc_.t), RING, LDIV, hact, halpha) if head else (None,) * 8 + (1, 1.0, 0, 0.0))
                rc = lib.csa_dense_update_defer(FK.ptr(dY), FK.ptr(p.W.t), FK.ptr(p.b.t), M, K, N, FK.ptr(xw), p.opt, LR,
                                                FK.ptr(step), *p.slot_ptrs(), 1.0, *hargs)
                assert rc == 1, rc
                if p.grad:
                    assert lib.csa_dense_update_grad_mode(FK.ptr(p.gW.t), FK.ptr(p.gb.t)) == 0
                if head == "inplace":
                    sp = hp.slot_ptrs()
                    assert lib.csa_dense_update_head_params(FK.ptr(hp.W.t), FK.ptr(hp.b.t), sp[0], sp[1], sp[2], sp[3]) == 0
                assert lib.csa_dense_update_pending() == 1
                assert lib.csa_dense_update_flush(FK.stream()) == 0
                assert lib.csa_dense_update_pending() == 0, f"{tag}: a segment is left"
                p.check(worst, tag)
                heads = [hgw, hgb, rl, rc_, *hp.outs()]
                assert all(o.intact() for o in heads), f"{tag}: wrote outside a head buffer"
                if head:
                    live = torch.arange(RING, device="cuda") == pos
                    assert bool((rl.t[~live] == FILL).all()) and bool((rc_.t[~live] == int(FILL)).all()), \
                        f"{tag}: another ring entry written"
                    want = float(hrl.double().sum() / LDIV)
                    # M <= 64 positive fp32 terms summed in any order, then one division
                    assert abs(float(rl.t[pos]) - want) <= 65 * 2.0 ** -24 * want, f"{tag}: ring loss"
                    assert int(rc_.t[pos]) == int(hrc.sum()), f"{tag}: ring hits"
                else:
                    assert bool((rl.t == FILL).all()) and bool((rc_.t == int(FILL)).all()), f"{tag}: ring written"
                if head == "store":
                    worst.add("dWh", hgw.t, gwh, tag)
                    worst.add("dWh", hgb.t, gbh, tag)
                else:
                    assert bool((hgw.t == FILL).all()) and bool((hgb.t == FILL).all()), f"{tag}: dWh / dbh written"
                if head == "inplace":
                    worst.add("hW", hp.W.t, hp.ref_w[0], tag)
                    worst.add("hW", hp.b.t, hp.ref_b[0], tag)
                    for k, (o, ob) in enumerate(zip(hp.sw, hp.sb)):
                        worst.add("hW", o.t, hp.ref_w[1][k], tag)
                        worst.add("hW", ob.t, hp.ref_b[1][k], tag)
                else:
                    assert torch.equal(hp.W.t, hW0) and torch.equal(hp.b.t, hb0), f"{tag}: head parameters changed"
                print(f"du-hash flush {tag} {_hash(p.outs() + heads)}")
    finally:
        lib.csa_dense_update_clear()
    worst.finish(f"flush K={K} N={N} M={M}")
