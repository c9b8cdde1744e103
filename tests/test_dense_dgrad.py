"""The wide dense input-gradient launch (``csa_dense_bwd_dgrad``, one workgroup per 16 input
features) against an fp64 computation done here (GPU only).

The entry point is called directly on random inputs.  What it must produce:

    g      = dY @ W^T                                   [M][K]
    z      = x * a[ch] + b[ch]   (BatchNorm of the input, ch = f % C)   or   z = x
    dX     = act'(z) * g                                (the gradient at z)
    slab   = per channel {sum_m,f dX, sum_m,f dX * (x - mean[ch]) * rstd[ch]}

Shapes: every (K, N, M) of K in {2036, 2048, 2320} (a last group of 12 features; exactly 128
groups, the least that takes the wide path; 145 groups, so ``grp % 16`` wraps), N in
{16, 48, 272, 512} (one chunk; reduction quarters of unequal length; the full case) and M in
{1, 17, 50, 64}.  Every shape runs every activation (none, sigmoid, leaky) with BatchNorm
off, on with C = 20 and on with C = 3 (a channel wraps inside a feature quad), each BatchNorm
case with and without the precomputed table, in atomic and in deterministic mode; in
deterministic mode a second call must reproduce the first bit for bit.  dX lives inside a
larger buffer whose other elements must keep their fill value.

The forward statistics arrive as 3 partial rows in atomic mode and, as in the program, as
one row already folded in deterministic mode: a workgroup folds the rows it is given with
LDS atomics, whose order is free, so only a single row is reproducible without the table.

Inputs keep |z| >= 0.02, away from the kink of the leaky activation: there the derivative
jumps, and a z that rounds across it in fp32 is not an error of the kernel.

Bounds.  The same inputs ran through the parent's kernel (``dense_bwd_update<0,16,false,true>``
in ``du_body``) on an MI355X; figures are errors against fp64, dX relative to max |dX| of the
case, the slab totals relative to their largest magnitude.  Parent, worst of all 1440 cases:
see PARENT_DX / PARENT_SLAB (profiles/r10_notes.md).  The bound is 4 x the parent's figure.
"""
import ctypes as C

import pytest
import torch

from cloud_server_amd.ops import fused as FK

pytestmark = pytest.mark.gpu

# worst error of the parent's kernel against fp64 over every case below, MI355X
PARENT_DX = 2.9159e-07        # K=2320 N=272 M=17
PARENT_SLAB = 1.1634e-06      # K=2048 N=512 M=50

KS, NS, MS = (2036, 2048, 2320), (16, 48, 272, 512), (1, 17, 50, 64)
ACTS = ((0, 0.0), (1, 0.0), (3, 0.2))            # none, sigmoid, leaky(alpha)
BNS = ((0, False), (20, True), (20, False), (3, True), (3, False))   # (C, precomputed table)
EPS, NSLAB, COUNT = 1e-3, 3, 800.0
GUARD, FILL = 64, -777.0


def _lib():
    lib = FK.load()
    assert lib is not None
    return lib


def _inputs(M, K, N, C_, gen):
    """Operands of one (shape, C): fp32 tensors and the fp64 statistics derived from them."""
    dev = "cuda"
    r = lambda *s: torch.randn(*s, generator=gen, device=dev, dtype=torch.float64)
    dY = r(M, N).float()
    W = (r(K, N) / N ** 0.5).float()
    sign = torch.where(r(M, K) < 0, -1.0, 1.0)
    z = sign * (0.02 + r(M, K).abs())
    d = dict(dY=dY, W=W, g=dY.double() @ W.double().t())
    if not C_:
        d["x"] = z.float()
        return d
    # forward statistics as NSLAB partial rows {sum x, sum x^2}; mean 0.3 +- 0.2, var 0.5 .. 1.5
    mean = 0.3 + 0.2 * r(C_).clamp(-2, 2)
    var = 0.5 + torch.rand(C_, generator=gen, device=dev, dtype=torch.float64)
    tot = torch.stack([mean * COUNT, (var + mean * mean) * COUNT])            # [2][C]
    w = torch.rand(NSLAB, 1, 1, generator=gen, device=dev, dtype=torch.float64) + 0.5
    slab = (tot[None] * (w / w.sum())).float().contiguous()                   # [NSLAB][2][C]
    scale = (0.5 + torch.rand(C_, generator=gen, device=dev, dtype=torch.float64)).float()
    offset = (0.3 * r(C_)).float()
    slab1 = slab.double().sum(0).float()[None].contiguous()                   # the rows folded: [1][2][C]

    def stats(rows):
        s = rows.double().sum(0)
        m = s[0] / COUNT
        rstd = ((s[1] / COUNT - m * m).clamp_min(0) + EPS).rsqrt()
        a = scale.double() * rstd
        return m, rstd, a, offset.double() - m * a

    st1 = stats(slab1)
    tab = torch.stack(st1).float().contiguous()                               # [4][C]
    ch = torch.arange(K, device=dev) % C_
    x = ((z - st1[3][ch]) / st1[2][ch]).float()
    d.update(x=x, slab=(slab, slab1), scale=scale, offset=offset, tab=tab, ch=ch, stats64=(stats(slab), st1))
    return d


def _reference(d, C_, use_tab, act, alpha, det):
    x = d["x"].double()
    if C_:
        m, rs, a, b = [t.double() for t in d["tab"]] if use_tab else d["stats64"][det]
        ch = d["ch"]
        z = x * a[ch] + b[ch]
    else:
        z = x
    g = d["g"]
    if act == 1:
        y = torch.sigmoid(z)
        g = g * y * (1 - y)
    elif act == 3:
        g = torch.where(z >= alpha * z, g, g * alpha)
    if not C_:
        return g, None
    v = torch.stack([g.sum(0), (g * (x - m[ch]) * rs[ch]).sum(0)])            # [2][K]
    tot = torch.zeros(2, C_, dtype=torch.float64, device=g.device).index_add_(1, ch, v)
    return g, tot


def _call(lib, d, M, K, N, C_, use_tab, act, alpha, rows, det):
    buf = torch.full((GUARD + M * K + GUARD,), FILL, device="cuda")
    dX = buf[GUARD:GUARD + M * K]
    bslab = torch.zeros(rows, 2, max(C_, 1), device="cuda") if C_ else None
    bn = ((FK.ptr(d["slab"][det]), 1 if det else NSLAB, C_, COUNT, EPS, FK.ptr(d["scale"]), FK.ptr(d["offset"])) if C_
          else (None, 0, 0, 0.0, 0.0, None, None))
    rc = lib.csa_dense_bwd_dgrad(FK.ptr(d["dY"]), FK.ptr(d["W"]), FK.ptr(dX), M, K, N, FK.ptr(d["x"]), act, alpha,
                                 *bn, FK.ptr(bslab), FK.ptr(d["tab"]) if C_ and use_tab else None, None, None,
                                 FK.stream())
    assert rc == 0, rc
    return buf, bslab


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_dgrad_matches_fp64(K, N, M):
    lib = _lib()
    ws = (C.c_longlong * 2)()
    assert lib.csa_dense_bwd_update_ok(M, K, N, 20) == 1
    assert lib.csa_dense_bwd_update_ws(K, N, ws) == 1, "not the wide (one workgroup per row group) path"
    gen = torch.Generator(device="cuda").manual_seed(K * 1000 + N * 7 + M)
    ins = {C_: _inputs(M, K, N, C_, gen) for C_ in (0, 20, 3)}
    worst_dx = worst_slab = 0.0
    fails = []
    prev_det = int(lib.csa_deterministic())
    try:
        for det in (0, 1):
            lib.csa_set_deterministic(det)
            rows = int(lib.csa_dense_bwd_update_slabs(K))
            assert rows == ((K + 15) // 16 if det else 16)
            for C_, use_tab in BNS:
                d = ins[C_]
                for act, alpha in ACTS:
                    tag = f"det{det}-C{C_}{'t' if use_tab else 's'}-act{act}"
                    ref, tot = _reference(d, C_, use_tab, act, alpha, det)
                    buf, bslab = _call(lib, d, M, K, N, C_, use_tab, act, alpha, rows, det)
                    got = buf[GUARD:GUARD + M * K].view(M, K).double()
                    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + M * K:] == FILL).all()), \
                        f"{tag}: wrote outside [M][K]"
                    e_dx = float((got - ref).abs().max() / ref.abs().max())
                    e_sl = 0.0
                    if C_:
                        e_sl = float((bslab.double().sum(0) - tot).abs().max() / tot.abs().max())
                    if det:
                        buf2, bslab2 = _call(lib, d, M, K, N, C_, use_tab, act, alpha, rows, det)
                        assert torch.equal(buf, buf2), f"{tag}: dX differs between two deterministic calls"
                        assert bslab is None or torch.equal(bslab, bslab2), f"{tag}: slab differs between calls"
                    worst_dx, worst_slab = max(worst_dx, e_dx), max(worst_slab, e_sl)
                    if PARENT_DX is not None and not (e_dx <= 4 * PARENT_DX and e_sl <= 4 * PARENT_SLAB):
                        fails.append(f"{tag}: dX {e_dx:.3e} slab {e_sl:.3e}")
    finally:
        lib.csa_set_deterministic(prev_det)
    print(f"dgrad-err K={K} N={N} M={M} dX {worst_dx:.4e} slab {worst_slab:.4e}")
    assert PARENT_DX is not None and PARENT_SLAB is not None, "bounds not measured"
    assert not fails, f"bound dX {4 * PARENT_DX:.3e} slab {4 * PARENT_SLAB:.3e}: " + "; ".join(fails[:6])
