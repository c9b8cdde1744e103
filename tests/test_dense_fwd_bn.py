"""The dense forward with the producer's BatchNorm + activation applied on load
(``csa_dd_fwd_bn``) against an fp64 computation done here (GPU only).

One launch must produce what ``csa_bn_act_apply`` followed by ``csa_dd_fwd`` produce:

    (a, b)[c] from the statistic slab [nslab][2][C]     mean, var = max(E[x^2] - mean^2, 0),
                                                        rstd, a = scale * rstd, b = offset - mean * a
    xt = act(X * a[c] + b[c]),  c = k % C               [M][K]
    Y  = xt @ W + bias                                  [M][N]
    tab = mean | rstd | a | b                           [4][C]
    the armed pending-flag word = 0

The fp64 reference starts from the same slab (its rows summed in fp64).  The slab holds
well-conditioned statistics drawn here (mean in [-0.5, 0.5], variance in [0.5, 2]) split over
its rows, not the statistics of X: with the two-element channels of the smallest shapes the
fp32 difference E[x^2] - mean^2 would otherwise decide the figures, in both forms alike.

Shapes (K, C), K % C == 0: (40, 20) fewer 8-k blocks than waves; (60, 3) and (100, 5) a float4
wrapping a channel boundary; (136, 1) one channel; (520, 20) unequal wave ranges and a cut last
block; (1024, 128) the largest C; (3920, 20) fc1 - crossed with N in {16, 40, 512}, M in
{1, 17, 33, 50}, and (3920, 20, 512) at M = 100 (four batch blocks, two load groups per wave).
Every shape runs with nslab in {1, 32, 45}, every activation (none, sigmoid, leaky 0.2), with
and without bias.

X, xt, Y, tab and the flag word live inside guard-filled buffers: nothing outside them may
change, every live element of xt must overwrite its sentinel, and Y (an accumulator where
``csa_dd_fwd_splits`` answers more than 1) starts at zero or at a sentinel as the program
would have it.

Bound.  Every case also runs through the two launches the fused form replaces
(``csa_bn_act_apply`` + ``csa_dd_fwd``, same library).  Their worst errors against fp64 on an
MI355X, relative to the largest magnitude of the array (of the table row) in the case, are
PAIR_Y, PAIR_XT and PAIR_TAB below (profiles/r14_notes.md); the bound on the fused form is
4 x each, as in test_dense_fwd.py: the order of the atomic adds varies from run to run, and
the slab is folded in another order.
"""
import copy

import pytest
import torch

from cloud_server_amd.ops import fused as FK

pytestmark = pytest.mark.gpu

# worst error of csa_bn_act_apply + csa_dd_fwd against fp64 over every case below, MI355X
PAIR_Y = 3.7510e-07             # K=3920 C=20 N=40 M=50
PAIR_XT = 1.8512e-07            # K=1024 C=128 N=512 M=1
PAIR_TAB = 4.7533e-07           # K=60 C=3 N=512 M=33
# (the fused form in the same run: Y 3.4599e-07, xt 2.1258e-07, tab 4.0823e-07)

KCS = ((40, 20), (60, 3), (100, 5), (136, 1), (520, 20), (1024, 128), (3920, 20))
NS, MS = (16, 40, 512), (1, 17, 33, 50)
SHAPES = [(K, C, N, M) for K, C in KCS for N in NS for M in MS] + [(3920, 20, 512, 100)]
NSLABS = (1, 32, 45)
ACTS = ((0, 0.0), (1, 0.0), (3, 0.2))            # none, sigmoid, leaky(alpha)
GUARD, FILL, SENTINEL, EPS = 64, -777.0, 12345.0, 1e-3


def _lib():
    lib = FK.load()
    assert lib is not None
    return lib


class _Profile:
    """Set one profile flag for the calls inside; the flags found are put back."""

    def __init__(self, lib, name):
        self.lib, self.name = lib, name

    def __enter__(self):
        lib = self.lib
        self.prev = (int(lib.csa_deterministic()), int(lib.csa_packed()), int(lib.csa_shared_gpu()))
        lib.csa_set_deterministic(1 if self.name == "det" else 0)
        lib.csa_set_packed(1 if self.name == "packed" else 0)
        lib.csa_set_shared_gpu(0)

    def __exit__(self, *exc):
        lib = self.lib
        lib.csa_set_deterministic(self.prev[0])
        lib.csa_set_packed(self.prev[1])
        lib.csa_set_shared_gpu(self.prev[2])


def _act64(x, act, alpha):
    if act == 1:
        return torch.sigmoid(x)
    if act == 3:
        return torch.where(x >= 0, x, alpha * x)
    return x


def _guarded(n, fill=FILL, dtype=torch.float32):
    """(buffer, view of its n live elements): GUARD elements of ``fill`` on either side."""
    buf = torch.full((GUARD + n + GUARD,), fill, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _guards_ok(buf, n, fill=FILL):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


class _Case:
    """Operands of one shape and its fp64 references per (nslab, act)."""

    def __init__(self, K, C, N, M, seed=None):
        gen = torch.Generator(device="cuda").manual_seed(seed if seed is not None else K * 1000 + C * 31 + N * 7 + M)
        r = lambda *s: torch.randn(*s, generator=gen, device="cuda", dtype=torch.float64)
        u = lambda *s: torch.rand(*s, generator=gen, device="cuda", dtype=torch.float64)
        self.K, self.C, self.N, self.M = K, C, N, M
        self.xbuf, xv = _guarded(M * K)
        xv.copy_((r(M, K) + 0.3).float().view(-1))
        self.X = xv.view(M, K)
        self.W = (r(K, N) / K ** 0.5).float()
        self.bias = r(N).float()
        self.scale = (0.5 + u(C)).float()
        self.offset = (r(C) * 0.3).float()
        self.count = float(M * (K // C))
        mean, var = u(C) - 0.5, 0.5 + 1.5 * u(C)
        self.tot = torch.stack([mean, var + mean * mean]) * self.count        # [2][C] sum x | sum x^2
        self.gen = gen
        self.slabs, self.refs = {}, {}

    def slab(self, nslab):
        """[nslab][2][C] fp32 rows whose sum is about ``tot``, and the fp64 table of THESE rows."""
        if nslab not in self.slabs:
            w = 0.2 + torch.rand(nslab, 1, 1, generator=self.gen, device="cuda", dtype=torch.float64)
            s = (self.tot[None] * (w / w.sum())).float().contiguous()
            tot = s.double().sum(0)
            mean = tot[0] / self.count
            var = (tot[1] / self.count - mean * mean).clamp_min(0.0)
            rstd = (var + EPS).rsqrt()
            a = self.scale.double() * rstd
            b = self.offset.double() - mean * a
            self.slabs[nslab] = (s, torch.stack([mean, rstd, a, b]))
        return self.slabs[nslab]

    def ref(self, nslab, act, alpha):
        if (nslab, act) not in self.refs:
            tab = self.slab(nslab)[1]
            ch = torch.arange(self.K, device="cuda") % self.C
            xt = _act64(self.X.double() * tab[2][ch] + tab[3][ch], act, alpha)
            self.refs[(nslab, act)] = (xt, xt @ self.W.double())
        return self.refs[(nslab, act)]


class _Out:
    def __init__(self, c, lib, flag):
        M, N, K, C = c.M, c.N, c.K, c.C
        splits = int(lib.csa_dd_fwd_splits(M, N, K))
        assert splits >= 1
        self.ybuf, self.y = _guarded(M * N)
        self.y.fill_(0.0 if splits > 1 else SENTINEL)
        self.xtbuf, self.xt = _guarded(M * K)
        self.xt.fill_(SENTINEL)
        self.tabbuf, self.tab = _guarded(4 * C)
        self.flagbuf, self.flag = _guarded(1, 7, torch.int32)
        self.armed = flag

    def check_bounds(self, c, tag):
        assert _guards_ok(c.xbuf, c.M * c.K), f"{tag}: wrote around X"
        assert _guards_ok(self.ybuf, c.M * c.N), f"{tag}: wrote outside Y [M][N]"
        assert _guards_ok(self.xtbuf, c.M * c.K), f"{tag}: wrote outside xt [M][K]"
        assert _guards_ok(self.tabbuf, 4 * c.C), f"{tag}: wrote outside tab [4][C]"
        assert _guards_ok(self.flagbuf, 1, 7), f"{tag}: wrote beside the flag word"
        assert int(self.flag.item()) == (0 if self.armed else 7), f"{tag}: flag word {int(self.flag.item())}"
        assert not bool((self.xt == SENTINEL).any()), f"{tag}: live xt elements not written"

    def errs(self, c, ref_xt, ref_y, ref_tab):
        M, N, K, C = c.M, c.N, c.K, c.C
        ey = float((self.y.view(M, N).double() - ref_y).abs().max() / ref_y.abs().max())
        ex = float((self.xt.view(M, K).double() - ref_xt).abs().max() / ref_xt.abs().max())
        d = (self.tab.view(4, C).double() - ref_tab).abs().amax(1) / ref_tab.abs().amax(1)
        return ey, ex, float(d.max())


def _bn_args(c, slab):
    return (FK.ptr(slab), slab.shape[0], c.count, EPS, FK.ptr(c.scale), FK.ptr(c.offset))


def _fused(lib, c, nslab, act, alpha, b, flag=True):
    o = _Out(c, lib, flag)
    slab = c.slab(nslab)[0]
    rc = lib.csa_dd_fwd_bn(FK.ptr(c.X), FK.ptr(c.W), FK.ptr(b), FK.ptr(o.y), c.M, c.N, c.K, c.C, *_bn_args(c, slab),
                           act, alpha, FK.ptr(o.xt), FK.ptr(o.tab), FK.ptr(o.flag) if flag else None, FK.stream())
    assert rc == 0, rc
    return o


def _pair(lib, c, nslab, act, alpha, b, flag=True):
    """The two launches the fused form replaces."""
    o = _Out(c, lib, flag)
    slab = c.slab(nslab)[0]
    if flag:
        lib.csa_ew_clear_next(FK.ptr(o.flag))
    rc = lib.csa_bn_act_apply(FK.ptr(c.X), FK.ptr(o.xt), c.M * c.K, c.C, *_bn_args(c, slab), act, alpha,
                              FK.ptr(o.tab), FK.stream())
    assert rc == 0, rc
    rc = lib.csa_dd_fwd(FK.ptr(o.xt), FK.ptr(c.W), FK.ptr(b), FK.ptr(o.y), c.M, c.N, c.K, 0, 0.0, FK.stream())
    assert rc == 0, rc
    return o


@pytest.mark.parametrize("K,C,N,M", SHAPES)
def test_fwd_bn_matches_fp64(K, C, N, M):
    lib = _lib()
    c = _Case(K, C, N, M)
    worst = {"fused": [0.0, 0.0, 0.0], "pair": [0.0, 0.0, 0.0]}
    fails = []
    with _Profile(lib, "default"):
        assert lib.csa_dd_fwd_bn_ok(M, N, K, C) == 1
        for nslab in NSLABS:
            ref_tab = c.slab(nslab)[1]
            for act, alpha in ACTS:
                ref_xt, ref_y0 = c.ref(nslab, act, alpha)
                for b in (c.bias, None):
                    tag = f"nslab{nslab}-act{act}-{'b' if b is not None else 'nob'}"
                    ref_y = ref_y0 + (b.double() if b is not None else 0.0)
                    for form, run in (("fused", _fused), ("pair", _pair)):
                        o = run(lib, c, nslab, act, alpha, b)
                        o.check_bounds(c, f"{form}-{tag}")
                        e = o.errs(c, ref_xt, ref_y, ref_tab)
                        worst[form] = [max(p, q) for p, q in zip(worst[form], e)]
                        if form == "fused" and None not in (PAIR_Y, PAIR_XT, PAIR_TAB):
                            if not (e[0] <= 4 * PAIR_Y and e[1] <= 4 * PAIR_XT and e[2] <= 4 * PAIR_TAB):
                                fails.append(f"{tag}: Y {e[0]:.3e} xt {e[1]:.3e} tab {e[2]:.3e}")
    print(f"fwdbn-err K={K} C={C} N={N} M={M} " + " ".join(
        f"{f} Y {w[0]:.4e} xt {w[1]:.4e} tab {w[2]:.4e}" for f, w in worst.items()))
    assert None not in (PAIR_Y, PAIR_XT, PAIR_TAB), "bound not measured"
    assert not fails, (f"bounds Y {4 * PAIR_Y:.3e} xt {4 * PAIR_XT:.3e} tab {4 * PAIR_TAB:.3e}: "
                       + "; ".join(fails[:6]))


def test_unarmed_flag_is_left_alone():
    """Without an armed word the launch writes no flag; tab is optional too."""
    lib = _lib()
    c = _Case(520, 20, 40, 33)
    with _Profile(lib, "default"):
        o = _fused(lib, c, 32, 1, 0.0, c.bias, flag=False)
        o.check_bounds(c, "unarmed")
        o2 = _Out(c, lib, False)
        slab = c.slab(32)[0]
        rc = lib.csa_dd_fwd_bn(FK.ptr(c.X), FK.ptr(c.W), FK.ptr(c.bias), FK.ptr(o2.y), c.M, c.N, c.K, c.C,
                               *_bn_args(c, slab), 1, 0.0, FK.ptr(o2.xt), None, None, FK.stream())
        assert rc == 0, rc
        assert bool((o2.tabbuf == FILL).all()), "tab written without a tab pointer"
        assert torch.equal(o2.xt, o.xt)


@pytest.mark.parametrize("K,C,N,M", [(3920, 20, 512, 50), (3920, 20, 512, 100), (1024, 128, 512, 33), (100, 5, 40, 17)])
def test_every_tile_derives_the_same_table(K, C, N, M):
    """Activation none, W = 0 but for one 1 per column: the atomically summed Y[m][n] is then
    exactly the xt[m][k_n] that column n's tile transformed for itself, and must equal the
    stored xt (written by ONE tile) bit for bit - every workgroup derived the same (a, b)."""
    lib = _lib()
    c = _Case(K, C, N, M)
    with _Profile(lib, "default"):
        for rnd, nslab in enumerate(NSLABS):
            kn = (torch.arange(N, device="cuda") * 7919 + 13 * rnd) % K
            c.W.zero_()
            c.W[kn, torch.arange(N, device="cuda")] = 1.0
            o = _fused(lib, c, nslab, 0, 0.0, None)
            o.check_bounds(c, f"onehot-{nslab}")
            got, want = o.y.view(M, N), o.xt.view(M, K)[:, kn]
            assert torch.equal(got, want), f"nslab {nslab}: {int((got != want).sum())} elements differ between tiles"


def test_predicate():
    lib = _lib()
    with _Profile(lib, "default"):
        assert lib.csa_dd_fwd_bn_ok(50, 512, 3920, 20) == 1
        assert lib.csa_dd_fwd_bn_ok(50, 512, 3918, 3) == 0          # K % 4 != 0
        assert lib.csa_dd_fwd_bn_ok(50, 512, 3920, 32) == 0         # K % C != 0
        assert lib.csa_dd_fwd_bn_ok(50, 512, 2580, 129) == 0        # C > 128
        assert lib.csa_dd_fwd_bn_ok(50, 512, 3920, 0) == 0
    for prof in ("packed", "det"):
        with _Profile(lib, prof):
            assert lib.csa_dd_fwd_bn_ok(50, 512, 3920, 20) == 0, prof
            c = _Case(40, 20, 16, 1)
            o = _Out(c, lib, False)
            rc = lib.csa_dd_fwd_bn(FK.ptr(c.X), FK.ptr(c.W), None, FK.ptr(o.y), 1, 16, 40, 20,
                                   *_bn_args(c, c.slab(1)[0]), 0, 0.0, FK.ptr(o.xt), None, None, FK.stream())
            assert rc < 0, (prof, rc)                                # refused, not run in another form


def test_engine_plans_the_fused_forward(monkeypatch):
    """The sample program runs fc1's forward as the fused launch by default and as the two
    launches under CSA_FWD_BN_FUSE=0; six steps of the two agree within the bound
    test_hip_step.py uses for two atomic-mode runs of one program (graph replay against eager:
    3e-3 on the parameters, Adagrad, lr 0.01)."""
    from cloud_server_amd.data.datasets import synthetic_mnist
    from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config
    from cloud_server_amd.runtime.engine import TrainEngine

    cf = copy.deepcopy(SAMPLE_CONFIG)
    cf.update(optimizer_name="AdagradOptimizer", learning_rate=0.01, options={"batch_size": 50})
    cfg = parse_train_config(cf)
    ds = synthetic_mnist(500, seed=7)
    monkeypatch.delenv("CSA_FWD_BN_FUSE", raising=False)
    a = TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=True)
    monkeypatch.setenv("CSA_FWD_BN_FUSE", "0")
    b = TrainEngine(cfg, ds, device="cuda", backend="hip", use_graph=True)
    monkeypatch.delenv("CSA_FWD_BN_FUSE", raising=False)
    da = [u for u in a.program.units if u.kind == "dense"]
    db = [u for u in b.program.units if u.kind == "dense"]
    assert da[0].xt is not None and da[0].fwd_bn, "fc1's forward is not planned as the fused launch"
    assert [u.fwd_bn for u in da[1:]] == [False] * (len(da) - 1)     # no BatchNorm in front of fc2
    assert [u.fwd_bn for u in db] == [False] * len(db)
    for _ in range(6):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert int(a.dstep.item()) == int(b.dstep.item()) == 6
    d = (a.flat - b.flat).abs().max().item()
    print(f"fused vs two launches, 6 steps: max |dparam| {d:.3e}")
    assert d < 3e-3, d
