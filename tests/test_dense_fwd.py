"""The dense forward (``csa_dd_fwd``) against an fp64 computation done here (GPU only).

The entry point is called directly on random operands.  What it must produce:

    Y = act(X) @ W + b                                  [M][N],  X [M][K], W [K][N]

Outside the deterministic, the packed and the shared-GPU profile a K % 4 == 0 shape runs as
``dd_fwd_wide_kernel`` (16-wave workgroups: one per 32-column tile, 32-row batch block and K
slice, every wave a contiguous k range that is a multiple of 8); the other profiles keep
``dd_fwd_kernel``.  Shapes: every (K, N, M) of K in {8, 20, 136, 520, 1000, 3920} (fewer 8-k
blocks than waves; K % 8 != 0; wave ranges of unequal length; a last range cut short; about
the fc2 size with a cut range, and the fc1 size), N in {16, 40, 512} (a partial last column
tile) and M in {1, 17, 33, 50, 64} (one batch block; a second block with one live row; the
workload's; full), and (K, N) = (520, 40) and (3920, 512) at M = 100 (four batch blocks).
Every shape runs with and without bias and with every activation (none, sigmoid, leaky), in
the default, the packed and the deterministic profile; in deterministic mode a second call
must reproduce the first bit for bit.

``csa_dd_fwd_splits`` is asked first, as the program does: where it answers 1 the launch
stores, so Y is pre-filled with a sentinel that every live element must overwrite; where it
answers more, Y accumulates and starts at zero.  Y lives inside a larger buffer whose other
elements must keep their fill value.

Bound.  The same cases ran through the parent's library (``dd_fwd_kernel`` in every profile)
on an MI355X; the figure is the error against fp64 relative to max |Y| of the case.  Parent,
worst of all cases: PARENT_Y (profiles/r12_notes.md).  The bound is 4 x the parent's figure:
the order of the atomic adds varies from run to run and the fold order differs.
"""
import pytest
import torch

from cloud_server_amd.ops import fused as FK

pytestmark = pytest.mark.gpu

# worst error of the parent's kernel against fp64 over every case below, MI355X
PARENT_Y = 1.1470e-06           # K=3920 N=512 M=100 (deterministic profile: whole-K sums)

KS, NS, MS = (8, 20, 136, 520, 1000, 3920), (16, 40, 512), (1, 17, 33, 50, 64)
SHAPES = [(K, N, M) for K in KS for N in NS for M in MS] + [(520, 40, 100), (3920, 512, 100)]
ACTS = ((0, 0.0), (1, 0.0), (3, 0.2))            # none, sigmoid, leaky(alpha)
PROFILES = ("default", "packed", "det")
GUARD, FILL, SENTINEL = 64, -777.0, 12345.0


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


def _call(lib, X, W, b, M, N, K, act, alpha):
    splits = int(lib.csa_dd_fwd_splits(M, N, K))
    assert splits >= 1
    buf = torch.full((GUARD + M * N + GUARD,), FILL, device="cuda")
    buf[GUARD:GUARD + M * N] = 0.0 if splits > 1 else SENTINEL
    rc = lib.csa_dd_fwd(FK.ptr(X), FK.ptr(W), FK.ptr(b), FK.ptr(buf[GUARD:]), M, N, K, act, alpha, FK.stream())
    assert rc == 0, rc
    return buf


@pytest.mark.parametrize("K,N,M", SHAPES)
def test_fwd_matches_fp64(K, N, M):
    lib = _lib()
    gen = torch.Generator(device="cuda").manual_seed(K * 1000 + N * 7 + M)
    r = lambda *s: torch.randn(*s, generator=gen, device="cuda", dtype=torch.float64)
    X = r(M, K).float()
    W = (r(K, N) / K ** 0.5).float()
    bias = r(N).float()
    refs = {act: _act64(X.double(), act, alpha) @ W.double() for act, alpha in ACTS}
    worst = dict.fromkeys(PROFILES, 0.0)
    fails = []
    for prof in PROFILES:
        with _Profile(lib, prof):
            for act, alpha in ACTS:
                for b in (bias, None):
                    tag = f"{prof}-act{act}-{'b' if b is not None else 'nob'}"
                    ref = refs[act] + (b.double() if b is not None else 0.0)
                    buf = _call(lib, X, W, b, M, N, K, act, alpha)
                    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + M * N:] == FILL).all()), \
                        f"{tag}: wrote outside [M][N]"
                    got = buf[GUARD:GUARD + M * N].view(M, N).double()
                    err = float((got - ref).abs().max() / ref.abs().max())
                    if prof == "det":
                        buf2 = _call(lib, X, W, b, M, N, K, act, alpha)
                        assert torch.equal(buf, buf2), f"{tag}: Y differs between two deterministic calls"
                    worst[prof] = max(worst[prof], err)
                    if PARENT_Y is not None and not err <= 4 * PARENT_Y:
                        fails.append(f"{tag}: {err:.3e}")
    print(f"fwd-err K={K} N={N} M={M} Y " + " ".join(f"{p} {worst[p]:.4e}" for p in PROFILES))
    assert PARENT_Y is not None, "bound not measured"
    assert not fails, f"bound {4 * PARENT_Y:.3e}: " + "; ".join(fails[:6])


def test_wide_kernel_is_taken():
    """The one-GPU training shapes run as the wide kernel in the default profile and as
    dd_fwd_kernel in the others; without this the file could pass on the old kernel alone."""
    lib = _lib()
    for M, N, K in ((50, 512, 3920), (50, 512, 512)):
        with _Profile(lib, "default"):
            assert lib.csa_dd_fwd_wide(M, N, K) == 1, (M, N, K)
        for prof in ("packed", "det"):
            with _Profile(lib, prof):
                assert lib.csa_dd_fwd_wide(M, N, K) == 0, (prof, M, N, K)
        with _Profile(lib, "det"):
            assert lib.csa_dd_fwd_splits(M, N, K) == 1
    with _Profile(lib, "default"):
        assert lib.csa_dd_fwd_wide(50, 512, 3918) == 0          # K % 4 != 0: dd_fwd_kernel<false>
        # fc1: 16 column tiles x 2 batch blocks x 8 K slices, one workgroup per CU
        assert lib.csa_dd_fwd_splits(50, 512, 3920) == 8
