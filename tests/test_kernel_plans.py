"""Host-side launch plans of the round-4 kernels (CPU: the library's planning functions run
without a GPU).  The GPU numerics of the same paths are in test_hip_step.py /
test_deterministic.py (@gpu)."""
import pytest

from cloud_server_amd.ops import fused as K


@pytest.fixture(scope="module")
def lib():
    lib = K.load(required=False)
    if lib is None:
        pytest.skip("kernel library not built")
    lib.csa_set_deterministic(0)
    lib.csa_set_packed(0)
    yield lib
    lib.csa_set_deterministic(0)
    lib.csa_set_packed(0)


# the sample pair: conv 2x2x10 -> conv 2x2x20 -> 2x2 pool on 28x28x1 (TF SAME), B = 50
SAMPLE_PAIR = [50, 28, 28, 1, 2, 2, 0, 0, 10, 28, 28, 2, 2, 0, 0, 20, 28, 28, 1, 14, 14]


def test_pair_backward_tables_fit_the_prologue(lib):
    """One table region per band, each within the prologue's register batch (4 ints per
    thread of 256), in both launch profiles."""
    for packed in (0, 1):
        lib.csa_set_packed(packed)
        assert lib.csa_conv_pair_ok(K.ints(SAMPLE_PAIR))
        n = lib.csa_conv_pair_bwd_tables_size(K.ints(SAMPLE_PAIR))
        assert 0 < n <= 4 * 256 * 14, n
        assert n % 4 == 0
    lib.csa_set_packed(0)


def _conv_geom(B, h, w, cin, kh, kw, cout):
    """3x3-style SAME stride-1 conv geometry as HipProgram._conv_geom lays it out."""
    return [B, h, w, cin, kh, kw, 1, 1, (kh - 1) // 2, (kw - 1) // 2, h, w, cout]


NO_POOL = [0] * 9


def test_conv_unit_predicate_is_the_launchers_refusal(lib):
    """``csa_conv_unit_ok``: a 3x3 conv 64 -> c on a 7x7 map keeps its whole weight tensor in
    LDS.  64 -> 48 (110 592 B of weights) fits; 64 -> 64 needs (4 * 7 * 64 + 9 * 64 * 64) * 4
    = 154 624 B in the VALU forward, above the 153 600 B the kernels may have: refused (-2)
    at plan time.  More than 128 channels on a side: not a conv unit (0)."""
    ok = lambda geom, pool=NO_POOL, bias=1, first=0: lib.csa_conv_unit_ok(K.ints(geom), K.ints(pool), bias, first)
    assert ok(_conv_geom(50, 7, 7, 64, 3, 3, 48)) == 1
    assert ok(_conv_geom(50, 7, 7, 64, 3, 3, 64)) == -2
    assert ok(_conv_geom(50, 7, 7, 64, 3, 3, 128)) == -2
    assert ok(_conv_geom(50, 7, 7, 64, 3, 3, 64), first=1) == -2        # forward and wgrad alone
    assert ok(_conv_geom(50, 7, 7, 129, 1, 1, 8)) == 0
    assert ok(_conv_geom(50, 7, 7, 8, 1, 1, 129)) == 0
    assert ok(_conv_geom(50, 28, 28, 1, 2, 2, 10), first=1) == 1        # the sample's conv A
    # a fused pool's window index is one byte: 14 x 14 = 196 positions fit, 17 x 17 = 289 do not
    g = _conv_geom(50, 28, 28, 1, 3, 3, 4)
    assert ok(g, [1, 14, 14, 14, 14, 0, 0, 2, 2], first=1) == 1
    assert ok(g, [1, 16, 16, 16, 16, 2, 2, 2, 2], first=1) == 1
    assert ok(g, [1, 17, 17, 17, 17, 3, 3, 2, 2], first=1) == -3


def test_pool_and_gconv_predicates(lib):
    pool = lambda k, s, oh: K.ints([50, 28, 28, 4, k, k, s, s, 0, 0, oh, oh])
    assert lib.csa_maxpool_ok(pool(14, 14, 2)) == 1
    assert lib.csa_maxpool_ok(pool(16, 16, 2)) == 1
    assert lib.csa_maxpool_ok(pool(17, 11, 3)) == 0
    assert lib.csa_maxpool_ok(K.ints([50, 28, 28, 4, 1, 257, 1, 1, 0, 0, 28, 28])) == 0
    assert lib.csa_gconv_ok(K.ints(_conv_geom(50, 7, 7, 64, 3, 3, 64))) == 1
    assert lib.csa_gconv_ok(K.ints(_conv_geom(50, 7, 7, 132, 2, 3, 200))) == 1
    # FastDiv is exact below 2^22: B * H * W rows beyond that are refused
    assert lib.csa_gconv_ok(K.ints(_conv_geom(8192, 28, 28, 4, 3, 3, 200))) == 0


def _plan_on_host(lib, layers, det=False, B=50):
    """``HipProgram._lower`` + ``_plan_pair`` alone: they read the layer plan and the
    library's host-side predicates, no device."""
    import types

    import oracle64 as X
    from cloud_server_amd.runtime.hip_program import HipProgram
    p = HipProgram.__new__(HipProgram)
    p.lib, p.det, p.forward_only, p.B = lib, det, False, B
    p.e = types.SimpleNamespace(model=types.SimpleNamespace(plan=X.make_cfg(layers, batch=B).plan()))
    lib.csa_set_deterministic(1 if det else 0)
    try:
        p._lower()
        p._plan_pair()
    finally:
        lib.csa_set_deterministic(0)
    return p


def test_geometry_grid_lowers_as_intended(lib):
    """Every network of the geometry grid reaches the units it was written for, and the four
    contract cases are decided at plan time: a reason that names the layer and the limit, or
    a gconv unit (test_gpu_geometry asserts the same on the real program)."""
    import geometry_nets as G
    from cloud_server_amd.runtime.hip_program import Unsupported
    for name in G.MUST_LOWER:
        G.assert_lowering(name, _plan_on_host(lib, G.NETS[name]))
    for name in G.LOWERING_DET:
        G.assert_lowering(name, _plan_on_host(lib, G.NETS[name], det=True), det=True)
    for name, (layer, limit) in G.CONTRACT.items():
        try:
            p = _plan_on_host(lib, G.NETS[name])
        except Unsupported as exc:
            assert layer in str(exc) and limit in str(exc), str(exc)
            assert name not in G.CONTRACT_LOWERING
        else:
            G.assert_lowering(name, p)


def test_step_test_networks_lower_as_before(lib):
    """The plan-time predicates move no network of the step tests: every conv of at most
    128 channels a side still fits a conv unit."""
    import oracle64 as X
    from test_hip_step import CASES
    from cloud_server_amd.models.dsl import ConvSpec
    for name, layers in CASES.items():
        kinds = [u.kind for u in _plan_on_host(lib, layers).units]
        convs = [lp for lp in X.make_cfg(layers).plan().layers if isinstance(lp.spec, ConvSpec)]
        wide = sum(lp.in_shape.c > 128 or lp.spec.cout > 128 for lp in convs)
        assert kinds.count("gconv") == wide and kinds.count("conv") == len(convs) - wide, (name, kinds)


def test_deterministic_rows_are_one_per_workgroup(lib):
    """Deterministic mode gives every statistic-producing workgroup its own slab row."""
    geom = [50, 14, 14, 20, 3, 3, 1, 1, 1, 1, 14, 14, 8]     # conv 3x3 20 -> 8, SAME, stride 1
    pool = [0, 1, 1, 1, 1, 0, 0, 14, 14]
    lib.csa_set_deterministic(0)
    assert lib.csa_conv_fwd_nslab(K.ints(geom), K.ints(pool)) == 32
    assert lib.csa_conv_dgrad_nslab(K.ints(geom)) == 32
    assert lib.csa_bn_stat_rows(50 * 14 * 14) == 16
    lib.csa_set_deterministic(1)
    try:
        fwd = lib.csa_conv_fwd_nslab(K.ints(geom), K.ints(pool))
        dgr = lib.csa_conv_dgrad_nslab(K.ints(geom))
        assert fwd >= 50 and fwd % 50 == 0        # one row per (image, band) workgroup
        assert dgr >= 50 and dgr % 50 == 0
        assert lib.csa_bn_stat_rows(50 * 14 * 14) == -(-50 * 14 * 14 // 64)
        wg = lib.csa_conv_wgrad_blocks(K.ints(geom), 1)
        assert wg >= 50 and wg % 50 == 0
    finally:
        lib.csa_set_deterministic(0)
