"""The pair backward's host plans (CPU: the library's planning functions run without a GPU).

``csa_conv_pair_bwd_units``: the dwB + dc1 tiles of a band as one list of units dealt to the
four waves (round 9).  ``csa_conv_pair_bwd_bias_mode``: where each bias gradient comes from
(0 none, 1 the spare M row of its GEMM, 2 the column-sum loop).  The GPU numerics of the same
paths are in test_pair_bwd_units.py (@gpu).
"""
import ctypes as C

import pytest

from cloud_server_amd.ops import fused as K

NONE, ROW, LOOP = 0, 1, 2


def pair_geom(batch, ka, c1, kb, c2, pool, valid_b=False, h=28, w=28, c0=1):
    """geom of csa_conv_pair_*: conv A ka x ka (TF SAME), conv B kb x kb (SAME or VALID)."""
    pta = (ka - 1) // 2
    h1, w1 = h, w
    ptb = 0 if valid_b else (kb - 1) // 2
    h2, w2 = (h1 - kb + 1, w1 - kb + 1) if valid_b else (h1, w1)
    ph, pw = (h2 // 2, w2 // 2) if pool else (h2, w2)
    return [batch, h, w, c0, ka, ka, pta, pta, c1, h1, w1, kb, kb, ptb, ptb, c2, h2, w2, 1 if pool else 0, ph, pw]


# the sample pair: conv 2x2x10 -> conv 2x2x20 -> 2x2 pool on 28x28x1 (TF SAME), B = 50
SAMPLE_PAIR = [50, 28, 28, 1, 2, 2, 0, 0, 10, 28, 28, 2, 2, 0, 0, 20, 28, 28, 1, 14, 14]

# name -> (geom, bias A, bias B, mode A, mode B): the networks of test_pair_bwd_units.py
GEOMS = {
    "sample": (SAMPLE_PAIR, 0, 0, NONE, NONE),
    "pair_relu_valid": (pair_geom(3, 3, 6, 3, 8, True, valid_b=True), 1, 1, ROW, ROW),      # KA 9, KB 54
    "leaky_alpha": (pair_geom(3, 3, 6, 2, 8, True), 1, 0, ROW, NONE),                       # KB 24
    "bias_b_loop": (pair_geom(3, 2, 8, 2, 8, True), 1, 1, ROW, LOOP),                       # KB 32
    "bias_a_loop": (pair_geom(3, 4, 8, 2, 8, False), 1, 0, LOOP, NONE),                     # KA 16
    "pair_nopool": (pair_geom(3, 2, 4, 3, 8, False), 0, 0, NONE, NONE),
}


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


def test_sample_geometry_is_the_one_above():
    assert pair_geom(50, 2, 10, 2, 20, True) == SAMPLE_PAIR


def _units(lib, geom, band):
    """(the plan's rows {wave, gemm, tm, tn, k0, k1}, busiest wave of the round-robin dealing,
    busiest wave of the best split)."""
    n = lib.csa_conv_pair_bwd_units(K.ints(geom), band, None, 0)
    assert n >= 0, n
    out = (C.c_int * (6 * max(n, 1)))()
    assert lib.csa_conv_pair_bwd_units(K.ints(geom), band, out, n) == n
    load = (C.c_int * 2)()
    assert lib.csa_conv_pair_bwd_units_load(K.ints(geom), band, load) == 0
    return [tuple(out[6 * i:6 * i + 6]) for i in range(n)], load[0], load[1]


def _tiles(geom, band, nbands):
    """The band's tiles and k-steps, from the geometry alone: {(gemm, tm, tn): k-steps}."""
    (B, H, W, C0, KAh, KAw, PTA, PLA, C1, H1, W1, KBh, KBw, PTB, PLB, C2, H2, W2, pool, PH, PW) = geom
    rows = PH if pool else H2
    pr = -(-rows // nbands)                                   # unit rows per band
    pr0, pr1 = band * pr, min(PH, band * pr + pr)
    last = band == nbands - 1
    o2a = 2 * pr0 if pool else pr0
    o2b = (H2 if last else 2 * pr1) if pool else pr1
    o1b = H1 if last else o2b
    npix2, npix1 = (o2b - o2a) * W2, (o1b - o2a) * W1
    KB, KD = KBh * KBw * C1, KBh * KBw * C2
    t = {}
    for tm in range(-(-KB // 16)):
        for tn in range(-(-C2 // 16)):
            t[(0, tm, tn)] = -(-npix2 // 4)
    for tm in range(-(-npix1 // 16)):
        t[(1, tm, 0)] = -(-KD // 4)
    return t


def _dealt(tiles):
    """Busiest wave when each GEMM's tiles go round-robin to the four waves."""
    load = [0] * 4
    for gemm in (0, 1):
        for i, key in enumerate(sorted(k for k in tiles if k[0] == gemm)):
            load[i % 4] += tiles[key]
    return max(load)


@pytest.mark.parametrize("name,packed", [(n, 0) for n in GEOMS] + [("sample", 1)])
def test_units_cover_every_tile_once(lib, name, packed):
    """Each (GEMM, tile, k range) exactly once, split tiles' ranges partition their steps;
    a plan only where its busiest wave beats the round-robin dealing.  (The sample pair in
    both launch profiles: packed = two pooled rows per band.)"""
    geom = GEOMS[name][0]
    lib.csa_set_packed(packed)
    try:
        nbands = lib.csa_conv_pair_grid(K.ints(geom)) // geom[0]
        assert nbands >= 1
        emitted = 0
        for band in range(nbands):
            rows, dealt, best = _units(lib, geom, band)
            tiles = _tiles(geom, band, nbands)
            assert dealt == _dealt(tiles), (name, band)
            assert best <= dealt
            if not rows:
                assert best == dealt, f"{name} band {band}: a better plan ({best} < {dealt}) was not emitted"
                continue
            emitted += 1
            assert best < dealt, f"{name} band {band}: a plan that does not beat the dealing"
            got = {}
            for wave, gemm, tm, tn, k0, k1 in rows:
                assert 0 <= wave < 4 and 0 <= k0 < k1
                got.setdefault((gemm, tm, tn), []).append((k0, k1))
            assert set(got) == set(tiles), (name, band)
            for key, ranges in got.items():
                ranges.sort()
                assert ranges[0][0] == 0 and ranges[-1][1] == tiles[key], (name, band, key, ranges)
                assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), (name, band, key, ranges)
            load = [0] * 4
            for wave, gemm, tm, tn, k0, k1 in rows:
                load[wave] += k1 - k0
            assert max(load) == best, (name, band, load)
        print(f"{name} packed={packed}: {emitted} of {nbands} bands planned")
    finally:
        lib.csa_set_packed(0)


def test_sample_busiest_wave(lib):
    """The sample's band: 6 dwB tiles of 14 k-steps and 4 dc1 tiles of 20; dealt 48, planned
    at most 42 (greedy longest-first would give 48)."""
    for band in range(14):
        rows, dealt, best = _units(lib, SAMPLE_PAIR, band)
        assert dealt == 48 and best <= 42 and len(rows) == 10, (band, dealt, best, len(rows))


@pytest.mark.parametrize("name", list(GEOMS))
def test_bias_modes(lib, name):
    geom, ba, bb, ma, mb = GEOMS[name]
    assert lib.csa_conv_pair_ok(K.ints(geom)), name
    assert lib.csa_conv_pair_bwd_bias_mode(K.ints(geom), ba, bb) == ma | mb << 4
    assert lib.csa_conv_pair_bwd_bias_mode(K.ints(geom), 0, 0) == 0
