"""The conv / pool geometry grid: small networks over the kernel shapes, strides, pads and
channel counts the other GPU tests never reach, and what each must lower to.

A plain helper module like ``oracle64`` (no tests, no fixtures).  ``test_geometry_cpu`` checks
the geometry itself against a loop reference and pins the fp64 oracle to the eager engine on
these networks; ``test_gpu_geometry`` runs the HIP program against the oracle;
``scripts/trajectory_parity.py --grid geometry`` measures both.

Every network reads 28x28x1 images; ``oracle64.make_cfg`` gives B = 50.  The wide ones sit
behind two 2x2/2 pools (7x7 maps) on purpose: the point is the index arithmetic, not the size.
"""
from __future__ import annotations

from typing import Dict, List, Tuple


def conv(kh, kw, c, stride=None, valid=False, bias=False) -> dict:
    d = {"layer": "conv", "filter": [kh, kw, c]}
    if stride is not None:
        d["stride"] = list(stride)
    if valid:
        d["padding"] = "VALID"
    if bias:
        d["isBias"] = "True"
    return d


def pool(k=None, s=None, valid=False) -> dict:
    d = {"layer": "pool"}
    if k is not None:
        d["kernel"] = list(k)
    if s is not None:
        d["stride"] = list(s)
    if valid:
        d["padding"] = "VALID"
    return d


def act(func, alpha=None) -> dict:
    d = {"layer": "active", "active_func": func}
    if alpha is not None:
        d["param"] = [alpha]
    return d


RELU, SIGMOID, NORM = act("relu"), act("sigmoid"), {"layer": "norm"}
FC = {"layer": "connect", "hidden": 16}


def _mid_channels(c: int) -> list:
    # 28 -> 14 -> 7; a 3x3 conv 64 -> c on the 7x7 map (weights: 9 * 64 * c * 4 bytes)
    return [pool(), pool(), conv(1, 1, 64), RELU, conv(3, 3, c, bias=True), RELU, pool(), FC]


def _pool_window(k: int) -> list:
    return [conv(3, 3, 4, bias=True), SIGMOID, pool((k, k), (k, k)), FC]


NETS: Dict[str, List[dict]] = {
    # rect kernels, even kh (pads (1, 2, 0, 1)), channels no multiple of 2 or 4 (an odd C1
    # keeps the two convs out of the pair kernels; the Cin remainder loops)
    "unit_rect": [conv(1, 5, 5, bias=True), RELU, conv(4, 2, 7), pool(), FC],
    # mixed strides, stride > kernel (the input gradient leaves skipped pixels at 0), a
    # strided 1x1 conv
    "unit_stride_mixed": [conv(3, 3, 6, stride=(1, 2)), RELU, conv(2, 2, 8, stride=(3, 3)), act("leaky_relu", 0.1),
                          conv(1, 1, 12, stride=(2, 1), valid=True, bias=True), FC],
    # 28 -> 24 -> 7 maps; the fused 2x2/2 pool on an odd map (pool pads (0, 1, 0, 1): a
    # partial last window in the MFMA forward family)
    "unit_valid_odd": [conv(5, 5, 6, valid=True), RELU, conv(4, 4, 8, stride=(3, 3), valid=True, bias=True), SIGMOID,
                       pool(), FC],
    # fused rect pool overlapping in h with gaps in w (atomic routing into a zeroed dc), a
    # stride-1 pool, a standalone VALID pool with an uncovered remainder (13x9 -> 4x3)
    "pool_shapes": [conv(3, 3, 6), RELU, pool((3, 2), (2, 3)), conv(2, 2, 8, bias=True),
                    pool((2, 2), (1, 1), valid=True), NORM, pool((3, 3), (3, 3), valid=True), FC],
    # kernel == stride with top / left pad 1 (route_bwd's plain-store path with PT, PL > 0);
    # the 10 -> 3 VALID pool never writes the remainder row
    "pool_tiling_padded": [conv(3, 3, 4), pool((3, 3), (3, 3)), conv(3, 3, 8, bias=True), RELU,
                           pool((3, 3), (3, 3), valid=True), FC],
    # the largest window regime that must be right: 196 <= 256 positions
    "pool_window_196": _pool_window(14),
    # 289 positions (pads 3, 3, 3, 3): beyond a one-byte window index
    "pool_window_289": _pool_window(17),
    "pool_first_289": [pool((17, 17), (11, 11)), conv(2, 2, 4), FC],
    # the largest whole-weights-in-LDS plan that fits (110 KB of weights), and two that do not
    "mid_channels_fit": _mid_channels(48),
    "mid_channels_64": _mid_channels(64),
    "mid_channels_128": _mid_channels(128),
    # VALU pair with a rect conv A (pads (0, 1, 1, 2))
    "pair_rect_valu": [conv(2, 4, 6, bias=True), RELU, conv(3, 3, 8), RELU, pool(), FC],
    # MFMA pair, rect conv B, a 24x27 map: the pool's partial window in w only
    "pair_rect_mfma": [conv(3, 5, 8), RELU, conv(5, 2, 12, valid=True, bias=True), RELU, pool(), FC],
    # 1x1 conv A
    "pair_1x1": [conv(1, 1, 2, bias=True), conv(2, 2, 4), SIGMOID, pool(), FC],
    # both gconv directions (Cout > 128, then Cin > 128) with rect kernels and mixed strides
    # on 7x7 -> 3x5 -> 3x3
    "gconv_rect": [pool(), pool(), conv(2, 3, 132, stride=(2, 1), valid=True, bias=True), RELU,
                   conv(3, 1, 8, stride=(1, 2)), FC],
}

# ---- the intended lowering -------------------------------------------------------------
# unit kinds in program order (``describe``): "conv" with what it fuses, "gconv", "pool" and
# "bn" (a materialised [norm] [act]) standalone units, "dense"; then whether the first two
# convs run as the pair kernels.
LOWERING: Dict[str, Tuple[Tuple[str, ...], bool]] = {
    "unit_rect": (("conv+act", "conv+pool", "dense"), False),
    "unit_stride_mixed": (("conv+act", "conv+act", "conv", "dense"), False),
    "unit_valid_odd": (("conv+act", "conv+act+pool", "dense"), False),
    "pool_shapes": (("conv+act+pool", "conv+pool", "bn", "pool", "dense"), False),
    "pool_tiling_padded": (("conv+pool", "conv+act+pool", "dense"), False),
    "pool_window_196": (("conv+act+pool", "dense"), False),
    "mid_channels_fit": (("pool", "pool", "conv+act", "conv+act+pool", "dense"), False),
    "pair_rect_valu": (("conv+act", "conv+act+pool", "dense"), True),
    "pair_rect_mfma": (("conv+act", "conv+act+pool", "dense"), True),
    "pair_1x1": (("conv", "conv+act+pool", "dense"), True),
    "gconv_rect": (("pool", "pool", "gconv", "bn", "gconv", "dense"), False),
}
# deterministic mode: an overlapping pool is never fused (a standalone gather-form unit), and
# only the VALU pair family is in the mode
LOWERING_DET: Dict[str, Tuple[Tuple[str, ...], bool]] = {
    "pool_shapes": (("conv+act", "pool", "conv", "pool", "bn", "pool", "dense"), False),
    "unit_rect": LOWERING["unit_rect"],
    "pair_rect_valu": LOWERING["pair_rect_valu"],
}
# csa_conv_pair_valu_ok of the two pair cases: the kernel family each was written for
PAIR_VALU = {"pair_rect_valu": 1, "pair_rect_mfma": 0}

MUST_LOWER = tuple(LOWERING)
# refused at plan time (the eager program runs, with a reason) or lowered and right; never
# an error from a step.  What each must say when it is refused; the lowering when it is not.
CONTRACT: Dict[str, Tuple[str, str]] = {
    "pool_window_289": ("layers.2", "256"),
    "pool_first_289": ("layers.0", "256"),
    "mid_channels_64": ("layers.4", "LDS"),
    "mid_channels_128": ("layers.4", "LDS"),
}
CONTRACT_LOWERING: Dict[str, Tuple[Tuple[str, ...], bool]] = {
    # a conv whose weights plus a band exceed the direct kernels' LDS is a gconv unit; its
    # activation and pool run standalone
    "mid_channels_64": (("pool", "pool", "conv+act", "gconv", "bn", "pool", "dense"), False),
    "mid_channels_128": (("pool", "pool", "conv+act", "gconv", "bn", "pool", "dense"), False),
}


def describe(u) -> str:
    """One unit of a HipProgram as the strings above."""
    if u.kind != "conv":
        return u.kind
    return "conv" + ("+act" if u.act is not None else "") + ("+pool" if u.pool is not None else "")


def lowering(program) -> Tuple[Tuple[str, ...], bool]:
    return tuple(describe(u) for u in program.units), program.pair is not None


def assert_lowering(name: str, program, det: bool = False) -> None:
    """The program runs the kernel family ``name`` was written for."""
    want = (LOWERING_DET if det else {**LOWERING, **CONTRACT_LOWERING}).get(name)
    got = lowering(program)
    assert want is not None, f"{name} has no intended lowering, it lowered to {got}"
    assert got == want, f"{name} lowered to {got}, not {want}"
    if name in PAIR_VALU and not det:
        from cloud_server_amd.ops import fused as K
        valu = int(program.lib.csa_conv_pair_valu_ok(K.ints(program.pair)))
        assert valu == PAIR_VALU[name], f"{name}: csa_conv_pair_valu_ok = {valu}"
