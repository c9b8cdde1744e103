"""Lower a DSL network to the hand-written gfx950 kernels (the MI355X training step).

Lowering groups the reference layer list (construct_distribute.py:208-265) into:

* **conv units** ``conv [act] [pool]`` — one ``csa_conv_fwd`` launch each (bias, act and
  max-pool fused, argmax kept for backward, BN partial statistics emitted when a norm
  follows);
* **transforms** ``[norm] [act]`` between units — never materialised: the CONSUMER applies
  BN-apply + activation while loading its input (conv input read, GEMM A-prologue,
  im2col loader) and its dgrad epilogue applies the activation backward and emits the
  BN-backward statistics;
* **dense units** ``connect`` — MFMA GEMMs (``csa_dense_fwd/_dgrad/_wgrad``);
* the **head** — one single-workgroup kernel: logits, loss, accuracy, head gradients,
  input gradient and the step/metric bookkeeping.

Backward runs the units in reverse (``csa_route_bwd`` = BN backward + act backward +
max-pool routing; ``csa_conv_dgrad``; ``csa_conv_wgrad`` as an implicit MFMA GEMM),
then gradient all-reduce (data parallel) and ONE fused optimizer launch which also
zeroes next step's atomic accumulators and updates BN running statistics.

A conv with more than 128 input or output channels (beyond the direct kernels' LDS
tables) is a **gconv unit**: forward, input gradient and weight gradient as implicit
MFMA GEMMs whose loaders gather the im2col / transposed operands on the fly
(``csa_gconv_*`` in gemm.hip); its activation, pool and norm run as standalone units.
So is a conv of at most 128 channels a side whose whole weight tensor plus one band of rows
does not fit the direct kernels' 150 KB of LDS (a 3x3 conv 64 -> 64 already): ``_lower``
asks ``csa_conv_unit_ok``, the launchers' own refusals as a host-only predicate, and makes
the layer a gconv unit instead of letting the first step fail.  Every refusal a launcher can
make on geometry is asked at plan time this way (``csa_conv_unit_ok``, ``csa_maxpool_ok``,
``csa_gconv_ok``).  A max-pool window of more than 256 positions, fused or standalone, is
``Unsupported`` (the pool kernels keep the window index in one byte): the engine then runs
the eager program and says why in ``fallback_reason``.

Layer orders the consumer transform cannot express — a 2-D norm after a dense layer, a
norm over > 128 channels or directly before the head, a pool that does not directly
follow a conv, act/norm sequences like ``act norm`` — become **standalone units**
(``norm_pool.hip``): ``bn`` (materialised ``[norm] [act]``: stats -> finalize -> apply,
with its own backward) and ``pool`` (max pool + gather-form backward).  So every DSL the
reference accepts (construct_distribute.py:155-165, 208-265) lowers to HIP kernels.

A ``dropout`` layer is a standalone ``drop`` unit (``dropout.hip``): one launch each way,
the mask redrawn from the counter RNG (ops/dropout_ref.py), never stored.  A lone
activation in front of it rides in the same launches, so the dense layer after it reads a
plain tensor.  Forward-only programs skip the layer altogether.

An average pool (``AvgPoolSpec``: ``"mode": "avg"``, also with ``"kernel": "global"``) is
always a standalone ``pool`` unit without an argmax (``avg_pool.hip``: one launch each way,
none backward when the unit is first); ``PoolSpec`` keeps meaning "max pool with a window
argmax" wherever it is tested, so the conv in front of an average pool fuses no pool and
``conv conv avgpool`` still forms the pair in its no-pool form.  ``csa_avgpool_ok`` is asked
at plan time; there is no 256-position limit.

A local response normalisation (``LrnSpec``: ``{"layer": "lrn"}``, ``tf.nn.lrn``) is always a
standalone ``lrn`` unit (``lrn.hip``: one launch each way, none backward when the unit is
first).  Pending norm / act layers are materialised in front of it; a conv in front keeps
fusing its own ``[act] [pool]`` and ``conv conv pool lrn`` still forms the pair; a norm after
it has no conv producer and is a standalone ``bn`` unit.  Training programs keep
``s = bias + alpha * window sum`` (``Unit.lrn_s``) for the backward; forward-only programs keep
the unit (the layer is active at inference) and keep nothing.  ``csa_lrn_ok`` is asked at plan
time.

A layer / group / instance normalisation (``GroupNormSpec``: a ``norm`` entry with ``mode``)
is always a standalone ``gn`` unit (``group_norm.hip``), forward-only programs included: it is
not a ``NormSpec``, so it never joins ``pending`` and never becomes a consumer transform.
Pending norm / act layers are materialised in front of it; an ``active`` right behind it rides
in the unit's launches (``Unit.act``; the backward recomputes the pre-activation from x and the
kept statistics, so any leaky alpha is fine) and the consumer behind reads a plain tensor.
Training programs keep ``{mean, rstd}`` per (sample, group) (``Unit.gn_stat``) and a
``[B][2][C]`` slab of per-sample channel sums (``Unit.gn_slab``), both stored whole every step:
no zero regions.  The backward launch runs even when the unit is first (no input gradient,
but the parameter gradients), then ``csa_gn_bwd_params`` stores them into the flat gradient.
``csa_gn_ok`` is asked at plan time.

A depthwise convolution (``DepthwiseConvSpec``: ``{"layer": "depthwise"}``,
``tf.nn.depthwise_conv2d``) is always a standalone ``dw`` unit (``depthwise_conv.hip``),
forward-only programs included: it is not a ``ConvSpec``, so it never joins the pair, never
fuses a pool and never becomes a gconv unit.  Pending norm / act layers are materialised in
front of it; an ``active`` right behind it rides in the unit's launches (``Unit.act``) when its
backward can be formed from y alone (``_y_ok``; a leaky alpha < 0 stays pending and is lowered
where x is at hand), a pool behind it is a standalone ``pool`` unit and a norm behind it a
standalone ``bn`` unit (``as_transform`` takes a norm only behind a ``conv`` unit).  The
backward launch runs even when the unit is first (no input gradient, but the weight and bias
gradients); it STORES them into the flat gradient, through a ``[R][(taps + 1) * C * M]`` slab
of exclusive rows (``Unit.dw_slab``, every row stored whole every step: no zero regions) that
``csa_dw_bwd_params`` folds in row order, or directly in the owner form.  No atomics: the
deterministic program is the same launches.  ``csa_dw_ok`` is asked at plan time.

``options.augment`` adds one launch in front of the training step (``augment.hip``): this
step's batch, warped for (seed, step, dataset row) as ops/augment_ref.py defines it, lands in
``aug_img`` and every training-time reader of the images takes that buffer (``_train_src``).
Predicting, validation and serving read the stored images.

(``Plan`` here; ``hip_buffers`` declares the state and allocates; ``hip_program`` launches.)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from ..models.dsl import (ActSpec, AvgPoolSpec, ConvSpec, DenseSpec, DepthwiseConvSpec, DropoutSpec, GroupNormSpec,
                          LayerPlan, LrnSpec, NormSpec, PoolSpec)
from ..ops import fused as K
from ..utils.streams import dedicated_stream


def _opt_call(lib, name: str, *args):
    """Call an entry point that an A/B baseline library (CSA_KERNEL_LIB, an older revision)
    may lack; the in-tree library has them all (ops.fused.load checks)."""
    try:
        fn = getattr(lib, name)
    except AttributeError:
        return None
    return fn(*args)


_NT_SET = [None]


def _set_nt_out(lib) -> None:
    """``CSA_NT_OUT=1``: the activations a launch writes for the next one (pair forward y,
    bn_act xt, head dh / dX, fc1's dX) go out as non-temporal stores (A/B knob; once per
    process and value)."""
    want = int(os.environ.get("CSA_NT_OUT", "0") == "1")
    if _NT_SET[0] == want:
        return
    for name in ("csa_nt_out_ew", "csa_nt_out_cp", "csa_nt_out_head", "csa_nt_out_du"):
        try:
            getattr(lib, name)(want)
        except AttributeError:          # an A/B baseline library without the knob
            pass
    _NT_SET[0] = want


class Unsupported(Exception):
    pass


def _act_id(sp: Optional[ActSpec]) -> int:
    if sp is None:
        return 0
    if sp.func == "leaky_relu" and sp.alpha == 0:
        return K.ACT_IDS["relu"]        # tf.maximum(x, 0 * x) IS relu
    return K.ACT_IDS[sp.func]


def _y_ok(sp: Optional[ActSpec]) -> bool:
    """Can this activation's backward be formed from its OUTPUT alone?  The kernels that
    fuse an activation into a producer's epilogue (conv / pair outputs, the row head's
    input) keep only y; ``maximum(x, a x)`` with a < 0 maps x > 0 and x < 0 both to y > 0,
    so such an activation is lowered where x is at hand instead: as a consumer transform
    (the dgrad epilogues read the pre-transform input) or a standalone act unit
    (construct_distribute.py:147-150 accepts any alpha)."""
    return sp is None or not (sp.func == "leaky_relu" and sp.alpha < 0)


def _alpha(sp: Optional[ActSpec]) -> float:
    return float(sp.alpha) if sp is not None else 0.0


@dataclass
class Transform:
    """Pending ``[norm] [act]`` applied by the consumer of a tensor."""
    norm: Optional[LayerPlan] = None
    act: Optional[ActSpec] = None
    slab: Optional[torch.Tensor] = None     # forward BN partial slab of the tensor
    nslab: int = 0
    count: float = 0.0
    bwd_slab: Optional[torch.Tensor] = None  # filled by the consumer's dgrad
    bwd_nslab: int = 0
    # deterministic mode: rows the producer writes (one per workgroup, folded to row 0 in
    # fixed order by csa_rows_fold; consumers then read nslab = 1)
    prod_rows: int = 0
    bwd_prod_rows: int = 0
    # BatchNorm tables [mean | rstd | a | b][C], written once per step by the launch that
    # materialises a dense consumer's xt (None: no such consumer)
    bn_tab: Optional[torch.Tensor] = None
    eval_slab: Optional[torch.Tensor] = None  # predict: the running statistics as a 1-row slab

    @property
    def has_bn(self) -> bool:
        return self.norm is not None


@dataclass
class Unit:
    kind: str                               # "conv" | "dense" | "gconv" | "bn" | "pool" | "drop" | "lrn" | "gn" | "dw"
    layer: LayerPlan
    act: Optional[ActSpec] = None           # conv / dw: fused output act; bn / drop: applied first; gn: applied last
    pool: Optional[LayerPlan] = None        # conv: fused pool
    in_tf: Transform = field(default_factory=Transform)   # transform of this unit's INPUT
    x: Optional[torch.Tensor] = None        # input tensor (pre-transform), None = raw images
    y: Optional[torch.Tensor] = None        # output (post act/pool)
    argmax: Optional[torch.Tensor] = None
    dy: Optional[torch.Tensor] = None       # grad wrt output (or wrt the next BN output)
    dc: Optional[torch.Tensor] = None       # conv: grad wrt pre-act conv output
    splits_fwd: int = 1
    xt: Optional[torch.Tensor] = None       # dense: materialised act(bn(x)) (BN inputs)
    wg_stripes: int = 1                     # conv: weight-gradient accumulator stripes
    dw_acc: Optional[torch.Tensor] = None   # conv: [stripes][taps*Cout] (or the flat-grad view)
    db_acc: Optional[torch.Tensor] = None   # conv: [stripes][Cout] (or the flat-grad view)
    norm: Optional[LayerPlan] = None        # bn unit: the norm layer (None: activation only)
    # dense (_plan_fused, _plan_fwd_bn, _alloc)
    fused: bool = False                     # backward + optimizer update in one launch
    direct: bool = False                    # register-direct MFMA forward (dense_direct.hip)
    fwd_bn: bool = False                    # the forward applies the producer's BatchNorm itself
    du_part: Optional[torch.Tensor] = None  # fused backward: partial input-gradient slabs
    du_cnt: Optional[torch.Tensor] = None   # ... and per-row-group arrival tickets
    # dense under lowrank data parallelism (_plan_lowrank)
    lr_update: bool = False                 # the gathered-operand wgrad updates W / b in-kernel
    lr_src: Optional[torch.Tensor] = None   # this rank's GEMM input rows
    lr_act: tuple = (0, 0.0)                # (act id, alpha) the wgrad applies to them
    lr_x: Optional[torch.Tensor] = None     # every rank's inputs, gathered [W * B, in]
    lr_dy: Optional[torch.Tensor] = None    # every rank's output gradients [W * B, out]
    # conv (_collect_zero_regions): who folds the weight-gradient stripes
    row_fold: bool = False                  # csa_rows_fold right after the backward
    tail_fold: bool = False                 # the pair backward's tail (":hf")
    # drop / bn units (_alloc)
    used_step: Optional[torch.Tensor] = None  # drop: the step whose mask the forward drew
    bn_tab: Optional[torch.Tensor] = None   # bn: [mean | rstd | a | b][C]
    bn_slab: Optional[torch.Tensor] = None  # bn: forward statistic rows
    bn_bslab: Optional[torch.Tensor] = None  # bn: backward statistic rows
    bn_k: Optional[torch.Tensor] = None     # bn: backward coefficients [2][C]
    # lrn units (_alloc)
    lrn_s: Optional[torch.Tensor] = None    # the forward's bias + alpha * window sum, kept for the backward
    # gn units (_alloc)
    gn_stat: Optional[torch.Tensor] = None  # the forward's {mean, rstd} per (sample, group), kept for the backward
    gn_slab: Optional[torch.Tensor] = None  # the backward's per-sample channel sums [B][2][C]
    # dw units (_alloc)
    dw_form: int = 0                        # the backward's form (1: split with a slab, 2: owner)
    dw_slab: Optional[torch.Tensor] = None  # split form: exclusive partial rows [R][(taps + 1) * C * M]


class Plan:
    """The lowering and every planner of ``HipProgram`` (which declares their fields; the
    geometry arrays they hand the library are ``Buffers._conv_geom`` and its kin)."""

    # ------------------------------------------------------------------ helpers
    def _next_tf(self, k: int) -> Transform:
        """The transform of unit ``k``'s OUTPUT: the next unit's input transform, or the head's."""
        return self.units[k + 1].in_tf if k + 1 < len(self.units) else self.head_tf

    def _keep_range(self, name: str) -> tuple:
        """The whole float4s of a parameter's flat gradient span."""
        lo = self.model.state.offsets[name]
        return (lo, lo + (self.gviews[name].numel() // 4) * 4)

    def _float4_segments(self, pick) -> List[list]:
        """Flat [lo, hi) spans of the parameters whose offset ``pick`` accepts, each padded to
        float4 (the flat layout's alignment padding is zero and stays zero) and merged where
        they touch."""
        n = self.e.flat.numel()
        spans = sorted(self.model.state.offsets.values())
        ends = {o: (spans[i + 1] if i + 1 < len(spans) else n) for i, o in enumerate(spans)}
        segs: List[list] = []
        for o in spans:
            if not pick(o):
                continue
            lo, hi = o - o % 4, -(-ends[o] // 4) * 4
            if segs and segs[-1][1] >= lo:
                segs[-1][1] = max(segs[-1][1], hi)
            else:
                segs.append([lo, hi])
        return segs

    # ------------------------------------------------------------------ lowering
    def _lower(self) -> None:
        layers = self.e.model.plan.layers
        units: List[Unit] = []
        pending: List[LayerPlan] = []            # norm / act layers since the last unit

        def as_transform(consumer: str) -> Optional[Transform]:
            """``pending`` as a transform the consumer applies while loading, or None."""
            tf = Transform()
            for lp in pending:
                if isinstance(lp.spec, NormSpec):
                    if tf.norm is not None or tf.act is not None:
                        return None              # norm after norm / act
                    tf.norm = lp
                else:
                    if tf.act is not None:
                        return None              # two activations in a row
                    tf.act = lp.spec
            if consumer == "head" and not _y_ok(tf.act):
                return None                      # the row head's backward reads y only
            if tf.norm is not None:
                # the forward statistics come from a conv unit's epilogue, the tables live
                # in LDS (<= 128 channels), and the head has no BN-apply prologue
                if (consumer == "head" or not units or units[-1].kind != "conv"
                        or not tf.norm.in_shape.is_spatial or tf.norm.in_shape.c > 128):
                    return None
            return tf

        def materialise() -> None:
            """``pending`` as standalone units: [norm][act] groups and lone activations."""
            i = 0
            while i < len(pending):
                lp = pending[i]
                if isinstance(lp.spec, NormSpec):
                    nxt = pending[i + 1] if i + 1 < len(pending) else None
                    act = nxt.spec if nxt is not None and isinstance(nxt.spec, ActSpec) else None
                    units.append(Unit("bn", lp, act=act, norm=lp))
                    i += 2 if act is not None else 1
                else:
                    units.append(Unit("bn", lp, act=lp.spec))
                    i += 1
            pending.clear()

        def conv_tail(i: int):
            """(act, pool, next index) of the ``[act] [pool]`` a conv unit at ``i`` would fuse."""
            act = pool = None
            j = i + 1
            if j < len(layers) and isinstance(layers[j].spec, ActSpec) and _y_ok(layers[j].spec):
                act = layers[j].spec
                j += 1
            if (j < len(layers) and isinstance(layers[j].spec, PoolSpec)
                    and not (self.det and tuple(layers[j].spec.kernel) != tuple(layers[j].spec.stride))):
                # (deterministic mode: an overlapping pool's routing adds windows into
                # dc with atomics — it stays a standalone gather-form pool unit)
                pool = layers[j]
                j += 1
            return act, pool, j

        # every pool kernel, fused or standalone, keeps its window index in one byte
        for lp in layers:
            if isinstance(lp.spec, PoolSpec):
                kh, kw = lp.spec.kernel
                if _opt_call(self.lib, "csa_maxpool_ok", self._pool_geom_full(Unit("pool", lp))) == 0:
                    raise Unsupported(f"pool layer {lp.name}: a {kh}x{kw} window has {kh * kw} positions, the "
                                      f"pool kernels' one-byte window index holds at most 256")
            elif isinstance(lp.spec, AvgPoolSpec):
                # (no index byte: any window; the kernels index their tensors with 32-bit ints)
                if _opt_call(self.lib, "csa_avgpool_ok", self._pool_geom_full(Unit("pool", lp))) != 1:
                    raise Unsupported(f"average pool layer {lp.name}: batch x map x channels beyond the "
                                      f"average-pool kernels' 2^30 index range")
            elif isinstance(lp.spec, LrnSpec):
                if self.lib.csa_lrn_ok(self._lrn_geom(lp), *self._lrn_consts(lp)) != 1:
                    raise Unsupported(f"lrn layer {lp.name}: batch x map x channels beyond the lrn kernels' "
                                      f"2^30 index range, or constants they refuse")
            elif isinstance(lp.spec, GroupNormSpec):
                if self.lib.csa_gn_ok(self._gn_geom(lp)) != 1:
                    raise Unsupported(f"norm layer {lp.name}: batch x map x channels beyond the group-norm "
                                      f"kernels' 2^30 index range")
            elif isinstance(lp.spec, DepthwiseConvSpec):
                if self.lib.csa_dw_ok(self._dw_geom(lp)) != 1:
                    raise Unsupported(f"depthwise layer {lp.name}: batch x map x channels or taps x channels "
                                      f"beyond the depthwise kernels' 2^30 index range (65534 taps)")

        i = 0
        while i < len(layers):
            lp = layers[i]
            sp = lp.spec
            if isinstance(sp, ConvSpec):
                gconv = lp.in_shape.c > 128 or sp.cout > 128
                if not gconv:
                    # the first unit reads the images and has no input gradient
                    first = not units and as_transform("conv") is not None
                    rc = _opt_call(self.lib, "csa_conv_unit_ok", self._conv_geom(lp, self.B),
                                   self._pool_geom(Unit("conv", lp, pool=conv_tail(i)[1])),
                                   int(bool(sp.bias)), int(first))
                    # (its weights plus one band of rows exceed the direct kernels' 150 KB of LDS)
                    gconv = rc is not None and rc != 1
                if gconv:
                    # wide conv: implicit-GEMM unit on a materialised input; the act / pool /
                    # norm after it become standalone units
                    if _opt_call(self.lib, "csa_gconv_ok", self._conv_geom(lp, self.B)) == 0:
                        raise Unsupported(f"conv layer {lp.name}: batch x map or taps x channels beyond the "
                                          f"implicit-GEMM kernels' 2^22 index range")
                    materialise()
                    units.append(Unit("gconv", lp))
                    i += 1
                    continue
            if isinstance(sp, (ConvSpec, DenseSpec)):
                kind = "conv" if isinstance(sp, ConvSpec) else "dense"
                tf = as_transform(kind)
                if tf is None:
                    materialise()
                    tf = Transform()
                pending.clear()
                u = Unit(kind, lp, in_tf=tf)
                j = i + 1
                if kind == "conv":
                    u.act, u.pool, j = conv_tail(i)
                units.append(u)
                i = j
            elif isinstance(sp, (PoolSpec, AvgPoolSpec)):
                # (an average pool is always a standalone unit: conv_tail fuses max pools only)
                materialise()                    # pool(act(norm(x))): the transform first
                units.append(Unit("pool", lp))
                i += 1
            elif isinstance(sp, LrnSpec):
                # always a standalone unit, forward-only programs included (active at inference)
                materialise()                    # lrn(act(norm(x))): the transform first
                units.append(Unit("lrn", lp))
                i += 1
            elif isinstance(sp, GroupNormSpec):
                # always a standalone unit, forward-only programs included; the activation
                # right behind it rides in its launches
                materialise()                    # gn(act(norm(x))): the transform first
                nxt = layers[i + 1].spec if i + 1 < len(layers) else None
                act = nxt if isinstance(nxt, ActSpec) else None
                _act_id(act)
                units.append(Unit("gn", lp, act=act))
                i += 2 if act is not None else 1
            elif isinstance(sp, DepthwiseConvSpec):
                # always a standalone unit, forward-only programs included; the activation right
                # behind it rides in its launches when its backward can be formed from y alone
                materialise()                    # dw(act(norm(x))): the transform first
                nxt = layers[i + 1].spec if i + 1 < len(layers) else None
                act = nxt if isinstance(nxt, ActSpec) and _y_ok(nxt) else None
                _act_id(act)
                units.append(Unit("dw", lp, act=act))
                i += 2 if act is not None else 1
            elif isinstance(sp, DropoutSpec):
                i += 1
                if self.forward_only:
                    continue                     # identity outside training: no unit, no launch
                if len(pending) == 1 and isinstance(pending[0].spec, ActSpec):
                    # a lone activation rides in the drop unit's launches (its backward
                    # reads the unit's input, so any alpha is fine)
                    units.append(Unit("drop", lp, act=pending[0].spec))
                    pending.clear()
                else:
                    materialise()
                    units.append(Unit("drop", lp))
            elif isinstance(sp, (NormSpec, ActSpec)):
                if isinstance(sp, ActSpec):
                    _act_id(sp)
                pending.append(lp)
                i += 1
            else:  # pragma: no cover
                raise Unsupported(str(sp))
        tf = as_transform("head")
        if tf is None:
            materialise()
            tf = Transform()
        if not units:
            raise Unsupported("no conv/dense layers")
        self.units = units
        self.head_tf = tf

    # ------------------------------------------------------------------ fused updates
    def _plan_fused(self) -> None:
        """On one GPU the dense weight gradients feed nothing but the optimizer: such a
        layer's backward becomes ``csa_dense_bwd_update`` (dgrad + wgrad + the optimizer
        update of its W rows in one launch, dense_update.hip) and the head writes
        per-row-group partial gradients + metrics that the (now small) optimizer launch
        folds (``csa_head_part2``).  Data parallel (all-reduce / ps) runs the SAME fused
        launch in gradient mode (``csa_dense_bwd_grad_head``): the dense weight / bias
        gradients are stored whole into the flat gradient for the all-reduce and the flat
        optimizer updates them (``fused_grad``); lowrank forms them from gathered operands."""
        e, B = self.e, self.B
        on = os.environ.get("CSA_FUSED_UPDATE", "1") == "1" and not self.forward_only
        self.fused = on and not e.ctx.enabled
        self.fused_grad = on and e.ctx.enabled and e.sync.strategy in ("allreduce", "ps", "async_ps")
        # measured on MI355X (profiles/r2_dense_fused.md): the row-group kernel (one
        # 1024-thread workgroup per 16 input features) replaces fc1's split-K pair + its
        # share of the flat optimizer (bench 0.1166 -> 0.1107 ms/step); CSA_FUSED_DENSE=0
        # restores the separate kernels
        fuse_dense = (self.fused or self.fused_grad) and os.environ.get("CSA_FUSED_DENSE", "1") == "1"
        for u in self.units:
            if not fuse_dense or u.kind != "dense":
                continue
            tf = u.in_tf
            fin, fout = u.layer.in_shape.numel, u.layer.spec.hidden
            if tf.has_bn and fin % 4:            # the BN'd input is not materialised (see _alloc)
                continue
            if tf.act is not None and not tf.has_bn:
                continue                         # weight-gradient operand would need the act
            ch = tf.norm.in_shape.c if tf.has_bn else 0
            # (a narrow layer's row groups are split over 128-column blocks with a partial
            # hand-off, so fc2's 32 row groups still use 128 CUs: profiles/r2_dense_fused.md)
            u.fused = bool(self.lib.csa_dense_bwd_update_ok(B, fin, fout, ch))
        # the flat optimizer launch updates at most 16 spans between the fused layers' own
        # parameters: beyond 15 fused layers the rest take the materialised-gradient path
        nf = 0
        for u in self.units:
            if u.fused:
                nf += 1
                u.fused = nf <= 15
        last = self.units[-1]
        if (not self.fused and not self.forward_only and self.head_tf.norm is None
                and not (self.fused_grad and last.kind == "dense" and last.fused)):
            # data parallel without a fused last dense layer (lowrank, or the unfused
            # program): the row-per-workgroup head, its weight gradient as a register-direct
            # wgrad launch (dWh = act(h)^T dlogits) into the flat gradient before the
            # all-reduce, its metrics folded by the optimizer launch (the atomic
            # 4-workgroup head took 15.6 us per DP step)
            if last.kind == "dense" and self.lib.csa_head_row_ok(B, last.layer.spec.hidden):
                self.head_row = self.head_sep = True
        if (self.fused or self.fused_grad) and self.head_tf.norm is None and not self.head_sep:
            kh = last.layer.spec.hidden if last.kind == "dense" else last.layer.out_shape.numel
            if last.kind == "conv" and last.pool is not None:
                kh = last.pool.out_shape.numel
            # one batch row per workgroup; the head's batch reductions (dWh, dbh, metrics)
            # ride in the last dense layer's fused backward (csa_head_row + the head epilogue
            # of csa_dense_bwd_update_head) — no partial rows for the optimizer to fold
            self.head_row = last.kind == "dense" and last.fused and bool(self.lib.csa_head_row_ok(B, kh))
            if not self.head_row and self.fused:
                self.head_rg = int(self.lib.csa_head_part_rows(B, kh))
        # register-direct MFMA dense forward (dense_direct.hip); the backward of a dense layer
        # is the fused backward + update (one GPU), the LDS-staged dgrad + wgrad pair (data
        # parallel: the gradient is all-reduced), or under lowrank the gathered-operand
        # weight gradient with the update in-kernel (profiles/r2_dense_direct.md measured
        # the register-direct backward slower than the paired kernels)
        for u in self.units:
            # (a BN'd input that is not materialised takes the LDS-staged GEMM)
            u.direct = u.kind == "dense" and not (u.in_tf.has_bn and u.layer.in_shape.numel % 4)

    # ------------------------------------------------------------------ conv pair
    def _plan_pair(self) -> None:
        """``conv [act] conv [act] [pool]`` on the raw images (the sample's conv1 -> conv2
        -> pool) runs as ONE forward and ONE backward launch (conv_pair.hip): dc2 / dc1 are
        never written.  c1: the VALU forward stores its band tiles (``pair_c1``, allocated by
        ``_alloc``) and the backward loads them in its prologue; the MFMA-forward family,
        deterministic mode and ``CSA_PAIR_C1=0`` keep c1 in LDS and recompute it."""
        if len(self.units) < 2:
            return
        ua, ub = self.units[0], self.units[1]
        if ua.kind != "conv" or ub.kind != "conv" or ua.pool is not None:
            return
        if ub.in_tf.norm is not None or ub.in_tf.act is not None:
            return
        la, lb = ua.layer, ub.layer
        if tuple(la.spec.stride) != (1, 1) or tuple(lb.spec.stride) != (1, 1):
            return
        pool = 0
        if ub.pool is not None:
            ps = ub.pool.spec
            if tuple(ps.kernel) != (2, 2) or tuple(ps.stride) != (2, 2) or ub.pool.pads[0] or ub.pool.pads[2]:
                return
            pool = 1
        h, w = la.in_shape.hw
        h1, w1 = la.out_shape.hw
        h2, w2 = lb.out_shape.hw
        ph, pw = ub.pool.out_shape.hw if pool else (h2, w2)
        geom = [self.B, h, w, la.in_shape.c, la.spec.kh, la.spec.kw, la.pads[0], la.pads[2], la.spec.cout,
                h1, w1, lb.spec.kh, lb.spec.kw, lb.pads[0], lb.pads[2], lb.spec.cout, h2, w2, pool, ph, pw]
        if not self.lib.csa_conv_pair_ok(K.ints(geom)):
            return
        if not (_y_ok(ua.act) and _y_ok(ub.act)):
            return
        if self.det and not self.lib.csa_conv_pair_valu_ok(K.ints(geom)):
            return                       # deterministic mode: two conv units instead
        self.pair = geom

    def _plan_pair_tables(self) -> None:
        """The pair backward's per-band index tables, computed once (csa_conv_pair_bwd_tables)."""
        if self.pair is None or self.forward_only:
            return
        n = int(self.lib.csa_conv_pair_bwd_tables_size(K.ints(self.pair)))
        if n > 0:
            self.pair_tabs = torch.zeros(n, dtype=torch.int32, device=self.e.device)
            self._rc(self.lib.csa_conv_pair_bwd_tables(K.ints(self.pair), K.ptr(self.pair_tabs), K.stream()),
                     "conv_pair_bwd_tables")

    # ------------------------------------------------------------------ horizontal fusion
    def _plan_hfuse(self) -> None:
        """One-GPU fused program with a conv pair: split every fused dense backward into its
        input gradient (``csa_dense_bwd_dgrad``, on the step's critical path) and its weight
        gradient + optimizer update, which is DEFERRED (``csa_dense_update_defer``) and runs
        as extra workgroups of the pair backward launch (conv_pair.hip,
        ``conv_pair_bwd_upd_kernel``).  The update only has to land before the next step's
        forward of its layer; inside the pair backward — a latency chain at 3 % of HBM and
        8 % of MFMA (profiles/r3_roofline.md) — it uses idle CUs instead of adding 10-15 us
        of serial work per dense layer.  The head's batch reductions ride in the last dense
        layer's deferred segment exactly as they rode in its fused backward."""
        # Packed profile too (round 6): with the round-6 carrier (5 workgroups per CU, the
        # tail program) K = 4 / 8 packs measured 1.295 / 1.313 M samples/s with the deferred
        # updates against 1.249 / 1.264 M without (scripts/archive/gpu_r6q.sh, profiles/
        # r6_multitenant.md; rounds 4-5 measured the opposite with the older carriers).
        # CSA_PACKED_HFUSE=0 restores the packed profile without it.
        # data parallel ("<strategy>:hf"): the same split in GRADIENT mode — the deferred
        # segments store dW / db whole into the flat gradient, the pair backward's tail folds
        # the conv stripes into it, then the exchange and the flat optimizer follow
        dp_hf = bool(self.fused_grad and getattr(self.e, "dp_variant", "") == "hf"
                     and self.e.sync.strategy in ("allreduce", "ps", "async_ps"))
        packed_ok = os.environ.get("CSA_PACKED_HFUSE", "1") == "1"
        if (self.forward_only or not (self.fused or dp_hf) or self.det or self.pair is None
                or (self.packed and not packed_ok) or os.environ.get("CSA_HFUSE", "1") != "1"):
            return
        dense = [u for u in self.units if u.kind == "dense" and u.fused]
        if not dense or len(dense) > 4 or any(u.layer.spec.hidden % 128 for u in dense):
            return
        self.hfuse, self.dp_hf = True, dp_hf
        # the last dense layer's input gradient rides in the head launch (csa_head_dgrad:
        # every workgroup recomputes the head for its rows, no batch reduction), when that
        # layer's input transform is at most an activation
        last = self.units[-1]
        self.head_dgrad = bool(
            self.head_row and last.kind == "dense" and last.fused and len(self.units) > 2
            and not last.in_tf.has_bn
            and self.lib.csa_head_dgrad_ok(self.B, last.layer.spec.hidden, last.layer.in_shape.numel))
        # CSA_DENSE_BRANCH=1: the FIRST dense layer's deferred update (fc1: 980 of the
        # carrying launch's ~1 700 workgroups) runs as its own launch on a side stream — a
        # graph branch from after its input-gradient launch to before the next step's
        # BatchNorm apply that rewrites its operand — instead of inside the pair backward
        # (its weight-gradient operand must be the materialised BatchNorm output, which only
        # the next step's bn_act_apply rewrites: _alloc's xt)
        d0 = dense[0]
        if (not self.dp_hf and os.environ.get("CSA_DENSE_BRANCH", "0") == "1" and d0.in_tf.has_bn
                and d0.layer.in_shape.numel % 4 == 0 and d0 is not self.units[-1]):
            self.br_unit = d0
            self.br_side = dedicated_stream(self.e.device)

    # ------------------------------------------------------------------ deterministic mode
    def _check_det(self) -> None:
        """Deterministic mode covers every one-GPU lowering and allreduce / ps data
        parallelism: the VALU conv pair and the conv units (fixed-order in-workgroup folds;
        one exclusive statistic row and weight-gradient stripe per workgroup, folded in row
        order by csa_rows_fold), standalone BatchNorm units (exclusive statistic rows summed
        in row order by the finalize kernels), gather-form pools (overlapping pools are never
        fused), gconv units (implicit GEMM without split-K), fused dense backward + update
        units (exclusive BN-backward rows, fixed-order column-block hand-off), materialised-
        gradient dense units and dense forwards (no split-K; a BatchNorm'd input's backward
        statistics go to one exclusive slab row per GEMM workgroup, folded in (wave, lane)
        order: gemm.hip), and the row-per-workgroup, partial-row or single-workgroup generic
        heads (head.hip csa_head picks the generic kernel: fixed-order sums, plain stores).
        Only async_ps data parallelism stays outside (pushes applied in arrival order)."""
        e = self.e
        # data parallel: every collective of the step is fixed-order (GradSync.det: the xGMI
        # kernels or an exact all-gather + rank-ordered fold), the stripes are exclusive rows
        # folded in order before the exchange, the dense layers run the fused backward in
        # gradient mode (exclusive BN-backward rows)
        if e.ctx.enabled and e.sync.strategy not in ("allreduce", "ps"):
            # (async_ps applies pushes in arrival order: nondeterministic by definition)
            raise Unsupported(f"deterministic mode: {e.sync.strategy} data parallelism")

    # ------------------------------------------------------------------ dense forwards
    def _plan_splits(self) -> None:
        """Split-K factor of each dense forward (> 1: its output is an atomic accumulator
        that must start at zero)."""
        B = self.B
        for u in self.units:
            if u.kind == "dense":
                fin, fout = u.layer.in_shape.numel, u.layer.spec.hidden
                u.splits_fwd = (self.lib.csa_dd_fwd_splits(B, fout, fin) if u.direct
                                else self.lib.csa_dense_fwd_splits(B, fout, fin))
            elif u.kind == "gconv":
                u.splits_fwd = self.lib.csa_gconv_fwd_splits(self._conv_geom(u.layer, B))

    def _plan_fwd_bn(self) -> None:
        """Dense units whose forward applies the producer's BatchNorm + activation itself
        (``csa_dd_fwd_bn``: xt, the BatchNorm tables and the carried update's pending flag come
        out of the forward's launch) instead of a ``csa_bn_act_apply`` launch in front of
        ``csa_dd_fwd``: a register-direct unit with xt whose shape runs as the wide kernel and
        whose K is a multiple of the producer's channels.  Serving programs, the forward chain
        and a baseline library without the entry point keep the two launches;
        ``CSA_FWD_BN_FUSE=0`` keeps them everywhere (A/B knob)."""
        on = os.environ.get("CSA_FWD_BN_FUSE", "1") != "0" and not self.forward_only
        for u in self.units:
            if on and u.kind == "dense" and u.xt is not None and u.direct and hasattr(self.lib, "csa_dd_fwd_bn"):
                u.fwd_bn = self._fwd_bn_ok(u)

    def _fwd_bn_ok(self, u: Unit) -> bool:
        lp = u.layer
        return bool(_opt_call(self.lib, "csa_dd_fwd_bn_ok", self.B, lp.spec.hidden, lp.in_shape.numel,
                              u.in_tf.slab.shape[2]))

    def _plan_chain(self) -> None:
        """One-GPU program: fc1's forward, fc2's forward and the head launch run as ONE
        launch (``csa_chain_begin`` / ``csa_chain_end``: dense_direct.hip fwd_chain_kernel,
        stages handed over by tickets) instead of three — each launch boundary cost ~2-3 us
        between one launch's last workgroup and the next one's first (scripts/mb/
        graph_life.py, profiles/r6_notes.md).  MEASURED SLOWER, so opt-in (``CSA_FWD_CHAIN=1``):
        a stage hand-off inside the launch — the producer's atomics drained, its ticket RMW,
        the go flag, the consumer's poll and acquire — took 4.5-5.8 us, against ~2.4 us for
        the kernel boundary it replaces (0.0889 vs 0.0753 ms/step, profiles/r6_notes.md)."""
        e = self.e
        try:
            chain_ok = self.lib.csa_chain_ok
        except AttributeError:              # an A/B baseline library (CSA_KERNEL_LIB) without it
            return
        dense = [u for u in self.units if u.kind == "dense"]
        if (e.ctx.enabled or self.det or self.packed or self.forward_only
                or not self.head_dgrad or os.environ.get("CSA_FWD_CHAIN", "0") != "1"
                or len(dense) != 2 or self.units[-2:] != dense or not all(u.direct for u in dense)
                or self.br_unit is not None
                or not chain_ok(self.units[-1].layer.spec.hidden)):
            return
        # counts and spread go flags, each on its own line
        self.chain_tk = torch.zeros(int(self.lib.csa_chain_words()), dtype=torch.int32, device=e.device)
        self.chain_err = torch.zeros(1, dtype=torch.int32, device=e.device)
        self.chain = True
        for u in dense:                     # the chain records csa_dd_fwd: bn_act_apply stays a launch
            u.fwd_bn = False

    # ------------------------------------------------------------------ DP "lowrank"
    def _plan_lowrank(self) -> None:
        """Exact data parallelism for the dense layers without all-reducing their weights.

        A dense weight gradient is ``Σ_ranks T(x_r)ᵀ·dy_r`` — a GEMM whose reduction
        dimension is the per-rank batch (50).  So instead of an RCCL all-reduce of the
        [in, out] gradient (8 MB for fc1 of the sample config; ring collectives over xGMI
        are per-link bound), every rank all-gathers the [B, in] GEMM inputs and the
        [B, out] output gradients (0.9 MB for fc1) and forms the global gradient locally
        with K = world·B on a side stream that overlaps the conv backward.  The 1/world
        mean is already folded into the loss-gradient seed.  Only the small remainder
        (conv, BatchNorm, head: ~25 KB for the sample config) is all-reduced.  A dense
        layer whose input goes through a BatchNorm that is not materialised per rank
        (batch statistics differ between ranks) stays on the all-reduce path."""
        e = self.e
        if not (e.ctx.enabled and e.sync.strategy == "lowrank"):
            return
        W, B, dev = e.ctx.world, self.B, e.device
        offs = self.model.state.offsets
        lr_spans = set()
        for u in self.units:
            if u.kind != "dense" or (u.in_tf.has_bn and u.xt is None):
                continue
            fin, fout = u.layer.in_shape.numel, u.layer.spec.hidden
            u.lr_src = u.xt if u.xt is not None else u.x.view(B, fin)
            u.lr_act = (0, 0.0) if u.xt is not None else (_act_id(u.in_tf.act), _alpha(u.in_tf.act))
            u.lr_x = torch.zeros(W * B, fin, device=dev)
            u.lr_dy = torch.zeros(W * B, fout, device=dev)
            # every rank forms the SAME global dW, so the optimizer update of W / b runs
            # inside that weight-gradient launch (csa_dd_wgrad update mode: dW never exists)
            # where the variables live — as ApplyAdagrad on the PS did
            # (construct_distribute.py:355-357, 372-373)
            u.lr_update = True
            for p in ("weight", "bias"):
                n = f"{u.layer.name}.{p}"
                lr_spans.add((offs[n], offs[n] + self.gviews[n].numel()))
            self.lr_units.append(u)
        # everything else is all-reduced: the other parameters' spans, merged across
        # alignment padding (with the dense-last flat layout that is ONE leading range)
        spans = sorted((o, o + self.gviews[n].numel()) for n, o in offs.items())
        open_range = False
        for a, b in spans:
            if (a, b) in lr_spans:
                open_range = False
            elif open_range:
                self.lr_ranges[-1] = (self.lr_ranges[-1][0], b)
            else:
                self.lr_ranges.append((a, b))
                open_range = True
        # each range's end rounded up to 16 bytes through the alignment padding behind it
        # (never-written zeros): the xGMI kernels take 16-byte multiples only, and a range
        # left on RCCL would be the one collective of this program inside the graph that the
        # peer-buffer path does not carry
        starts = sorted(a for a, _ in spans) + [e.flat.numel()]
        self.lr_ranges = [(a, min(-(-b // 4) * 4, min(x for x in starts if x >= b))) for a, b in self.lr_ranges]
        if self.lr_units:
            self.lr_side = dedicated_stream(dev)
            self.lr_first = min(self.units.index(u) for u in self.lr_units)

    # ------------------------------------------------------------------ DP overlap
    def _plan_grad_buckets(self) -> None:
        """Overlap the RCCL gradient all-reduce with the rest of the backward pass.

        The flat buffer holds layers in DSL order with the head last, and backward runs
        from the head down, so after unit k's backward every parameter of layer index
        >= unit k's main layer is final: a growing contiguous SUFFIX of ``flat_grad``.
        (A norm layer's scale/offset grads come from the route kernel of the conv unit
        BEFORE it, so they join the suffix one unit later — the rule still holds.)
        (A layer / group / instance norm is a ``gn`` unit whose main layer is the norm itself:
        its own backward, ``csa_gn_bwd`` then ``csa_gn_bwd_params``, STORES the scale / offset
        gradients of that layer index before unit k's bucket is issued, and the activation that
        rides in the unit has no parameters — checked against the launches, the rule holds.)
        (A depthwise convolution is a ``dw`` unit whose main layer is the layer itself: its own
        backward, ``csa_dw_bwd`` then ``csa_dw_bwd_params`` in the split form, STORES the weight
        and bias gradients of that layer index before unit k's bucket is issued.)
        Each time the ready suffix has grown by >= ``min_bucket`` bytes it is all-reduced
        on a side stream (captured into the same HIP graph) while the main stream keeps
        computing conv gradients; the optimizer waits for the side stream.  With the
        sample config that is one ~1 MB bucket (head+fc2) launched after fc2, the 8 MB
        fc1 bucket launched right after fc1's weight gradient, and a small tail."""
        e = self.e
        # ps (the parameter-server capability): the same suffix buckets are REDUCE-SCATTERED
        # to their owner shards (GradSync.reduce_scatter_range; xGMI: one launch per bucket,
        # every element leaves its GPU at most once) while the backward continues — only
        # when EVERY bucket's range reduce-scatter measured faster on the xGMI kernel than
        # on RCCL (GradSync.rs_choice, decided below): on RCCL the per-owner reduces per
        # bucket measured 0.156 ms/step at world 1 against 0.107 for one reduce-scatter
        # after the backward (profiles/r4_notes.md)
        # (the ":hf" program forms every dense gradient inside the pair backward launch:
        # nothing is ready early, one exchange after the backward)
        self.overlap = (e.ctx.enabled and e.sync.strategy in ("allreduce", "ps")
                        and (e.sync.strategy == "allreduce" or e.sync.xgmi is not None)
                        and not self.dp_hf
                        and os.environ.get("CSA_DP_OVERLAP", "1") == "1")
        if not self.overlap:
            return
        self.side = dedicated_stream(e.device)      # (captured: outside torch's stream pool)
        offs = e.model.state.offsets
        end = e.flat.numel()

        def frontier(layer_index: int) -> int:
            c = [o for n, o in offs.items()
                 if n.startswith("head.") or int(n.split(".")[1]) >= layer_index]
            return min(c) if c else end

        min_elems = int(os.environ.get("CSA_DP_MIN_BUCKET", str(512 << 10))) // 4
        hi = end
        points = [("head", frontier(10 ** 9))] + [(k, frontier(self.units[k].layer.index))
                                                  for k in range(len(self.units) - 1, -1, -1)]
        for i, (key, f) in enumerate(points):
            last = i == len(points) - 1
            lo = 0 if last else f
            if hi - lo >= min_elems or (last and hi > lo):
                self.bucket_at[key] = (lo, hi)
                hi = lo
        if e.sync.strategy == "ps":
            # every bucket's path decided now (collectively, timed under CSA_XGMI=auto)
            paths = [e.sync.rs_choice(e.flat_grad, e.grad_shard, lo, hi) for lo, hi in self.bucket_at.values()]
            if any(ch is None for ch in paths):
                self.overlap, self.bucket_at = False, {}

    # ------------------------------------------------------------------ DP deferred update
    def _plan_carry(self) -> None:
        """Data-parallel all-reduce programs: the dense layers' parameter update, which must
        follow the gradient exchange, runs as extra workgroups of the NEXT step's pair
        forward (conv_pair.hip ``CPOptCarry``) instead of in the flat optimizer launch after
        the exchange — those parameters are read again only by that step's dense forwards.
        The flat optimizer launch keeps the rest (conv, BatchNorm, head parameters and the
        side jobs) and raises a device flag; ``flush`` applies a pending update before any
        host read of the parameters (TrainEngine.flush_params).  Only gradients stored whole
        every step (keep ranges) are carried: the carry does not zero accumulators."""
        e = self.e
        if (not e.ctx.enabled or e.sync.strategy != "allreduce" or e.aps is not None or self.pair is None
                or os.environ.get("CSA_DP_CARRY", "1") != "1"
                or not self.lib.csa_conv_pair_valu_ok(K.ints(self.pair))):
            return
        offs = self.model.state.offsets
        keep = set(self.keep_ranges)
        carried = set()
        for u in self.units:
            if u.kind != "dense" or (u.fused and self.fused) or u.lr_update:
                continue
            names = [f"{u.layer.name}.weight", f"{u.layer.name}.bias"]
            if not all(self._keep_range(nm) in keep for nm in names):
                continue
            for nm in names:
                carried.add(offs[nm])
        if not carried:
            return
        segs = self._float4_segments(lambda o: o in carried)
        if len(segs) > 4:
            return
        m4 = sum(hi - lo for lo, hi in segs) // 4
        self.carry = segs
        self.carry_offsets = carried
        self.carry_blocks = max(1, min(1024, -(-m4 // 256)))
        # the pending flag: set by the optimizer launch, read by the carrying forward, cleared
        # by the launch right after it (bn_act_apply, when the first dense layer takes the
        # pair's BatchNorm output; else only by a flush)
        self.carry_pending = torch.zeros(1, dtype=torch.int32, device=e.device)
        u2 = self.units[2] if len(self.units) > 2 else None
        self.carry_clear = bool(u2 is not None and u2.kind == "dense" and u2.xt is not None)

    def _opt_segments(self):
        """Flat [lo, hi) spans the optimizer launch updates: everything except the
        parameters a fused dense backward already updated."""
        offs = self.model.state.offsets
        skip = set(self.carry_offsets if self.carry else set())
        for u in self.units:
            if u.kind == "dense" and ((u.fused and self.fused) or u.lr_update):
                skip |= {offs[f"{u.layer.name}.weight"], offs[f"{u.layer.name}.bias"]}
        if not skip:
            return []
        segs = self._float4_segments(lambda o: o not in skip)
        assert len(segs) <= 16, "at most 15 fused dense layers (_plan_fused)"
        return segs

    # ------------------------------------------------------------------ pair-backward tail
    def _plan_tail(self) -> None:
        """Round 5: the one-GPU fused program without an optimizer launch.

        After horizontal fusion the flat optimizer launch only updated the conv pair's
        (striped) and the BatchNorm's parameters, zeroed the next step's accumulators and
        staged the next batch — 8.1 us of a ~88 us step (profiles/r4_step_trace.md).  Now:

        * the conv / BN updates, the statistic-slab zeroing and the batch staging run as
          TAIL workgroups of the pair backward launch (``csa_conv_pair_tail_set``), which
          wait (bounded) for the pair workgroups — done ~7 us before that launch's dense
          update workgroups;
        * the head's parameters are updated in place by the last dense segment's head
          epilogue (``csa_dense_update_head_params``), which also writes the metric ring;
        * the dense forwards' split-K outputs, read until the end of the pair backward, are
          zeroed by the NEXT step's pair forward threads (its zero list).

        Applies to the horizontal-fusion program with the staged batch and the row head
        when every other parameter and accumulator is one of those (``CSA_PAIR_TAIL=0``
        restores the optimizer launch)."""
        if self.dp_hf:
            self._plan_tail_fold()
            return
        if not (self.hfuse and self.staged and self.head_row
                and self.pair is not None and os.environ.get("CSA_PAIR_TAIL", "1") == "1"):
            return
        ua, ub = self.units[0], self.units[1]
        if not (ua.wg_stripes > 1 and ub.wg_stripes == ua.wg_stripes and not ua.row_fold
                and ua.wg_stripes <= 16):
            return
        nt = self._next_tf(1)
        offs = self.model.state.offsets
        fused = {f"{u.layer.name}.{p}" for u in self.units if u.kind == "dense" and u.fused for p in ("weight", "bias")}
        params = []           # (name, src tensor, S, ld, zero)
        for u, acc, nm in ((ua, ua.dw_acc, "weight"), (ua, ua.db_acc, "bias"), (ub, ub.dw_acc, "weight"),
                           (ub, ub.db_acc, "bias")):
            if acc is not None:
                params.append((f"{u.layer.name}.{nm}", acc, u.wg_stripes, acc.shape[1], 1))
        if nt.has_bn:
            for pn in ("scale", "offset"):
                n = f"{nt.norm.name}.{pn}"
                params.append((n, self.gviews[n], 1, self.gviews[n].numel(), 0))
        rest = set(offs) - fused - {p[0] for p in params} - {"head.weight", "head.bias"}
        if rest or len(params) > 8:
            return                      # parameters the tail does not know about
        # zero regions: the BN statistic slabs (read by every pair workgroup) in the tail,
        # the dense split-K outputs at the next pair forward; anything else: no tail
        slabs = []
        for u in self.units:
            if u.in_tf.has_bn:
                slabs += [u.in_tf.slab.view(-1), u.in_tf.bwd_slab.view(-1)]
        ys = [u.y.view(-1) for u in self.units if u.kind == "dense" and u.splits_fwd > 1]
        regions = self.zero_regions + self.zero_early
        ptrs = {t.data_ptr() for t in slabs} | {t.data_ptr() for t in ys}
        # (the pair forward's zero list holds FWD_ZERO_MAX entries and one of them is the
        # tail's tickets: more split-K outputs than the rest keep the optimizer launch)
        if (any(r.data_ptr() not in ptrs for r in regions) or len(slabs) > 4
                or len(ys) + 1 > self.FWD_ZERO_MAX):
            return
        if any(t.numel() % 4 or t.data_ptr() % 16 for t in ys):
            return
        s0, s1 = self._slots()

        def slot(s, name):
            return None if s is None else s[offs[name]:]

        self.tail_zero = [t for t in slabs if any(r.data_ptr() == t.data_ptr() for r in regions)]
        self.fwd_zero = [t for t in ys if any(r.data_ptr() == t.data_ptr() for r in regions)]
        self.head_params = (self.views["head.weight"], self.views["head.bias"], slot(s0, "head.weight"),
                            slot(s1, "head.weight"), slot(s0, "head.bias"), slot(s1, "head.bias"))
        self._tail_table(self.e.opt_id, [
            (self.views[n], slot(s0, n), slot(s1, n), src, S, ld, self.views[n].numel(), z)
            for n, src, S, ld, z in params], fold=0)
        # the tickets are zeroed by the NEXT step's pair forward (no closing reset counter in
        # the carrier's tail: conv_pair.hip cp_tail_body)
        self.fwd_zero.append(self.tail_tk)
        assert len(self.fwd_zero) <= self.FWD_ZERO_MAX
        self.tail = self.tail_update = True

    def _plan_tail_fold(self) -> None:
        """The ":hf" data-parallel program's tail: fold the pair's weight-gradient stripes
        into the flat gradient (stored sums, no update) before the exchange — the optimizer
        launch after the exchange keeps the updates, zeroing and staging."""
        ua, ub = self.units[0], self.units[1]
        if not (ua.tail_fold and ua.wg_stripes > 1 and ua.wg_stripes <= 16):
            raise Unsupported("data-parallel :hf program: the pair stripes need the tail fold")
        G = self.gviews
        jobs = []
        for u in (ua, ub):
            lp = u.layer
            for acc, p in ((u.dw_acc, "weight"), (u.db_acc, "bias")):
                if acc is not None:
                    dst = G[f"{lp.name}.{p}"].view(-1)
                    jobs.append((dst, None, None, acc, u.wg_stripes, acc.shape[1], dst.numel(), 1))
        self._tail_table(0, jobs, fold=1)
        self.fwd_zero = [self.tail_tk]            # (zeroed by the next step's pair forward)
        self.tail = True

    def _tail_table(self, opt_id: int, jobs, fold: int) -> None:
        """The tail's tickets, error / debug words and its parameter workgroups' table (one
        entry per 256 elements of a parameter).  ``jobs``: up to 8 of (destination, slot 0,
        slot 1, source, stripes, row stride, elements, zero the source)."""
        e = self.e
        self.tail_tk = torch.zeros(int(self.lib.csa_conv_pair_tail_ticket_words()), dtype=torch.int32,
                                   device=e.device)                           # spread tickets
        self.tail_err = torch.zeros(1, dtype=torch.int32, device=e.device)
        self.tail_force = torch.zeros(1, dtype=torch.int32, device=e.device)   # debug: arm_tail_timeout
        n = len(jobs)
        P, I8 = C.c_void_p * 8, C.c_int * 8
        ns = I8(*[j[6] for j in jobs])
        nbytes = int(self.lib.csa_conv_pair_tail_table_bytes(ns, n))
        self.tail_table = torch.zeros((nbytes + 15) // 16 * 4, dtype=torch.float32, device=e.device)
        torch.cuda.synchronize(e.device)
        self.tail_blocks = int(self.lib.csa_conv_pair_tail_plan(
            K.ptr(self.tail_table), opt_id, n, P(*[j[0].data_ptr() for j in jobs]),
            P(*[K.ptr(j[1]) for j in jobs]), P(*[K.ptr(j[2]) for j in jobs]),
            P(*[j[3].data_ptr() for j in jobs]), I8(*[j[4] for j in jobs]),
            I8(*[j[5] for j in jobs]), ns, I8(*[j[7] for j in jobs]), fold))
        if self.tail_blocks < 1:
            raise RuntimeError(f"conv_pair_tail_plan failed: {self.tail_blocks}")
