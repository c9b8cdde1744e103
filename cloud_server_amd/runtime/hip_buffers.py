"""State and buffers of the HIP step program: every field the planners fill, declared, and
the allocation: activations and gradients per unit, statistic slabs, the accumulators that
start every step at zero, the staged and the augmented batch."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import List, Optional

import torch

from ..models.dsl import AvgPoolSpec, LayerPlan
from ..ops import augment_ref
from ..ops import fused as K
from .hip_plan import Transform, Unit, Unsupported, _opt_call, _set_nt_out


class Buffers:
    # ---- plan state: every field a planner or ``_alloc`` fills, with the value it has when
    # that planner does not apply or never runs (``forward_only`` stops after the forward's
    # plan); the containers are made per program in ``__init__``.  (``aug_c``, ``aug_rows``
    # and ``aug_cur`` exist only beside ``aug``.)
    fused = False            # _plan_fused: one GPU, dense backward + update in one launch
    fused_grad = False       # ... data parallel: the same launch in gradient mode
    head_rg = 0              # rows per workgroup of the partial-row head (0: another head)
    head_row = False         # one batch row per workgroup
    head_sep = False         # ... with its weight gradient as a separate launch
    pair = None              # _plan_pair: the leading conv pair's geometry
    pair_tabs = None         # ... its backward's per-band index tables (_plan_pair_tables)
    pair_c1 = None           # ... the conv-A tiles its forward stores for its backward (_alloc)
    hfuse = False            # _plan_hfuse: dense updates deferred into the pair backward launch
    dp_hf = False            # ... in gradient mode (data-parallel ":hf")
    head_dgrad = False       # the last dense layer's input gradient rides in the head
    br_unit = br_side = None    # CSA_DENSE_BRANCH: the unit whose update is a graph branch, its stream
    _br_pending = False
    x_dense_in = None        # _alloc: the gathered float input when the first unit is no conv
    dlast = None             # the head's input gradient
    hdl = hrl = hrc = None   # row head: per-row dlogits, loss, correct
    head_part = head_mloss = head_mcorr = None      # partial-row head: per-group outputs
    head_kw = 0
    lr_side, lr_first = None, -1    # _plan_lowrank: the side stream, the first lowrank unit
    ps_mode = False          # _collect_zero_regions: sharded parameters
    head_ws = None           # the atomic head's arrival counter + sums
    staged = False           # _plan_stage: the batch is staged at fixed addresses
    stage_img = stage_lbl = None
    aug = None               # _plan_augment: ops.augment_ref.Plan when options.augment is active
    aug_img = None           # ... and this step's augmented batch, uint8 [B, 784]
    overlap = False          # _plan_grad_buckets: gradient buckets exchanged during the backward
    side = None
    carry = None             # _plan_carry: flat segments updated by the NEXT step's pair forward
    carry_blocks = 0
    carry_pending = None     # device flag: an update is pending
    carry_clear = False      # ... and the launch after the pair forward clears it
    tail = False             # _plan_tail: the pair backward launch has tail workgroups
    tail_update = False      # ... which do the optimizer launch's work
    head_params = None
    tail_tk = tail_err = tail_force = tail_table = None
    tail_blocks = 0
    chain = False            # _plan_chain: the dense forwards and the head as one launch
    chain_tk = chain_err = None
    _eval_bn = False         # predict: BN with running statistics (no batch-stat slabs)
    _predicting = False      # inside the forward-only pass
    _aps_dummy = None        # async_ps: the optimizer launch's scratch operands

    def __init__(self, eng, forward_only: bool = False):
        """``forward_only``: the serving program (``serve.hip_infer``) — the same forward
        launches over another engine's weights, with no gradient, optimizer, staging or
        collective state (``eng`` then needs only cfg/device/model/flat/ctx/data/stream)."""
        self.e = eng
        self.forward_only = forward_only
        self.lib = K.load(required=True)
        _set_nt_out(self.lib)
        if eng.device.type != "cuda":
            raise Unsupported("HIP program needs a GPU device")
        # CSA_DETERMINISTIC=1: bitwise-reproducible steps on the same kernels (det.hip):
        # exclusive slab rows / weight-gradient stripes per workgroup, fixed-order folds,
        # no split-K.  The library flag is process state: set around every planning and
        # launch sequence of this program, restored afterwards.
        self.det = bool(getattr(eng, "deterministic", False)) and not forward_only
        # packed profile (engines built to run as branches of one multi-job graph): launch
        # shapes with less CU-time per step (conv_pair.hip, dense_update.hip)
        # (CSA_PACKED_PROFILE=0: packed engines keep the one-job launch shapes — A/B knob)
        self.packed = bool(getattr(eng, "packed", False)) and os.environ.get("CSA_PACKED_PROFILE", "1") == "1"
        # shared-GPU profile (several ranks of this job on ONE device): no 16-wave
        # workgroups (dense_update.hip du_cs; profiles/r5_notes.md, the world-2 stall)
        self.shared_gpu = bool(getattr(eng, "shared_gpu", False))
        self.units, self.head_tf = [], Transform()      # _lower: the launch units, the head's input transform
        self.lr_units, self.lr_ranges = [], []          # _plan_lowrank: gathered-operand units, all-reduced ranges
        # _collect_zero_regions: cleared by the optimizer launch (<= 16) / at the start of the step;
        # conv weight-gradient stripes; flat gradient ranges stored whole every step
        self.zero_regions, self.zero_early, self.stripe_bufs, self.keep_ranges = [], [], [], []
        self.bucket_at = {}                             # "head" / unit index -> flat range ready after it
        self.carry_offsets, self.opt_segments = set(), []   # carried parameters; the optimizer's segments ([]: all)
        self.fwd_zero, self.tail_zero = [], []          # zeroed by the pair forward's threads / by the tail
        with self._det_scope():
            self._init_plan(eng)

    @contextlib.contextmanager
    def _det_scope(self):
        lib = self.lib
        prev = (int(lib.csa_deterministic()), int(lib.csa_packed()), int(lib.csa_shared_gpu()))
        lib.csa_set_deterministic(1 if self.det else 0)
        lib.csa_set_packed(1 if self.packed else 0)
        lib.csa_set_shared_gpu(1 if self.shared_gpu else 0)
        try:
            yield
        finally:
            lib.csa_set_deterministic(prev[0])
            lib.csa_set_packed(prev[1])
            lib.csa_set_shared_gpu(prev[2])

    def _rc(self, rc: int, what: str, positive_ok: bool = False) -> int:
        """Negative: an error; so is positive, unless the launcher returns a count (``positive_ok``)."""
        if rc < 0 or (rc > 0 and not positive_ok):
            raise RuntimeError(f"{what} failed: {rc}")
        return rc

    def _init_plan(self, eng) -> None:
        self.B = eng.cfg.batch_size
        self.model = eng.model
        # SyncBN under DP: forward {sum, sumsq} slabs and backward {sum dz, sum dz*xhat}
        # slabs are all-reduced between their producer and consumer launches, counts
        # become global, and the BN parameter gradients (formed from the GLOBAL backward
        # sums) are scaled by 1/world before the gradient all-reduce adds them up again
        self.sync_bn = bool(eng.model.sync_bn)
        self.W = eng.ctx.world if self.sync_bn else 1
        self.views = eng.model.state.views(eng.flat)
        self.gviews = {} if self.forward_only else eng.model.state.views(eng.flat_grad)
        self._lower()
        self._plan_fused()
        self._plan_pair()
        self._plan_hfuse()
        if self.det:
            self._check_det()
        self._alloc()
        self._plan_splits()
        self._plan_fwd_bn()
        self._plan_pair_tables()
        if self.forward_only:
            return
        self._plan_lowrank()
        self._collect_zero_regions()
        self._zero_now()
        self._plan_stage()
        self._plan_augment()
        self._plan_grad_buckets()
        self._plan_carry()
        self.opt_segments = self._opt_segments()
        self._plan_tail()
        self._plan_chain()

    # ------------------------------------------------------------------ geometry (the launchers' int arrays)
    @staticmethod
    def _conv_geom(lp: LayerPlan, B: int):
        sp = lp.spec
        h, w = lp.in_shape.hw
        oh, ow = lp.out_shape.hw
        return K.ints([B, h, w, lp.in_shape.c, sp.kh, sp.kw, sp.stride[0], sp.stride[1],
                       lp.pads[0], lp.pads[2], oh, ow, sp.cout])

    @staticmethod
    def _pool_geom(u: Unit):
        if u.pool is None:
            return K.ints([0] * 9)
        lp = u.pool
        sp = lp.spec
        oh, ow = lp.out_shape.hw
        return K.ints([1, sp.kernel[0], sp.kernel[1], sp.stride[0], sp.stride[1],
                       lp.pads[0], lp.pads[2], oh, ow])

    def _pool_geom_full(self, u: Unit):
        lp = u.layer
        sp = lp.spec
        h, w = lp.in_shape.hw
        oh, ow = lp.out_shape.hw
        return K.ints([self.B, h, w, lp.in_shape.c, sp.kernel[0], sp.kernel[1], sp.stride[0], sp.stride[1],
                       lp.pads[0], lp.pads[2], oh, ow])

    def _lrn_geom(self, lp: LayerPlan):
        """{rows, C, depth_radius} of an lrn layer: a row is one pixel's channels."""
        h, w = lp.in_shape.hw
        return K.ints([self.B * h * w, lp.in_shape.c, lp.spec.depth_radius])

    @staticmethod
    def _lrn_consts(lp: LayerPlan):
        sp = lp.spec
        return (float(sp.bias), float(sp.alpha), float(sp.beta))

    def _gn_geom(self, lp: LayerPlan):
        """{B, HW, C, G} of a layer / group / instance norm; a flat input has HW = 1, C = F."""
        sh = lp.in_shape
        hw = sh.hw[0] * sh.hw[1] if sh.is_spatial else 1
        return K.ints([self.B, hw, sh.c, lp.spec.groups])

    def _dw_geom(self, lp: LayerPlan):
        """{B, H, W, C, kh, kw, sh, sw, pad_top, pad_left, OH, OW, M} of a depthwise convolution."""
        sp = lp.spec
        h, w = lp.in_shape.hw
        oh, ow = lp.out_shape.hw
        return K.ints([self.B, h, w, lp.in_shape.c, sp.kh, sp.kw, sp.stride[0], sp.stride[1],
                       lp.pads[0], lp.pads[2], oh, ow, sp.mult])

    @staticmethod
    def _bn_channels(u: Unit) -> int:
        """Channel count of a bn unit: C of an NHWC tensor, the features of a 2-D one."""
        sh = u.layer.in_shape
        return sh.c if sh.is_spatial else sh.numel

    # ------------------------------------------------------------------ buffers
    def _alloc(self) -> None:
        dev, B = self.e.device, self.B
        f32 = dict(device=dev, dtype=torch.float32)
        fo = self.forward_only
        prev: Optional[Unit] = None
        for u in self.units:
            u.x = prev.y if prev is not None else None
            if prev is None and u.kind != "conv":
                # first unit reads no raw images: materialise the gathered float input once
                # per step (NHWC [B, 28, 28, 1] for a bn / pool / lrn / gn / dw unit)
                self.x_dense_in = torch.zeros(B, u.layer.in_shape.numel, **f32)
                ish = u.layer.in_shape
                u.x = (self.x_dense_in if u.kind == "dense" or not ish.is_spatial
                       else self.x_dense_in.view(B, ish.hw[0], ish.hw[1], ish.c))
            lp = u.layer
            if u.kind == "drop":
                u.y = torch.zeros_like(u.x)
                # the step whose mask the forward drew (the backward redraws that one)
                u.used_step = torch.zeros(1, dtype=torch.int64, device=dev)
            elif u.kind == "lrn":
                u.y = torch.zeros_like(u.x)
                u.lrn_s = None if fo else torch.zeros_like(u.x)
            elif u.kind == "gn":
                u.y = torch.zeros_like(u.x)
                if not fo:                       # (both stored whole every step: no zero regions)
                    u.gn_stat = torch.zeros(B, lp.spec.groups, 2, **f32)
                    u.gn_slab = torch.zeros(B, 2, lp.in_shape.c, **f32)
            elif u.kind == "dw":
                oh, ow = lp.out_shape.hw
                u.y = torch.zeros(B, oh, ow, lp.out_shape.c, **f32)
                if not fo:
                    geom = self._dw_geom(lp)
                    u.dw_form = int(self.lib.csa_dw_bwd_form(geom))
                    if u.dw_form == 1:           # (every row stored whole every step: no zero regions)
                        row = (lp.spec.kh * lp.spec.kw + 1) * lp.out_shape.c
                        u.dw_slab = torch.zeros(int(self.lib.csa_dw_slab_rows(geom)), row, **f32)
            elif u.kind == "bn":
                u.y = torch.zeros_like(u.x)
                ch = self._bn_channels(u)
                if u.norm is not None:
                    R = self.lib.csa_bn_stat_rows(u.x.numel() // ch)
                    u.bn_tab = torch.zeros(4, ch, **f32)
                    u.bn_slab = torch.zeros(R, 2, ch, **f32)
                    if not fo:
                        u.bn_bslab = torch.zeros(R, 2, ch, **f32)
                        u.bn_k = torch.zeros(2, ch, **f32)
            elif u.kind == "pool":
                ph, pw = lp.out_shape.hw
                u.y = torch.zeros(B, ph, pw, lp.out_shape.c, **f32)
                if not isinstance(lp.spec, AvgPoolSpec):
                    u.argmax = torch.zeros(B, ph, pw, lp.out_shape.c, device=dev, dtype=torch.uint8)
            elif u.kind == "gconv":
                oh, ow = lp.out_shape.hw
                u.y = torch.zeros(B, oh, ow, lp.spec.cout, **f32)
            elif u.kind == "conv":
                oh, ow = lp.out_shape.hw
                if u.pool is not None:
                    ph, pw = u.pool.out_shape.hw
                    u.y = torch.zeros(B, ph, pw, lp.out_shape.c, **f32)
                    u.argmax = torch.zeros(B, ph, pw, lp.out_shape.c, device=dev, dtype=torch.uint8)
                else:
                    u.y = torch.zeros(B, oh, ow, lp.out_shape.c, **f32)
                u.dc = None if fo else torch.zeros(B, oh, ow, lp.out_shape.c, **f32)
            else:
                u.y = torch.zeros(B, lp.spec.hidden, **f32)
            u.dy = None if fo else torch.zeros_like(u.y)
            prev = u
        # forward stat slabs: the unit BEFORE a transform with norm produces the slab
        for k, u in enumerate(self.units):
            tf = u.in_tf
            if tf.has_bn:
                src = self.units[k - 1]
                ph, pw = src.y.shape[1], src.y.shape[2]
                # (deterministic mode: one row per producer workgroup, folded to row 0)
                if self.det and self.pair is not None and k == 2:
                    nslab = int(self.lib.csa_conv_pair_grid(K.ints(self.pair)))
                else:
                    nslab = self.lib.csa_conv_fwd_nslab(self._conv_geom(src.layer, B), self._pool_geom(src))
                tf.prod_rows = nslab
                tf.slab = torch.zeros(nslab, 2, src.y.shape[3], **f32)
                tf.nslab = 1 if self.det else nslab
                tf.count = float(B * ph * pw * self.W)
                if fo:
                    continue
                # backward slab is produced by THIS unit's dgrad
                ch = src.y.shape[3]
                if u.kind == "dense" and u.fused:
                    nb = self.lib.csa_dense_bwd_update_slabs(u.layer.in_shape.numel)
                elif u.kind == "dense":
                    nb = self.lib.csa_dense_dgrad_slabs(B, u.layer.in_shape.numel, u.layer.spec.hidden)
                else:
                    nb = self.lib.csa_conv_dgrad_nslab(self._conv_geom(u.layer, B))
                tf.bwd_slab = torch.zeros(nb, 2, ch, **f32)
                tf.bwd_nslab = nb
                if self.det:            # one row per row group (csa_dense_bwd_update_slabs)
                    tf.bwd_prod_rows, tf.bwd_nslab = nb, 1
        # dense consumers of a BatchNorm'd tensor get it materialised once per step
        for u in self.units:
            if u.kind == "dense" and u.in_tf.has_bn and u.layer.in_shape.numel % 4 == 0:
                u.xt = torch.zeros(B, u.layer.in_shape.numel, **f32)
            if u.kind == "dense" and u.fused and not fo:
                # partial input-gradient slabs + per-row-group arrival tickets when the
                # kernel splits a row group over column blocks (the last arriver resets
                # its ticket; zero-initialised here)
                ws = (C.c_longlong * 2)()
                self.lib.csa_dense_bwd_update_ws(u.layer.in_shape.numel, u.layer.spec.hidden, ws)
                u.du_part = torch.zeros(max(int(ws[0]), 1), **f32)
                u.du_cnt = torch.zeros(max(int(ws[1]), 1), dtype=torch.int32, device=dev)
            # BatchNorm tables [mean | rstd | a | b][C] written once per step by the
            # bn_act_apply that materialises xt (the fused dense backward's epilogue reads
            # them instead of reducing the statistic slab again)
            u.in_tf.bn_tab = torch.zeros(4, u.in_tf.slab.shape[2], **f32) if u.xt is not None else None
        self.dlast = self.units[-1].dy     # head input grad (None: forward only)
        if self.head_row:
            self.hdl = torch.zeros(B, 10, **f32)                            # dlogits rows
            self.hrl = torch.zeros(B, **f32)                                # per-row loss
            self.hrc = torch.zeros(B, dtype=torch.int32, device=dev)        # per-row correct
        if self.head_rg:
            kh = self.dlast[0].numel()
            groups = -(-B // self.head_rg)
            # per-group dWh | dbh, rows padded to float4 (the optimizer's fold then reads
            # whole float4s: an odd row stride sent every head float4 down the per-element
            # path, 4 dependent round trips, 7 us of the 8.6 us launch)
            self.head_part = torch.zeros(groups, (kh * 10 + 10 + 3) // 4 * 4, **f32)
            self.head_kw = kh * 10
            self.head_mloss = torch.zeros(groups, **f32)
            self.head_mcorr = torch.zeros(groups, dtype=torch.int32, device=dev)
        # c1 reuse: the conv-A tiles the VALU pair forward stores for the pair backward
        # (band-tile layout, csa_conv_pair_c1_size; CSA_PAIR_C1=0: the backward recomputes
        # them).  Training programs of the VALU family only: serving never stores, the
        # deterministic backward (cpv_bwd) and the MFMA-forward family keep the recompute.
        if (self.pair is not None and not fo and not self.det and os.environ.get("CSA_PAIR_C1", "1") == "1"
                and self.lib.csa_conv_pair_valu_ok(K.ints(self.pair))):
            n = _opt_call(self.lib, "csa_conv_pair_c1_size", K.ints(self.pair))
            if n is not None and int(n) > 0:
                self.pair_c1 = torch.zeros(int(n), **f32)

    def _collect_zero_regions(self) -> None:
        """Accumulators that must start every step at zero.  ``zero_regions`` are cleared
        by the optimizer's zero-list pass; flat-gradient accumulators are cleared by the
        update itself (each thread zeroes the gradient it read — a separate pass over the
        same memory would race with the reads), except under the sharded "ps" strategy,
        where the update reads the reduce-scattered shard and the flat ranges go to the
        zero list; conv weight-gradient stripes are cleared by the fold that reads them."""
        B = self.B
        regs: List[torch.Tensor] = []
        flat: List[torch.Tensor] = []
        fold_budget = 8 - (2 if self.head_rg else 0)
        for k, u in enumerate(self.units):
            lp = u.layer
            if u.kind == "dense":
                fin, fout = lp.in_shape.numel, lp.spec.hidden
                if u.splits_fwd > 1:
                    regs.append(u.y)
                if u.fused:
                    continue                     # plain stores; W never has a gradient buffer
                if k > 0:
                    tfm = u.in_tf.has_bn or u.in_tf.act is not None
                    if self.lib.csa_dense_dgrad_splits(B, fin, fout, int(tfm)) > 1:
                        regs.append(self.units[k - 1].dy)
                if self.lib.csa_dense_wgrad_splits(B, fin, fout) > 1:
                    flat.append(self.gviews[f"{lp.name}.weight"].view(-1))
                    flat.append(self.gviews[f"{lp.name}.bias"])
            elif u.kind == "gconv":
                geom = self._conv_geom(lp, B)
                if u.splits_fwd > 1:
                    regs.append(u.y.view(-1))
                if k > 0 and self.lib.csa_gconv_dgrad_splits(geom) > 1:
                    regs.append(self.units[k - 1].dy.view(-1))
                if self.lib.csa_gconv_wgrad_splits(geom, int(bool(lp.spec.bias))) > 1:
                    flat.append(self.gviews[f"{lp.name}.weight"].view(-1))
                    if lp.spec.bias:
                        flat.append(self.gviews[f"{lp.name}.bias"])
            elif u.kind == "bn":
                if u.norm is not None:        # atomic stat rows (forward and backward)
                    regs += [u.bn_slab.view(-1), u.bn_bslab.view(-1)]
            elif u.kind == "conv":
                # conv weight gradients: S stripes on one GPU (folded by the optimizer:
                # at most 8 folds, the head's partials included), otherwise accumulated
                # straight into the flat gradient (data parallelism, or beyond that budget)
                nf = 1 + (1 if lp.spec.bias else 0)
                S = 1 if self.e.ctx.enabled or fold_budget < nf else self.WGRAD_STRIPES
                # the conv pair's stripes are folded right after the pair backward (fixed-order
                # csa_rows_fold into the flat gradient) in deterministic mode — one stripe per
                # workgroup — and under data parallelism, where the gradient must be complete
                # before its all-reduce (700 workgroups adding into ONE copy contend: the pair
                # backward took 37 us instead of 25)
                # — and every conv unit's in deterministic mode (one stripe per wgrad workgroup)
                in_pair = self.pair is not None and k < 2
                # (":hf": the pair backward's tail folds the stripes into the flat gradient)
                u.tail_fold = in_pair and self.dp_hf
                u.row_fold = self.det or (in_pair and self.e.ctx.enabled and not u.tail_fold)
                if u.tail_fold:
                    S = self.WGRAD_STRIPES
                if u.row_fold:
                    if not self.det:
                        S = self.WGRAD_STRIPES
                    elif in_pair:
                        S = int(self.lib.csa_conv_pair_grid(K.ints(self.pair)))
                    else:
                        S = int(self.lib.csa_conv_wgrad_blocks(self._conv_geom(lp, B), int(bool(lp.spec.bias))))
                        if S <= 0:
                            raise Unsupported(f"conv unit {lp.name}: no weight-gradient plan")
                elif S > 1:
                    fold_budget -= nf
                u.wg_stripes = S
                nw = self.gviews[f"{lp.name}.weight"].numel()
                if S > 1:       # zeroed by the fold that reads them (their only reader)
                    u.dw_acc = torch.zeros(S, nw, device=self.e.device)
                    u.db_acc = torch.zeros(S, lp.spec.cout, device=self.e.device) if lp.spec.bias else None
                    self.stripe_bufs += [t for t in (u.dw_acc, u.db_acc) if t is not None]
                else:
                    u.dw_acc = self.gviews[f"{lp.name}.weight"]
                    u.db_acc = self.gviews[f"{lp.name}.bias"] if lp.spec.bias else None
                    flat.append(u.dw_acc.view(-1))
                    if lp.spec.bias:
                        flat.append(u.db_acc.view(-1))
                if u.pool is not None:
                    pk, ps = u.pool.spec.kernel, u.pool.spec.stride
                    if tuple(pk) != tuple(ps):
                        regs.append(u.dc.view(-1))
        # the atomic head accumulates dWh/dbh across its row-group workgroups (the
        # partial-output head of the fused program writes per-group rows instead)
        if not self.head_rg:
            flat.append(self.e.flat_grad[self.e.model.state.offsets["head.weight"]:])
        self.head_ws = torch.zeros(4, dtype=torch.int32, device=self.e.device)   # arrival counter + sums
        for u in self.units:
            if u.in_tf.has_bn:
                regs.append(u.in_tf.slab.view(-1))          # forward stats (atomic rows)
                regs.append(u.in_tf.bwd_slab.view(-1))      # every producer folds rows atomically
        # dense weight gradients produced without split-K are STORED whole every step (by the
        # fused dense backward, the separate wgrad or the lowrank wgrad), so the optimizer
        # skips re-zeroing them (keep ranges, float4-aligned: the flat layout aligns to 64)
        for u in self.units:
            if u.kind != "dense" or (u.fused and self.fused) or u.lr_update:
                continue                         # (updated in-kernel: no gradient in memory)
            fin, fout = u.layer.in_shape.numel, u.layer.spec.hidden
            m = B * (self.e.ctx.world if u in self.lr_units else 1)
            # the fused backward in gradient mode stores dW / db whole every step
            if (u.fused and self.fused_grad) or self.lib.csa_dense_wgrad_splits(m, fin, fout) == 1:
                self.keep_ranges += [self._keep_range(f"{u.layer.name}.{p}") for p in ("weight", "bias")]
        if self.head_row:
            self.keep_ranges += [self._keep_range(n) for n in ("head.weight", "head.bias")
                                 if self.gviews[n].numel() >= 4]
        # sharded parameters (ps, async_ps): the update reads a shard, the flat gradient is
        # zeroed through the zero list after the exchange consumed it
        self.ps_mode = self.e.sync.sharded
        regions = regs + (flat if self.ps_mode else [])
        # the optimizer's zero list holds 16; any further accumulators are cleared at the
        # start of the step instead (one fill launch each, inside the same graph)
        self.zero_regions, self.zero_early = regions[:16], regions[16:]

    def _zero_now(self) -> None:
        for r in self.zero_regions + self.zero_early + self.stripe_bufs:
            r.zero_()
        self.e.flat_grad.zero_()
        if self.tail:
            self.tail_tk.zero_()            # (an aborted launch must not leave tickets behind)

    def reset_after_warmup(self) -> None:
        self._zero_now()
        if self.carry is not None:
            self.carry_pending.zero_()      # the restored parameters have no pending update
        self.prime()

    # ------------------------------------------------------------------ batch staging
    def _plan_stage(self) -> None:
        """Stage each step's batch at fixed addresses (one-GPU fused program).  The head
        advances the stream cursor and the optimizer's trailing workgroups copy the NEXT
        step's images and labels (rows[cursor]) into ``stage_img`` / ``stage_lbl``, so the
        conv pair and head kernels start with one memory round trip instead of the
        cursor -> row index -> image chain.  ``prime()`` fills them for the current cursor
        whenever the host moved it (construction, warm-up restore, seek).

        Default on (``CSA_STAGE_BATCH=0`` turns it off): 3 alternating bench pairs on
        MI355X, 0.1169 vs 0.1175 ms/step (scripts/ab_env.sh) — small, because the conv
        pair's start-up phase is mostly bound by 700 workgroups reading the same weights
        at once, but consistent."""
        e = self.e
        img = e.data.images
        imsz = img[0].numel() if img.dim() > 1 else 0
        self.staged = (self.pair is not None and bool(self.head_rg or self.head_row) and img.dtype == torch.uint8
                       and imsz % 4 == 0 and os.environ.get("CSA_STAGE_BATCH", "1") == "1")
        if self.staged:
            self.stage_img = torch.zeros(self.B, imsz, dtype=torch.uint8, device=e.device)
            self.stage_lbl = torch.zeros(self.B, dtype=torch.int64, device=e.device)
            self.prime()

    def _stage_args(self):
        """The staging copy's arguments: the dataset through the device cursor -> the stage."""
        e = self.e
        return (K.ptr(e.data.images), K.ptr(e.data.labels), K.ptr(e.stream.rows), K.ptr(e.stream.cursor), self.B,
                self.stage_img.shape[1], K.ptr(self.stage_img), K.ptr(self.stage_lbl))

    def prime(self) -> None:
        if self.staged:
            self._rc(self.lib.csa_gather_batch(*self._stage_args(), K.stream()), "gather_batch")

    def _batch_src(self):
        """(images, rows, cursor) for a kernel reading this step's batch: the staged batch
        (rows = cursor = None) or the dataset through the device cursor."""
        e = self.e
        if self.staged and not self._predicting:
            return self.stage_img, None, None
        return e.data.images, e.stream.rows, e.stream.cursor

    # ------------------------------------------------------------------ augmentation
    def _plan_augment(self) -> None:
        """``options.augment`` (ops/augment_ref.py): the first launch of every training step
        writes this step's batch, warped for (seed, step, dataset row), into ``aug_img``, and
        every training-time reader of the images takes ``aug_img`` instead of the dataset
        (``_train_src``).  The launch reads the dataset through the device cursor and the
        step counter, so it replays inside graphs like the rest of the step.

        A staged program keeps its in-launch staging copy running: the labels the head
        reads are staged by the same workgroups, and turning the image half off would change
        an existing kernel.  ``stage_img`` then has no training-time reader."""
        e = self.e
        self.aug = getattr(e, "aug", None)
        if self.aug is None:
            return
        self.aug_c = self.aug.to_c()
        self.aug_img = torch.zeros(self.B, augment_ref.HW * augment_ref.HW, dtype=torch.uint8, device=e.device)
        # for readers that take a row table: image b of aug_img is row b of a one-line table
        self.aug_rows = torch.arange(self.B, dtype=torch.int64, device=e.device).view(1, self.B)
        self.aug_cur = torch.zeros(1, dtype=torch.int64, device=e.device)

    def _train_src(self, table: bool = False):
        """(images, rows, cursor) for a kernel reading this step's images.  ``table``: the
        reader needs a row table and a cursor (the raw first conv, the float gather); the
        pair kernels also take a batch at a fixed address (rows = cursor = None).  Without
        augmentation, and when predicting, exactly what these readers were handed before."""
        e = self.e
        if self.aug is None or self._predicting:
            return (e.data.images, e.stream.rows, e.stream.cursor) if table else self._batch_src()
        if table:
            return self.aug_img, self.aug_rows, self.aug_cur
        return self.aug_img, None, None
