"""The HIP step program: ``hip_plan`` lowers and plans (its docstring is the design),
``hip_buffers`` declares the program's state and allocates, and ``HipProgram`` here joins
them and holds the step: forward, head, backward, gradient exchange, optimizer, predict."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from ..models.dsl import AvgPoolSpec
from ..ops import augment_ref, dropout_ref
from ..ops import fused as K
from .hip_buffers import Buffers
from .hip_plan import Plan, Transform, Unit, Unsupported, _act_id, _alpha, _opt_call

__all__ = ["HipProgram", "Unsupported", "Unit", "Transform"]

_NO_BN = (None, 0, 0.0, 0.0, None, None)


class HipProgram(Plan, Buffers):
    WGRAD_STRIPES = int(os.environ.get("CSA_WGRAD_STRIPES", "16"))   # (A/B knob; <= 16: the tail's loads)
    FWD_ZERO_MAX = 4          # the pair forward's zero list (conv_pair.hip CP_MAXZ)

    # ------------------------------------------------------------------ DP deferred update
    def _carry_args(self):
        e = self.e
        s0, s1 = self._slots()
        lo = (C.c_long * 4)(*[x[0] for x in self.carry])
        hi = (C.c_long * 4)(*[x[1] for x in self.carry])
        return (e.opt_id, float(e.lr), K.ptr(e.dstep), K.ptr(e.flat), K.ptr(e.flat_grad), K.ptr(s0), K.ptr(s1),
                K.ptr(self.carry_pending), len(self.carry), lo, hi, self.carry_blocks)

    def flush(self, st=None) -> None:
        """Apply a pending deferred dense update now (stream-ordered; a no-op on the device
        when none is pending) and clear its flag."""
        if self.carry is None:
            return
        self._rc(K.sched_call(self.lib, "csa_opt_carry_flush", self.e.lr_sched_c, *self._carry_args(),
                              st if st is not None else K.stream()), "opt_carry_flush")

    # ------------------------------------------------------------------ DP "lowrank"
    def _lowrank_gather_inputs(self) -> None:
        """After the forward pass: all-gather the dense GEMM inputs on the side stream
        (overlaps the head and the dense input-gradient GEMMs)."""
        if not self.lr_units:
            return
        self.lr_side.wait_stream(torch.cuda.current_stream(self.e.device))
        with torch.cuda.stream(self.lr_side):
            self.e.sync.all_gather_rows_many([(u.lr_src, u.lr_x) for u in self.lr_units], tag="lr_x")

    def _lowrank_wgrads(self) -> None:
        """Once every lowrank unit's output gradient is final: gather them and form the
        global weight gradients (K = world·B) on the side stream."""
        W, B = self.e.ctx.world, self.B
        self.lr_side.wait_stream(torch.cuda.current_stream(self.e.device))
        with torch.cuda.stream(self.lr_side):
            ss = self.lr_side.cuda_stream
            self.e.sync.all_gather_rows_many([(u.dy.view(B, -1), u.lr_dy) for u in self.lr_units], tag="lr_dy")
            for u in self.lr_units:         # (every one has lr_update: _plan_lowrank)
                self._dd_wgrad_update(u, u.lr_x, u.lr_dy, W * B, u.lr_act, ss)

    def _grad_ready(self, key) -> None:
        b = self.bucket_at.get(key)
        if b is None:
            return
        cur = torch.cuda.current_stream(self.e.device)
        self.side.wait_stream(cur)
        with torch.cuda.stream(self.side):
            if self.e.sync.strategy == "ps":
                self.e.sync.reduce_scatter_range(self.e.flat_grad, self.e.grad_shard, b[0], b[1])
            else:
                self.e.sync.allreduce(self.e.flat_grad, b[0], b[1])

    def join_branch(self) -> None:
        """Join a pending dense-update branch into the current stream (a capture ends with
        every forked stream joined; the next step's BatchNorm apply needs it done)."""
        if self._br_pending:
            torch.cuda.current_stream(self.e.device).wait_stream(self.br_side)
            self._br_pending = False

    # ------------------------------------------------------------------ pair-backward tail
    def _tail_set(self) -> None:
        """Record the tail of this step's pair backward launch (host state, like the
        deferred dense segments) and switch the head segment to in-place updates."""
        e, lib = self.e, self.lib
        P = C.c_void_p
        _opt_call(lib, "csa_conv_pair_tail_force", K.ptr(self.tail_force))
        if not self.tail_update:           # the ":hf" data-parallel fold: nothing else
            self._rc(lib.csa_conv_pair_tail_set(
                K.ptr(self.tail_tk), K.ptr(self.tail_err), 0, 0.0, K.ptr(e.dstep), K.ptr(self.tail_table),
                self.tail_blocks, 0, (P * 4)(), (C.c_long * 4)(), None, None, None, None, 0, 0, None, None),
                "conv_pair_tail_set")
            return
        self._rc(lib.csa_dense_update_head_params(*[K.ptr(t) for t in self.head_params]), "dense_update_head_params")
        self._rc(K.sched_call(
            lib, "csa_conv_pair_tail_set", e.lr_sched_c,
            K.ptr(self.tail_tk), K.ptr(self.tail_err), e.opt_id, float(e.lr), K.ptr(e.dstep),
            K.ptr(self.tail_table), self.tail_blocks,
            len(self.tail_zero), (P * 4)(*[t.data_ptr() for t in self.tail_zero]),
            (C.c_long * 4)(*[t.numel() for t in self.tail_zero]), *self._stage_args()), "conv_pair_tail_set")

    def tail_error(self) -> int:
        """Nonzero when a tail workgroup's bounded wait timed out (its work did not run).

        STICKY by design: a timed-out tail skipped parameter updates, the statistic-slab
        zeroing and the next batch's staging, so the engine's state is no longer a valid
        training state — nothing resets the word; the job fails (``TrainEngine.check_health``)
        and restarts from its last checkpoint in a fresh engine."""
        return int(self.tail_err.item()) if self.tail else 0

    def health_words(self):
        """Device int32 words that are nonzero once an in-kernel bounded wait timed out
        (read without a host sync by the job loop's metric drain): the pair-backward tail's
        and the forward chain's."""
        words = [self.tail_err] if self.tail else []
        if self.chain:
            words.append(self.chain_err)
        return words

    def arm_tail_timeout(self) -> bool:
        """Debug / fault injection: the NEXT pair-backward launch's tail waits
        for one ticket more than exists, times out after its 1 s bound and sets the error
        word, as a starved or hung pair workgroup would.  Stream-ordered (a fill before the
        launch); the launch's closing tail disarms it.  False when this program has no tail."""
        if not self.tail:
            return False
        self.tail_force.fill_(1)
        return True

    # ------------------------------------------------------------------ deterministic mode
    def _row_fold(self, t: torch.Tensor, rows: int, width: int, dst: torch.Tensor, zero_src: int, st) -> None:
        """dst[:width] = fixed-order sum of the first ``rows`` rows of ``t`` (row stride width)."""
        self._rc(self.lib.csa_rows_fold(K.ptr(t), width, rows, width, K.ptr(dst), zero_src, st), "rows_fold")

    def _slab_fold(self, slab: torch.Tensor, rows: int, st) -> None:
        """Deterministic mode: a slab's exclusive rows (one per producer workgroup) to row 0, in order."""
        self._row_fold(slab, rows, slab.shape[1] * slab.shape[2], slab, 0, st)

    def _bwd_slab_fold(self, tf: Transform, st) -> None:
        """Deterministic mode, after a unit's input gradient: its BN-backward rows to row 0."""
        if self.det and tf.has_bn:
            self._slab_fold(tf.bwd_slab, tf.bwd_prod_rows, st)

    def _fwd_bn_now(self, u: Unit) -> bool:
        """A planned unit, under the profile flags of the thread that issues this forward."""
        return u.fwd_bn and self._fwd_bn_ok(u)

    def _augment(self, st) -> None:
        e = self.e
        self._rc(self.lib.csa_augment_batch(
            K.ptr(e.data.images), K.ptr(e.stream.rows), K.ptr(e.stream.cursor), self.B, augment_ref.HW,
            augment_ref.HW, C.byref(self.aug_c), self.aug.seed, K.ptr(e.dstep), K.ptr(self.aug_img), st),
            "augment_batch")

    # ------------------------------------------------------------------ helpers
    def _bn_args(self, tf: Transform):
        if not tf.has_bn:
            return _NO_BN
        name = tf.norm.name
        slab = (K.ptr(tf.eval_slab), 1, 1.0) if self._eval_bn else (K.ptr(tf.slab), tf.nslab, tf.count)
        return (*slab, float(tf.norm.spec.epsilon),
                K.ptr(self.views[f"{name}.scale"]), K.ptr(self.views[f"{name}.offset"]))

    def _bn_args_c(self, tf: Transform):
        """BN args with the channel count (dense launchers: channel = feature % C)."""
        a = self._bn_args(tf)
        C_ = tf.slab.shape[2] if tf.has_bn else 0
        return (a[0], a[1], C_, a[2], a[3], a[4], a[5])

    def _running_stats(self, norm):
        """(running mean, running variance) of a norm layer: buffers of the model."""
        return getattr(self.model, f"bn{norm.index}_mean"), getattr(self.model, f"bn{norm.index}_var")

    def _bn_bwd_args(self, tf: Transform):
        """What the BN backward of a unit's OUTPUT transform writes: the scale / offset
        gradients, the running statistics it updates, and their momentum."""
        if not tf.has_bn:
            return (None, None, None, None, float(self.model.bn_momentum))
        G = self.gviews
        rm, rv = self._running_stats(tf.norm)
        return (K.ptr(G[f"{tf.norm.name}.scale"]), K.ptr(G[f"{tf.norm.name}.offset"]), K.ptr(rm), K.ptr(rv),
                float(self.model.bn_momentum))

    def _slots(self):
        """The optimizer's (up to two) slot vectors, None where the optimizer has fewer."""
        sl = self.e.slots
        return (sl[0] if sl.shape[0] > 0 else None, sl[1] if sl.shape[0] > 1 else None)

    def _slot_ptrs(self, lp):
        """The slot pointers of a layer's parameters: (slot 0, slot 1) of W, then of b."""
        offs = self.model.state.offsets
        return tuple(K.ptr(s[offs[f"{lp.name}.{p}"]:]) if s is not None else None
                     for p in ("weight", "bias") for s in self._slots())

    # ------------------------------------------------------------------ the step
    def run(self) -> None:
        with self._det_scope():
            self._run()

    def _run(self) -> None:
        e, lib = self.e, self.lib
        st = K.stream()
        if self.aug is not None:
            self._augment(st)
        for r in self.zero_early:
            r.zero_()
        if self.hfuse:
            lib.csa_dense_update_clear()        # no stale segment from an aborted step
        if self.chain:
            lib.csa_chain_begin()               # the two dense forwards + the head: recorded
        try:
            self._forward(st)
        except BaseException:
            if self.chain:
                lib.csa_chain_reset()
            raise
        self._lowrank_gather_inputs()
        self._head(st)
        self._grad_ready("head")
        for k in range(len(self.units) - 1, -1, -1):
            self._unit_bwd(k, st)
            self._grad_ready(k)
        self._exchange()
        if self.tail and e.aps is None:
            if lib.csa_dense_update_pending() or lib.csa_conv_pair_tail_pending():
                raise RuntimeError("pair-backward tail / deferred updates not consumed")
            if self.tail_update:
                return                      # the pair backward's tail did the optimizer's work
        self._optimizer(st)

    def _exchange(self) -> None:
        """The gradient exchange between the backward and the optimizer launch."""
        e = self.e
        main = torch.cuda.current_stream(e.device)
        if e.aps is not None:
            # async_ps: push / apply-on-arrival / publish / pull in one launch; the optimizer
            # launch keeps only its side jobs (zeroing, metrics, batch staging)
            e.aps.step(e.flat_grad, e.flat, e.slots)
        elif self.overlap:
            main.wait_stream(self.side)
        elif e.ctx.enabled and e.sync.strategy == "lowrank":
            e.sync.allreduce_ranges(e.flat_grad, self.lr_ranges, tag="lr_rem")
            if self.lr_units:
                main.wait_stream(self.lr_side)
        else:
            e.after_backward_sync()

    def _head(self, st) -> None:
        """Loss, head gradients, input gradient and metrics: one launch in one of four forms
        (the row head + the last dense layer's input gradient, the row head, the partial-row
        head, the atomic head), which share their leading arguments."""
        e, lib, B = self.e, self.lib, self.B
        V, G, htf = self.views, self.gviews, self.head_tf
        last = self.units[-1]
        hin = last.y.view(B, -1)
        rows, cur = e.stream.rows, e.stream.cursor
        act = (_act_id(htf.act), _alpha(htf.act))
        common = (K.ptr(hin), B, hin.shape[1], *act, K.ptr(V["head.weight"]), K.ptr(V["head.bias"]))
        loss = (0 if e.cfg.loss_name == "entropy" else 1, float(e.sync.grad_scale))
        if not (self.head_dgrad or self.head_row or self.head_rg):
            self._rc(lib.csa_head(
                *common, K.ptr(e.data.labels), K.ptr(rows), *loss,
                K.ptr(G["head.weight"]), K.ptr(G["head.bias"]), K.ptr(last.dy), None,
                K.ptr(e.dstep), K.ptr(e.ring_loss), K.ptr(e.ring_correct), e.ring_correct.numel(),
                K.ptr(cur), K.ptr(self.head_ws), st), "head")
            return
        # the staged labels at their fixed address (the head then advances the cursor for the
        # staging copy), or the dataset's through the row table and the cursor
        if self.staged:
            labels, advance = (K.ptr(self.stage_lbl), None, None), (K.ptr(cur), e.stream.wrap)
        else:
            labels, advance = (K.ptr(e.data.labels), K.ptr(rows), K.ptr(cur)), (None, 0)
        row_out = (K.ptr(last.dy), K.ptr(self.hdl), K.ptr(self.hrl), K.ptr(self.hrc)) if self.head_row else ()
        if self.head_dgrad:
            ltf = last.in_tf
            rc_hd = lib.csa_head_dgrad(
                *common, *labels, *loss, *row_out, K.ptr(e.dstep), *advance,
                K.ptr(V[f"{last.layer.name}.weight"]), last.layer.in_shape.numel, K.ptr(last.x.view(B, -1)),
                _act_id(ltf.act), _alpha(ltf.act), K.ptr(self.units[-2].dy), st)
            if self.chain:                      # fc1 forward | fc2 forward | head: one launch
                rc = lib.csa_chain_end(K.ptr(self.chain_tk), K.ptr(self.chain_err), st) if rc_hd >= 0 else 0
                if rc_hd < 0:
                    lib.csa_chain_reset()
                self._rc(rc, "fwd_chain")
            self._rc(rc_hd, "head_dgrad")
        elif self.head_row:
            self._rc(lib.csa_head_row(*common, *labels, *loss, *row_out, K.ptr(e.dstep), *advance, st), "head_row")
            if self.head_sep:
                # dWh = act(h)^T dlogits, dbh = colsum(dlogits) into the flat gradient
                self._rc(lib.csa_dd_wgrad(
                    K.ptr(hin), K.ptr(self.hdl), B, hin.shape[1], 10, *act, 1.0,
                    K.ptr(G["head.weight"]), K.ptr(G["head.bias"]),
                    None, None, None, None, None, None, -1, 0.0, None, st), "dd_wgrad(head)")
        else:
            self._rc(lib.csa_head_part2(
                *common, *labels, *loss, K.ptr(last.dy),
                K.ptr(self.head_part), K.ptr(self.head_mloss), K.ptr(self.head_mcorr), None, K.ptr(e.dstep),
                *advance, st), "head_part")

    def _unit_bwd(self, k: int, st) -> None:
        u = self.units[k]
        prev = self.units[k - 1] if k > 0 else None
        if self.pair is not None and k < 2:
            if k == 1:
                self._pair_bwd(st)
        elif u.kind in ("bn", "pool", "drop", "lrn", "gn", "dw"):
            self._standalone_bwd(u, prev, st)
        elif u.kind == "gconv":
            self._gconv_bwd(u, prev, st)
        else:
            if self.sync_bn and k + 1 < len(self.units) and self.units[k + 1].in_tf.has_bn:
                # unit k+1's dgrad produced its input transform's backward slab; this
                # unit's route consumes it: make it the global sum first
                self.e.sync.allreduce_tensors([self.units[k + 1].in_tf.bwd_slab], tag=f"bnb{k + 1}")
            if u.kind == "dense":
                self._dense_bwd(u, k, prev, st)
            else:
                self._conv_bwd(u, k, prev, st)

    def _conv_bwd(self, u: Unit, k: int, prev: Optional[Unit], st) -> None:
        lib, B, V = self.lib, self.B, self.views
        lp, tf, sp = u.layer, u.in_tf, u.layer.spec
        bn = self._bn_args(tf)
        in_act, in_alpha = _act_id(tf.act), _alpha(tf.act)
        # output side: (BN backward of the NEXT transform) + act backward + pool routing
        next_tf = self._next_tf(k)
        dc = u.dy
        if next_tf.has_bn or u.act is not None or u.pool is not None:
            self._rc(lib.csa_route_bwd(
                K.ptr(u.dy), K.ptr(u.y), K.ptr(u.argmax), K.ptr(u.dc), K.ints(self._route_geom(u)),
                _act_id(u.act), _alpha(u.act), *self._bn_args(next_tf), K.ptr(next_tf.bwd_slab), next_tf.bwd_nslab,
                *self._bn_bwd_args(next_tf), st), "route_bwd")
            self._sync_bn_param_grads(next_tf)
            dc = u.dc
        geom = self._conv_geom(lp, B)
        db = K.ptr(u.db_acc) if sp.bias else None
        if prev is not None:
            # input gradient + weight gradient in one launch
            self._rc(lib.csa_conv_bwd(
                K.ptr(dc), K.ptr(V[f"{lp.name}.weight"]), K.ptr(prev.dy), geom,
                K.ptr(u.x), in_act, in_alpha, *bn, K.ptr(tf.bwd_slab),
                K.ptr(u.dw_acc), db, u.wg_stripes, st), "conv_bwd")
        else:
            raw = u.x is None
            img, rows, cur = self._train_src(table=True)     # (a raw first conv's weight gradient)
            h, w = lp.in_shape.hw
            oh, ow = lp.out_shape.hw
            self._rc(lib.csa_conv_wgrad(
                None if raw else K.ptr(u.x), K.ptr(img) if raw else None, K.ptr(rows) if raw else None,
                K.ptr(dc), K.ptr(u.dw_acc), db, u.wg_stripes,
                B, h, w, lp.in_shape.c, sp.kh, sp.kw, sp.stride[0], sp.stride[1], lp.pads[0], lp.pads[2],
                oh, ow, sp.cout, *bn, in_act, in_alpha, K.ptr(cur) if raw else None, st), "conv_wgrad")
        self._conv_det_folds(u, tf, st)

    def _dense_bwd(self, u: Unit, k: int, prev: Optional[Unit], st) -> None:
        lib, B, V, G = self.lib, self.B, self.views, self.gviews
        lp, tf = u.layer, u.in_tf
        fin, fout = lp.in_shape.numel, lp.spec.hidden
        in_act, in_alpha = _act_id(tf.act), _alpha(tf.act)
        lowrank = u in self.lr_units
        if u.fused:
            self._dense_bwd_update(u, prev, st)
            return
        if prev is not None and not lowrank and self._dense_bwd_fused(u, prev, st):
            return                          # dgrad + wgrad in one launch
        if prev is not None:
            self._rc(lib.csa_dense_dgrad(
                K.ptr(u.dy), K.ptr(V[f"{lp.name}.weight"]), K.ptr(prev.dy), B, fin, fout,
                K.ptr(u.x.view(B, -1)), in_act, in_alpha, *self._bn_args_c(tf), K.ptr(tf.bwd_slab), st),
                "dense_dgrad", positive_ok=True)    # (returns its slab rows)
            self._bwd_slab_fold(tf, st)
        if lowrank:                         # global wgrad formed after the gathers
            if k == self.lr_first:
                self._lowrank_wgrads()
            return
        dw, db = K.ptr(G[f"{lp.name}.weight"]), K.ptr(G[f"{lp.name}.bias"])
        if u.xt is not None:
            self._rc(lib.csa_dense_wgrad(K.ptr(u.xt), K.ptr(u.dy), dw, db, B, fin, fout,
                                         None, 0, 0, 0.0, 0.0, None, None, 0, 0.0, 1.0, st), "dense_wgrad")
        else:
            self._rc(lib.csa_dense_wgrad(K.ptr(u.x), K.ptr(u.dy), dw, db, B, fin, fout,
                                         *self._bn_args_c(tf), in_act, in_alpha, 1.0, st), "dense_wgrad")

    # ------------------------------------------------------------------ forward
    def _forward(self, st) -> None:
        """Every unit's forward launch (the first half of ``run``; ``predict`` reuses it)."""
        e, lib, B = self.e, self.lib, self.B
        img, rows, cur = self._train_src(table=True)
        if self.x_dense_in is not None:
            D = self.x_dense_in.shape[1]
            if e.data.images.dtype == torch.uint8 and D % 4 == 0:
                self._rc(lib.csa_gather_images_f32(K.ptr(img), K.ptr(rows), K.ptr(cur), B, D,
                                                   K.ptr(self.x_dense_in), st), "gather_images_f32")
            else:
                idx = rows.index_select(0, cur).view(-1)
                self.x_dense_in.copy_(img.index_select(0, idx).to(torch.float32).mul_(1.0 / 255.0))
        V = self.views
        pend = None                      # the carried update's pending flag, when fc1's forward clears it
        if self.pair is not None:
            pend = self._pair_fwd(st)
        for k, u in enumerate(self.units):
            if self.pair is not None and k < 2:
                continue
            if u.kind in ("bn", "pool", "drop", "lrn", "gn", "dw"):
                self._standalone_fwd(u, st)
                continue
            if u.kind == "gconv":
                self._gconv_fwd(u, st)
                continue
            lp, tf = u.layer, u.in_tf
            bn = self._bn_args(tf)
            in_act, in_alpha = _act_id(tf.act), _alpha(tf.act)
            if u.kind == "conv":
                next_tf = self._next_tf(k)
                oslab = next_tf.slab if next_tf.has_bn and not self._eval_bn else None
                raw = u.x is None
                self._rc(lib.csa_conv_fwd(
                    None if raw else K.ptr(u.x), K.ptr(img) if raw else None, K.ptr(rows) if raw else None,
                    K.ptr(V[f"{lp.name}.weight"]), K.ptr(V.get(f"{lp.name}.bias")) if lp.spec.bias else None,
                    K.ptr(u.y), K.ptr(u.argmax), K.ptr(oslab),
                    self._conv_geom(lp, B), self._pool_geom(u), *bn, in_act, in_alpha,
                    _act_id(u.act), _alpha(u.act), K.ptr(cur) if raw else None, st), "conv_fwd")
                self._fwd_slab_ready(oslab, next_tf, f"bnf{k}", st)
                continue
            fin, fout = lp.in_shape.numel, lp.spec.hidden
            w, b = K.ptr(V[f"{lp.name}.weight"]), K.ptr(V[f"{lp.name}.bias"])
            if u is self.br_unit:
                self.join_branch()          # the previous step's update read u.xt and W
            if u.xt is not None and self._fwd_bn_now(u):
                # BatchNorm + activation on load: xt, the tables and the pending flag come
                # out of the forward's own launch (dense_direct.hip dd_fwd_wide_bn_kernel)
                self._rc(lib.csa_dd_fwd_bn(
                    K.ptr(u.x), w, b, K.ptr(u.y), B, fout, fin, tf.slab.shape[2], *bn, in_act, in_alpha,
                    K.ptr(u.xt), K.ptr(tf.bn_tab), K.ptr(pend if k == 2 else None), st), "dd_fwd_bn")
                continue
            if u.xt is not None:
                self._rc(lib.csa_bn_act_apply(
                    K.ptr(u.x), K.ptr(u.xt), B * fin, tf.slab.shape[2], *bn, in_act, in_alpha,
                    K.ptr(tf.bn_tab), st), "bn_act_apply")
            if u.direct:
                xin = u.xt if u.xt is not None else u.x.view(B, -1)
                act = (0, 0.0) if u.xt is not None else (in_act, in_alpha)
                self._rc(lib.csa_dd_fwd(K.ptr(xin), w, b, K.ptr(u.y), B, fout, fin, act[0], act[1], st), "dd_fwd")
            elif u.xt is not None:
                self._rc(lib.csa_dense_fwd(K.ptr(u.xt), w, b, K.ptr(u.y), B, fout, fin, None, 0, 0, 0.0, 0.0,
                                           None, None, 0, 0.0, st), "dense_fwd")
            else:
                self._rc(lib.csa_dense_fwd(K.ptr(u.x), w, b, K.ptr(u.y), B, fout, fin, *self._bn_args_c(tf),
                                           in_act, in_alpha, st), "dense_fwd")

    def _fwd_slab_ready(self, oslab, next_tf: Transform, tag: str, st) -> None:
        """After the producer of a forward statistic slab: the deterministic fold of its
        exclusive rows, then (SyncBN) the global sum."""
        if oslab is not None and self.det:
            self._slab_fold(oslab, next_tf.prod_rows, st)
        if oslab is not None and self.sync_bn:
            self.e.sync.allreduce_tensors([oslab], tag=tag)

    def _pair_fwd(self, st):
        """The conv pair's forward launch.  Returns the carried update's pending flag when
        the first dense layer's forward is the launch that clears it."""
        e, lib, V = self.e, self.lib, self.views
        ua, ub = self.units[0], self.units[1]
        nt = self._next_tf(1)
        oslab = nt.slab if nt.has_bn and not self._eval_bn else None
        simg, srows, scur = self._train_src()
        # (the tail program: the dense split-K outputs of this step, zeroed by the pair
        # forward's threads — not when predicting, which zeroes them itself)
        fz = [] if self._predicting else self.fwd_zero
        carrying = self.carry is not None and not self._predicting
        if carrying:
            self._rc(K.sched_call(lib, "csa_conv_pair_fwd_carry", e.lr_sched_c, *self._carry_args()),
                     "conv_pair_fwd_carry")
        c1 = None if self._predicting else self.pair_c1
        if c1 is not None:
            _opt_call(lib, "csa_conv_pair_c1_fwd", K.ptr(c1), c1.numel())
        self._rc(lib.csa_conv_pair_fwd(
            K.ints(self.pair), K.ptr(simg), K.ptr(srows), K.ptr(scur),
            K.ptr(V[f"{ua.layer.name}.weight"]), K.ptr(V.get(f"{ua.layer.name}.bias")) if ua.layer.spec.bias else None,
            _act_id(ua.act), _alpha(ua.act),
            K.ptr(V[f"{ub.layer.name}.weight"]), K.ptr(V.get(f"{ub.layer.name}.bias")) if ub.layer.spec.bias else None,
            _act_id(ub.act), _alpha(ub.act), K.ptr(ub.y), K.ptr(ub.argmax), K.ptr(oslab),
            nt.prod_rows if self.det else self.lib.csa_conv_fwd_nslab(None, None),
            (C.c_void_p * 4)(*[t.data_ptr() for t in fz]), (C.c_long * 4)(*[t.numel() for t in fz]), len(fz),
            st), "conv_pair_fwd")
        pend = None
        if carrying and self.carry_clear:
            if self._fwd_bn_now(self.units[2]):
                pend = self.carry_pending                                    # (csa_dd_fwd_bn clears it)
            else:
                _opt_call(lib, "csa_ew_clear_next", K.ptr(self.carry_pending))   # (next: bn_act_apply)
        self._fwd_slab_ready(oslab, nt, "bnf1", st)
        return pend

    # ------------------------------------------------------------------ standalone units
    def _drop_args(self, u: Unit):
        """(n, F, row_mul, row_add, seed) of a drop unit: element (b, f) of this rank's batch
        draws counter (b * world + rank) * F + f (ops/dropout_ref.py)."""
        ctx = self.e.ctx
        return (u.x.numel(), u.x[0].numel(), ctx.world, ctx.rank,
                dropout_ref.drop_seed(self.e.cfg.seed, u.layer.index))

    def _drop_consts(self, u: Unit):
        kp = u.layer.spec.keep_prob
        return (dropout_ref.keep_threshold(kp), dropout_ref.keep_scale(kp), _act_id(u.act), _alpha(u.act))

    def _standalone_fwd(self, u: Unit, st) -> None:
        lib = self.lib
        if u.kind == "drop":
            train = 0 if self._predicting else 1
            self._rc(lib.csa_drop_fwd(K.ptr(u.x), K.ptr(u.y), *self._drop_args(u), K.ptr(self.e.dstep),
                                      K.ptr(u.used_step), *self._drop_consts(u), train, st), "drop_fwd")
            return
        if u.kind == "lrn":
            # (a training program's forward-only pass leaves the step's kept tensor alone)
            keep = None if self._predicting else u.lrn_s
            self._rc(lib.csa_lrn_fwd(K.ptr(u.x), K.ptr(u.y), K.ptr(keep), self._lrn_geom(u.layer),
                                     *self._lrn_consts(u.layer), 0, st), "lrn_fwd")
            return
        if u.kind == "gn":
            # (a training program's forward-only pass leaves the step's kept statistics alone)
            nm = u.layer.name
            stat = None if self._predicting else u.gn_stat
            self._rc(lib.csa_gn_fwd(K.ptr(u.x), K.ptr(self.views[f"{nm}.scale"]), K.ptr(self.views[f"{nm}.offset"]),
                                    K.ptr(u.y), K.ptr(stat), self._gn_geom(u.layer), float(u.layer.spec.epsilon),
                                    _act_id(u.act), _alpha(u.act), 0, st), "gn_fwd")
            return
        if u.kind == "dw":
            lp = u.layer
            bias = self.views[f"{lp.name}.bias"] if lp.spec.bias else None
            self._rc(lib.csa_dw_fwd(K.ptr(u.x), K.ptr(self.views[f"{lp.name}.weight"]), K.ptr(bias), K.ptr(u.y),
                                    self._dw_geom(lp), _act_id(u.act), _alpha(u.act), 0, st), "dw_fwd")
            return
        if u.kind == "pool" and isinstance(u.layer.spec, AvgPoolSpec):
            self._rc(lib.csa_avgpool_fwd(K.ptr(u.x), K.ptr(u.y), self._pool_geom_full(u), 0, st), "avgpool_fwd")
            return
        if u.kind == "pool":
            self._rc(lib.csa_maxpool_fwd(K.ptr(u.x), K.ptr(u.y), K.ptr(u.argmax), self._pool_geom_full(u), st),
                     "maxpool_fwd")
            return
        n = u.x.numel()
        C_ = self._bn_channels(u)
        act, alpha = _act_id(u.act), _alpha(u.act)
        if u.norm is None:
            self._rc(lib.csa_bn_apply(K.ptr(u.x), K.ptr(u.y), n, C_, None, act, alpha, st), "act_apply")
            return
        nm = u.norm.name
        rm, rv = self._running_stats(u.norm)
        eps = float(u.norm.spec.epsilon)
        if self._eval_bn:
            self._rc(lib.csa_bn_finalize(None, 0, C_, 1.0, eps, K.ptr(self.views[f"{nm}.scale"]),
                                         K.ptr(self.views[f"{nm}.offset"]), K.ptr(rm), K.ptr(rv), 0.0, 1,
                                         K.ptr(u.bn_tab), st), "bn_finalize(eval)")
        else:
            R = u.bn_slab.shape[0]
            self._rc(lib.csa_bn_stats(K.ptr(u.x), n // C_, C_, K.ptr(u.bn_slab), R, st), "bn_stats")
            if self.sync_bn:
                self.e.sync.allreduce_tensors([u.bn_slab], tag=f"bns{u.norm.index}")
            upd = self.model.training and not self._predicting
            self._rc(lib.csa_bn_finalize(K.ptr(u.bn_slab), R, C_, float(n // C_ * self.W), eps,
                                         K.ptr(self.views[f"{nm}.scale"]), K.ptr(self.views[f"{nm}.offset"]),
                                         K.ptr(rm) if upd else None, K.ptr(rv) if upd else None,
                                         float(self.model.bn_momentum), 0, K.ptr(u.bn_tab), st), "bn_finalize")
        self._rc(lib.csa_bn_apply(K.ptr(u.x), K.ptr(u.y), n, C_, K.ptr(u.bn_tab), act, alpha, st), "bn_apply")

    def _gconv_fwd(self, u: Unit, st) -> None:
        lp, V = u.layer, self.views
        self._rc(self.lib.csa_gconv_fwd(
            K.ptr(u.x), K.ptr(V[f"{lp.name}.weight"]), K.ptr(V[f"{lp.name}.bias"]) if lp.spec.bias else None,
            K.ptr(u.y), self._conv_geom(lp, self.B), st), "gconv_fwd")

    def _gconv_bwd(self, u: Unit, prev: Optional[Unit], st) -> None:
        """Input gradient (reads the pre-update weights) then weight gradient."""
        lp, G = u.layer, self.gviews
        geom = self._conv_geom(lp, self.B)
        if prev is not None:
            self._rc(self.lib.csa_gconv_dgrad(K.ptr(u.dy), K.ptr(self.views[f"{lp.name}.weight"]),
                                              K.ptr(prev.dy), geom, st), "gconv_dgrad")
        self._rc(self.lib.csa_gconv_wgrad(
            K.ptr(u.x), K.ptr(u.dy), K.ptr(G[f"{lp.name}.weight"]), K.ptr(G[f"{lp.name}.bias"]) if lp.spec.bias else None,
            geom, 1.0, st), "gconv_wgrad")

    def _standalone_bwd(self, u: Unit, prev: Optional[Unit], st) -> None:
        lib = self.lib
        dx = prev.dy if prev is not None else None
        if u.kind == "drop":
            if dx is not None:
                self._rc(lib.csa_drop_bwd(K.ptr(u.x), K.ptr(u.dy), K.ptr(dx), *self._drop_args(u),
                                          K.ptr(u.used_step), *self._drop_consts(u), st), "drop_bwd")
            return
        if u.kind == "lrn":
            if dx is not None:
                self._rc(lib.csa_lrn_bwd(K.ptr(u.x), K.ptr(u.lrn_s), K.ptr(u.dy), K.ptr(dx), self._lrn_geom(u.layer),
                                         *self._lrn_consts(u.layer), 0, st), "lrn_bwd")
            return
        if u.kind == "gn":
            # (a first unit has no input gradient and still has parameter gradients)
            nm, G = u.layer.name, self.gviews
            self._rc(lib.csa_gn_bwd(K.ptr(u.x), K.ptr(self.views[f"{nm}.scale"]), K.ptr(self.views[f"{nm}.offset"]),
                                    K.ptr(u.gn_stat), K.ptr(u.dy), K.ptr(dx), K.ptr(u.gn_slab),
                                    self._gn_geom(u.layer), _act_id(u.act), _alpha(u.act), 0, st), "gn_bwd")
            self._rc(lib.csa_gn_bwd_params(K.ptr(u.gn_slab), self.B, u.layer.in_shape.c, K.ptr(G[f"{nm}.scale"]),
                                           K.ptr(G[f"{nm}.offset"]), st), "gn_bwd_params")
            return
        if u.kind == "dw":
            # (a first unit has no input gradient and still has weight and bias gradients)
            lp, G = u.layer, self.gviews
            gw = G[f"{lp.name}.weight"]
            gb = G[f"{lp.name}.bias"] if lp.spec.bias else None
            geom = self._dw_geom(lp)
            self._rc(lib.csa_dw_bwd(K.ptr(u.x), K.ptr(self.views[f"{lp.name}.weight"]), K.ptr(u.y), K.ptr(u.dy),
                                    K.ptr(dx), K.ptr(u.dw_slab), K.ptr(gw), K.ptr(gb), geom, _act_id(u.act),
                                    _alpha(u.act), u.dw_form, st), "dw_bwd")
            if u.dw_form == 1:
                self._rc(lib.csa_dw_bwd_params(K.ptr(u.dw_slab), u.dw_slab.shape[0], geom, K.ptr(gw), K.ptr(gb), st),
                         "dw_bwd_params")
            return
        if u.kind == "pool" and isinstance(u.layer.spec, AvgPoolSpec):
            if dx is not None:
                self._rc(lib.csa_avgpool_bwd(K.ptr(u.dy), K.ptr(dx), self._pool_geom_full(u), st), "avgpool_bwd")
            return
        if u.kind == "pool":
            if dx is not None:
                self._rc(lib.csa_maxpool_bwd(K.ptr(u.dy), K.ptr(u.argmax), K.ptr(dx), self._pool_geom_full(u), st),
                         "maxpool_bwd")
            return
        n = u.x.numel()
        C_ = self._bn_channels(u)
        act, alpha = _act_id(u.act), _alpha(u.act)
        if u.norm is None:
            if dx is not None:
                self._rc(lib.csa_bn_bwd_apply(K.ptr(u.x), K.ptr(u.y), K.ptr(u.dy), K.ptr(dx), n, C_, None, None,
                                              act, alpha, st), "act_bwd")
            return
        nm = u.norm.name
        R = u.bn_bslab.shape[0]
        self._rc(lib.csa_bn_bwd_reduce(K.ptr(u.x), K.ptr(u.y), K.ptr(u.dy), n // C_, C_, K.ptr(u.bn_tab), act, alpha,
                                       K.ptr(u.bn_bslab), R, st), "bn_bwd_reduce")
        if self.sync_bn:
            self.e.sync.allreduce_tensors([u.bn_bslab], tag=f"bnbs{u.norm.index}")
        # under SyncBN the slab is already the global sum, so the parameter gradients are
        # scaled by 1/world before the gradient all-reduce adds them up again
        self._rc(lib.csa_bn_bwd_finalize(K.ptr(u.bn_bslab), R, C_, float(n // C_ * self.W), 1.0 / self.W,
                                         K.ptr(self.gviews[f"{nm}.scale"]), K.ptr(self.gviews[f"{nm}.offset"]),
                                         K.ptr(u.bn_k), st), "bn_bwd_finalize")
        if dx is not None:
            self._rc(lib.csa_bn_bwd_apply(K.ptr(u.x), K.ptr(u.y), K.ptr(u.dy), K.ptr(dx), n, C_, K.ptr(u.bn_tab),
                                          K.ptr(u.bn_k), act, alpha, st), "bn_bwd_apply")

    def predict_logits_into(self, logits: torch.Tensor) -> None:
        with self._det_scope():
            self._predict_logits_into(logits)

    def _predict_logits_into(self, logits: torch.Tensor) -> None:
        """Forward-only pass over this program's input rows -> ``logits`` [B, 10] (graph
        capturable; ``serve.hip_infer`` captures it per batch bucket).  BatchNorm uses the
        running statistics unless the model normalises with batch statistics in eval
        (``bn_mode == "batch"``), exactly as ``DigitNet.forward`` in eval mode."""
        hin = self._predict_head_input()
        kh = hin.shape[1]
        if self.lib.csa_dense_fwd_splits(self.B, 10, kh) > 1:
            logits.zero_()
        self._rc(self.lib.csa_dense_fwd(
            K.ptr(hin), K.ptr(self.views["head.weight"]), K.ptr(self.views["head.bias"]), K.ptr(logits),
            self.B, 10, kh, None, 0, 0, 0.0, 0.0, None, None,
            _act_id(self.head_tf.act), _alpha(self.head_tf.act), K.stream()), "head_fwd")

    def _predict_head_input(self) -> torch.Tensor:
        """The forward-only pass up to the head's input: returns the last unit's output
        [B, Kh] BEFORE the head's own activation (``head_tf.act``), which the consumer
        applies (the logits GEMM above, or ``csa_eval_rows`` in ``runtime.validation``)."""
        st = K.stream()
        self.flush(st)                      # a deferred dense update lands before the forward
        self._eval_bn = self.model.bn_mode != "batch"
        self._predicting = True
        # split-K forward outputs (and, with batch statistics, the forward BN slabs) are
        # atomic accumulators that the training step's optimizer launch re-zeroes
        for u in self.units:
            if u.kind in ("dense", "gconv") and u.splits_fwd > 1:
                u.y.zero_()
            if not self._eval_bn and u.in_tf.has_bn:
                u.in_tf.slab.zero_()
            if not self._eval_bn and u.kind == "bn" and u.norm is not None:
                u.bn_slab.zero_()
        try:
            if self._eval_bn:
                for tf in [u.in_tf for u in self.units] + [self.head_tf]:
                    if tf.has_bn:
                        # a 1-row slab whose {sum, sumsq} / count=1 IS {mean, var + mean^2}
                        if tf.eval_slab is None:
                            tf.eval_slab = torch.zeros(1, 2, tf.slab.shape[2], device=self.e.device)
                        rm, rv = self._running_stats(tf.norm)
                        tf.eval_slab[0, 0].copy_(rm)
                        torch.addcmul(rv, rm, rm, out=tf.eval_slab[0, 1])
            self._forward(st)
        finally:
            self._eval_bn = False
            self._predicting = False
        return self.units[-1].y.view(self.B, -1)

    def _pair_bwd(self, st) -> None:
        e, lib = self.e, self.lib
        ua, ub = self.units[0], self.units[1]
        V, G = self.views, self.gviews
        nt = self._next_tf(1)
        if self.sync_bn and nt.has_bn:
            e.sync.allreduce_tensors([nt.bwd_slab], tag="bnb2")
        simg, srows, scur = self._train_src()
        if self.tail:
            self._tail_set()
        # this step's forward BatchNorm tables (bn_act_apply wrote them for the dense
        # consumer): the pair's workgroups load them instead of each folding the slab
        tab = nt.bn_tab if nt.has_bn else None
        if tab is not None and os.environ.get("CSA_PAIR_BN_TAB", "1") == "1":
            lib.csa_conv_pair_bn_tab(K.ptr(tab))
        if self.pair_c1 is not None:
            _opt_call(lib, "csa_conv_pair_c1_bwd", K.ptr(self.pair_c1), self.pair_c1.numel())
        self._rc(lib.csa_conv_pair_bwd(
            K.ints(self.pair), K.ptr(simg), K.ptr(srows), K.ptr(scur),
            K.ptr(V[f"{ua.layer.name}.weight"]), K.ptr(V.get(f"{ua.layer.name}.bias")) if ua.layer.spec.bias else None,
            _act_id(ua.act), _alpha(ua.act), K.ptr(V[f"{ub.layer.name}.weight"]), 1 if ub.layer.spec.bias else 0,
            _act_id(ub.act), _alpha(ub.act), K.ptr(ub.dy), K.ptr(ub.y), K.ptr(ub.argmax),
            *self._bn_args(nt), K.ptr(nt.bwd_slab) if nt.has_bn else None, nt.bwd_nslab if nt.has_bn else 0,
            *self._bn_bwd_args(nt),
            K.ptr(ua.dw_acc), K.ptr(ua.db_acc) if ua.layer.spec.bias else None,
            K.ptr(ub.dw_acc), K.ptr(ub.db_acc) if ub.layer.spec.bias else None,
            min(ua.wg_stripes, ub.wg_stripes), K.ptr(self.pair_tabs), st), "conv_pair_bwd")
        self._sync_bn_param_grads(nt)
        if ua.row_fold:
            # the pair's (up to) four striped gradients into the flat gradient: ONE launch
            jobs = []
            for u in (ua, ub):
                lp = u.layer
                jobs.append((u.dw_acc, u.wg_stripes, u.dw_acc.shape[1], G[f"{lp.name}.weight"]))
                if u.db_acc is not None:
                    jobs.append((u.db_acc, u.wg_stripes, u.db_acc.shape[1], G[f"{lp.name}.bias"]))
            n = len(jobs)
            self._rc(lib.csa_rows_fold_multi(
                n, (C.c_void_p * 4)(*[j[0].data_ptr() for j in jobs]), (C.c_long * 4)(*[j[2] for j in jobs]),
                (C.c_int * 4)(*[j[1] for j in jobs]), (C.c_long * 4)(*[j[2] for j in jobs]),
                (C.c_void_p * 4)(*[j[3].data_ptr() for j in jobs]), (C.c_int * 4)(*([1] * n)), st), "rows_fold_multi")

    def _conv_det_folds(self, u: Unit, tf, st) -> None:
        """Deterministic mode, after a conv unit's backward: its BN-backward rows (one per
        dgrad workgroup) to row 0 and its weight-gradient stripes (one per wgrad workgroup)
        into the flat gradient, both in row order (the stripes are re-zeroed by the fold)."""
        if not self.det:
            return
        if u.x is not None:
            self._bwd_slab_fold(tf, st)
        if u.row_fold and u.wg_stripes > 1:
            G, lp = self.gviews, u.layer
            self._row_fold(u.dw_acc, u.wg_stripes, u.dw_acc.shape[1], G[f"{lp.name}.weight"], 1, st)
            if u.db_acc is not None:
                self._row_fold(u.db_acc, u.wg_stripes, u.db_acc.shape[1], G[f"{lp.name}.bias"], 1, st)

    def _route_geom(self, u: Unit):
        lp, B = u.layer, self.B
        oh, ow = lp.out_shape.hw
        g = [B, u.y.shape[1], u.y.shape[2], u.y.shape[3], oh, ow, 1 if u.pool is not None else 0]
        if u.pool is not None:
            ps = u.pool.spec
            g += [ps.kernel[0], ps.kernel[1], ps.stride[0], ps.stride[1], u.pool.pads[0], u.pool.pads[2]]
        else:
            g += [1, 1, 1, 1, 0, 0]
        return g

    def _sync_bn_param_grads(self, tf: Transform) -> None:
        if self.sync_bn and tf.has_bn and self.W > 1:
            for p in ("scale", "offset"):
                self.gviews[f"{tf.norm.name}.{p}"].mul_(1.0 / self.W)

    def _dense_bwd_fused(self, u: Unit, prev: Unit, st) -> bool:
        """Input gradient + weight gradient of a dense unit as ONE launch
        (``csa_dense_bwd``) when its weight-gradient operand needs no transform (a
        materialised BN/act input, or an identity transform).  False: not applicable."""
        tf, lp, B = u.in_tf, u.layer, self.B
        if u.xt is None and (tf.has_bn or tf.act is not None):
            return False
        V, G = self.views, self.gviews
        fin, fout = lp.in_shape.numel, lp.spec.hidden
        xw = u.xt if u.xt is not None else u.x.view(B, -1)
        rc = self._rc(self.lib.csa_dense_bwd(
            K.ptr(u.dy), K.ptr(V[f"{lp.name}.weight"]), K.ptr(prev.dy), B, fin, fout,
            K.ptr(u.x.view(B, -1)), _act_id(tf.act), _alpha(tf.act), *self._bn_args_c(tf),
            K.ptr(tf.bwd_slab), K.ptr(xw), K.ptr(G[f"{lp.name}.weight"]), K.ptr(G[f"{lp.name}.bias"]),
            1.0, st), "dense_bwd", positive_ok=True)       # (0: not applicable to this shape)
        if rc > 0:
            self._bwd_slab_fold(tf, st)
        return rc > 0

    def _dd_wgrad_update(self, u: Unit, x: torch.Tensor, dy: torch.Tensor, M: int, act, st) -> None:
        """Weight gradient X^T dY over ``M`` rows with the optimizer update of W / b applied
        in the same launch (csa_dd_wgrad update mode; the head advanced the step counter)."""
        e, lp, V = self.e, u.layer, self.views
        self._rc(K.sched_call(
            self.lib, "csa_dd_wgrad", e.lr_sched_c,
            K.ptr(x), K.ptr(dy), M, lp.in_shape.numel, lp.spec.hidden, act[0], act[1], 1.0, None, None,
            K.ptr(V[f"{lp.name}.weight"]), K.ptr(V[f"{lp.name}.bias"]), *self._slot_ptrs(lp),
            e.opt_id, float(e.lr), K.ptr(e.dstep), st), "dd_wgrad(update)")

    def _dense_bwd_update(self, u: Unit, prev: Optional[Unit], st) -> None:
        """Dense backward + optimizer update of W / b in one launch (dense_update.hip)."""
        e, lib, B, G = self.e, self.lib, self.B, self.gviews
        lp, tf = u.layer, u.in_tf
        fin, fout = lp.in_shape.numel, lp.spec.hidden
        w, b = K.ptr(self.views[f"{lp.name}.weight"]), K.ptr(self.views[f"{lp.name}.bias"])
        xw = K.ptr(u.xt if u.xt is not None else u.x.view(B, -1))
        dx = K.ptr(prev.dy) if prev is not None else None
        opt = (e.opt_id, float(e.lr), K.ptr(e.dstep), *self._slot_ptrs(lp), 1.0)
        # the input side of every form: x, its transform, the BN-backward slab
        xin = (K.ptr(u.x.view(B, -1)), _act_id(tf.act), _alpha(tf.act), *self._bn_args_c(tf),
               K.ptr(tf.bwd_slab) if tf.has_bn else None)
        work = (K.ptr(tf.bn_tab), K.ptr(u.du_part), K.ptr(u.du_cnt))
        if self.head_row and u is self.units[-1]:
            # the head's batch reductions ride along: dWh / dbh into the flat gradient (the
            # optimizer updates them), the step's loss / #correct into the metric ring
            head = (K.ptr(u.y), K.ptr(self.hdl), K.ptr(G["head.weight"]), K.ptr(G["head.bias"]),
                    K.ptr(self.hrl), K.ptr(self.hrc), K.ptr(e.ring_loss), K.ptr(e.ring_correct),
                    e.ring_correct.numel(), float(B if e.cfg.loss_name == "entropy" else B * 10),
                    _act_id(self.head_tf.act), _alpha(self.head_tf.act))
        else:
            head = (None, None, None, None, None, None, None, None, 1, 1.0, 0, 0.0)
        if self.hfuse:
            # weight gradient + update deferred into the pair backward launch; the input
            # gradient (+ transform backward + BN statistics) now
            if self.dp_hf:
                # gradient mode: dW / db stored whole into the flat gradient (slot-free rule)
                rc = lib.csa_dense_update_defer(
                    K.ptr(u.dy), w, b, B, fin, fout, xw, 0, 0.0, K.ptr(e.dstep), None, None, None, None, 1.0, *head)
                if rc >= 0:
                    rc = lib.csa_dense_update_grad_mode(K.ptr(G[f"{lp.name}.weight"]), K.ptr(G[f"{lp.name}.bias"]))
            else:
                rc = K.sched_call(lib, "csa_dense_update_defer", e.lr_sched_c,
                                  K.ptr(u.dy), w, b, B, fin, fout, xw, *opt, *head)
            self._rc(rc, "dense_update_defer", positive_ok=True)
            if prev is not None and not (self.head_dgrad and u is self.units[-1]):
                self._rc(lib.csa_dense_bwd_dgrad(K.ptr(u.dy), w, dx, B, fin, fout, *xin, *work, st),
                         "dense_bwd_dgrad")
            if u is self.br_unit:
                # the update reads W before nothing else does: fork after the input gradient
                cur = torch.cuda.current_stream(e.device)
                self.br_side.wait_stream(cur)
                self._rc(lib.csa_dense_update_flush_last(self.br_side.cuda_stream), "dense_update_branch")
                self._br_pending = True
            return
        if self.fused_grad:
            # data parallel: the same launch stores dW / db whole into the flat gradient
            self._rc(lib.csa_dense_bwd_grad_head(
                K.ptr(u.dy), w, dx, B, fin, fout, *xin, xw, 1.0, *work,
                K.ptr(G[f"{lp.name}.weight"]), K.ptr(G[f"{lp.name}.bias"]),
                *head, K.ptr(e.dstep), st), "dense_bwd_grad")
        else:
            self._rc(K.sched_call(lib, "csa_dense_bwd_update_head", e.lr_sched_c,
                                  K.ptr(u.dy), w, b, dx, B, fin, fout, *xin, xw, *opt, *work, *head, st),
                     "dense_bwd_update")
        self._bwd_slab_fold(tf, st)          # exclusive rows -> row 0, fixed order

    def _optimizer(self, st) -> None:
        """The flat optimizer launch: the update of every parameter no fused kernel updated
        plus the step's side jobs (accumulator zeroing, folds, metrics, cursor, staging).
        (Round 5 measured per-bucket updates on the DP side stream, each right after its
        bucket's exchange: 0.137 against 0.102 ms/step at world 1 — the graph's branches
        serialised behind them: profiles/r5_notes.md.)"""
        e, lib = self.e, self.lib
        lo, hi = e.sync.shard_range()
        s0, s1 = self._slots()
        if e.aps is not None:
            # parameters / slots were updated by the async_ps launch: the update part of this
            # launch runs on four scratch floats (w, g, two slots) and changes nothing real
            if self._aps_dummy is None:
                self._aps_dummy = torch.zeros(4, 4, device=e.device)
            w, g, s0, s1 = self._aps_dummy[0], self._aps_dummy[1], self._aps_dummy[2], self._aps_dummy[3]
        elif e.sync.strategy == "ps" and e.ctx.enabled:
            w, g = e.flat[lo:hi], e.grad_shard
        else:
            w, g = e.flat, e.flat_grad
        zregs = self.zero_regions
        zp = (C.c_void_p * 16)(*[r.data_ptr() for r in zregs])
        zn = (C.c_long * 16)(*[r.numel() for r in zregs])
        folds = []          # striped conv weight gradients / head partials -> summed inside the update
        offs = self.model.state.offsets
        for u in self.units:
            if u.kind == "conv" and u.wg_stripes > 1 and not u.row_fold and not u.tail_fold:
                lp = u.layer
                folds.append((offs[f"{lp.name}.weight"], u.dw_acc.shape[1], u.dw_acc, u.wg_stripes, u.dw_acc.shape[1], 1))
                if u.db_acc is not None:
                    folds.append((offs[f"{lp.name}.bias"], u.db_acc.shape[1], u.db_acc, u.wg_stripes, u.db_acc.shape[1], 1))
        if self.head_rg:
            hp = self.head_part
            kw = self.head_kw
            folds.append((offs["head.weight"], kw, hp, hp.shape[0], hp.shape[1], 0))
            # the bias span rounded up to a float4: the partial rows' padding and the flat
            # layout's padding are zero, so the extra lanes update zero parameters by zero
            # (no per-element edge path: one round trip instead of four)
            nb = 12 if hp.shape[1] >= kw + 12 and self.e.flat.numel() >= offs["head.bias"] + 12 else 10
            folds.append((offs["head.bias"], nb, hp[:, kw:], hp.shape[0], hp.shape[1], 0))
        if len(folds) > 8:
            raise Unsupported("more than 8 striped gradients")
        fo, fn, fl = ((C.c_long * 8)(*[f[i] for f in folds]) for i in (0, 1, 4))
        fS, fz = ((C.c_int * 8)(*[f[i] for f in folds]) for i in (3, 5))
        fs = (C.c_void_p * 8)(*[f[2].data_ptr() for f in folds])
        keep = self.keep_ranges
        if len(keep) > 32:
            raise RuntimeError(f"{len(keep)} stored dense gradient ranges (optimizer holds 32)")
        klo = (C.c_long * 32)(*[k[0] for k in keep])
        khi = (C.c_long * 32)(*[k[1] for k in keep])
        segs = self.opt_segments
        slo = (C.c_long * 16)(*[x[0] for x in segs])
        shi = (C.c_long * 16)(*[x[1] for x in segs])
        div = float(self.B if e.cfg.loss_name == "entropy" else self.B * 10)
        if self.head_rg:
            met = (K.ptr(self.head_mloss), K.ptr(self.head_mcorr), self.head_mloss.numel(), div,
                   K.ptr(e.ring_loss), K.ptr(e.ring_correct), e.ring_correct.numel())
        elif self.head_sep:             # the row head's per-row loss / #correct
            met = (K.ptr(self.hrl), K.ptr(self.hrc), self.B, div,
                   K.ptr(e.ring_loss), K.ptr(e.ring_correct), e.ring_correct.numel())
        else:
            met = (None, None, 0, 1.0, None, None, 1)
        if self.staged:
            # the head advanced the cursor; the trailing workgroups stage the next batch
            stage = self._stage_args()
            cursor_args = (None, 0)
        else:
            stage = (None, None, None, None, 0, 0, None, None)
            cursor_args = (K.ptr(e.stream.cursor), e.stream.wrap)
        if self.carry is not None:
            lib.csa_optimizer_set_pending(K.ptr(self.carry_pending))
        self._rc(K.sched_call(
            lib, "csa_optimizer2s", e.lr_sched_c,
            e.opt_id, K.ptr(w), K.ptr(g), K.ptr(s0), K.ptr(s1), w.numel(), slo, shi, len(segs),
            0 if self.ps_mode else 1, float(e.lr), K.ptr(e.dstep),
            zp, zn, len(zregs), fo, fn, fs, fS, fl, fz, len(folds), klo, khi, len(keep),
            *met, *cursor_args, *stage, st), "optimizer")
        if self.hfuse and lib.csa_dense_update_pending():
            raise RuntimeError("deferred dense updates were not consumed by the pair backward")
        if e.sync.strategy == "ps" and e.ctx.enabled:
            e.sync.all_gather_params(e.flat)
