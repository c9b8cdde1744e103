"""The DSL-built digit CNN (reference ``cnn()``, construct_distribute.py:208-265).

Parameters live in ONE flat fp32 buffer (``FlatState``) with every named tensor a view
into it.  That layout is what the MI355X path is built around:

* the fused optimizer kernel updates all 2.28 M parameters in one launch,
* data-parallel gradient sync is one (or a few) large RCCL collectives over the flat
  gradient buffer instead of one call per tensor,
* checkpoints are a single contiguous copy.

Tensors use the reference's layouts: activations NHWC, conv weights HWIO
(``[kh, kw, cin, cout]``), dense weights ``[in, out]`` so the flatten order (H, W, C)
matches construct_distribute.py:176-178.

``DigitNet.forward`` here is the eager PyTorch implementation — the numerics oracle
for the HIP kernels and the CPU path used by tests.  The MI355X training step lives in
``cloud_server_amd.runtime.engine`` and calls the fused kernels in ``ops``.
"""
from __future__ import annotations

import math
from typing import Dict, Iterator, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import dropout_ref
from .dsl import (ActSpec, AvgPoolSpec, ConvSpec, DenseSpec, DepthwiseConvSpec, DropoutSpec, GroupNormSpec, LayerPlan,
                  LrnSpec, NetPlan, NormSpec, PoolSpec, TrainConfig)


def trunc_normal_(t: torch.Tensor, std: float, gen: Optional[torch.Generator] = None) -> torch.Tensor:
    """tf.truncated_normal: N(0, std) redrawn outside ±2 std (construct_distribute.py:72-78)."""
    with torch.no_grad():
        t.normal_(0.0, 1.0, generator=gen)
        for _ in range(8):
            bad = t.abs() > 2.0
            if not bool(bad.any()):
                break
            t[bad] = torch.randn(int(bad.sum()), generator=gen, dtype=t.dtype, device=t.device)
        t.clamp_(-2.0, 2.0).mul_(std)
    return t


class FlatState:
    """Contiguous storage for named tensors, with named views (params, grads, optimizer slots)."""

    ALIGN = 64  # elements (256 B): every tensor starts 256-B aligned for dwordx4 access

    def __init__(self, shapes: Dict[str, Tuple[int, ...]], device="cpu", dtype=torch.float32,
                 pad_multiple: int = 1):
        self.shapes = dict(shapes)
        self.offsets: Dict[str, int] = {}
        off = 0
        for k, s in self.shapes.items():
            self.offsets[k] = off
            n = math.prod(s)
            off += -(-n // self.ALIGN) * self.ALIGN
        m = self.ALIGN * max(1, pad_multiple)   # sharded ("ps") mode needs numel % world == 0
        self.numel = -(-off // m) * m
        self.buffer = torch.zeros(self.numel, device=device, dtype=dtype)

    def view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        buf = self.buffer if buf is None else buf
        o, s = self.offsets[name], self.shapes[name]
        return buf[o:o + math.prod(s)].view(s)

    def views(self, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        return {k: self.view(k, buf) for k in self.shapes}

    def like(self) -> torch.Tensor:
        return torch.zeros_like(self.buffer)


def init_params(plan: NetPlan, state: FlatState, seed: int = 0) -> None:
    """Reference initialisers: trunc-normal σ / zeros / 'xavier' (σ/fan_in), bias 0.1,
    BN scale 1 offset 0 (construct_distribute.py:57-87, 155-165, 180-181, 262-263)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    host = torch.zeros(state.numel, dtype=torch.float32)
    for lp in plan.layers:
        sp = lp.spec
        if isinstance(sp, (ConvSpec, DepthwiseConvSpec)):
            # (a depthwise weight is [kh, kw, C, M]: the same three initialisers on that shape)
            w = state.view(f"{lp.name}.weight", host)
            if sp.init == "zero":
                w.zero_()
            elif sp.init == "xavier":
                kh, kw, cin, _ = w.shape
                trunc_normal_(w, sp.stddev / float(kw * cin * w.shape[3]), gen)  # shape[1]*[2]*[3] (:80)
            else:
                trunc_normal_(w, sp.stddev, gen)
            if sp.bias:
                state.view(f"{lp.name}.bias", host).fill_(sp.bias_constant)
        elif isinstance(sp, DenseSpec):
            trunc_normal_(state.view(f"{lp.name}.weight", host), 0.1, gen)
            state.view(f"{lp.name}.bias", host).fill_(0.1)
        elif isinstance(sp, (NormSpec, GroupNormSpec)):
            state.view(f"{lp.name}.scale", host).fill_(1.0)
            state.view(f"{lp.name}.offset", host).zero_()
    trunc_normal_(state.view("head.weight", host), 0.1, gen)
    state.view("head.bias", host).fill_(0.1)
    state.buffer.copy_(host)


def act_fwd(x: torch.Tensor, sp: ActSpec) -> torch.Tensor:
    if sp.func == "relu":
        return torch.relu(x)
    if sp.func == "leaky_relu":
        return torch.maximum(x, sp.alpha * x)   # tf.maximum(x, a*x) (:148-151)
    return torch.sigmoid(x)


def _global_moments(h: torch.Tensor, dims) -> "tuple[torch.Tensor, torch.Tensor]":
    """Biased mean / variance of ``h`` over ``dims`` AND over every rank of the default
    process group: one all-reduce of [sum, sum of squares, count] (2C + 1 floats)."""
    import torch.distributed as dist
    from torch.distributed.nn.functional import all_reduce
    C = h.shape[-1]
    n = torch.full((1,), float(h.numel() // C), dtype=h.dtype, device=h.device)
    st = torch.cat([h.sum(dim=dims), (h * h).sum(dim=dims), n])
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        st = all_reduce(st)
    cnt = st[2 * C]
    mean = st[:C] / cnt
    var = (st[C:2 * C] / cnt - mean * mean).clamp_min(0.0)
    return mean, var


class DigitNet(nn.Module):
    """Eager model over a ``FlatState``.  ``forward(x)`` takes NHWC [B,28,28,1] or [B,784]."""

    def __init__(self, plan: NetPlan, device="cpu", seed: int = 0, bn_mode: str = "running",
                 bn_momentum: float = 0.1, pad_multiple: int = 1, dense_last: bool = False):
        super().__init__()
        self.plan = plan
        self.bn_mode = bn_mode
        self.bn_momentum = bn_momentum
        # SyncBN: under data parallelism the reference's single worker
        # normalised over its whole batch; with sync_bn the per-channel {sum, sum of
        # squares, count} are all-reduced (autograd-aware, so the backward statistics are
        # global too) and every replica normalises with the GLOBAL batch statistics
        self.sync_bn = False
        self.deterministic = False          # CSA_DETERMINISTIC: atomics-free op choices
        # dropout masks (ops/dropout_ref.py) are a function of (seed, layer, step, element):
        # the engine hands over its device step counter and its place in the global batch
        # (``drop_step = eng.dstep``); a model built on its own draws the masks of step 0
        self.seed = seed
        self.drop_step = torch.zeros(1, dtype=torch.int64, device=device)
        self.drop_world, self.drop_rank = 1, 0
        self.state = FlatState(plan.param_shapes(dense_last), device=device, pad_multiple=pad_multiple)
        init_params(plan, self.state, seed)
        self.flat = nn.Parameter(self.state.buffer)
        self.state.buffer = self.flat.data
        # running BN statistics (fix for quirk 3); NOT part of the optimised flat buffer
        for lp in plan.layers:
            if isinstance(lp.spec, NormSpec):
                c = lp.in_shape.c
                self.register_buffer(f"bn{lp.index}_mean", torch.zeros(c, device=device))
                self.register_buffer(f"bn{lp.index}_var", torch.ones(c, device=device))

    # ---- named parameter views (grad flows to self.flat) ----
    def p(self, name: str) -> torch.Tensor:
        o, s = self.state.offsets[name], self.state.shapes[name]
        return self.flat[o:o + math.prod(s)].view(s)

    def named_tensors(self) -> Dict[str, torch.Tensor]:
        return {k: self.p(k) for k in self.state.shapes}

    def forward(self, x: torch.Tensor, use_batch_stats: Optional[bool] = None) -> torch.Tensor:
        if use_batch_stats is None:
            use_batch_stats = self.training or self.bn_mode == "batch"
        B = x.shape[0]
        h = x.reshape(B, 28, 28, 1) if x.dim() == 2 else x
        for lp in self.plan.layers:
            h = self._layer(lp, h, use_batch_stats)
        if h.dim() != 2:
            h = h.reshape(B, -1)  # quirk 2 fixed: flatten the LAST hidden tensor
        return h @ self.p("head.weight") + self.p("head.bias")

    def _layer(self, lp: LayerPlan, h: torch.Tensor, use_batch_stats: bool) -> torch.Tensor:
        sp = lp.spec
        if isinstance(sp, ConvSpec):
            pt, pb, pl, pr = lp.pads
            t = h.permute(0, 3, 1, 2)
            if any(lp.pads):
                t = F.pad(t, (pl, pr, pt, pb))
            w = self.p(f"{lp.name}.weight").permute(3, 2, 0, 1)
            b = self.p(f"{lp.name}.bias") if sp.bias else None
            stride = tuple(sp.stride)
            if (sp.kh, sp.kw) == (1, 1) and stride != (1, 1):
                # A strided 1x1 conv reads only every (sh, sw)-th pixel: subsample, then a
                # stride-1 conv — the same sums, exactly.  torch 2.10.0+rocm7.0 on the CPU
                # corrupts the heap in the mkldnn backward of F.conv2d with a 1x1 kernel and
                # stride (2,1), (1,2) or (2,2) (segfault, or "corrupted size vs. prev_size").
                t = t[:, :, ::stride[0], ::stride[1]]
                stride = (1, 1)
            return F.conv2d(t, w, b, stride=stride).permute(0, 2, 3, 1)
        if isinstance(sp, DepthwiseConvSpec):
            # tf.nn.depthwise_conv2d as a grouped conv with groups = C: torch's group of output
            # channel o is o // M, which is TF's c * M + q order.  One form in normal and
            # deterministic mode (the CPU backward sums in a fixed order).
            pt, pb, pl, pr = lp.pads
            Cn = h.shape[-1]
            t = h.permute(0, 3, 1, 2)
            if any(lp.pads):
                t = F.pad(t, (pl, pr, pt, pb))
            w = self.p(f"{lp.name}.weight").permute(2, 3, 0, 1).reshape(Cn * sp.mult, 1, sp.kh, sp.kw)
            b = self.p(f"{lp.name}.bias") if sp.bias else None
            stride = tuple(sp.stride)
            if (sp.kh, sp.kw) == (1, 1) and stride != (1, 1):
                # (the strided 1x1 workaround of the conv branch above)
                t = t[:, :, ::stride[0], ::stride[1]]
                stride = (1, 1)
            return F.conv2d(t, w, b, stride=stride, groups=Cn).permute(0, 2, 3, 1)
        if isinstance(sp, PoolSpec):
            pt, pb, pl, pr = lp.pads
            t = h.permute(0, 3, 1, 2)
            if any(lp.pads):
                t = F.pad(t, (pl, pr, pt, pb), value=float("-inf"))
            if self.deterministic:
                # gather-form max pool: unfold + max (backward = one scatter per window +
                # col2im, both free of atomics) instead of max_pool2d's atomic backward
                Bn, Cn, Hn, Wn = t.shape
                kh, kw = sp.kernel
                oh, ow = (Hn - kh) // sp.stride[0] + 1, (Wn - kw) // sp.stride[1] + 1
                cols = F.unfold(t, (kh, kw), stride=sp.stride).view(Bn, Cn, kh * kw, oh * ow)
                return cols.max(dim=2).values.view(Bn, Cn, oh, ow).permute(0, 2, 3, 1)
            return F.max_pool2d(t, sp.kernel, sp.stride).permute(0, 2, 3, 1)
        if isinstance(sp, AvgPoolSpec):
            # tf.nn.avg_pool: the window's sum over a zero-padded tensor, divided by the same
            # window sum of a padded tensor of ones (the number of in-image taps)
            pt, pb, pl, pr = lp.pads
            t = h.permute(0, 3, 1, 2)
            ones = torch.ones((1, 1) + tuple(t.shape[2:]), dtype=h.dtype, device=h.device)
            if any(lp.pads):
                t = F.pad(t, (pl, pr, pt, pb))
                ones = F.pad(ones, (pl, pr, pt, pb))
            kh, kw = sp.kernel
            stride = tuple(sp.stride)
            if self.deterministic:
                # gather form, as the max pool above: no atomic backward
                Bn, Cn, Hn, Wn = t.shape
                oh, ow = (Hn - kh) // stride[0] + 1, (Wn - kw) // stride[1] + 1
                tot = F.unfold(t, (kh, kw), stride=stride).view(Bn, Cn, kh * kw, oh * ow).sum(dim=2)
                cnt = F.unfold(ones, (kh, kw), stride=stride).sum(dim=1).view(1, 1, oh * ow)
                return (tot / cnt).view(Bn, Cn, oh, ow).permute(0, 2, 3, 1)
            tot = F.avg_pool2d(t, (kh, kw), stride, divisor_override=1)
            cnt = F.avg_pool2d(ones, (kh, kw), stride, divisor_override=1)
            return (tot / cnt).permute(0, 2, 3, 1)
        if isinstance(sp, LrnSpec):
            # tf.nn.lrn: the window sum as 2r + 1 shifted adds over zero-padded squares, in
            # ascending channel order (its backward is shifted adds too: nothing atomic, one
            # form in normal and deterministic mode).  alpha is not divided by the window size.
            # (taps beyond C - 1 channels away are all padding: adding their zeros changes no bit)
            Cn = h.shape[-1]
            r = min(sp.depth_radius, Cn - 1)
            sq = F.pad(h * h, (r, r))
            q = sq[..., 0:Cn]
            for d in range(1, 2 * r + 1):
                q = q + sq[..., d:d + Cn]
            return h * (sp.bias + sp.alpha * q) ** (-sp.beta)
        if isinstance(sp, ActSpec):
            return act_fwd(h, sp)
        if isinstance(sp, DropoutSpec):
            if not self.training:
                return h
            B = h.shape[0]
            keep = dropout_ref.keep_mask_torch(dropout_ref.drop_seed(self.seed, lp.index), self.drop_step, B,
                                               h[0].numel(), sp.keep_prob, self.drop_world, self.drop_rank)
            s = dropout_ref.keep_scale(sp.keep_prob)
            return h * (keep.view(h.shape).to(h.dtype) * s)
        if isinstance(sp, GroupNormSpec):
            # every group of every sample on its own, biased centred moments: x as
            # [B, HW, G, C/G], reduced over HW and C/G (one form in normal and deterministic
            # mode; no running statistics, nothing registered)
            Bn, Cn = h.shape[0], h.shape[-1]
            t = h.reshape(Bn, -1, sp.groups, Cn // sp.groups)
            mean = t.mean(dim=(1, 3), keepdim=True)
            d = t - mean
            var = (d * d).mean(dim=(1, 3), keepdim=True)
            xhat = (d * torch.rsqrt(var + sp.epsilon)).reshape(h.shape)
            return xhat * self.p(f"{lp.name}.scale") + self.p(f"{lp.name}.offset")
        if isinstance(sp, NormSpec):
            dims = tuple(range(h.dim() - 1))
            scale, offset = self.p(f"{lp.name}.scale"), self.p(f"{lp.name}.offset")
            rm, rv = getattr(self, f"bn{lp.index}_mean"), getattr(self, f"bn{lp.index}_var")
            if use_batch_stats and self.sync_bn and self.training:
                mean, var = _global_moments(h, dims)
                with torch.no_grad():
                    m = self.bn_momentum
                    rm.mul_(1 - m).add_(mean.detach(), alpha=m)
                    rv.mul_(1 - m).add_(var.detach(), alpha=m)
            elif use_batch_stats:
                mean = h.mean(dim=dims)
                var = h.var(dim=dims, unbiased=False)   # tf.nn.moments: biased
                if self.training:
                    with torch.no_grad():
                        m = self.bn_momentum
                        rm.mul_(1 - m).add_(mean.detach(), alpha=m)
                        rv.mul_(1 - m).add_(var.detach(), alpha=m)
            else:
                mean, var = rm, rv
            return (h - mean) * torch.rsqrt(var + sp.epsilon) * scale + offset
        if isinstance(sp, DenseSpec):
            if h.dim() != 2:
                h = h.reshape(h.shape[0], -1)
            return h @ self.p(f"{lp.name}.weight") + self.p(f"{lp.name}.bias")
        raise TypeError(sp)

    # ---- checkpoint helpers: named keys derived from layer index (quirk 14 fixed) ----
    def export_state(self) -> Dict[str, torch.Tensor]:
        out = {k: v.detach().clone().cpu() for k, v in self.named_tensors().items()}
        for name, buf in self.named_buffers():
            out["buffers." + name] = buf.detach().clone().cpu()
        return out

    def import_state(self, sd: Dict[str, torch.Tensor]) -> None:
        with torch.no_grad():
            for k, v in self.named_tensors().items():
                if k not in sd:
                    raise KeyError(f"checkpoint missing {k}")
                v.copy_(sd[k].to(v.device).view(v.shape))
            for name, buf in self.named_buffers():
                key = "buffers." + name
                if key in sd:
                    buf.copy_(sd[key].to(buf.device))


def loss_fn(name: str, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """construct_distribute.py:285-298.  ``labels`` are int class ids; one-hot is implicit."""
    if name == "mse":
        onehot = F.one_hot(labels.long(), logits.shape[1]).to(logits.dtype)
        return ((onehot - logits) ** 2).mean()
    return F.cross_entropy(logits, labels.long())


def build_model(cfg: TrainConfig, device="cpu", pad_multiple: int = 1,
                dense_last: bool = False) -> DigitNet:
    return DigitNet(cfg.plan(), device=device, seed=cfg.seed, bn_mode=cfg.bn_mode,
                    pad_multiple=pad_multiple, dense_last=dense_last)
