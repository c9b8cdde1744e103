"""Network-config DSL: the reference's ``model.json`` schema, validated and shape-inferred.

The reference accepts a JSON object (API.md:306-332) and walks ``net_config.middle_layer``
inside ``cnn()`` (apps/construction/util/construct_distribute.py:208-265) with per-layer
defaults read via ``key in every_inner.keys()`` checks.  Here the same JSON is parsed
once, on submit, into typed layer specs with explicit defaults, and the whole network is
shape-inferred so a bad config is rejected by the API instead of crashing a worker.

Reference quirks and how they are handled:

* quirk 1 – optimizer / learning rate ignored (construct_distribute.py:372): honoured
  here; ``compat_adagrad`` restores the hard-coded ``Adagrad(1e-4)``.
* quirk 2 – head flattens ``x`` instead of ``last`` (construct_distribute.py:257): fixed,
  the head flattens the last hidden tensor.
* quirk 3 – BN uses batch statistics at inference (construct_distribute.py:164):
  ``bn_mode="running"`` (default) keeps running stats for eval; ``"batch"`` is the compat mode.
* ``isBias`` is a string compare against ``"False"`` (construct_distribute.py:228): kept.
* unknown layer names are skipped silently in the reference; we keep them in the parsed
  config (so ``model.json`` round-trips) but they produce no layer.
* the step size never changes in the reference (one ``AdagradOptimizer(1e-4)``):
  ``options.lr_schedule`` adds decay and warm-up as a pure function of the step counter
  (ops/lr_schedule.py); a config without it trains at the constant rate, as before.
* the reference trains on the stored files only (the offline ``/preprocess/`` "copy twins"
  are its one augmentation): ``options.augment`` redraws a shift / rotation / zoom / erased
  rectangle for every training image at every step (ops/augment_ref.py); a config without it
  trains on the stored images, as before.
* the reference only ever builds ``tf.nn.max_pool`` (construct_distribute.py:121-130): a
  ``pool`` entry takes ``"mode": "avg"`` (``tf.nn.avg_pool``: padding never enters the sum or
  the divisor) and ``"kernel": "global"`` (the window is the whole input map); an entry
  without either is the reference's max pool, as before.
* ``keep_prob`` fed but never used (construct_distribute.py:364-417 feeds 0.5 / 1.0; the
  ``tf.nn.dropout`` line is a comment, construct_distribute_url.py:328): a ``dropout``
  layer is a real layer here; a config without one trains without dropout, as before.
* the reference has no ``tf.nn.lrn`` although the TF1 nets its users copy do (the CIFAR-10
  tutorial's ``norm1`` / ``norm2``): ``{"layer": "lrn"}`` was an unknown name, silently
  skipped, so the job trained another network than the one written.  It is a real layer now
  (``LrnSpec``: ``depth_radius``, ``bias``, ``alpha``, ``beta`` with TF's defaults; alpha is
  not divided by the window size and the window is clipped to the channels, never padded).
* the reference's only normalisation is BatchNorm over the batch.  A ``norm`` entry with
  ``"mode": "layer" | "group" | "instance"`` normalises every group of every sample on its own
  (``GroupNormSpec``, ``tf.contrib.layers``' ``layer_norm`` / ``group_norm`` /
  ``instance_norm``): no running statistics, the same arithmetic in training and inference.
  Without ``mode`` (or with ``"batch"``) the entry is the reference's BatchNorm as before.
* the reference has no ``tf.nn.depthwise_conv2d`` although the TF1 nets its users copy are
  built from it (slim's MobileNet, ``separable_conv2d``): ``{"layer": "depthwise"}`` was an
  unknown name, silently skipped, so the job trained another network than the one written.
  It is a real layer now (``DepthwiseConvSpec``: ``filter: [kh, kw, M]`` with M the channel
  multiplier, weight ``[kh, kw, C, M]``, output channel ``c * M + q`` reads input channel c;
  every other key as a ``conv``'s).  A separable convolution is this layer and a 1x1 ``conv``.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass, field, asdict, replace
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

INPUT_HW = 28          # construct_distribute.py:216 — input fixed 28x28x1
INPUT_C = 1
NUM_CLASSES = 10       # construct_distribute.py:261 — fixed 10-way head

LOSSES = ("entropy", "mse")
OPTIMIZERS = ("GradientDescentOptimizer", "AdagradOptimizer", "AdamOptimizer", "AdadeltaOptimizer")
ACTIVATIONS = ("sigmoid", "relu", "leaky_relu")
INITS = ("norm", "zero", "xavier")
PADDINGS = ("SAME", "VALID")
POOL_MODES = ("max", "avg")
NORM_MODES = ("batch", "layer", "group", "instance")
GLOBAL = "global"      # a pool's ``kernel`` and ``stride`` until plan_network knows the map
LR_SCHEDULES = ("constant", "exponential", "inverse_time", "cosine")


class ConfigError(ValueError):
    """Raised when a net config is invalid (API turns it into a 400)."""


def _as_int(v: Any, name: str) -> int:
    try:
        return int(v)
    except (TypeError, ValueError):
        raise ConfigError(f"{name}: expected int, got {v!r}")


def _as_float(v: Any, name: str) -> float:
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ConfigError(f"{name}: expected float, got {v!r}")


def _pair(v: Any, name: str) -> Tuple[int, int]:
    if isinstance(v, (list, tuple)) and len(v) >= 2:
        return _as_int(v[0], name), _as_int(v[1], name)
    if isinstance(v, (int, float, str)):
        i = _as_int(v, name)
        return i, i
    raise ConfigError(f"{name}: expected [h, w], got {v!r}")


def same_pads(size: int, k: int, s: int) -> Tuple[int, int, int]:
    """TF 'SAME' padding: returns (out, pad_before, pad_after). Even kernels pad after."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


def valid_out(size: int, k: int, s: int) -> int:
    return (size - k) // s + 1


@dataclass
class ConvSpec:
    kh: int
    kw: int
    cout: int
    stride: Tuple[int, int] = (1, 1)
    padding: str = "SAME"
    init: str = "norm"
    bias: bool = False
    bias_constant: float = 0.1
    stddev: float = 0.1
    kind: str = "conv"


@dataclass
class DepthwiseConvSpec:
    """``tf.nn.depthwise_conv2d``: every input channel c is convolved on its own with ``mult``
    kernels, weight ``[kh, kw, C, mult]``, output channel ``c * mult + q``.  Not a ConvSpec:
    that class means "dense convolution" wherever it is tested (the pair plan, ``conv_tail``,
    the gconv rule)."""
    kh: int
    kw: int
    mult: int = 1
    stride: Tuple[int, int] = (1, 1)
    padding: str = "SAME"
    init: str = "norm"
    bias: bool = False
    bias_constant: float = 0.1
    stddev: float = 0.1
    kind: str = "depthwise"


@dataclass
class PoolSpec:
    kernel: Tuple[int, int] = (2, 2)
    stride: Tuple[int, int] = (2, 2)
    padding: str = "SAME"
    kind: str = "pool"


@dataclass
class AvgPoolSpec:
    """``tf.nn.avg_pool``: the sum of a window's in-image taps over their number.  Not a
    PoolSpec: that class means "max pool with a window argmax" wherever it is tested."""
    kernel: Tuple[int, int] = (2, 2)
    stride: Tuple[int, int] = (2, 2)
    padding: str = "SAME"
    kind: str = "pool"
    mode: str = "avg"


@dataclass
class ActSpec:
    func: str = "sigmoid"
    alpha: float = 0.2
    kind: str = "active"


@dataclass
class DenseSpec:
    hidden: int = 512
    kind: str = "connect"


@dataclass
class NormSpec:
    epsilon: float = 1e-3
    kind: str = "norm"


@dataclass
class DropoutSpec:
    keep_prob: float = 0.5                 # the value the reference feeds on training steps
    kind: str = "dropout"


@dataclass
class LrnSpec:
    """``tf.nn.lrn`` over the channels of a pixel: ``y_c = x_c * s_c ** -beta`` with
    ``s_c = bias + alpha * sum(x_j ** 2 for |j - c| <= depth_radius)``, the window clipped to
    the channels (TF's defaults)."""
    depth_radius: int = 5
    bias: float = 1.0
    alpha: float = 1.0
    beta: float = 0.5
    kind: str = "lrn"


@dataclass
class GroupNormSpec:
    """Normalisation of every group of every sample on its own: with x as ``[B, HW, G, C/G]``
    and m = HW * C/G, ``y = (x - mean) * rsqrt(var + epsilon) * scale_c + offset_c`` with the
    biased moments over a group's m elements (TF's).  ``layer`` is G = 1, ``instance`` G = C;
    ``groups`` is None until plan_network knows C.  Not a NormSpec: that class means
    "BatchNorm with running statistics" wherever it is tested."""
    groups: Optional[int] = None
    epsilon: float = 1e-6                  # tf.contrib.layers.group_norm's
    mode: str = "layer"
    kind: str = "norm"


LayerSpec = Union[ConvSpec, PoolSpec, AvgPoolSpec, ActSpec, DenseSpec, NormSpec, DropoutSpec, LrnSpec,
                  GroupNormSpec, DepthwiseConvSpec]


def parse_layer(d: Dict[str, Any], idx: int) -> Optional[LayerSpec]:
    """One ``middle_layer`` entry -> spec (defaults from construct_distribute.py:219-250)."""
    if not isinstance(d, dict):
        raise ConfigError(f"middle_layer[{idx}] must be an object")
    name = d.get("layer")
    where = f"middle_layer[{idx}]"
    if name == "conv":
        if "filter" not in d:
            raise ConfigError(f"{where}: conv needs 'filter': [kh, kw, cout]")
        f = d["filter"]
        if not isinstance(f, (list, tuple)) or len(f) != 3:
            raise ConfigError(f"{where}: filter must be [kh, kw, cout]")
        kh, kw, cout = (_as_int(x, where + ".filter") for x in f)
        if min(kh, kw, cout) <= 0:
            raise ConfigError(f"{where}: filter dims must be positive")
        pad = str(d.get("padding", "SAME")).upper()
        init = str(d.get("init", "norm"))
        if pad not in PADDINGS:
            raise ConfigError(f"{where}: padding must be SAME or VALID")
        if init not in INITS:
            raise ConfigError(f"{where}: init must be one of {INITS}")
        stride = _pair(d.get("stride", [1, 1]), where + ".stride")
        if min(stride) <= 0:
            raise ConfigError(f"{where}: stride must be positive")
        # reference: isBias = every_inner["isBias"] != "False"  (string compare, :228)
        bias = ("isBias" in d) and (d["isBias"] != "False") and (d["isBias"] is not False)
        return ConvSpec(kh, kw, cout, stride, pad, init, bias,
                        _as_float(d.get("bias_constant", 0.1), where),
                        _as_float(d.get("stddev_norm", 0.1), where))
    if name == "depthwise":
        # conv's keys, defaults and quirks; ``filter`` is [kh, kw, channel multiplier]
        if "filter" not in d:
            raise ConfigError(f"{where}: depthwise needs 'filter': [kh, kw, multiplier]")
        f = d["filter"]
        if not isinstance(f, (list, tuple)) or len(f) != 3:
            raise ConfigError(f"{where}: depthwise filter must be [kh, kw, multiplier]")
        kh, kw, mult = (_as_int(x, where + ".filter") for x in f)
        if min(kh, kw, mult) <= 0:
            raise ConfigError(f"{where}: depthwise filter dims and multiplier must be positive")
        pad = str(d.get("padding", "SAME")).upper()
        init = str(d.get("init", "norm"))
        if pad not in PADDINGS:
            raise ConfigError(f"{where}: depthwise padding must be SAME or VALID")
        if init not in INITS:
            raise ConfigError(f"{where}: depthwise init must be one of {INITS}")
        stride = _pair(d.get("stride", [1, 1]), where + ".stride")
        if min(stride) <= 0:
            raise ConfigError(f"{where}: depthwise stride must be positive")
        bias = ("isBias" in d) and (d["isBias"] != "False") and (d["isBias"] is not False)
        return DepthwiseConvSpec(kh, kw, mult, stride, pad, init, bias,
                                 _as_float(d.get("bias_constant", 0.1), where),
                                 _as_float(d.get("stddev_norm", 0.1), where))
    if name == "pool":
        mode = d.get("mode", "max")
        if not isinstance(mode, str) or mode not in POOL_MODES:
            raise ConfigError(f"{where}: mode must be one of {POOL_MODES}")
        cls = AvgPoolSpec if mode == "avg" else PoolSpec
        if isinstance(d.get("kernel"), str) and d["kernel"].strip().lower() == GLOBAL:
            # the whole input map, whatever its size: plan_network fills in the numbers
            if "stride" in d or "padding" in d:
                raise ConfigError(f"{where}: kernel 'global' takes no stride or padding")
            return cls(GLOBAL, GLOBAL, "VALID")
        pad = str(d.get("padding", "SAME")).upper()
        if pad not in PADDINGS:
            raise ConfigError(f"{where}: padding must be SAME or VALID")
        k = _pair(d.get("kernel", [2, 2]), where + ".kernel")
        s = _pair(d.get("stride", [2, 2]), where + ".stride")
        if min(k) <= 0 or min(s) <= 0:
            raise ConfigError(f"{where}: kernel/stride must be positive")
        return cls(k, s, pad)
    if name == "active":
        func = str(d.get("active_func", "sigmoid"))
        if func not in ACTIVATIONS:
            raise ConfigError(f"{where}: active_func must be one of {ACTIVATIONS}")
        p = d.get("param", [0.2])
        alpha = _as_float(p[0], where + ".param") if isinstance(p, (list, tuple)) and p else 0.2
        return ActSpec(func, alpha)
    if name == "connect":
        h = _as_int(d.get("hidden", 512), where + ".hidden")
        if h <= 0:
            raise ConfigError(f"{where}: hidden must be positive")
        return DenseSpec(h)
    if name == "norm":
        mode = d.get("mode", "batch")
        if not isinstance(mode, str) or mode not in NORM_MODES:
            raise ConfigError(f"{where}: mode must be one of {NORM_MODES}")
        if mode == "batch":
            return NormSpec(_as_float(d.get("epsilon", 1e-3), where + ".epsilon"))
        groups = None
        if mode == "group":
            if "groups" not in d:
                raise ConfigError(f"{where}: mode 'group' needs groups")
            groups = _as_whole(d["groups"], where + ".groups")
            if not (1 <= groups < 2 ** 31):
                raise ConfigError(f"{where}.groups must be a whole number >= 1")
        elif "groups" in d:
            raise ConfigError(f"{where}: groups goes with mode 'group' only")
        if isinstance(d.get("epsilon"), bool):
            raise ConfigError(f"{where}.epsilon: expected float, got {d['epsilon']!r}")
        eps = _as_float(d.get("epsilon", 1e-6), where + ".epsilon")
        if not (math.isfinite(eps) and eps > 0):
            raise ConfigError(f"{where}.epsilon must be finite and > 0")
        return GroupNormSpec(groups, eps, mode)
    if name == "dropout":
        kp = _as_float(d.get("keep_prob", 0.5), where + ".keep_prob")
        if not (0.0 < kp <= 1.0):
            raise ConfigError(f"{where}: keep_prob must be in (0, 1]")
        return DropoutSpec(kp)
    if name == "lrn":
        r = _as_whole(d.get("depth_radius", 5), where + ".depth_radius")
        if not (0 <= r < 2 ** 15):
            raise ConfigError(f"{where}: depth_radius must be in 0..{2 ** 15 - 1}")
        vals = {}
        for key, default in (("bias", 1.0), ("alpha", 1.0), ("beta", 0.5)):
            if isinstance(d.get(key, default), bool):
                raise ConfigError(f"{where}.{key}: expected float, got {d[key]!r}")
            vals[key] = _as_float(d.get(key, default), f"{where}.{key}")
            if not math.isfinite(vals[key]):
                raise ConfigError(f"{where}.{key} must be finite")
        if not vals["bias"] > 0:
            raise ConfigError(f"{where}.bias must be > 0")
        if not vals["alpha"] >= 0:
            raise ConfigError(f"{where}.alpha must be >= 0")
        if not vals["beta"] > 0:
            raise ConfigError(f"{where}.beta must be > 0")
        return LrnSpec(r, vals["bias"], vals["alpha"], vals["beta"])
    return None  # unknown layers are skipped, as in the reference (:208-250)


@dataclass
class TensorShape:
    """Per-sample activation shape. ``hw`` is None once flattened to a vector."""
    c: int
    hw: Optional[Tuple[int, int]] = None

    @property
    def numel(self) -> int:
        return self.c * (self.hw[0] * self.hw[1] if self.hw else 1)

    @property
    def is_spatial(self) -> bool:
        return self.hw is not None


@dataclass
class LayerPlan:
    """A spec bound to concrete input/output shapes and padding."""
    index: int
    spec: LayerSpec
    in_shape: TensorShape
    out_shape: TensorShape
    pads: Tuple[int, int, int, int] = (0, 0, 0, 0)   # top, bottom, left, right
    params: Dict[str, Tuple[int, ...]] = field(default_factory=dict)

    @property
    def name(self) -> str:
        return f"layers.{self.index}"


@dataclass
class NetPlan:
    layers: List[LayerPlan]
    head_in: int
    num_classes: int = NUM_CLASSES

    def param_shapes(self, dense_last: bool = False) -> Dict[str, Tuple[int, ...]]:
        """Named parameter shapes in flat-buffer order: DSL order, head last — or, with
        ``dense_last``, every non-dense parameter and the head first and the dense layers
        after them (the "lowrank" DP strategy all-reduces exactly that leading range)."""
        out: Dict[str, Tuple[int, ...]] = {}
        dense: Dict[str, Tuple[int, ...]] = {}
        for lp in self.layers:
            for k, s in lp.params.items():
                (dense if dense_last and isinstance(lp.spec, DenseSpec) else out)[f"{lp.name}.{k}"] = s
        out["head.weight"] = (self.head_in, self.num_classes)
        out["head.bias"] = (self.num_classes,)
        out.update(dense)
        return out

    def num_params(self) -> int:
        return sum(math.prod(s) for s in self.param_shapes().values())

    def flops_per_sample(self) -> int:
        """Forward multiply-add FLOPs (2/MAC) per sample for the matmul-like layers."""
        f = 0
        for lp in self.layers:
            sp = lp.spec
            if isinstance(sp, ConvSpec):
                oh, ow = lp.out_shape.hw
                f += 2 * oh * ow * sp.cout * sp.kh * sp.kw * lp.in_shape.c
            elif isinstance(sp, DepthwiseConvSpec):
                oh, ow = lp.out_shape.hw
                f += 2 * oh * ow * lp.out_shape.c * sp.kh * sp.kw
            elif isinstance(sp, DenseSpec):
                f += 2 * lp.in_shape.numel * sp.hidden
        f += 2 * self.head_in * self.num_classes
        return f


def plan_network(layers: Sequence[LayerSpec], in_hw: int = INPUT_HW, in_c: int = INPUT_C,
                 num_classes: int = NUM_CLASSES) -> NetPlan:
    """Shape inference (replaces TF's graph-build-time shape checks)."""
    shape = TensorShape(in_c, (in_hw, in_hw))
    plans: List[LayerPlan] = []
    for i, sp in enumerate(layers):
        if isinstance(sp, ConvSpec):
            if not shape.is_spatial:
                raise ConfigError(f"layer {i}: conv after a connect layer (input is flat)")
            (h, w), (sh, sw) = shape.hw, sp.stride
            if sp.padding == "SAME":
                oh, pt, pb = same_pads(h, sp.kh, sh)
                ow, pl, pr = same_pads(w, sp.kw, sw)
            else:
                oh, ow, pt, pb, pl, pr = valid_out(h, sp.kh, sh), valid_out(w, sp.kw, sw), 0, 0, 0, 0
            if oh <= 0 or ow <= 0:
                raise ConfigError(f"layer {i}: conv kernel larger than its {h}x{w} input")
            params = {"weight": (sp.kh, sp.kw, shape.c, sp.cout)}
            if sp.bias:
                params["bias"] = (sp.cout,)
            out = TensorShape(sp.cout, (oh, ow))
            plans.append(LayerPlan(i, sp, shape, out, (pt, pb, pl, pr), params))
        elif isinstance(sp, DepthwiseConvSpec):
            if not shape.is_spatial:
                raise ConfigError(f"layer {i}: depthwise after a connect layer (input is flat)")
            (h, w), (sh, sw) = shape.hw, sp.stride
            if sp.padding == "SAME":
                oh, pt, pb = same_pads(h, sp.kh, sh)
                ow, pl, pr = same_pads(w, sp.kw, sw)
            else:
                oh, ow, pt, pb, pl, pr = valid_out(h, sp.kh, sh), valid_out(w, sp.kw, sw), 0, 0, 0, 0
            if oh <= 0 or ow <= 0:
                raise ConfigError(f"layer {i}: depthwise kernel larger than its {h}x{w} input")
            cm = shape.c * sp.mult
            params = {"weight": (sp.kh, sp.kw, shape.c, sp.mult)}
            if sp.bias:
                params["bias"] = (cm,)
            plans.append(LayerPlan(i, sp, shape, TensorShape(cm, (oh, ow)), (pt, pb, pl, pr), params))
        elif isinstance(sp, (PoolSpec, AvgPoolSpec)):
            if not shape.is_spatial:
                raise ConfigError(f"layer {i}: pool after a connect layer (input is flat)")
            if sp.kernel == GLOBAL:
                sp = replace(sp, kernel=tuple(shape.hw), stride=tuple(shape.hw))
            (h, w), (kh, kw), (sh, sw) = shape.hw, sp.kernel, sp.stride
            if sp.padding == "SAME":
                oh, pt, pb = same_pads(h, kh, sh)
                ow, pl, pr = same_pads(w, kw, sw)
            else:
                oh, ow, pt, pb, pl, pr = valid_out(h, kh, sh), valid_out(w, kw, sw), 0, 0, 0, 0
            if oh <= 0 or ow <= 0:
                raise ConfigError(f"layer {i}: pool window larger than its {h}x{w} input")
            plans.append(LayerPlan(i, sp, shape, TensorShape(shape.c, (oh, ow)), (pt, pb, pl, pr)))
        elif isinstance(sp, (ActSpec, DropoutSpec)):
            plans.append(LayerPlan(i, sp, shape, shape))
        elif isinstance(sp, LrnSpec):
            if not shape.is_spatial:
                raise ConfigError(f"layer {i}: lrn after a connect layer (input is flat)")
            plans.append(LayerPlan(i, sp, shape, shape))
        elif isinstance(sp, NormSpec):
            plans.append(LayerPlan(i, sp, shape, shape, params={"scale": (shape.c,), "offset": (shape.c,)}))
        elif isinstance(sp, GroupNormSpec):
            # (after a connect the input is [B, F]: C means F, the parameters are per feature)
            if sp.mode == "instance" and not shape.is_spatial:
                raise ConfigError(f"layer {i}: instance norm after a connect layer (every group would be "
                                  f"one element)")
            G = {"layer": 1, "instance": shape.c}.get(sp.mode, sp.groups)
            if not isinstance(G, int) or isinstance(G, bool) or G < 1:
                raise ConfigError(f"layer {i}: norm mode {sp.mode!r} needs groups, a whole number >= 1")
            if shape.c % G:
                raise ConfigError(f"layer {i}: norm groups {G} does not divide its {shape.c} channels")
            sp = replace(sp, groups=G)
            plans.append(LayerPlan(i, sp, shape, shape, params={"scale": (shape.c,), "offset": (shape.c,)}))
        elif isinstance(sp, DenseSpec):
            fan_in = shape.numel
            out = TensorShape(sp.hidden, None)
            plans.append(LayerPlan(i, sp, shape, out,
                                   params={"weight": (fan_in, sp.hidden), "bias": (sp.hidden,)}))
        else:  # pragma: no cover
            raise ConfigError(f"layer {i}: unsupported spec {sp!r}")
        shape = plans[-1].out_shape
    return NetPlan(plans, shape.numel, num_classes)


@dataclass(frozen=True)
class LrSchedule:
    """``options.lr_schedule``: the step's rate as a function of the step counter
    (ops/lr_schedule.py is the definition of the arithmetic)."""
    type: str = "constant"
    decay_steps: int = 1                   # S
    decay_rate: float = 1.0                # r
    staircase: bool = False                # floor the step ratio (exponential, inverse_time)
    alpha: float = 0.0                     # cosine: floor, as a fraction of the base rate
    warmup_steps: int = 0                  # W: linear warm-up on top of any type


_LR_SCHEDULE_KEYS = ("type", "decay_steps", "decay_rate", "staircase", "alpha", "warmup_steps")


def _as_bool(v: Any, name: str) -> bool:
    if isinstance(v, bool):
        return v
    if isinstance(v, (int, float)) and v in (0, 1):
        return bool(v)
    if isinstance(v, str) and v.strip().lower() in ("true", "false", "1", "0", "yes", "no"):
        return v.strip().lower() in ("true", "1", "yes")
    raise ConfigError(f"{name}: expected bool, got {v!r}")


def _as_whole(v: Any, name: str) -> int:
    """An int, or a string / float that holds one (``"3"``, ``3.0``): never a truncation."""
    if isinstance(v, bool):
        raise ConfigError(f"{name}: expected int, got {v!r}")
    f = _as_float(v, name)
    if not math.isfinite(f) or f != int(f):
        raise ConfigError(f"{name}: expected int, got {v!r}")
    return int(f)


def parse_lr_schedule(d: Any) -> LrSchedule:
    """``options.lr_schedule`` -> LrSchedule (numbers may be strings)."""
    where = "options.lr_schedule"
    if not isinstance(d, dict):
        raise ConfigError(f"{where} must be an object")
    unknown = sorted(set(d) - set(_LR_SCHEDULE_KEYS))
    if unknown:
        raise ConfigError(f"{where}: unknown key(s) {unknown}; valid: {list(_LR_SCHEDULE_KEYS)}")
    kind = d.get("type", "constant")
    if kind not in LR_SCHEDULES:
        raise ConfigError(f"{where}.type must be one of {LR_SCHEDULES}")
    S, r = 1, 1.0
    if kind != "constant" or "decay_steps" in d:
        if "decay_steps" not in d:
            raise ConfigError(f"{where}: {kind} needs decay_steps")
        S = _as_whole(d["decay_steps"], where + ".decay_steps")
        if not (1 <= S < 2 ** 31):
            raise ConfigError(f"{where}.decay_steps must be >= 1")
    if kind in ("exponential", "inverse_time") or "decay_rate" in d:
        if "decay_rate" not in d:
            raise ConfigError(f"{where}: {kind} needs decay_rate")
        r = _as_float(d["decay_rate"], where + ".decay_rate")
        if not math.isfinite(r) or r < 0 or (kind == "exponential" and not (0.0 < r <= 1.0)):
            raise ConfigError(f"{where}.decay_rate must be in (0, 1] for exponential, >= 0 for inverse_time")
    alpha = _as_float(d.get("alpha", 0.0), where + ".alpha")
    if not (0.0 <= alpha <= 1.0):
        raise ConfigError(f"{where}.alpha must be in [0, 1]")
    W = _as_whole(d.get("warmup_steps", 0), where + ".warmup_steps")
    if not (0 <= W < 2 ** 31):
        raise ConfigError(f"{where}.warmup_steps must be >= 0")
    return LrSchedule(kind, S, r, _as_bool(d.get("staircase", False), where + ".staircase"), alpha, W)


@dataclass(frozen=True)
class Augment:
    """``options.augment``: random warps of the training images, redrawn every step from
    (seed, step, dataset row) (ops/augment_ref.py is the definition of the arithmetic)."""
    shift: int = 0                         # s: dx, dy uniform integers in [-s, s] pixels
    rotate: int = 0                        # R: angle a uniform integer of degrees in [-R, R]
    scale: int = 0                         # P: zoom (100 + q) / 100, q uniform integer in [-P, P]
    erase_prob: float = 0.0                # probability that one rectangle becomes ``fill``
    erase_max: int = 8                     # E: rectangle height and width uniform in [1, E]
    fill: int = 0                          # pixels sampled outside the image, erased pixels


_AUGMENT_KEYS = ("shift", "rotate", "scale", "erase_prob", "erase_max", "fill")
_AUGMENT_INT_RANGES = {"shift": (0, 8, 0), "rotate": (0, 45, 0), "scale": (0, 30, 0), "erase_max": (1, 14, 8),
                       "fill": (0, 255, 0)}


def parse_augment(d: Any) -> Augment:
    """``options.augment`` -> Augment (numbers may be strings).  Every amount zero is the
    option absent: the default ``Augment()``."""
    where = "options.augment"
    if not isinstance(d, dict):
        raise ConfigError(f"{where} must be an object")
    unknown = sorted(set(d) - set(_AUGMENT_KEYS))
    if unknown:
        raise ConfigError(f"{where}: unknown key(s) {unknown}; valid: {list(_AUGMENT_KEYS)}")
    vals: Dict[str, Any] = {}
    for key, (lo, hi, default) in _AUGMENT_INT_RANGES.items():
        v = _as_whole(d.get(key, default), f"{where}.{key}")
        if not (lo <= v <= hi):
            raise ConfigError(f"{where}.{key} must be in {lo}..{hi}")
        vals[key] = v
    if isinstance(d.get("erase_prob", 0.0), bool):
        raise ConfigError(f"{where}.erase_prob: expected float, got {d['erase_prob']!r}")
    p = _as_float(d.get("erase_prob", 0.0), where + ".erase_prob")
    if not (0.0 <= p <= 1.0):                       # (a NaN fails both compares)
        raise ConfigError(f"{where}.erase_prob must be in [0, 1]")
    aug = Augment(erase_prob=p, **vals)
    if not (aug.shift or aug.rotate or aug.scale or aug.erase_prob > 0.0):
        return Augment()
    return aug


@dataclass
class TrainConfig:
    """The whole ``model.json`` (API.md:306-332) in typed form."""
    iter: int = 1000
    learning_rate: float = 0.01
    ratio: float = 0.8
    loss_name: str = "entropy"
    optimizer_name: str = "GradientDescentOptimizer"
    net_type: str = "CNN"
    layers: List[LayerSpec] = field(default_factory=list)
    raw: Dict[str, Any] = field(default_factory=dict)
    # --- new-framework knobs (not in the reference JSON; all optional) ---
    batch_size: int = 50                   # construct_distribute.py:403 hard-codes 50
    log_every: int = 100                   # :405 — accuracy line every 100 global steps
    ckpt_every: int = 0                    # optional step-based checkpoints (0 = off)
    ckpt_secs: float = 60.0                # Supervisor(save_model_secs=60) (:391)
    bn_mode: str = "running"               # "batch" = reference quirk 3
    compat_adagrad: bool = False           # True = reference quirk 1 (Adagrad 1e-4)
    sync_bn: bool = False                  # DP: BatchNorm statistics over the GLOBAL batch
    seed: int = 0
    eval_every: int = 0                    # held-out validation sweep every k steps (0 = off)
    eval_batch: int = 256                  # rows per validation batch
    lr_schedule: LrSchedule = LrSchedule()  # decay / warm-up of the rate by the step counter
    augment: Augment = Augment()           # training-time augmentation (all zero: none)

    @property
    def effective_optimizer(self) -> str:
        return "AdagradOptimizer" if self.compat_adagrad else self.optimizer_name

    @property
    def effective_lr(self) -> float:
        return 1e-4 if self.compat_adagrad else self.learning_rate

    def plan(self) -> NetPlan:
        return plan_network(self.layers)

    def to_json(self) -> Dict[str, Any]:
        return dict(self.raw)


def parse_train_config(cfg: Union[str, bytes, Dict[str, Any]]) -> TrainConfig:
    """Parse the reference JSON verbatim (numbers may be strings, cf. cmd.py:63-69)."""
    if isinstance(cfg, (str, bytes)):
        try:
            cfg = json.loads(cfg)
        except json.JSONDecodeError as e:
            raise ConfigError(f"config is not valid JSON: {e}")
    if not isinstance(cfg, dict):
        raise ConfigError("config must be a JSON object")
    net = cfg.get("net_config")
    if not isinstance(net, dict) or not isinstance(net.get("middle_layer", []), list):
        raise ConfigError("net_config.middle_layer must be a list")
    layers = []
    for i, d in enumerate(net.get("middle_layer", [])):
        sp = parse_layer(d, i)
        if sp is not None:
            layers.append(sp)
    loss = str(cfg.get("loss_name", "entropy"))
    if loss not in LOSSES:
        raise ConfigError(f"loss_name must be one of {LOSSES}")
    opt = str(cfg.get("optimizer_name", "GradientDescentOptimizer"))
    if opt not in OPTIMIZERS:
        # reference: anything that is not GD falls back to Adagrad (construct_distribute.py:308-311)
        opt = "AdagradOptimizer"
    ext = cfg.get("options", {}) if isinstance(cfg.get("options", {}), dict) else {}
    tc = TrainConfig(
        iter=_as_int(cfg.get("iter", 1000), "iter"),
        learning_rate=_as_float(cfg.get("learning_rate", 0.01), "learning_rate"),
        ratio=_as_float(cfg.get("ratio", 0.8), "ratio"),
        loss_name=loss, optimizer_name=opt,
        net_type=str(cfg.get("net_type", "CNN")),
        layers=layers, raw=dict(cfg),
        batch_size=_as_int(ext.get("batch_size", 50), "batch_size"),
        log_every=_as_int(ext.get("log_every", 100), "log_every"),
        ckpt_every=_as_int(ext.get("ckpt_every", 0), "ckpt_every"),
        ckpt_secs=_as_float(ext.get("ckpt_secs", 60.0), "ckpt_secs"),
        bn_mode=str(ext.get("bn_mode", "running")),
        compat_adagrad=bool(ext.get("compat_adagrad", False)),
        sync_bn=str(ext.get("sync_bn", False)).lower() in ("1", "true", "yes"),
        seed=_as_int(ext.get("seed", 0), "seed"),
        eval_every=_as_int(ext.get("eval_every", 0), "eval_every"),
        eval_batch=_as_int(ext.get("eval_batch", 256), "eval_batch"),
        lr_schedule=parse_lr_schedule(ext["lr_schedule"]) if "lr_schedule" in ext else LrSchedule(),
        augment=parse_augment(ext["augment"]) if "augment" in ext else Augment(),
    )
    if tc.compat_adagrad and tc.lr_schedule.type != "constant":
        # the flag means "the reference's fixed Adagrad 1e-4"
        raise ConfigError("options.lr_schedule: compat_adagrad fixes the rate (only type 'constant' goes with it)")
    if tc.eval_every < 0:
        raise ConfigError("eval_every must be >= 0")
    if tc.eval_batch <= 0:
        raise ConfigError("eval_batch must be > 0")
    if tc.iter < 0:
        raise ConfigError("iter must be >= 0")
    if not (0.0 < tc.ratio <= 1.0):
        raise ConfigError("ratio must be in (0, 1]")
    if tc.learning_rate <= 0:
        raise ConfigError("learning_rate must be > 0")
    if tc.batch_size <= 0:
        raise ConfigError("batch_size must be > 0")
    if tc.bn_mode not in ("running", "batch"):
        raise ConfigError("bn_mode must be 'running' or 'batch'")
    tc.plan()  # shape-check now
    return tc


# The canonical sample config: API.md:306-332 (== a.sh:8 == cmd.py:89-93).
SAMPLE_CONFIG: Dict[str, Any] = {
    "iter": 1000,
    "learning_rate": 0.01,
    "ratio": 0.8,
    "loss_name": "entropy",
    "optimizer_name": "GradientDescentOptimizer",
    "net_type": "CNN",
    "net_config": {
        "middle_layer": [
            {"layer": "conv", "filter": [2, 2, 10]},
            {"layer": "conv", "filter": [2, 2, 20]},
            {"layer": "pool"},
            {"layer": "norm"},
            {"layer": "active"},
            {"layer": "connect"},
            {"layer": "connect"},
        ],
        "output_layer": {},
    },
}


def spec_to_dict(sp: LayerSpec) -> Dict[str, Any]:
    return asdict(sp)
