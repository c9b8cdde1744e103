"""Shadow oracle: one training step in fp64 on the CPU, from the engine's own state.

Before every step the caller reads the engine's state (``read_state``: flat parameters,
optimizer slots, BN running statistics); ``Oracle64.step`` computes that ONE step in fp64
from exactly those values; after the step ``compare_step`` compares what the engine did
with what the oracle did.  Every step starts from bit-identical values, so errors do not
compound and state carried from one step to the next (accumulators that must be cleared,
slot pointers, step counters, running statistics) is checked at every step against
something that is not another program of the same engine.

A plain helper module (no tests, no fixtures): ``test_oracle64_cpu`` pins it to the eager
engine on the CPU, ``test_hip_trajectory`` uses it against the HIP program.
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import torch.nn.functional as F

from cloud_server_amd.models.cnn import build_model, loss_fn
from cloud_server_amd.models.dsl import ActSpec, PoolSpec, SAMPLE_CONFIG, parse_train_config
from cloud_server_amd.ops import optim_ref as O

MARGIN = 1e-4        # a sample whose fp64 top-2 logit margin is below this may flip in fp32
# A ReLU pre-activation or a max-pool top-2 gap below this fraction of the layer's largest
# input may fall the other way in fp32: 4 x the worst difference between the fp32 eager
# forward and the fp64 forward at the inputs of these layers, relative to the layer's range,
# over the 21 networks (2.41e-6, dense_norm_head; BatchNorm layers dominate).
DECISION_MARGIN = 9.6e-6


# Tolerances (rtol, atol): err <= rtol * max|ref over the tensor| + atol * max|ref over all
# tensors|.  Each is 4 x the worst error of fp32 eager on the MI355X against this oracle over
# the whole grid (profiles/r7_trajectory_parity.md; scripts/trajectory_parity.py measures
# them), rtol capped at 2e-2 — one dropped row of a 50-row batch (the two Adagrad rtols
# measured 2.01e-2 and 2.09e-2).  ``loss`` and ``bn`` are plain relative errors.
TOL = {
    "loss": (1.06e-6, 0.0),
    "bn": (4.70e-6, 0.0),
    "gd.dw": (1.81e-2, 2.27e-4),
    "adagrad.dacc": (2.0e-2, 2.89e-4),
    "adagrad.dw": (2.0e-2, 3.24e-3),
    "adam.dm": (1.17e-2, 5.87e-4),
    "adam.dv": (6.38e-3, 2.89e-4),
    "adam.dw_self": (1.64e-3, 2.78e-4),
    "adadelta.dacc": (3.22e-5, 1.22e-5),
    "adadelta.dw": (1.60e-3, 4.41e-3),
    "adadelta.dup_self": (1.06e-3, 1.06e-3),
}
# The GD / Adagrad parameter steps are also held to test_step_matches_torch's own bound on
# the gradient, |g - g_ref| <= 2e-3 * max|g_ref over the tensor| + 1e-5 * max|g_ref| + 1e-6,
# carried to the step through the update's largest slope (lr for GD; lr / sqrt(0.1) for
# Adagrad, whose accumulator starts at 0.1 and only grows): a third, absolute term.  The
# three networks below keep the grid-wide bound: fp32 eager itself exceeds the tighter one
# there (1.07, 2.41, 1.07 times: profiles/r7_trajectory_parity.md).
STEP_TEST_DW = (2e-3, 1e-5)
STEP_TEST_G_ABS = 1e-6
DW_GRID_ONLY = {"wide_c1", "deep20", "wide_conv_chain"}


def tolerances(network: str, lr: float = 0.01):
    """The tolerance table of one network's cases: quantity -> (rtol, atol[, absolute])."""
    tol = dict(TOL)
    if network not in DW_GRID_ONLY:
        slope = {"gd.dw": lr, "adagrad.dw": lr / math.sqrt(O.ADAGRAD_INIT)}
        for q in ("gd.dw", "adagrad.dw"):
            tol[q] = (min(TOL[q][0], STEP_TEST_DW[0]), min(TOL[q][1], STEP_TEST_DW[1]), STEP_TEST_G_ABS * slope[q])
    return tol


def make_cfg(layers, optimizer="AdagradOptimizer", lr=0.01, loss="entropy", batch=50):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = layers
    c["optimizer_name"] = optimizer
    c["learning_rate"] = lr
    c["loss_name"] = loss
    c["options"] = dict(batch_size=batch)
    return parse_train_config(c)


# the two networks the step tests do not have -------------------------------------------
# conv pair -> pool -> FOUR 128-wide dense layers: at B = 50 every dense forward is
# split-K, so the pair forward's zero list would need 4 outputs + the tail tickets
DENSE4_SPLIT = [
    {"layer": "conv", "filter": [2, 2, 10]},
    {"layer": "conv", "filter": [2, 2, 20]},
    {"layer": "pool"},
    {"layer": "connect", "hidden": 128},
    {"layer": "active", "active_func": "relu"},
    {"layer": "connect", "hidden": 128},
    {"layer": "connect", "hidden": 128},
    {"layer": "active", "active_func": "sigmoid"},
    {"layer": "connect", "hidden": 128},
]


def norm_chain(blocks: int) -> list:
    """conv 3x3x4, norm, relu, pool, then ``blocks`` x (connect 32, norm, relu): every norm
    brings two statistic accumulators that must start each step at zero."""
    layers = [{"layer": "conv", "filter": [3, 3, 4]}, {"layer": "norm"},
              {"layer": "active", "active_func": "relu"}, {"layer": "pool"}]
    for _ in range(blocks):
        layers += [{"layer": "connect", "hidden": 32}, {"layer": "norm"},
                   {"layer": "active", "active_func": "relu"}]
    return layers


# five blocks (6 norms) give the HIP program 13 zero regions, six give 15; SEVEN blocks (8
# norms, 25 layers) give 17: the optimizer's 16-entry zero list plus one early fill launch.
# (The case keeps the name the tests were specified with; the network has 8 norms, not 9.)
NINE_NORMS = norm_chain(7)

LRS = {"GradientDescentOptimizer": 0.01, "AdagradOptimizer": 0.01, "AdamOptimizer": 1e-3,
       "AdadeltaOptimizer": 1.0}
SHORT = {"GradientDescentOptimizer": "gd", "AdagradOptimizer": "adagrad", "AdamOptimizer": "adam",
         "AdadeltaOptimizer": "adadelta"}
REPRESENTATIVES = ("sample", "dense3_act", "deep20", "wide_conv_192", "five_biased_convs", "dense_only")


def networks(cases: Dict[str, list]) -> Dict[str, list]:
    """The step tests' networks plus the two above."""
    return dict(cases, dense4_split=DENSE4_SPLIT, nine_norms=NINE_NORMS)


def grid(cases: Dict[str, list]) -> List[Tuple[str, str, str, int, bool]]:
    """(network, optimizer, loss, batch, use_graph) of every trajectory case."""
    nets = networks(cases)
    g = [(n, o, "entropy", 50, False) for n in nets for o in ("AdagradOptimizer", "AdamOptimizer")]
    g += [(n, o, "entropy", 50, False) for n in REPRESENTATIVES
          for o in ("GradientDescentOptimizer", "AdadeltaOptimizer")]
    g += [(n, "AdagradOptimizer", "mse", 50, False) for n in REPRESENTATIVES]
    g += [("sample", "AdagradOptimizer", "entropy", b, False) for b in (1, 7, 64)]
    g += [(n, "AdagradOptimizer", "entropy", 50, True) for n in ("sample", "dense3_act", "dense4_split")]
    return g


def case_id(c) -> str:
    n, o, loss, b, graph = c
    return f"{n}-{SHORT[o]}-{loss}-b{b}" + ("-graph" if graph else "")


# ---------------------------------------------------------------------------------------
@dataclass
class State:
    flat: torch.Tensor                 # fp64, CPU
    slots: torch.Tensor                # fp64 [n_slots, numel]
    buffers: Dict[str, torch.Tensor]   # fp64
    dstep: int


def read_state(eng) -> State:
    """The engine's carried state, landed and copied to the host in fp64."""
    eng.flush_params()
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    return State(eng.flat.detach().double().cpu().clone(), eng.slots.detach().double().cpu().clone(),
                 {k: b.detach().double().cpu().clone() for k, b in eng.model.named_buffers()},
                 int(eng.dstep.item()))


@dataclass
class StepRef:
    flat: torch.Tensor
    slots: torch.Tensor
    grad: torch.Tensor
    loss: float
    correct: int
    margins: torch.Tensor              # per sample: top-1 minus top-2 logit
    buffers: Dict[str, torch.Tensor]
    allow: torch.Tensor                # per element: gradient change borderline decisions can cause
    borderline: int                    # number of borderline ReLU / max-pool decisions


class Oracle64:
    def __init__(self, cfg, ds, decisions: bool = True):
        """``decisions=False``: no borderline-decision allowances (every comparison exact)."""
        self.cfg = cfg
        self.decisions = decisions
        self.model = build_model(cfg, "cpu").train().double()
        assert self.model.flat.dtype == torch.float64
        self.images = torch.from_numpy(np.ascontiguousarray(ds.images)).double() / 255.0
        self.labels = torch.from_numpy(np.ascontiguousarray(ds.labels)).long()
        self.n = len(ds)
        self.opt_id = O.OPT_IDS[cfg.effective_optimizer]
        self.lr = cfg.effective_lr
        self._rng = np.random.default_rng(cfg.seed)
        self._seq = np.zeros(0, np.int64)

    def batch_indices(self, s: int) -> np.ndarray:
        """Step ``s`` consumes positions [s*B, (s+1)*B) of the concatenated per-epoch
        permutations of ``default_rng(seed)`` (the definition, not BatchStream's code)."""
        B = self.cfg.batch_size
        while len(self._seq) < (s + 1) * B:
            self._seq = np.concatenate([self._seq, self._rng.permutation(self.n)])
        return self._seq[s * B:(s + 1) * B]

    def _forward_traced(self, x: torch.Tensor):
        """The model's forward, layer by layer, keeping every discrete decision: for a
        ReLU / leaky ReLU its pre-activation, for a max-pool window the gap between its two
        largest values.  Returns (logits, [(decision values, layer output, slope change)])."""
        m = self.model
        B = x.shape[0]
        h = x.reshape(B, 28, 28, 1)
        decisions = []
        for lp in m.plan.layers:
            sp = lp.spec
            z = h
            h = m._layer(lp, h, True)
            if isinstance(sp, ActSpec) and sp.func in ("relu", "leaky_relu"):
                alpha = 0.0 if sp.func == "relu" else float(sp.alpha)
                if alpha != 1.0 and z.requires_grad:
                    decisions.append((z, h, abs(1.0 - alpha)))
            elif isinstance(sp, PoolSpec) and sp.kernel[0] * sp.kernel[1] > 1 and z.requires_grad:
                pt, pb, pl, pr = lp.pads
                t = z.permute(0, 3, 1, 2)
                if any(lp.pads):
                    t = F.pad(t, (pl, pr, pt, pb), value=float("-inf"))
                Bn, Cn = t.shape[:2]
                cols = F.unfold(t, tuple(sp.kernel), stride=tuple(sp.stride)).view(Bn, Cn, sp.kernel[0] * sp.kernel[1], -1)
                top = cols.topk(2, dim=2).values
                gap = (top[:, :, 0] - top[:, :, 1]).view(Bn, Cn, h.shape[1], h.shape[2]).permute(0, 2, 3, 1)
                decisions.append((gap, h, 1.0))
        if h.dim() != 2:
            h = h.reshape(B, -1)
        return h @ m.p("head.weight") + m.p("head.bias"), decisions

    def step(self, s: int, st: State) -> StepRef:
        m = self.model
        with torch.no_grad():
            m.flat.copy_(st.flat)
            for k, b in m.named_buffers():
                b.copy_(st.buffers[k])
        idx = torch.from_numpy(self.batch_indices(s))
        x, y = self.images[idx], self.labels[idx]
        logits, decisions = self._forward_traced(x)
        if not self.decisions:
            decisions = []
        loss = loss_fn(self.cfg.loss_name, logits, y)
        grads = torch.autograd.grad(loss, [m.flat] + [d[1] for d in decisions], retain_graph=bool(decisions))
        g = grads[0]
        # Borderline decisions: a ReLU whose pre-activation, or a max-pool window whose top-2
        # gap, is below DECISION_MARGIN of the layer's range may fall the other way in fp32 (as a
        # logit margin below MARGIN may flip the correct count).  Flipping decision e moves
        # the gradient, to first order, by (slope change) * dL/dy_e * d(decision e)/d(params):
        # the sum of the magnitudes over the borderline decisions is what a gradient
        # comparison must allow, element by element.  Exact ties (identical operands in any
        # precision) are decided by the same index rule everywhere and are not counted.
        allow = torch.zeros_like(g)
        n_border = 0
        for (d, _, w), gy in zip(decisions, grads[1:]):
            dd = d.detach()
            fin = torch.isfinite(dd)
            scale = dd[fin].abs().max().item() if bool(fin.any()) else 0.0
            sel = fin & (dd.abs() < DECISION_MARGIN * scale) & (dd.abs() > 1e-12 * scale) & (gy != 0)
            for e in sel.nonzero().tolist():
                e = tuple(e)
                (dz,) = torch.autograd.grad(d[e], m.flat, retain_graph=True)
                allow += (w * abs(gy[e].item())) * dz.abs()
                n_border += 1
        w, sl = st.flat.clone(), st.slots.clone()
        O.step_ref(self.opt_id, w, g, sl, self.lr, s + 1)
        lg = logits.detach()
        if lg.shape[1] > 1:
            top = lg.topk(2, dim=1).values
            margins = top[:, 0] - top[:, 1]
        else:
            margins = torch.full((lg.shape[0],), float("inf"), dtype=torch.float64)
        return StepRef(w, sl, g.detach(), float(loss.item()), int((lg.argmax(1) == y).sum().item()), margins,
                       {k: b.detach().clone() for k, b in m.named_buffers()}, allow, n_border)


# ---------------------------------------------------------------------------------------
@dataclass
class Record:
    quantity: str
    tensor: str
    err: float          # max |engine - reference| over the tensor
    tmax: float         # max |reference| over the tensor
    gmax: float         # max |reference| over all tensors of the quantity

    @property
    def rel_tensor(self) -> Optional[float]:
        """Relative to the tensor; only tensors that are not ~1000x below the largest."""
        return self.err / self.tmax if self.tmax >= 1e-3 * self.gmax and self.tmax > 0 else None

    @property
    def rel_global(self) -> float:
        return self.err / self.gmax if self.gmax > 0 else (0.0 if self.err == 0 else float("inf"))


def _per_tensor(quantity, state, got, ref, allow=None) -> List[Record]:
    """``allow``: per element, what borderline decisions may move the reference by (taken off
    the error before the tensor's maximum; inf excludes an element)."""
    gmax = max(state.view(k, ref).abs().max().item() for k in state.shapes)
    err = (got - ref).abs()
    if allow is not None:
        err = (err - allow).clamp_min(0.0)
    return [Record(quantity, k, state.view(k, err).max().item(), state.view(k, ref).abs().max().item(), gmax)
            for k in state.shapes]


def compare_step(eng, s: int, pre: State, post: State, ref: StepRef, steps_batch: int) -> List[Record]:
    """Every comparison of one step as records; ``loss``/``bn`` records hold the relative
    error in ``err`` with ``tmax = gmax = 1``; the ``correct`` record holds the count
    difference in ``err`` and the number of borderline samples in ``tmax``."""
    state, opt, lr = eng.model.state, eng.opt_id, eng.lr
    recs: List[Record] = []
    loss = float(eng.ring_loss[s].item())
    recs.append(Record("loss", "loss", abs(loss - ref.loss) / max(abs(ref.loss), 1e-30), 1.0, 1.0))
    correct = int(eng.ring_correct[s].item())
    recs.append(Record("correct", "correct", float(abs(correct - ref.correct)),
                       float((ref.margins < MARGIN).sum().item()), float(steps_batch)))
    for k, b in ref.buffers.items():
        scale = b.abs().max().item()
        recs.append(Record("bn", k, (post.buffers[k] - b).abs().max().item() / scale, 1.0, 1.0))
    dw = post.flat - pre.flat
    dsl = post.slots - pre.slots
    dsl_ref = ref.slots - pre.slots
    name = {O.OPT_SGD: "gd", O.OPT_ADAGRAD: "adagrad", O.OPT_ADAM: "adam", O.OPT_ADADELTA: "adadelta"}[opt]
    # what the borderline decisions of this step may do to each quantity: a (gradient) through
    # the quantity's own formula, g^2 terms as 2|g|a + a^2, parameter steps through the
    # update's slope at this element
    a, g = ref.allow, ref.grad.abs()
    a2 = 2 * g * a + a * a
    if opt == O.OPT_ADAGRAD:
        recs += _per_tensor("adagrad.dacc", state, dsl[0], dsl_ref[0], a2)
    elif opt == O.OPT_ADAM:
        recs += _per_tensor("adam.dm", state, dsl[0], dsl_ref[0], (1 - O.ADAM_B1) * a)
        recs += _per_tensor("adam.dv", state, dsl[1], dsl_ref[1], (1 - O.ADAM_B2) * a2)
    elif opt == O.OPT_ADADELTA:
        recs += _per_tensor("adadelta.dacc", state, dsl[0], dsl_ref[0], (1 - O.ADADELTA_RHO) * a2)
    if opt == O.OPT_SGD:
        recs += _per_tensor("gd.dw", state, dw, ref.flat - pre.flat, lr * a)
    elif opt == O.OPT_ADAGRAD:
        # d/dg [g / sqrt(acc + g^2)] <= 1 / sqrt(acc)
        recs += _per_tensor("adagrad.dw", state, dw, ref.flat - pre.flat, lr * a / pre.slots[0].sqrt())
    elif opt == O.OPT_ADAM:
        # a gradient that is exactly zero becomes an lr-sized step from fp32 noise, so the
        # parameter step is checked against the engine's OWN new slots and step counter
        want = -O.adam_lr_t(lr, s + 1) * post.slots[0] / (post.slots[1].sqrt() + O.ADAM_EPS)
        recs += _per_tensor("adam.dw_self", state, dw, want)
    else:
        eps, rho = O.ADADELTA_EPS, O.ADADELTA_RHO
        factor = lr * (pre.slots[1] + eps).sqrt() / (post.slots[0] + eps).sqrt()
        # Adadelta, like Adam, gives every element a step of the same size whatever its
        # gradient's: where the gradient is zero in exact arithmetic (fp64 leaves < 1e-12 of
        # the largest; a bias ahead of a BatchNorm) the step is the fp32 noise of a sum that
        # cancels and is not compared with the oracle; its g^2 stays under adadelta.dacc and
        # its step under adadelta.dup_self
        al = factor * a
        al[g <= 1e-12 * g.max()] = float("inf")
        recs += _per_tensor("adadelta.dw", state, dw, -factor * ref.grad, al)
        up = rho * pre.slots[1] + (1 - rho) * (dw / lr) ** 2
        recs += _per_tensor("adadelta.dup_self", state, dsl[1], up - pre.slots[1])
    return recs


def run_trajectory(eng, oracle: Oracle64, steps: int = 3) -> List[List[Record]]:
    """``steps`` engine steps, each shadowed by the oracle; one record list per step."""
    out = []
    for s in range(steps):
        pre = read_state(eng)
        assert pre.dstep == s, (pre.dstep, s)
        ref = oracle.step(s, pre)
        eng.step()
        post = read_state(eng)
        assert post.dstep == s + 1, (post.dstep, s)
        assert math.isfinite(ref.loss) and bool(torch.isfinite(ref.flat).all())
        out.append(compare_step(eng, s, pre, post, ref, eng.cfg.batch_size))
    return out


def worst(records_by_step: List[List[Record]]) -> Dict[str, Tuple[float, float]]:
    """Per quantity: (worst error relative to the tensor, worst relative to the global max)."""
    w: Dict[str, Tuple[float, float]] = {}
    for recs in records_by_step:
        for r in recs:
            if r.quantity == "correct":
                continue
            a, b = w.get(r.quantity, (0.0, 0.0))
            rt = r.rel_tensor
            w[r.quantity] = (max(a, rt) if rt is not None else a, max(b, r.rel_global))
    return w


def check(records_by_step: List[List[Record]], tol, label: str = "", max_borderline: Optional[int] = None) -> None:
    """``tol``: quantity -> (rtol, atol[, absolute]); err <= rtol * max|ref over the tensor| +
    atol * max|ref over all tensors| (+ absolute).  Prints every step's worst figures before it asserts.
    ``max_borderline``: also bound the number of borderline samples per step."""
    bad = []
    for s, recs in enumerate(records_by_step):
        for r in recs:
            if r.quantity == "correct":
                # the counts may differ by no more than the number of borderline samples
                if r.err > r.tmax or (max_borderline is not None and r.tmax > max_borderline):
                    bad.append(f"step {s + 1} correct: differs by {r.err:.0f}, {r.tmax:.0f} borderline samples")
                continue
            rtol, atol, *rest = tol[r.quantity]
            bound = rtol * r.tmax + atol * r.gmax + (rest[0] if rest else 0.0)
            if not r.err <= bound:
                bad.append(f"step {s + 1} {r.quantity} {r.tensor}: err {r.err:.3e} > {bound:.3e} "
                           f"(tensor max {r.tmax:.3e}, global max {r.gmax:.3e})")
        print(f"{label} step {s + 1}: " + ", ".join(f"{q} {a:.1e}/{b:.1e}" for q, (a, b) in worst([recs]).items()))
    assert not bad, f"{label}: " + "; ".join(bad[:12]) + (f" (+{len(bad) - 12} more)" if len(bad) > 12 else "")
