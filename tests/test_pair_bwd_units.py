"""The MFMA pair backward after round 9, against the fp64 shadow oracle (GPU only).

Round 9 changed the second half of the pair workgroup: the dwB + dc1 tiles run from one
balanced unit list, and a bias gradient comes from a spare M row of its GEMM fed 1.0 (or is
not computed at all without a bias; the column-sum loop remains for a bias whose GEMM has no
spare row).  Every path is run here for three steps, each step recomputed in fp64 from the
engine's own state (``oracle64``), with the c1-reuse body and with the recompute body
(``CSA_PAIR_C1=0``); each case asserts the bias path it is meant to hit
(``csa_conv_pair_bwd_bias_mode``).  Batch 3, eager, unless stated.

  network          bias A    bias B    what it checks
  sample           none      none      the dead path (also at batch 1)
  pair_relu_valid  GEMM row  GEMM row  act A's derivative is applied before the A sum
  leaky_alpha      GEMM row  none      one live bias, one absent
  bias_b_loop      GEMM row  loop      KB = 32: conv B's GEMM has no spare row
  bias_a_loop      loop      none      KA = 16: conv A's GEMM has no spare row
  pair_nopool      none      none      two rows per band: the unit plan on another shape

What is asserted: every quantity ``oracle64.check`` holds except the loss.  The loss of a
step is the work of the forward and head launches from the engine's own state, none of which
this change touches; its bound (``oracle64.TOL``: relative 1.06e-6) was measured at batch 50
(batch 1, 7, 64 for the sample only), where the batch mean averages the per-sample rounding.
At batch 3 pair_relu_valid showed 3.0e-7, 3.6e-7 and 1.2e-6 in the three steps of one run.
The loss is printed for every case; ``test_hip_trajectory`` holds it at the batch sizes of
its bound.

Run-to-run noise (``test_two_engines_agree``): the stripes are filled by cross-workgroup
atomics, so two engines differ by fp32 summation order.  Figure: after 3 GradientDescent
steps of pair_relu_valid at batch 3, the largest |w_1 - w_2| of a parameter tensor relative
to that tensor's largest total step.  Two engines on the PARENT's kernels, 8 pairs, on an
MI355X: see PARENT_NOISE below (profiles/r9_notes.md); the bound is 4 x it.
"""
import functools
import os

import pytest
import torch

import oracle64 as X
from test_hip_step import CASES

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.ops import fused as FK
from cloud_server_amd.runtime.engine import TrainEngine

pytestmark = pytest.mark.gpu

NONE, ROW, LOOP = 0, 1, 2

NETS = dict(
    {k: CASES[k] for k in ("sample", "pair_relu_valid", "leaky_alpha", "pair_nopool")},
    bias_b_loop=[
        {"layer": "conv", "filter": [2, 2, 8], "isBias": "True"},
        {"layer": "conv", "filter": [2, 2, 8], "isBias": "True"},
        {"layer": "pool"},
        {"layer": "connect", "hidden": 16},
    ],
    bias_a_loop=[
        {"layer": "conv", "filter": [4, 4, 8], "isBias": "True"},
        {"layer": "active", "active_func": "relu"},
        {"layer": "conv", "filter": [2, 2, 8]},
        {"layer": "connect", "hidden": 16},
    ],
)
MODES = {"sample": (NONE, NONE), "pair_relu_valid": (ROW, ROW), "leaky_alpha": (ROW, NONE),
         "bias_b_loop": (ROW, LOOP), "bias_a_loop": (LOOP, NONE), "pair_nopool": (NONE, NONE)}
OPTS = ("GradientDescentOptimizer", "AdagradOptimizer")
RUNS = [(n, 3) for n in NETS] + [("sample", 1)]

# Largest run-to-run figure (see above) of two engines on the parent's kernels, MI355X.
# 8 pairs: 1.216e-05 x4, 1.005e-05 x3, 2.432e-05 (this change, 8 pairs: at most 1.216e-05)
PARENT_NOISE = 2.432e-05


@functools.lru_cache(maxsize=None)
def _ds():
    return synthetic_mnist(400, seed=3)


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.prev = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _engine(cfg, c1="1", graph=False):
    with _env(CSA_PAIR_C1=c1, CSA_DETERMINISTIC="0"):
        eng = TrainEngine(cfg, _ds(), device="cuda", backend="hip", use_graph=graph)
    assert eng.backend == "hip", eng.fallback_reason
    assert eng.program.pair is not None, "the leading convs did not lower to the fused pair"
    return eng


def _bias_mode(eng):
    p = eng.program
    ua, ub = p.units[0], p.units[1]
    m = int(p.lib.csa_conv_pair_bwd_bias_mode(FK.ints(p.pair), 1 if ua.layer.spec.bias else 0,
                                              1 if ub.layer.spec.bias else 0))
    assert m >= 0
    return m & 15, m >> 4


@pytest.mark.parametrize("c1", ["1", "0"], ids=["c1reuse", "recompute"])
@pytest.mark.parametrize("opt", OPTS, ids=[X.SHORT[o] for o in OPTS])
@pytest.mark.parametrize("name,batch", RUNS, ids=[f"{n}-b{b}" for n, b in RUNS])
def test_three_steps_match_fp64_oracle(name, batch, opt, c1):
    cfg = X.make_cfg(NETS[name], opt, X.LRS[opt], "entropy", batch)
    eng = _engine(cfg, c1)
    assert _bias_mode(eng) == MODES[name], f"{name}: bias paths {_bias_mode(eng)}"
    if c1 == "0":
        assert eng.program.pair_c1 is None
    label = f"{name}-{X.SHORT[opt]}-b{batch}-c1={c1}"
    recs = X.run_trajectory(eng, X.Oracle64(cfg, _ds()), 3)
    torch.cuda.synchronize()
    assert all(int(w.item()) == 0 for w in eng.health_words())
    # the gradients (parameter steps, optimizer slots), the BN statistics and the correct count
    # are asserted; the loss is printed only (module docstring)
    print(f"{label} loss: " + " ".join(f"{r.err:.1e}" for step in recs for r in step if r.quantity == "loss"))
    X.check([[r for r in step if r.quantity != "loss"] for step in recs], X.tolerances(name, X.LRS[opt]), label)


def test_graph_replay_of_a_biased_pair_matches_eager():
    """20 graph-replayed steps of pair_relu_valid (both biases from GEMM rows) against the
    same network eager: test_graph_replay_matches_eager's bound."""
    cfg = X.make_cfg(NETS["pair_relu_valid"], "AdagradOptimizer", 0.01, "entropy", 3)
    a, b = _engine(cfg, graph=True), _engine(cfg, graph=False)
    assert _bias_mode(a) == (ROW, ROW)
    for _ in range(20):
        a.step()
        b.step()
    torch.cuda.synchronize()
    d = (a.flat - b.flat).abs().max().item()
    print(f"graph vs eager, 20 steps: max |dw| {d:.3e}")
    assert d < 3e-3
    assert a.host_step == b.host_step == 20
    assert int(a.dstep.item()) == 20


def pair_noise():
    """The run-to-run figure of the module docstring, of two fresh engines."""
    cfg = X.make_cfg(NETS["pair_relu_valid"], "GradientDescentOptimizer", 0.01, "entropy", 3)
    e = [_engine(cfg), _engine(cfg)]
    w0 = e[0].flat.clone()
    assert torch.equal(w0, e[1].flat)
    for _ in range(3):
        for x in e:
            x.step()
    torch.cuda.synchronize()
    worst = 0.0
    st = e[0].model.state
    for k in st.shapes:
        a, b, z = st.view(k, e[0].flat), st.view(k, e[1].flat), st.view(k, w0)
        step = (a - z).abs().max().item()
        if step > 0:
            worst = max(worst, (a - b).abs().max().item() / step)
    return worst


def test_two_engines_agree():
    """CSA_DETERMINISTIC=0: two fresh engines of pair_relu_valid agree within 4 x the
    atomic-order noise two engines on the parent's kernels show."""
    got = pair_noise()
    print(f"two engines: {got:.3e} (parent {PARENT_NOISE:.3e}, bound {4 * PARENT_NOISE:.3e})")
    assert got <= 4 * PARENT_NOISE
