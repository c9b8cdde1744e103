"""Three HIP training steps, each against the fp64 shadow oracle (GPU only).

``test_hip_step`` takes one step from freshly zeroed buffers, or compares one HIP program
with another.  Here every step of a 3-step run starts from the engine's own state and is
recomputed in fp64 on the CPU (``oracle64``): parameters, optimizer slots, BN running
statistics, loss and correct count are compared after EVERY step, so an accumulator that
is not cleared, a slot pointer off for one layout or an update applied twice shows at step
2 (what step 1 left behind) or step 3 (what step 2's own clearing left behind), through
every in-kernel update path: tail workgroups, head epilogue, deferred dense segments, flat
optimizer.  Tolerances: ``oracle64.TOL`` (4 x fp32 eager's own error against the oracle).

A ReLU pre-activation or a max-pool top-2 gap inside fp32 forward noise can fall the other
way than in fp64 and move the gradients upstream of it by percent (seen on the MI355X:
``deep20`` x Adadelta, step 3, one mask of layers.6 in about half of the runs, 4.0e-2 of the
upstream tensors' steps).  The oracle lists these borderline decisions and what each can do
to every gradient element (``oracle64.DECISION_MARGIN``); the comparisons allow exactly that
much, element by element, and nothing else.  Under Adadelta an exactly-zero gradient's step
is not compared with the oracle (as under Adam); its slots are.

Measured on an MI355X: profiles/r7_trajectory_parity.md.
"""
import pytest
import torch

import oracle64 as X
from test_hip_step import CASES

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.runtime.engine import TrainEngine

pytestmark = pytest.mark.gpu

STEPS = 3
NETS = X.networks(CASES)

# which program each network lowered to on the MI355X: (fused, hfuse, tail, conv pair)
PINNED = {
    "sample": (True, True, True, True),
    "dense3_act": (True, True, True, True),
    "deep20": (True, True, False, True),
    "wide_conv_192": (True, False, False, False),
    "five_biased_convs": (True, False, False, False),
    "dense_only": (True, False, False, False),
    # four split-K dense outputs + the tail tickets do not fit the pair forward's zero
    # list: horizontal fusion with the optimizer launch
    "dense4_split": (True, True, False, True),
    "nine_norms": (True, False, False, False),
}


@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


@pytest.mark.parametrize("case", X.grid(CASES), ids=X.case_id)
def test_trajectory_matches_fp64_oracle(case, dataset):
    name, opt, loss, batch, graph = case
    cfg = X.make_cfg(NETS[name], opt, X.LRS[opt], loss, batch)
    eng = TrainEngine(cfg, dataset, device="cuda", backend="hip", use_graph=graph)
    assert eng.backend == "hip", eng.fallback_reason
    p = eng.program
    if name in PINNED:
        got = (bool(p.fused), bool(p.hfuse), bool(p.tail), p.pair is not None)
        assert got == PINNED[name], f"{name} lowered to (fused, hfuse, tail, pair) = {got}"
    if p.tail:
        assert len(p.fwd_zero) <= p.FWD_ZERO_MAX
    if name == "nine_norms":
        # more accumulators than the optimizer's 16-entry zero list: early fill launches
        assert len(p.zero_regions) >= 16 and len(p.zero_early) > 0
    recs = X.run_trajectory(eng, X.Oracle64(cfg, dataset), STEPS)
    torch.cuda.synchronize()
    assert all(int(w.item()) == 0 for w in eng.health_words())
    X.check(recs, X.tolerances(name, X.LRS[opt]), X.case_id(case))
