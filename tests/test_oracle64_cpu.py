"""The fp64 shadow oracle against the eager engine on the CPU (no GPU needed).

Pins the oracle's batch order, optimizer semantics, step counter and BN momentum to the
engine's: the same grid and the same checks as ``test_hip_trajectory``, with fp32 eager in
place of the HIP program, plus one run over a 120-sample dataset whose third step crosses
an epoch boundary of the batch stream.  Eager is held to the bounds WITHOUT the oracle's
allowances for borderline ReLU / max-pool decisions (it needs none on these inputs); one
test checks the allowances themselves.  On these inputs at most one sample per step has an
fp64 top-2 logit margin below 1e-4, which the correct-count check relies on.
"""
import pytest

import oracle64 as X
from test_hip_step import CASES

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.runtime.engine import TrainEngine

NETS = X.networks(CASES)
GRID = [c for c in X.grid(CASES) if not c[4]]       # (graph replay: a GPU matter)


@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


def _run(case, ds, decisions=False):
    name, opt, loss, batch, _ = case
    cfg = X.make_cfg(NETS[name], opt, X.LRS[opt], loss, batch)
    eng = TrainEngine(cfg, ds, device="cpu", backend="torch")
    recs = X.run_trajectory(eng, X.Oracle64(cfg, ds, decisions=decisions), 3)
    X.check(recs, X.tolerances(name, X.LRS[opt]), X.case_id(case), max_borderline=1)


@pytest.mark.parametrize("case", GRID, ids=X.case_id)
def test_oracle_matches_eager_cpu(case, dataset):
    _run(case, dataset)


@pytest.mark.parametrize("opt", ["AdagradOptimizer", "AdamOptimizer"])
def test_oracle_matches_eager_across_epoch_boundary(opt):
    ds = synthetic_mnist(120)
    # 3 x 50 samples of a 120-sample dataset: step 3 takes 20 samples of the first
    # permutation and 30 of the second
    _run(("sample", opt, "entropy", 50, False), ds)


def test_batch_indices_follow_the_definition():
    import numpy as np
    ds = synthetic_mnist(120)
    orc = X.Oracle64(X.make_cfg(NETS["dense_only"]), ds)
    rng = np.random.default_rng(0)
    seq = np.concatenate([rng.permutation(120), rng.permutation(120)])
    for s in range(4):
        assert (orc.batch_indices(s) == seq[s * 50:(s + 1) * 50]).all()
    assert len(set(orc.batch_indices(0).tolist())) == 50


def test_borderline_decisions_bound_a_flipped_relu(dataset):
    """The allowance of a borderline ReLU is the gradient change of flipping it: recompute the
    gradient with one borderline mask forced the other way and compare."""
    import torch
    cfg = X.make_cfg(NETS["deep20"], "GradientDescentOptimizer", 0.01)
    eng = TrainEngine(cfg, dataset, device="cpu", backend="torch")
    orc = X.Oracle64(cfg, dataset)
    ref = orc.step(0, X.read_state(eng))
    assert ref.borderline > 0 and bool((ref.allow >= 0).all()) and bool(torch.isfinite(ref.allow).all())
    assert ref.allow.max().item() < 0.1 * ref.grad.abs().max().item()      # a few decisions, not the net
    # flip every borderline ReLU by nudging its pre-activation across zero
    import cloud_server_amd.models.cnn as cnn
    orig = cnn.act_fwd

    def flipped(x, sp):
        if sp.func in ("relu", "leaky_relu"):
            scale = x.detach().abs().max()
            near = (x.detach().abs() < X.DECISION_MARGIN * scale) & (x.detach() != 0)
            x = torch.where(near, -x, x)
        return orig(x, sp)
    cnn.act_fwd = flipped
    try:
        ref2 = X.Oracle64(cfg, dataset, decisions=False).step(0, X.read_state(eng))
    finally:
        cnn.act_fwd = orig
    moved = (ref2.grad - ref.grad).abs()
    assert moved.max().item() > 0
    # first order in the number of flips (34 at once here: 13 % over at the worst element);
    # the nudge itself moves the forward by 2e-5 of a layer's range: 1e-6 of the gradient
    assert bool((moved <= 1.25 * ref.allow + 1e-6 * ref.grad.abs().max()).all())
