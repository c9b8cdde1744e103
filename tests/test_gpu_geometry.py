"""The conv / pool geometry grid on the HIP program, against the fp64 oracle (GPU only).

The other GPU tests use square 2..5-wide kernels, strides 1 and 2, 2x2/2 and 3x3/2 SAME pools
and at most 48 channels a conv unit.  The kernels carry KH / KW, SH / SW, PT / PL separately
everywhere; ``geometry_nets`` holds small networks over what that leaves out (rect and 1x1
kernels, mixed strides, stride > kernel, VALID and stride-1 and large-window pools, pools with
gaps, 64..128 channels on both sides, rect gconv), and what each must lower to.  Every case is
the ``test_hip_trajectory`` procedure: three steps, each recomputed in fp64 from the engine's
own state (an overlapping or gapped pool relies on ``dc`` being zeroed again every step, a
remainder row on never being written), health words 0, ``oracle64`` tolerances unchanged.

The contract cases (a pool window beyond the kernels' one-byte index, a conv whose weights do
not fit the direct kernels' LDS) must be decided when the engine is built: the HIP program
and right numbers, or the eager program and a reason that names the layer and the limit.
Never an error from a step.

Measured on an MI355X: profiles/geometry_parity.md.
"""
import pytest
import torch

import geometry_nets as G
import oracle64 as X

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.runtime.engine import TrainEngine

pytestmark = pytest.mark.gpu

STEPS = 3
ADAGRAD, ADAM = "AdagradOptimizer", "AdamOptimizer"

# (network, optimizer, loss, batch)
GRID = [(n, ADAGRAD, "entropy", 50) for n in G.MUST_LOWER]
GRID += [(n, ADAM, "entropy", 50) for n in ("pool_shapes", "unit_stride_mixed", "pair_rect_mfma")]
GRID += [(n, ADAGRAD, "mse", 50) for n in ("unit_rect", "gconv_rect")]
GRID += [(n, ADAGRAD, "entropy", 7) for n in ("unit_valid_odd", "pool_shapes")]


def case_id(c) -> str:
    n, o, loss, b = c
    return f"{n}-{X.SHORT[o]}-{loss}-b{b}"


@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


def _trajectory(eng, cfg, dataset, name, lr, label):
    recs = X.run_trajectory(eng, X.Oracle64(cfg, dataset), STEPS)
    torch.cuda.synchronize()
    if eng.backend == "hip":
        assert all(int(w.item()) == 0 for w in eng.health_words())
    X.check(recs, X.tolerances(name, lr), label)


@pytest.mark.parametrize("case", GRID, ids=case_id)
def test_geometry_matches_fp64_oracle(case, dataset):
    name, opt, loss, batch = case
    cfg = X.make_cfg(G.NETS[name], opt, X.LRS[opt], loss, batch)
    eng = TrainEngine(cfg, dataset, device="cuda", backend="hip", use_graph=False)
    assert eng.backend == "hip", eng.fallback_reason
    G.assert_lowering(name, eng.program)
    _trajectory(eng, cfg, dataset, name, X.LRS[opt], case_id(case))


@pytest.mark.parametrize("name", list(G.LOWERING_DET))
def test_geometry_deterministic_mode(name, dataset, monkeypatch):
    """CSA_DETERMINISTIC=1 lowers an overlapping pool to a standalone gather-form unit and
    stripes the conv weight gradients per workgroup — other index paths: against the oracle,
    and two runs bitwise equal."""
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    try:
        cfg = X.make_cfg(G.NETS[name], ADAGRAD, X.LRS[ADAGRAD])
        runs = []
        for _ in range(2):
            eng = TrainEngine(cfg, dataset, device="cuda", backend="hip", use_graph=False)
            assert eng.backend == "hip" and eng.program.det, eng.fallback_reason
            G.assert_lowering(name, eng.program, det=True)
            _trajectory(eng, cfg, dataset, name, X.LRS[ADAGRAD], f"{name}-det")
            eng.sync_device()
            runs.append((eng.flat.clone(), eng.slots.clone()))
        assert torch.equal(runs[0][0], runs[1][0]), "parameters differ between two deterministic runs"
        assert torch.equal(runs[0][1], runs[1][1]), "optimizer slots differ between two deterministic runs"
    finally:
        torch.use_deterministic_algorithms(False)


@pytest.mark.parametrize("name", list(G.CONTRACT))
def test_refused_at_plan_time_or_right(name, dataset):
    cfg = X.make_cfg(G.NETS[name], ADAGRAD, X.LRS[ADAGRAD])
    eng = TrainEngine(cfg, dataset, device="cuda", backend="hip", use_graph=False)
    if eng.backend == "hip":
        G.assert_lowering(name, eng.program)
    else:
        layer, limit = G.CONTRACT[name]
        assert eng.backend == "torch"
        assert layer in eng.fallback_reason and limit in eng.fallback_reason, eng.fallback_reason
        assert name not in G.CONTRACT_LOWERING, eng.fallback_reason
    # (a RuntimeError from a step fails the test; so do numbers outside the tolerances)
    _trajectory(eng, cfg, dataset, name, X.LRS[ADAGRAD], f"{name}-{eng.backend}")
