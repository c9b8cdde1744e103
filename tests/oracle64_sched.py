"""The fp64 shadow oracle under a learning-rate schedule (helper module: no tests).

``oracle64`` computes every step at the constant base rate.  Here the step's rate is the
float64 form of the schedule (``ops.lr_schedule.lr_f64``) at the step's 1-based t, and every
comparison — the parameter steps and the tolerances' slope terms — is taken at that rate.
"""
from __future__ import annotations

import copy
import math
from types import SimpleNamespace
from typing import List

import torch

import oracle64 as X

from cloud_server_amd.models.cnn import build_model
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config
from cloud_server_amd.ops import lr_schedule as L

# the sample layer list with 128-wide dense layers (the horizontally fused program needs
# multiples of 128)
SAMPLE128 = [dict(l, hidden=128) if l.get("layer") == "connect" else dict(l)
             for l in SAMPLE_CONFIG["net_config"]["middle_layer"]]

STAIR_HALF = {"type": "exponential", "decay_steps": 1, "decay_rate": 0.5, "staircase": True}
COSINE_WARM = {"type": "cosine", "decay_steps": 4, "warmup_steps": 2}


def make_cfg(layers, optimizer, lr, schedule=None, batch=50, **options):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c["optimizer_name"] = optimizer
    c["learning_rate"] = lr
    c["options"] = dict(batch_size=batch, **options)
    if schedule is not None:
        c["options"]["lr_schedule"] = dict(schedule)
    return parse_train_config(c)


def lr64(cfg, t: int) -> float:
    """The step's rate in float64 from the config alone (not from the engine)."""
    return float(L.lr_f64(cfg.lr_schedule, cfg.effective_lr, t))


class SchedOracle64(X.Oracle64):
    def __init__(self, cfg, ds, decisions: bool = True, dense_last: bool = False):
        """``dense_last``: the flat layout of the "lowrank" data-parallel strategy."""
        super().__init__(cfg, ds, decisions)
        if dense_last:
            self.model = build_model(cfg, "cpu", dense_last=True).train().double()

    def step(self, s: int, st: X.State) -> X.StepRef:
        self.lr = lr64(self.cfg, s + 1)
        return super().step(s, st)


def run_trajectory(eng, oracle: SchedOracle64, steps: int, network: str = "sample", label: str = "",
                   start: int = 0, **check_kw) -> None:
    """``steps`` engine steps from step ``start``, each shadowed by the oracle and checked at
    ``oracle64.tolerances`` taken at that step's lr_t."""
    for s in range(start, start + steps):
        pre = X.read_state(eng)
        assert pre.dstep == s, (pre.dstep, s)
        ref = oracle.step(s, pre)
        eng.step()
        post = X.read_state(eng)
        assert post.dstep == s + 1, (post.dstep, s)
        assert math.isfinite(ref.loss) and bool(torch.isfinite(ref.flat).all())
        lr_t = lr64(eng.cfg, s + 1)
        view = SimpleNamespace(model=eng.model, opt_id=eng.opt_id, lr=lr_t, ring_loss=eng.ring_loss,
                               ring_correct=eng.ring_correct)
        recs: List[X.Record] = X.compare_step(view, s, pre, post, ref, eng.cfg.batch_size)
        # (check numbers its steps from 1: one list per call keeps the step in the label)
        X.check([recs], X.tolerances(network, lr_t), f"{label} t={s + 1} lr_t={lr_t:.3e}", **check_kw)
