#!/usr/bin/env python
"""What a dropout layer costs in the training step: ms/step of three networks on one GPU,
timed like bench.py (graph-captured steps through ``TrainEngine.run_steps``).

* ``drop``   the sample's layers with ``active relu, dropout 0.5`` between the two connects
* ``nodrop`` the same network without the dropout layer (the activation is then a consumer
             transform of the second dense layer, which leaves the fused path)
* ``sample`` the plain sample config

    python scripts/dropout_cost.py [--steps 2000] [--warmup 200] [--rounds 3]

Prints one JSON line per (round, network) and a closing line of medians."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _nets():
    from cloud_server_amd.models.dsl import SAMPLE_CONFIG
    base = SAMPLE_CONFIG["net_config"]["middle_layer"]
    relu, drop = {"layer": "active", "active_func": "relu"}, {"layer": "dropout", "keep_prob": 0.5}
    return {"drop": base[:6] + [relu, drop] + base[6:],
            "nodrop": base[:6] + [relu] + base[6:],
            "sample": list(base)}


def _time(layers, args) -> dict:
    from cloud_server_amd.data.datasets import synthetic_mnist
    from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config
    from cloud_server_amd.runtime.engine import TrainEngine
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c.update(optimizer_name="AdagradOptimizer", learning_rate=1e-4, options={"batch_size": 50})
    eng = TrainEngine(parse_train_config(c), synthetic_mnist(60000, seed=0), device="cuda:0", backend="hip",
                      use_graph=True)
    assert eng.backend == "hip", eng.fallback_reason
    eng.step()
    eng.prepare_group_graph()
    eng.run_steps(max(args.warmup - 1, 0))
    eng.sync_device()
    t0 = time.perf_counter()
    eng.run_steps(args.steps)
    eng.sync_device()
    dt = time.perf_counter() - t0
    eng.check_health()
    p = eng.program
    return {"ms_per_step": round(dt * 1e3 / args.steps, 5), "units": [u.kind for u in p.units],
            "hfuse": bool(p.hfuse), "tail": bool(p.tail),
            "dense_fused": [bool(u.fused) for u in p.units if u.kind == "dense"],
            "loss": round(eng.metrics_since(eng.host_step - 100)["loss"], 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    nets = _nets()
    seen = {k: [] for k in nets}
    for r in range(args.rounds):            # alternating: drift hits every network alike
        for name, layers in nets.items():
            out = _time(layers, args)
            seen[name].append(out["ms_per_step"])
            print(json.dumps(dict(round=r, net=name, **out)), flush=True)
    print(json.dumps({"median_ms_per_step": {k: statistics.median(v) for k, v in seen.items()},
                      "steps": args.steps, "warmup": args.warmup}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
