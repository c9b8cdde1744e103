#!/usr/bin/env python
"""What ``options.augment`` costs in the training step: ms/step of the sample config with and
without the option on one GPU, timed like bench.py (graph-captured steps through
``TrainEngine.run_steps``, 32-step graphs).

* ``plain``    the sample config, B = 50, Adagrad 1e-4 (the bench's setting)
* ``augment``  the same with ``augment = {shift 2, rotate 10, scale 10, erase_prob 0.25}``

    python scripts/augment_cost.py [--steps 2000] [--warmup 200] [--rounds 3]

Prints one JSON line per (round, config) and a closing line of medians.  Under
``rocprofv3 --kernel-trace --stats -- python scripts/augment_cost.py --only augment --rounds 1``
the trace's ``augment_kernel`` row is the launch's own time."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AUGMENT = {"shift": 2, "rotate": 10, "scale": 10, "erase_prob": 0.25}


def _time(aug, args) -> dict:
    from cloud_server_amd.data.datasets import synthetic_mnist
    from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config
    from cloud_server_amd.runtime.engine import TrainEngine
    c = copy.deepcopy(SAMPLE_CONFIG)
    c.update(optimizer_name="AdagradOptimizer", learning_rate=1e-4, options={"batch_size": 50})
    if aug:
        c["options"]["augment"] = AUGMENT
    eng = TrainEngine(parse_train_config(c), synthetic_mnist(60000, seed=0), device="cuda:0", backend="hip",
                      use_graph=True)
    assert eng.backend == "hip", eng.fallback_reason
    assert (eng.program.aug_img is not None) == bool(aug)
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
    return {"ms_per_step": round(dt * 1e3 / args.steps, 5), "hfuse": bool(p.hfuse), "tail": bool(p.tail),
            "staged": bool(p.staged), "graph_steps": eng.group_steps(),
            "loss": round(eng.metrics_since(eng.host_step - 100)["loss"], 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["plain", "augment"], default=None)
    args = ap.parse_args()
    names = [args.only] if args.only else ["plain", "augment"]
    seen = {k: [] for k in names}
    for r in range(args.rounds):            # alternating: drift hits both configs alike
        for name in names:
            out = _time(name == "augment", args)
            seen[name].append(out["ms_per_step"])
            print(json.dumps(dict(round=r, config=name, **out)), flush=True)
    print(json.dumps({"median_ms_per_step": {k: statistics.median(v) for k, v in seen.items()},
                      "steps": args.steps, "warmup": args.warmup}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
