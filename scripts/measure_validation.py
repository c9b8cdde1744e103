"""Held-out validation measurements (profiles/validation_notes.md).

    python scripts/measure_validation.py [--out DIR]      sweep time and training cost
    python scripts/measure_validation.py --trace          six sweeps only, for a kernel trace:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sweep -- \
            python scripts/measure_validation.py --trace

1. Sweep time: 10,000 synthetic rows, eval_batch 256, fused mode (the sample net, head input
   512) and logits mode (conv-conv-pool net, head input 3920).  Per sweep, after one warm
   sweep: total = issue -> result on the host (median of 7), host-blocked = the issue call
   alone.  Baseline: ``TrainEngine.evaluate`` (the eager path, which blocks throughout) on
   the same engine and rows (median of 5 after one warm call).
2. Training cost with the feature on: ms/step of a 2000-step job loop (steps 200..2000
   timed, device synchronised at both ends) with eval_every in {0, 500, 100} on a 2,000-row
   test set, twice each.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cloud_server_amd.data.datasets import synthetic_mnist  # noqa: E402
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config  # noqa: E402
from cloud_server_amd.runtime.engine import TrainEngine  # noqa: E402
from cloud_server_amd.runtime.trainer import JobRun  # noqa: E402

DEV = "cuda:0"
CONV_POOL = [{"layer": "conv", "filter": [2, 2, 10]}, {"layer": "conv", "filter": [2, 2, 20]}, {"layer": "pool"}]


def cfg(layers=None, iters=2000, **options):
    c = copy.deepcopy(SAMPLE_CONFIG)
    if layers is not None:
        c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c.update(iter=iters, optimizer_name="AdagradOptimizer", learning_rate=1e-4)
    c["options"] = dict(batch_size=50, log_every=100, ckpt_every=0, ckpt_secs=0, **options)
    return c


def engine(layers, steps):
    eng = TrainEngine(parse_train_config(cfg(layers)), synthetic_mnist(2000, seed=1), device=DEV, backend="hip")
    assert eng.backend == "hip", eng.fallback_reason
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    return eng


def trace_sweeps():
    eng = engine(None, 0)
    val = eng.validator(synthetic_mnist(10000, seed=5), 256)
    for _ in range(6):
        val.issue()
        r = val.wait()[1]
    torch.cuda.synchronize()
    print("sweeps done", r.n, r.accuracy)


def sweep_time(out):
    test = synthetic_mnist(10000, seed=5)
    for name, layers in (("fused_sample", None), ("logits_conv_pool", CONV_POOL)):
        eng = engine(layers, 50)
        val = eng.validator(test, 256)
        row = {"validator": type(val).__name__, "fused": bool(getattr(val, "fused", False)),
               "Kh": getattr(val, "Kh", None)}
        tot, blk = [], []
        for i in range(8):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val.issue()
            t1 = time.perf_counter()
            r = val.wait()[1]
            t2 = time.perf_counter()
            if i:
                tot.append((t2 - t0) * 1e3)
                blk.append((t1 - t0) * 1e3)
        row.update(hip_total_ms=statistics.median(tot), hip_host_issue_ms=statistics.median(blk), hip_all_total=tot,
                   accuracy=r.accuracy, loss=r.loss)
        ev = []
        for i in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = eng.evaluate(test)
            torch.cuda.synchronize()
            if i:
                ev.append((time.perf_counter() - t0) * 1e3)
        row.update(evaluate_total_ms=statistics.median(ev), evaluate_all=ev, evaluate_accuracy=acc)
        out[name] = row
        print(name, json.dumps(row), flush=True)
        del val, eng


def training_cost(out):
    data = synthetic_mnist(10000, seed=0).split(0.8)
    for k in (0, 500, 100, 0, 500, 100):
        with tempfile.TemporaryDirectory() as mdir:
            job = JobRun(mdir, cfg(None, 2000, eval_every=k), device=DEV, backend="hip", data=data)
            t0 = None
            while job.pending():
                if t0 is None and job.eng.host_step >= 200:
                    torch.cuda.synchronize()
                    t0, s0 = time.perf_counter(), job.eng.host_step
                job.before_step()
                job.step()
                if job.after_step():
                    break
            torch.cuda.synchronize()
            n = job.eng.host_step - s0
            ms = (time.perf_counter() - t0) * 1e3 / n
            res = job.finish()
            nrows = sum(1 for _ in open(os.path.join(mdir, "validation.jsonl"))) if k else 0
            out.setdefault("train_ms_per_step", {}).setdefault(str(k), []).append(ms)
            print(f"eval_every={k}: {ms:.5f} ms/step over {n} steps, {nrows} validation rows, "
                  f"final_accuracy {res['final_accuracy']:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true", help="six sweeps only (run under a kernel tracer)")
    ap.add_argument("--out", default=".", help="directory for validation_measurements.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measurements need the GPU"
    if a.trace:
        trace_sweeps()
        return
    out = {}
    sweep_time(out)
    training_cost(out)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "validation_measurements.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
