#!/usr/bin/env python
"""What the local-response-normalisation launches cost (one GPU).

1. ``kernels``: ``csa_lrn_fwd`` and ``csa_lrn_bwd`` in both forced forms (1: a thread per
   element or per four channels walking its window in global memory, 2: a row loaded once,
   window sums from cross-lane moves or an LDS row) over a grid of channel counts and radii:
   the table the form threshold (``csa_lrn_row_taps``) is chosen from.  Each is timed as a
   captured graph of ``--chain`` back-to-back launches replayed ``--replays`` times (device
   events), so the figure is the launch's time on the device, launch gap included; the
   variants alternate inside every round.
2. ``step``: ms/step of the sample config and of the sample with an ``lrn`` after the pool
   (the pair, an lrn unit and -- the norm having lost its conv producer -- a standalone bn
   unit).  Timed like bench.py (graph-captured steps through ``TrainEngine.run_steps``),
   alternating.

    python scripts/lrn_cost.py [--rounds 3] [--chain 50] [--replays 40] [--steps 2000] [--warmup 200]

Prints one JSON line per measurement and a closing line of medians."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (rows, C): the sample's pooled map, the CIFAR-10 tutorial's shapes at 28 x 28 input, the widest
# direct conv and the gconv range
SHAPES = {
    "50x14x14x20": (50 * 14 * 14, 20),
    "50x14x14x8": (50 * 14 * 14, 8),
    "50x14x14x16": (50 * 14 * 14, 16),
    "50x28x28x20": (50 * 28 * 28, 20),
    "50x14x14x32": (50 * 14 * 14, 32),
    "50x7x7x48": (50 * 7 * 7, 48),
    "50x7x7x64": (50 * 7 * 7, 64),
    "50x7x7x128": (50 * 7 * 7, 128),
    "50x7x7x160": (50 * 7 * 7, 160),
}
RADII = (0, 1, 2, 4, 5, 9, 14, 19, 32, 63)


def _variants(rows, C, r, beta):
    """name -> a callable that enqueues one launch on the current stream."""
    import torch
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    gi = K.ints([rows, C, r])
    x = torch.randn(rows, C, device="cuda:0")
    dy = torch.randn(rows, C, device="cuda:0")
    y, s, dx = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    consts = (1.0, 1e-2, beta)
    assert lib.csa_lrn_fwd(K.ptr(x), K.ptr(y), K.ptr(s), gi, *consts, 0, K.stream()) == 0     # s for the backward
    keep = (x, dy, y, s, dx, gi)

    def chk(rc):
        assert rc == 0, rc

    out = {}
    for form in (1, 2):
        out[f"fwd_form{form}"] = (lambda f=form: chk(lib.csa_lrn_fwd(K.ptr(x), K.ptr(y), K.ptr(s), gi, *consts, f,
                                                                      K.stream())))
        out[f"bwd_form{form}"] = (lambda f=form: chk(lib.csa_lrn_bwd(K.ptr(x), K.ptr(s), K.ptr(dy), K.ptr(dx), gi,
                                                                      *consts, f, K.stream())))
    return out, keep


def _graph(fn, chain):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()                                  # (warm: the code object is loaded before the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(chain):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def _time_graph(g, replays, chain) -> float:
    """microseconds per launch"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (replays * chain)


def kernels(args) -> dict:
    med = {}
    for sname, (rows, C) in SHAPES.items():
        for r in RADII:
            if r > 0 and min(r, C - 1) == min(RADII[RADII.index(r) - 1], C - 1):
                continue                        # the same clipped window as the radius before
            for beta in args.betas:
                key = f"{sname} r{r} b{beta:g}"
                variants, keep = _variants(rows, C, r, beta)
                graphs = {k: _graph(fn, args.chain) for k, fn in variants.items()}
                seen = {k: [] for k in graphs}
                for rnd in range(args.rounds):      # alternating: drift hits every variant alike
                    for k, gr in graphs.items():
                        us = _time_graph(gr, args.replays, args.chain)
                        seen[k].append(us)
                        print(json.dumps({"what": "kernel", "shape": sname, "r": r, "beta": beta, "variant": k,
                                          "round": rnd, "us_per_launch": round(us, 3)}), flush=True)
                med[key] = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3),
                                "max_us": round(max(v), 3)} for k, v in seen.items()}
                del graphs, keep
    return med


def _time_step(layers, args) -> dict:
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
            "pair": p.pair is not None, "hfuse": bool(p.hfuse), "tail": bool(p.tail),
            "loss": round(eng.metrics_since(eng.host_step - 100)["loss"], 4)}


def steps(args) -> dict:
    from cloud_server_amd.models.dsl import SAMPLE_CONFIG
    base = SAMPLE_CONFIG["net_config"]["middle_layer"]
    lrn = copy.deepcopy(base)
    lrn.insert(3, {"layer": "lrn"})
    nets = {"sample": base, "lrn_sample": lrn}
    seen = {k: [] for k in nets}
    for r in range(args.rounds):
        for name, layers in nets.items():
            out = _time_step(layers, args)
            seen[name].append(out["ms_per_step"])
            print(json.dumps(dict(what="step", round=r, net=name, **out)), flush=True)
    return {k: statistics.median(v) for k, v in seen.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chain", type=int, default=50)
    ap.add_argument("--replays", type=int, default=40)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--betas", type=float, nargs="+", default=[0.5, 0.6])
    ap.add_argument("--only", choices=("kernels", "step"), default=None)
    args = ap.parse_args()
    out = {}
    if args.only in (None, "kernels"):
        out["kernels_us_per_launch"] = kernels(args)
    if args.only in (None, "step"):
        out["median_ms_per_step"] = steps(args)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
