#!/usr/bin/env python
"""What the average-pool launches cost (one GPU).

1. ``kernels``: ``csa_avgpool_fwd`` in both forced forms (1: a thread per output element,
   2: a wave per output position), ``csa_avgpool_bwd``, and ``csa_maxpool_fwd`` where its
   window index fits, on the geometries the form threshold is chosen from.  Each is timed as
   a captured graph of ``--chain`` back-to-back launches replayed ``--replays`` times (device
   events), so the figure is the launch's time on the device, launch gap included; the
   variants alternate inside every round.
2. ``step``: ms/step of the sample config, of the sample with ``mode: avg`` (the pair in its
   no-pool form, a pool unit and -- the norm having lost its conv producer -- a standalone bn
   unit), and of that network with an identity average pool (1 x 1 / 1) behind the first:
   the same lowering plus exactly one more pool unit, i.e. two more launches.  Timed like
   bench.py (graph-captured steps through ``TrainEngine.run_steps``), alternating.

    python scripts/avgpool_cost.py [--rounds 3] [--chain 50] [--replays 40] [--steps 2000] [--warmup 200]

Prints one JSON line per measurement and a closing line of medians."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (B, H, W, C, kh, kw, sh, sw, padding)
GEOMS = {
    "28x28x20 2x2/2": (50, 28, 28, 20, 2, 2, 2, 2, "SAME"),
    "14x14x20 3x3/2": (50, 14, 14, 20, 3, 3, 2, 2, "SAME"),
    "14x14x20 global": (50, 14, 14, 20, 14, 14, 14, 14, "VALID"),
    "28x28x1 global": (50, 28, 28, 1, 28, 28, 28, 28, "VALID"),
    # between 9 and 196 positions: where the threshold goes
    "14x14x20 4x4/2": (50, 14, 14, 20, 4, 4, 2, 2, "SAME"),
    "14x14x20 5x5/2": (50, 14, 14, 20, 5, 5, 2, 2, "SAME"),
    "14x14x20 6x6/2": (50, 14, 14, 20, 6, 6, 2, 2, "SAME"),
    "14x14x20 7x7/7": (50, 14, 14, 20, 7, 7, 7, 7, "VALID"),
}


def _geom(g):
    from cloud_server_amd.models.dsl import same_pads, valid_out
    B, H, W, C, kh, kw, sh, sw, pad = g
    if pad == "SAME":
        (oh, pt, _), (ow, pl, _) = same_pads(H, kh, sh), same_pads(W, kw, sw)
    else:
        oh, ow, pt, pl = valid_out(H, kh, sh), valid_out(W, kw, sw), 0, 0
    return [B, H, W, C, kh, kw, sh, sw, pt, pl, oh, ow]


def _variants(g):
    """name -> a callable that enqueues one launch on the current stream."""
    import torch
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    v = _geom(g)
    B, H, W, C, oh, ow = v[0], v[1], v[2], v[3], v[10], v[11]
    gi = K.ints(v)
    x = torch.randn(B, H, W, C, device="cuda:0")
    y = torch.zeros(B, oh, ow, C, device="cuda:0")
    dy = torch.randn(B, oh, ow, C, device="cuda:0")
    dx = torch.zeros(B, H, W, C, device="cuda:0")
    am = torch.zeros(B, oh, ow, C, device="cuda:0", dtype=torch.uint8)
    keep = (x, y, dy, dx, am, gi)

    def chk(rc):
        assert rc == 0, rc

    out = {
        "avg_fwd_form1": lambda: chk(lib.csa_avgpool_fwd(K.ptr(x), K.ptr(y), gi, 1, K.stream())),
        "avg_fwd_form2": lambda: chk(lib.csa_avgpool_fwd(K.ptr(x), K.ptr(y), gi, 2, K.stream())),
        "avg_bwd": lambda: chk(lib.csa_avgpool_bwd(K.ptr(dy), K.ptr(dx), gi, K.stream())),
    }
    if lib.csa_maxpool_ok(gi) == 1:
        out["max_fwd"] = lambda: chk(lib.csa_maxpool_fwd(K.ptr(x), K.ptr(y), K.ptr(am), gi, K.stream()))
        out["max_bwd"] = lambda: chk(lib.csa_maxpool_bwd(K.ptr(dy), K.ptr(am), K.ptr(dx), gi, K.stream()))
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
    for gname, g in GEOMS.items():
        variants, keep = _variants(g)
        graphs = {k: _graph(fn, args.chain) for k, fn in variants.items()}
        seen = {k: [] for k in graphs}
        for r in range(args.rounds):            # alternating: drift hits every variant alike
            for k, gr in graphs.items():
                us = _time_graph(gr, args.replays, args.chain)
                seen[k].append(us)
                print(json.dumps({"what": "kernel", "geometry": gname, "variant": k, "round": r,
                                  "us_per_launch": round(us, 3)}), flush=True)
        med[gname] = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3),
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
    avg = copy.deepcopy(base)
    avg[2]["mode"] = "avg"
    ident = avg[:3] + [{"layer": "pool", "mode": "avg", "kernel": [1, 1], "stride": [1, 1]}] + avg[3:]
    nets = {"sample": base, "sample_avg": avg, "sample_avg_plus_identity_pool": ident}
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
