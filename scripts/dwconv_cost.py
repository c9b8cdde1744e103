#!/usr/bin/env python
"""What the depthwise convolution launches cost (one GPU).

1. ``kernels``: ``csa_dw_fwd`` in both forms (1: weights staged in LDS, 2: weights from global
   memory), ``csa_dw_bwd`` in both forms (1: split into a slab, 2: owner) with and without the
   input gradient, and the fold ``csa_dw_bwd_params``: the table the automatic form choice
   (``csa_dw_form`` / ``csa_dw_bwd_form``) rests on.  Each is timed as a captured graph of
   ``--chain`` back-to-back launches replayed ``--replays`` times (device events), so the figure is
   the launch's time on the device, launch gap included; the variants alternate inside every
   round.  With every figure goes the bandwidth it amounts to over the bytes the launch must move
   once (forward x + y; backward x + y + dy + dx).
2. ``emulation``: what a user had before the layer: the same map as a dense ``conv`` with a
   ``[kh, kw, C, C * M]`` weight (a ``conv`` or ``gconv`` unit, as the plan picks).  Two networks
   that differ in that one entry, ``pool conv1x1xC <layer> connect16``, timed like bench.py
   (graph-captured steps through ``TrainEngine.run_steps``), alternating; the difference of the
   two ms/step figures is the difference of the two units.
3. ``step``: ms/step of the sample config and of the sample with a 3x3 ``depthwise`` + 1x1
   ``conv`` in place of its second conv.

    python scripts/dwconv_cost.py [--rounds 3] [--chain 50] [--replays 40] [--steps 2000] [--warmup 200]

Prints one JSON line per measurement and a closing line of medians."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shapes():
    """name -> (B, H, W, C, M, k, s): 50x28x28x{1, 10} and 50x14x14x{20, 64, 128}, M in {1, 2},
    3x3 and 5x5, stride 1 and 2 (SAME)."""
    out = {}
    for H, C in ((28, 1), (28, 10), (14, 20), (14, 64), (14, 128)):
        for M in (1, 2):
            for k in (3, 5):
                for s in (1, 2):
                    out[f"50x{H}x{H}x{C} M{M} {k}x{k} s{s}"] = (50, H, H, C, M, k, s)
    return out


def _geom(shape):
    from cloud_server_amd.models.dsl import same_pads
    B, H, W, C, M, k, s = shape
    oh, pt, _ = same_pads(H, k, s)
    ow, pl, _ = same_pads(W, k, s)
    return [B, H, W, C, k, k, s, s, pt, pl, oh, ow, M]


def _variants(shape, act):
    """name -> a callable that enqueues one launch on the current stream; and the bytes each moves."""
    import torch
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    B, H, W, C, M, k, s = shape
    g = _geom(shape)
    gi = K.ints(g)
    OH, OW, CM = g[10], g[11], C * M
    dev = "cuda:0"
    x, dy = torch.randn(B, H, W, C, device=dev), torch.randn(B, OH, OW, CM, device=dev)
    w, b = torch.randn(k, k, C, M, device=dev) / k, torch.randn(CM, device=dev)
    y, dx = torch.zeros_like(dy), torch.zeros_like(x)
    rows = int(lib.csa_dw_slab_rows(gi))
    slab = torch.zeros(rows, (k * k + 1) * CM, device=dev)
    gw, gb = torch.zeros_like(w), torch.zeros_like(b)
    keep = (x, dy, w, b, y, dx, slab, gw, gb, gi)

    def chk(rc):
        assert rc == 0, rc

    st = K.stream
    chk(lib.csa_dw_fwd(K.ptr(x), K.ptr(w), K.ptr(b), K.ptr(y), gi, act, 0.0, 0, st()))
    out = {}
    for form in (1, 2):
        if form == 1 and k * k * CM > lib.csa_dw_lds_floats():
            continue
        out[f"fwd_form{form}"] = (lambda f=form: chk(lib.csa_dw_fwd(
            K.ptr(x), K.ptr(w), K.ptr(b), K.ptr(y), gi, act, 0.0, f, st())))
    for form in (1, 2):
        out[f"bwd_form{form}"] = (lambda f=form: chk(lib.csa_dw_bwd(
            K.ptr(x), K.ptr(w), K.ptr(y), K.ptr(dy), K.ptr(dx), K.ptr(slab), K.ptr(gw), K.ptr(gb), gi, act, 0.0, f,
            st())))
        out[f"bwd_form{form}_nodx"] = (lambda f=form: chk(lib.csa_dw_bwd(
            K.ptr(x), K.ptr(w), K.ptr(y), K.ptr(dy), None, K.ptr(slab), K.ptr(gw), K.ptr(gb), gi, act, 0.0, f,
            st())))
    out["bwd_params"] = lambda: chk(lib.csa_dw_bwd_params(K.ptr(slab), rows, gi, K.ptr(gw), K.ptr(gb), st()))
    nbytes = {"fwd": 4 * (x.numel() + y.numel()), "bwd": 4 * (2 * x.numel() + 2 * y.numel())}
    return out, keep, (int(lib.csa_dw_form(gi)), int(lib.csa_dw_bwd_form(gi)), rows), nbytes


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
    for sname, shape in shapes().items():
        variants, keep, auto, nbytes = _variants(shape, args.act)
        graphs = {k: _graph(fn, args.chain) for k, fn in variants.items()}
        seen = {k: [] for k in graphs}
        for rnd in range(args.rounds):          # alternating: drift hits every variant alike
            for k, gr in graphs.items():
                us = _time_graph(gr, args.replays, args.chain)
                seen[k].append(us)
                print(json.dumps({"what": "kernel", "shape": sname, "variant": k, "round": rnd,
                                  "us_per_launch": round(us, 3)}), flush=True)
        med[sname] = {}
        for k, v in seen.items():
            m = statistics.median(v)
            row = {"median_us": round(m, 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3)}
            if k != "bwd_params":
                row["GBps"] = round(nbytes["fwd" if k.startswith("fwd") else "bwd"] / m * 1e-3, 1)
            med[sname][k] = row
        med[sname]["auto"] = {"fwd_form": auto[0], "bwd_form": auto[1], "slab_rows": auto[2]}
        del graphs, keep
    return med


def _time_step(layers, args) -> dict:
    from cloud_server_amd.data.datasets import synthetic_mnist
    from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config
    from cloud_server_amd.runtime.engine import TrainEngine
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c.update(optimizer_name="AdagradOptimizer", learning_rate=1e-4, options={"batch_size": 50})
    eng = TrainEngine(parse_train_config(c), synthetic_mnist(6000, seed=0), device="cuda:0", backend="hip",
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
            "pair": p.pair is not None, "hfuse": bool(p.hfuse), "tail": bool(p.tail)}


# (H, C, M, k, s) of the emulation comparison: one of each map, the sizes where the dense conv
# changes unit kind, a multiplier, a 5x5 and a stride
EMULATION = [(28, 1, 1, 3, 1), (28, 10, 1, 3, 1), (14, 20, 1, 3, 1), (14, 20, 2, 5, 1), (14, 64, 1, 3, 1),
             (14, 64, 1, 3, 2), (14, 128, 1, 3, 1), (14, 128, 2, 5, 1)]


def _emulation_nets(H, C, M, k, s):
    front = ([] if H == 28 else [{"layer": "pool"}]) + [{"layer": "conv", "filter": [1, 1, C]}]
    back = [{"layer": "connect", "hidden": 16}]
    dw = {"layer": "depthwise", "filter": [k, k, M], "stride": [s, s]}
    cv = {"layer": "conv", "filter": [k, k, C * M], "stride": [s, s]}
    return {"depthwise": front + [dw] + back, "dense_conv": front + [cv] + back}


def emulation(args) -> dict:
    med = {}
    for H, C, M, k, s in EMULATION:
        name = f"50x{H}x{H}x{C} M{M} {k}x{k} s{s}"
        nets = _emulation_nets(H, C, M, k, s)
        seen = {n: [] for n in nets}
        kinds = {}
        for r in range(args.rounds):
            for n, layers in nets.items():
                out = _time_step(layers, args)
                seen[n].append(out["ms_per_step"])
                kinds[n] = out["units"]
                print(json.dumps(dict(what="emulation", shape=name, round=r, net=n, **out)), flush=True)
        med[name] = {n: {"median_ms": statistics.median(v), "units": kinds[n]} for n, v in seen.items()}
        med[name]["dense_minus_depthwise_us"] = round(
            (med[name]["dense_conv"]["median_ms"] - med[name]["depthwise"]["median_ms"]) * 1e3, 2)
    return med


def steps(args) -> dict:
    from cloud_server_amd.models.dsl import SAMPLE_CONFIG
    base = SAMPLE_CONFIG["net_config"]["middle_layer"]
    sep = copy.deepcopy(base)
    assert sep[1] == {"layer": "conv", "filter": [2, 2, 20]}
    sep[1:2] = [{"layer": "depthwise", "filter": [3, 3, 1]}, {"layer": "conv", "filter": [1, 1, 20]}]
    nets = {"sample": base, "dw_separable": sep}
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
    ap.add_argument("--act", type=int, default=2, help="fused activation id (2: relu)")
    ap.add_argument("--only", choices=("kernels", "emulation", "step"), default=None)
    args = ap.parse_args()
    out = {}
    if args.only in (None, "kernels"):
        out["kernels_us_per_launch"] = kernels(args)
    if args.only in (None, "emulation"):
        out["emulation_ms_per_step"] = emulation(args)
    if args.only in (None, "step"):
        out["median_ms_per_step"] = steps(args)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
