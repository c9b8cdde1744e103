#!/usr/bin/env python
"""What the layer / group / instance normalisation launches cost (one GPU).

1. ``kernels``: ``csa_gn_fwd`` (statistics kept), ``csa_gn_bwd`` and ``csa_gn_bwd_params`` in
   every forced form the shape has (1: a wave holds the group in registers, 2: a 256-thread
   workgroup does, 3: a 1024-thread workgroup streams it through L2): the table the automatic
   form choice (``csa_gn_form``) rests on.  Each is timed as a captured graph of ``--chain``
   back-to-back launches replayed ``--replays`` times (device events), so the figure is the
   launch's time on the device, launch gap included; the variants alternate inside every round.
2. ``step``: ms/step of the sample config and of the sample with its norm in ``layer`` mode (the
   plain sample's BatchNorm is fused into the pair and fc1; the layer norm is a unit of its own
   with two backward launches, and its parameters keep the flat optimizer launch).  Timed like
   bench.py (graph-captured steps through ``TrainEngine.run_steps``), alternating.

    python scripts/gn_cost.py [--rounds 3] [--chain 50] [--replays 40] [--steps 2000] [--warmup 200]

Prints one JSON line per measurement and a closing line of medians."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (B, HW, C, G): the sample's pooled map as layer, group and instance norm, a flat input, the
# streaming shape; two layer norms between the group and the layer norm of the sample's map
# (1960 and 2940 elements a group), where forms 2 and 3 cross
SHAPES = {
    "50x14x14x20 G1": (50, 196, 20, 1),
    "50x14x14x10 G1": (50, 196, 10, 1),
    "50x14x14x15 G1": (50, 196, 15, 1),
    "50x14x14x20 G4": (50, 196, 20, 4),
    "50x14x14x20 G20": (50, 196, 20, 20),
    "50x512 G1": (50, 1, 512, 1),
    "1x28x28x128 G1": (1, 784, 128, 1),
}


def _variants(geom, act):
    """name -> a callable that enqueues one launch on the current stream."""
    import torch
    from cloud_server_amd.ops import fused as K
    lib = K.load(required=True)
    B, HW, C, G = geom
    gi = K.ints(list(geom))
    dev = "cuda:0"
    x, dy = torch.randn(B, HW, C, device=dev), torch.randn(B, HW, C, device=dev)
    sc, of = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    y, dx = torch.zeros_like(x), torch.zeros_like(x)
    stat, slab = torch.zeros(B, G, 2, device=dev), torch.zeros(B, 2, C, device=dev)
    dsc, dof = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    keep = (x, dy, sc, of, y, dx, stat, slab, dsc, dof, gi)

    def chk(rc):
        assert rc == 0, rc

    chk(lib.csa_gn_fwd(K.ptr(x), K.ptr(sc), K.ptr(of), K.ptr(y), K.ptr(stat), gi, 1e-6, act, 0.0, 0, K.stream()))
    out = {}
    m = HW * C // G
    for form in (1, 2, 3):
        if m > lib.csa_gn_form_max(form):
            continue
        out[f"fwd_form{form}"] = (lambda f=form: chk(lib.csa_gn_fwd(
            K.ptr(x), K.ptr(sc), K.ptr(of), K.ptr(y), K.ptr(stat), gi, 1e-6, act, 0.0, f, K.stream())))
        out[f"bwd_form{form}"] = (lambda f=form: chk(lib.csa_gn_bwd(
            K.ptr(x), K.ptr(sc), K.ptr(of), K.ptr(stat), K.ptr(dy), K.ptr(dx), K.ptr(slab), gi, act, 0.0, f,
            K.stream())))
    out["bwd_params"] = lambda: chk(lib.csa_gn_bwd_params(K.ptr(slab), B, C, K.ptr(dsc), K.ptr(dof), K.stream()))
    return out, keep, int(lib.csa_gn_form(gi))


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
    for sname, geom in SHAPES.items():
        variants, keep, auto = _variants(geom, args.act)
        graphs = {k: _graph(fn, args.chain) for k, fn in variants.items()}
        seen = {k: [] for k in graphs}
        for rnd in range(args.rounds):          # alternating: drift hits every variant alike
            for k, gr in graphs.items():
                us = _time_graph(gr, args.replays, args.chain)
                seen[k].append(us)
                print(json.dumps({"what": "kernel", "shape": sname, "variant": k, "round": rnd,
                                  "us_per_launch": round(us, 3)}), flush=True)
        med[sname] = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3),
                          "max_us": round(max(v), 3)} for k, v in seen.items()}
        med[sname]["auto_form"] = auto
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
    ln = copy.deepcopy(base)
    assert ln[3] == {"layer": "norm"}
    ln[3] = {"layer": "norm", "mode": "layer"}
    nets = {"sample": base, "gn_sample_layer": ln}
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
    ap.add_argument("--act", type=int, default=1, help="fused activation id (1: the sample's sigmoid)")
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
