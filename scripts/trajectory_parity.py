#!/usr/bin/env python
"""Per-step fp64 parity tables (tests/oracle64.py): the HIP program and fp32 eager, both on
the GPU, each shadowed by the fp64 oracle over the grid of tests/test_hip_trajectory.py.

    python scripts/trajectory_parity.py OUT.md [OUT.json]
    python scripts/trajectory_parity.py --grid geometry profiles/geometry_parity.md [OUT.json]

``--grid geometry``: the conv / pool geometry grid of tests/geometry_nets.py with the cases of
tests/test_gpu_geometry.py (the contract cases included: their "hip" run is whatever the
engine built, named in the lowering table with its reason) instead of the step tests' grid;
the tables then also give every network's worst error as a fraction of its bound
(``oracle64.tolerances``), for both programs, and the units it lowered to.

Writes, per network, the worst error of every compared quantity (relative to the tensor /
relative to the largest tensor), the grid-wide worst of eager, 4 x that (the tolerances
of tests/oracle64.py:TOL come from this table) and which program every network lowered to.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import oracle64 as X  # noqa: E402
from test_hip_step import CASES  # noqa: E402
from cloud_server_amd.data.datasets import synthetic_mnist  # noqa: E402
from cloud_server_amd.runtime.engine import TrainEngine  # noqa: E402


def merge(dst, w):
    for q, (a, b) in w.items():
        p = dst.get(q, (0.0, 0.0))
        dst[q] = (max(p[0], a), max(p[1], b))


def table(title, per_net, quantities):
    lines = [f"### {title}", "", "| network | " + " | ".join(quantities) + " |", "|---|" + "---|" * len(quantities)]
    for n, w in per_net.items():
        lines.append(f"| {n} | " + " | ".join(f"{w[q][0]:.1e} / {w[q][1]:.1e}" if q in w else "" for q in quantities) + " |")
    return lines + [""]


def geometry_grid():
    """(networks, cases) of the geometry grid: test_gpu_geometry's cases + the contract cases."""
    import geometry_nets as G
    from test_gpu_geometry import GRID
    cases = [(n, o, loss, b, False) for n, o, loss, b in GRID]
    cases += [(n, "AdagradOptimizer", "entropy", 50, False) for n in G.CONTRACT]
    return G.NETS, cases


def bound_fraction(recs, tol):
    """Worst err / bound over the records of one run (``oracle64.check``'s bound)."""
    worst = 0.0
    for rs in recs:
        for r in rs:
            if r.quantity == "correct":
                continue
            rtol, atol, *rest = tol[r.quantity]
            bound = rtol * r.tmax + atol * r.gmax + (rest[0] if rest else 0.0)
            worst = max(worst, r.err / bound if bound > 0 else (0.0 if r.err == 0 else float("inf")))
    return worst


def main():
    argv = sys.argv[1:]
    geometry = False
    if argv[:1] == ["--grid"]:
        if argv[1:2] not in (["geometry"], ["steps"]):
            sys.exit("--grid geometry | steps")
        geometry = argv[1] == "geometry"
        argv = argv[2:]
    out_md = argv[0]
    out_json = argv[1] if len(argv) > 1 else None
    ds = synthetic_mnist(400, seed=3)
    nets, cases = geometry_grid() if geometry else (X.networks(CASES), X.grid(CASES))
    res = {"hip": {}, "torch": {}}
    info, times, notes, raw = {}, {}, [], {}
    frac = {"hip": {}, "torch": {}}
    stop = False
    for c in cases:
        n, o, loss, b, graph = c
        cid = X.case_id(c)
        cfg = X.make_cfg(nets[n], o, X.LRS[o], loss, b)
        for backend in ("hip", "torch"):
            if backend == "torch" and graph:
                continue
            t0 = time.time()
            try:
                eng = TrainEngine(cfg, ds, device="cuda", backend=backend, use_graph=graph)
                if backend == "hip":
                    p = eng.program
                    info[n] = dict(backend=eng.backend, reason=eng.fallback_reason,
                                   fused=bool(getattr(p, "fused", False)), hfuse=bool(getattr(p, "hfuse", False)),
                                   tail=bool(getattr(p, "tail", False)), pair=getattr(p, "pair", None) is not None,
                                   zero_regions=len(getattr(p, "zero_regions", [])),
                                   zero_early=len(getattr(p, "zero_early", [])),
                                   fwd_zero=len(getattr(p, "fwd_zero", [])),
                                   units=" ".join(("conv" + ("+act" if u.act is not None else "") +
                                                   ("+pool" if u.pool is not None else "")) if u.kind == "conv"
                                                  else u.kind for u in getattr(p, "units", [])))
                recs = X.run_trajectory(eng, X.Oracle64(cfg, ds))
            except Exception as exc:          # noqa: BLE001
                # whatever went wrong, start nothing more on the device
                notes.append(f"{cid} [{backend}]: {type(exc).__name__}: {exc}")
                print(notes[-1], flush=True)
                stop = True
                break
            w = X.worst(recs)
            frac[backend][n] = max(frac[backend].get(n, 0.0), bound_fraction(recs, X.tolerances(n, X.LRS[o])))
            res[backend][cid] = {q: list(v) for q, v in w.items()}
            raw.setdefault(backend, {})[cid] = [[(r.quantity, r.tensor, r.err, r.tmax, r.gmax) for r in rs]
                                                for rs in recs]
            res[backend][cid]["correct"] =[max(r.err for rs in recs for r in rs if r.quantity == "correct"),
                                            max(r.tmax for rs in recs for r in rs if r.quantity == "correct")]
            times[f"{cid} [{backend}]"] = time.time() - t0
            print(f"{cid} [{backend}] {time.time() - t0:.2f}s " +
                  " ".join(f"{q}={a:.1e}/{bb:.1e}" for q, (a, bb) in w.items()), flush=True)
            if out_json:
                with open(out_json, "w") as f:
                    json.dump(dict(res=res, info=info, times=times, notes=notes, records=raw, bound_fraction=frac), f)
            del eng
        if stop:
            break
    quantities = ["loss", "bn", "gd.dw", "adagrad.dacc", "adagrad.dw", "adam.dm", "adam.dv", "adam.dw_self",
                  "adadelta.dacc", "adadelta.dw", "adadelta.dup_self"]
    md = ["# Per-step fp64 parity" + (" of the conv / pool geometry grid" if geometry else "") +
          ": HIP program and fp32 eager against the fp64 shadow oracle", "",
          "Every cell: worst over the 3 steps and over the network's cases of max|engine - oracle| relative",
          "to the tensor's largest reference value (tensors within 1000x of the largest only) / relative to",
          "the largest reference value of any tensor.  `loss` and `bn` are plain relative errors.", ""]
    grid_w = {}
    for backend, title in (("hip", "HIP program vs oracle"), ("torch", "fp32 eager (GPU) vs oracle")):
        per_net, tot = {}, {}
        for cid, w in res[backend].items():
            w = {q: tuple(v) for q, v in w.items() if q != "correct"}
            merge(per_net.setdefault(cid.split("-")[0], {}), w)
            merge(tot, w)
        per_net["**worst**"] = tot
        grid_w[backend] = tot
        md += table(title, per_net, quantities)
    md += ["### 4 x the worst eager figure over this grid (for comparison: the geometry tests keep oracle64.TOL)"
           if geometry else "### Tolerances: 4 x the worst eager figure over the grid", "",
           "| quantity | eager worst (tensor / global) | rtol | atol | HIP worst |", "|---|---|---|---|---|"]
    for q in quantities:
        if q in grid_w["torch"]:
            a, b = grid_w["torch"][q]
            h = grid_w["hip"].get(q, (float("nan"),) * 2)
            md.append(f"| {q} | {a:.2e} / {b:.2e} | {4 * a:.2e} | {4 * b:.2e} | {h[0]:.2e} / {h[1]:.2e} |")
    md += ["", "### Correct count: |engine - oracle| / borderline samples (fp64 margin < 1e-4), worst step", ""]
    for backend in ("hip", "torch"):
        odd = {c: w["correct"] for c, w in res[backend].items() if w["correct"][0] or w["correct"][1]}
        md.append(f"- {backend}: " + (", ".join(f"{c} {d:.0f}/{m:.0f}" for c, (d, m) in odd.items()) or "none"))
    if geometry:
        md += ["", "### Worst error as a fraction of its bound (oracle64.tolerances; above 1 fails the test)", "",
               "| network | HIP program | fp32 eager (GPU) |", "|---|---|---|"]
        for n in frac["hip"]:
            md.append(f"| {n} | {frac['hip'][n]:.3f} | " +
                      (f"{frac['torch'][n]:.3f}" if n in frac["torch"] else "") + " |")
    md += ["", "### Lowering of every network (HIP)", "",
           "| network | backend | fused | hfuse | tail | pair | zero_regions | zero_early | fwd_zero | units | reason |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, i in info.items():
        md.append(f"| {n} | {i['backend']} | {i['fused']} | {i['hfuse']} | {i['tail']} | {i['pair']} | "
                  f"{i['zero_regions']} | {i['zero_early']} | {i['fwd_zero']} | {i['units']} | {i['reason']} |")
    slow = sorted(times.items(), key=lambda kv: -kv[1])[:5]
    md += ["", f"Wall time: {sum(times.values()):.1f} s for {len(times)} runs; slowest: " +
           ", ".join(f"{k} {v:.1f} s" for k, v in slow), ""]
    if notes:
        md += ["### Cases that raised", ""] + [f"- {x}" for x in notes] + [""]
    with open(out_md, "w") as f:
        f.write("\n".join(md))
    print("\n".join(md))
    return 1 if stop else 0


if __name__ == "__main__":
    sys.exit(main())
