#!/usr/bin/env python3
"""The sequence of kernel-library calls a HIP step program makes, normalised (GPU).

For a named case: the calls made while the engine is constructed (``plan``), the first
and second ``run()`` (``step1`` / ``step2``: the carry and tail flags differ between them)
and one ``predict_logits_into`` (``predict``).  Every call becomes its name plus arguments:
ints by value, floats by ``repr``, null pointers 0, every other pointer or stream the
ordinal of that address's first appearance in the case's trace (aliasing survives,
addresses and allocation order do not), integer arrays by element values, pointer arrays
by ordinals, a ``byref`` struct by its bytes.

    python scripts/launch_trace.py --write tests/golden/launch_trace.json   # the whole grid
    python scripts/launch_trace.py --case sample --dump                     # full text
    torchrun-style ranks (RANK / WORLD_SIZE set): --case dp:allreduce --dump-to DIR

tests/test_gpu_launch_trace.py replays the grid against the committed file.
"""
from __future__ import annotations

import argparse
import contextlib
import copy
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from cloud_server_amd.data.datasets import synthetic_mnist  # noqa: E402
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config  # noqa: E402
from cloud_server_amd.ops import fused as K  # noqa: E402
from cloud_server_amd.ops import optim_ref  # noqa: E402
from cloud_server_amd.runtime.engine import TrainEngine  # noqa: E402
from recorder import Recorder  # noqa: E402  (scripts/recorder.py)

B = 8
# process-wide knobs a program sets once per process and value (the first program of the
# process, whichever it is): not part of any one program's trace
ONCE_PER_PROCESS = ("csa_nt_out_",)
PHASES = ("plan", "step1", "step2", "predict")
_INT_TYPES = (C.c_int, C.c_long, C.c_longlong, C.c_uint, C.c_ulong, C.c_ulonglong)
_CArg = type(C.byref(C.c_int()))


# ---------------------------------------------------------------------------- normalising
class Normaliser:
    """One per case: the address -> ordinal table spans all four phases."""

    def __init__(self):
        self.ordinals = {}

    def addr(self, a) -> int:
        a = int(a or 0)
        if a == 0:
            return 0
        return self.ordinals.setdefault(a, len(self.ordinals) + 1)

    def arg(self, a, ctype) -> str:
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:
                return "[" + ",".join(f"@{self.addr(x)}" for x in a) + "]"
            if a._type_ in _INT_TYPES:
                return "[" + ",".join(str(int(x)) for x in a) + "]"
            return f"buffer*{len(a)}" if a._type_ is C.c_char else "bytes:" + bytes(a).hex()
        if isinstance(a, bytes):                    # (an IPC handle: process-specific content)
            return f"buffer*{len(a)}"
        if isinstance(a, C.c_void_p):
            return f"@{self.addr(a.value)}"
        if isinstance(a, _CArg):
            return "out" if isinstance(a._obj, C.c_void_p) else "bytes:" + bytes(a._obj).hex()
        if isinstance(a, C.Structure):
            return "bytes:" + bytes(a).hex()
        if a is None:
            return "0" if ctype is None or ctype is C.c_void_p else "None"
        if ctype is C.c_void_p:
            return f"@{self.addr(a)}"
        if isinstance(a, float) or ctype in (C.c_float, C.c_double):
            return repr(float(a))
        if isinstance(a, bool):
            return str(int(a))
        if isinstance(a, int):
            return str(a)
        return f"?{type(a).__name__}"

    def call(self, name, fn, args) -> str:
        types = list(getattr(fn, "argtypes", None) or [])
        types += [None] * (len(args) - len(types))
        return name + "(" + ", ".join(self.arg(a, t) for a, t in zip(args, types)) + ")"


def digest(text: str) -> str:
    return hashlib.sha256(text.encode()).hexdigest()[:12]


# ---------------------------------------------------------------------------- the grid
SAMPLE = SAMPLE_CONFIG["net_config"]["middle_layer"]
_CONV = {"layer": "conv", "filter": [3, 3, 8], "isBias": "True"}
_RELU = {"layer": "active", "active_func": "relu"}
NETS = {
    "dropout": SAMPLE[:-1] + [{"layer": "dropout", "keep_prob": 0.5}] + SAMPLE[-1:],
    "avgpool": [_CONV, _RELU, {"layer": "pool", "mode": "avg"}, {"layer": "connect", "hidden": 32}],
    "global_avgpool": [_CONV, _RELU, {"layer": "pool", "mode": "avg", "kernel": "global"},
                       {"layer": "connect", "hidden": 32}],
    "gconv": [{"layer": "conv", "filter": [3, 3, 192], "isBias": "True", "stride": [2, 2]}, _RELU, {"layer": "pool"},
              {"layer": "connect", "hidden": 32}],
    "standalone_bn": [_CONV, {"layer": "pool"}, {"layer": "connect", "hidden": 64}, {"layer": "norm"}, _RELU,
                      {"layer": "connect", "hidden": 32}],
}
ENV_CASES = ("CSA_DETERMINISTIC=1", "CSA_STAGE_BATCH=0", "CSA_FUSED_UPDATE=0", "CSA_HFUSE=0", "CSA_PAIR_TAIL=0",
             "CSA_FWD_BN_FUSE=0", "CSA_FWD_CHAIN=1")


def grid():
    """name -> dict(layers, optimizer, options, env, packed, forward_only)."""
    from test_hip_step import CASES
    g = {}
    for n in CASES:
        g[f"net:{n}"] = dict(layers=CASES[n])
    for kv in ENV_CASES:
        g[f"sample:{kv}"] = dict(layers=SAMPLE, optimizer="AdagradOptimizer", env=dict([kv.split("=")]))
    g["sample:packed"] = dict(layers=SAMPLE, optimizer="AdagradOptimizer", packed=True)
    g["sample:forward_only"] = dict(layers=SAMPLE, optimizer="AdagradOptimizer", forward_only=True)
    for n, layers in NETS.items():
        g[f"layer:{n}"] = dict(layers=layers)
    g["augment"] = dict(layers=SAMPLE, options={"augment": {"shift": 2, "rotate": 10, "scale": 10,
                                                            "erase_prob": 0.25}})
    g["lr_schedule"] = dict(layers=SAMPLE, optimizer="AdagradOptimizer",
                            options={"lr_schedule": {"type": "cosine", "decay_steps": 10, "warmup_steps": 2}})
    for opt in optim_ref.OPT_IDS:
        g[f"optimizer:{opt}"] = dict(layers=SAMPLE, optimizer=opt, lr=0.01)
    return g


def _cfg(case):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c["net_config"]["middle_layer"] = copy.deepcopy(case["layers"])
    c["optimizer_name"] = case.get("optimizer", "GradientDescentOptimizer")
    c["learning_rate"] = case.get("lr", 0.5)
    c["loss_name"] = "entropy"
    c["options"] = dict(batch_size=case.get("batch", B), **case.get("options", {}))
    return parse_train_config(c)


@contextlib.contextmanager
def _env(kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def _recording():
    """Every ``K.load()`` of the block hands out one recorder around the real library."""
    real = K.load(required=True)
    rec = Recorder(real, queries=True)
    K._LIB = rec
    try:
        yield rec
    finally:
        K._LIB = real


def trace(case, ctx=None, strategy="allreduce"):
    """{phase: [normalised call text]} of one case (one small engine, two steps)."""
    norm = Normaliser()
    out = {}
    ds = synthetic_mnist(200, seed=3)
    with _env(case.get("env", {})), _recording() as rec:
        def cut(phase):
            out[phase] = [norm.call(*c) for c in rec.calls if not c[0].startswith(ONCE_PER_PROCESS)]
            rec.calls.clear()

        kw = dict(ctx=ctx, strategy=strategy) if ctx is not None else {}
        eng = TrainEngine(_cfg(case), ds, device=ctx.device if ctx is not None else "cuda", backend="hip",
                          use_graph=False, packed=case.get("packed", False), **kw)
        assert eng.backend == "hip", eng.fallback_reason
        prog = eng.program
        if case.get("forward_only"):
            rec.calls.clear()
            from cloud_server_amd.runtime.hip_program import HipProgram
            prog = HipProgram(eng, forward_only=True)
        cut("plan")
        if not case.get("forward_only"):
            for phase in ("step1", "step2"):
                eng.step()
                torch.cuda.synchronize()
                cut(phase)
        logits = torch.zeros(eng.cfg.batch_size, 10, device="cuda")
        prog.predict_logits_into(logits)
        torch.cuda.synchronize()
        cut("predict")
        prog.lib = rec.lib
    return out


def compact(tr):
    return {ph: [f"{t.split('(', 1)[0]}:{digest(t)}" for t in calls] for ph, calls in tr.items()}


def pack(traces):
    """{case: compact trace} as a file: every distinct ``name:digest`` once, cases as indices."""
    calls = sorted({c for case in traces.values() for ph in case.values() for c in ph})
    ix = {c: i for i, c in enumerate(calls)}
    return {"calls": calls,
            "cases": {n: {ph: [ix[c] for c in cs] for ph, cs in case.items()} for n, case in traces.items()}}


def unpack(packed):
    calls = packed["calls"]
    return {n: {ph: [calls[i] for i in cs] for ph, cs in case.items()} for n, case in packed["cases"].items()}


def first_difference(tr, want):
    """None, or a message naming the first call of ``tr`` that differs from the compact
    ``want`` with that call's full normalised text."""
    for ph in PHASES:
        got, exp = tr.get(ph), want.get(ph)
        if got is None and exp is None:
            continue
        if got is None or exp is None:
            return f"phase {ph}: {'missing' if got is None else 'unexpected'}"
        for i, t in enumerate(got):
            if i >= len(exp):
                return f"{ph}[{i}]: {len(got) - len(exp)} call(s) more than recorded, first:\n  {t}"
            c = f"{t.split('(', 1)[0]}:{digest(t)}"
            if c != exp[i]:
                return f"{ph}[{i}]: recorded {exp[i]}, now {c}:\n  {t}"
        if len(got) < len(exp):
            return f"{ph}: {len(exp) - len(got)} call(s) fewer than recorded, first missing {exp[len(got)]}"
    return None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", help="a grid case, or dp:<strategy> under a launcher")
    ap.add_argument("--write", help="write the compact traces of the cases here (JSON)")
    ap.add_argument("--dump", action="store_true", help="print the full normalised text")
    ap.add_argument("--dump-to", help="write the full text to DIR/<case>.rank<r>.txt")
    a = ap.parse_args()
    g = grid()
    names = a.case or list(g)
    result = {}
    for n in names:
        if n.startswith("dp:"):
            from cloud_server_amd.parallel.dist import init_distributed, shutdown
            ctx = init_distributed("cuda")
            tr = trace(dict(layers=SAMPLE, optimizer="AdagradOptimizer", batch=B), ctx=ctx, strategy=n[3:])
            rank = ctx.rank
            shutdown(ctx)
        else:
            tr, rank = trace(g[n]), 0
        result[n] = compact(tr)
        text = "".join(f"## {ph}\n" + "".join(f"{t}\n" for t in tr[ph]) for ph in PHASES if ph in tr)
        if a.dump:
            print(f"# {n}\n{text}")
        if a.dump_to:
            os.makedirs(a.dump_to, exist_ok=True)
            with open(os.path.join(a.dump_to, f"{n.replace(':', '_')}.rank{rank}.txt"), "w") as f:
                f.write(text)
        print(f"{n}: " + " ".join(f"{ph}={len(tr[ph])}" for ph in PHASES if ph in tr), flush=True)
    if a.write:
        with open(a.write, "w") as f:
            json.dump(pack(result), f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
