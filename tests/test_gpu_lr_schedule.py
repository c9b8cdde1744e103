"""Learning-rate schedules on the MI355X: the device arithmetic against the float64 form, every
update site of the HIP program against a schedule-aware fp64 oracle, multi-step graphs,
deterministic mode, packed jobs, async_ps on the device transport and resume.

A tree without the feature runs every launch at the base rate: from step 2 on a parameter step
is then at least 2 x off (the site tests fail there)."""
import ctypes as C
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import oracle64 as X
import oracle64_sched as XS
from test_gpu_dp_overlap import _DPContext, pg  # noqa: F401  (the world-1 RCCL group fixture)
from test_lr_schedule_cpu import SCHEDULES, _sid

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import LrSchedule
from cloud_server_amd.ops import fused as K
from cloud_server_amd.ops import lr_schedule as L
from cloud_server_amd.ops import optim_ref as O
from cloud_server_amd.runtime import checkpoint as ckpt
from cloud_server_amd.runtime.engine import TrainEngine

pytestmark = pytest.mark.gpu

T = np.arange(1, 65)
# a net outside the conv-pair family: its dense layers take the fused backward + update
NO_PAIR = [{"layer": "conv", "filter": [3, 3, 8]}, {"layer": "pool"},
           {"layer": "connect", "hidden": 128}, {"layer": "connect", "hidden": 128}]


@pytest.fixture(scope="module")
def dataset():
    return synthetic_mnist(400, seed=3)


# ------------------------------------------------------------------------------ 1. the formula
def _eval(opt_id, lr, sched, t=T):
    lib = K.load(required=True)
    steps = torch.from_numpy(np.asarray(t, dtype=np.int64)).cuda()
    out = torch.full((len(t),), float("nan"), device="cuda")
    c = None if sched is None else (sched if isinstance(sched, L.LrSchedC) else L.to_c(sched))
    rc = lib.csa_lr_sched_eval(opt_id, lr, None if c is None else C.byref(c), K.ptr(steps), len(t), K.ptr(out),
                               K.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _adam64(t):
    t = np.asarray(t, dtype=np.float64)
    return np.sqrt(1.0 - float(np.float32(O.ADAM_B2)) ** t) / (1.0 - float(np.float32(O.ADAM_B1)) ** t)


@pytest.mark.parametrize("s", SCHEDULES, ids=_sid)
def test_device_formula_matches_float64(s):
    """relative 5e-6: pow within 16 ulp and cos within 4 ulp (the OpenCL bounds ocml is built
    to), the rounding of x amplified by |x ln r| <= 21 ln 2 = 14.6 <= 16 where the quotient is
    inexact (<= 1e-6), a few single roundings: about 2.2e-6 in all."""
    lr = 0.01
    ref = L.lr_f64(s, lr, T)
    got = _eval(O.OPT_SGD, lr, s)
    err = np.abs(got.astype(np.float64) - ref)
    print(_sid(s), "worst relative error", (err[ref > 0] / ref[ref > 0]).max())
    assert (err <= 5e-6 * ref).all(), (got, ref)
    # Adam: the bias correction on top of lr_t, with t (its own pow: two more 16-ulp terms)
    got = _eval(O.OPT_ADAM, lr, s)
    ref_a = ref * _adam64(T)
    err = np.abs(got.astype(np.float64) - ref_a)
    print(_sid(s), "adam worst relative error", (err[ref_a > 0] / ref_a[ref_a > 0]).max())
    assert (err <= 1e-5 * ref_a).all()
    if s.staircase and s.warmup_steps == 0:        # plateaus and edges, bitwise
        v = _eval(O.OPT_SGD, lr, s)
        g = T - 1
        assert ((v[1:] == v[:-1]) == (g[1:] % s.decay_steps != 0)).all(), v
        assert (v[1:] <= v[:-1]).all()
    if s.type == "cosine":                          # stays at alpha * lr for g >= S
        tail = _eval(O.OPT_SGD, lr, s)[max(s.decay_steps, s.warmup_steps):]
        assert (tail == np.float32(lr) * np.float32(s.alpha)).all(), tail


def test_device_constant_is_lr_bitwise():
    lr = 0.0123
    const = L.LrSchedC(0, 0, 1, 0, 1.0, 0.0)
    for opt in (O.OPT_SGD, O.OPT_ADAGRAD, O.OPT_ADADELTA):
        assert (_eval(opt, lr, const) == np.float32(lr)).all()
        assert (_eval(opt, lr, None) == np.float32(lr)).all()
    new, old = _eval(O.OPT_ADAM, lr, const), _eval(O.OPT_ADAM, lr, None)     # None: the schedule-free overload
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32))
    ref = lr * _adam64(T)
    assert (np.abs(old - ref) <= 1e-5 * ref).all()
    # warm-up on the constant type
    s = LrSchedule("constant", 1, 1.0, False, 0.0, 5)
    got, want = _eval(O.OPT_SGD, lr, s), L.lr_f64(s, lr, T)
    assert (np.abs(got - want) <= 5e-6 * want).all() and (got[5:] == np.float32(lr)).all()


# ------------------------------------------------------------------------------ 2. every update site
@pytest.fixture()
def launches(monkeypatch):
    """Names of the update launchers called WITH a schedule (``fused.sched_call``)."""
    seen = set()
    orig = K.sched_call

    def rec(lib, name, sched, *args):
        if sched is not None:
            seen.add(name)
        return orig(lib, name, sched, *args)
    monkeypatch.setattr(K, "sched_call", rec)
    return seen


def _dp_ctx():
    return _DPContext(rank=0, world=1, local_rank=0, backend="nccl", device=torch.device("cuda", 0))


# lowering -> (layers, environment, strategy or None, launchers that must have run, plan check)
LOWERINGS = {
    # carrier (deferred dense updates + the head's own update: dense_update.h update-only body)
    # + the pair backward's tail (conv / BatchNorm parameters: conv_pair.hip tail)
    "default": (XS.SAMPLE128, {}, None, {"csa_dense_update_defer", "csa_conv_pair_tail_set"},
                lambda p: p.hfuse and p.tail and p.tail_update),
    # no tail: the flat optimizer with striped folds (optim_kernel) takes the rest
    "no_tail": (XS.SAMPLE128, {"CSA_PAIR_TAIL": "0"}, None, {"csa_dense_update_defer", "csa_optimizer2s"},
                lambda p: p.hfuse and not p.tail_update),
    # nothing fused: every parameter in the flat optimizer
    "unfused": (XS.SAMPLE128, {"CSA_FUSED_DENSE": "0", "CSA_FUSED_UPDATE": "0"}, None, {"csa_optimizer2s"},
                lambda p: not p.fused and not p.hfuse and not any(u.fused for u in p.units)),
    # outside the pair family: the fused dense backward + update (dense_update.h full body)
    "no_pair": (NO_PAIR, {}, None, {"csa_dense_bwd_update_head", "csa_optimizer2s"},
                lambda p: p.pair is None and not p.hfuse and sum(u.fused for u in p.units) == 2),
    # data parallel, world 1: the dense update carried by the next step's pair forward
    # (+ csa_opt_carry_flush from flush_params) and the streaming optimizer (optim_fast_kernel)
    "dp_allreduce": (XS.SAMPLE128, {"CSA_XGMI": "0"}, "allreduce",
                     {"csa_conv_pair_fwd_carry", "csa_opt_carry_flush", "csa_optimizer2s"},
                     lambda p: p.carry is not None),
    "dp_allreduce_hf": (XS.SAMPLE128, {"CSA_XGMI": "0"}, "allreduce:hf", {"csa_optimizer2s"},
                        lambda p: p.dp_hf and p.tail and not p.tail_update),
    # lowrank: the gathered dense gradient applied inside the weight-gradient launch (dd_wgrad)
    "dp_lowrank": (XS.SAMPLE128, {"CSA_XGMI": "0"}, "lowrank", {"csa_dd_wgrad", "csa_optimizer2s"},
                   lambda p: len(p.lr_units) == 2 and all(u.lr_update for u in p.lr_units)),
    # async_ps, world 1: the owner's apply (async_ps.hip), t = the apply count
    "dp_async_ps": (XS.SAMPLE128, {}, "async_ps", {"csa_aps_step"}, lambda p: True),
}
SITE_CASES = [(n, o, "stair") for n in LOWERINGS for o in ("AdagradOptimizer", "GradientDescentOptimizer")]
SITE_CASES += [("default", o, "stair") for o in ("AdamOptimizer", "AdadeltaOptimizer")]
SITE_CASES += [("default", o, "cosine") for o in X.LRS]


@pytest.mark.parametrize("name,opt,sched", SITE_CASES, ids=lambda v: X.SHORT.get(v, v))
def test_update_sites_follow_the_schedule(name, opt, sched, dataset, launches, monkeypatch, request):
    layers, env, strategy, want, plan_ok = LOWERINGS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = {}
    if strategy is not None:
        request.getfixturevalue("pg")
        kw = dict(ctx=_dp_ctx(), strategy=strategy)
    cfg = XS.make_cfg(layers, opt, X.LRS[opt], XS.STAIR_HALF if sched == "stair" else XS.COSINE_WARM)
    eng = TrainEngine(cfg, dataset, device="cuda:0", backend="hip", use_graph=False, **kw)
    assert eng.backend == "hip", eng.fallback_reason
    assert plan_ok(eng.program), name
    # (read_state flushes the parameters before and after every step: a carried update is
    # applied by the flush, at the step it belongs to; the run below lets the forward carry it)
    oracle = XS.SchedOracle64(cfg, dataset, dense_last=strategy == "lowrank")
    XS.run_trajectory(eng, oracle, 4, "sample", f"{name}-{X.SHORT[opt]}-{sched}")
    if strategy == "async_ps":
        eng.aps.check()
        assert eng.aps.applied == 4
    assert want <= launches, (want - launches, launches)
    for w in eng.health_words():
        assert int(w.item()) == 0


def test_carried_update_sees_its_own_step(dataset, launches, monkeypatch, pg):  # noqa: F811
    """The carried dense update runs in step t + 1's forward, before the head advances the
    counter: it must use lr_t, not lr_{t+1}.  6 steps with no flush in between (the forward
    carries every update but the last) equal 6 steps with a flush after each."""
    monkeypatch.setenv("CSA_XGMI", "0")
    cfg = XS.make_cfg(XS.SAMPLE128, "GradientDescentOptimizer", 0.01, XS.STAIR_HALF)
    a = TrainEngine(cfg, dataset, device="cuda:0", backend="hip", use_graph=False, ctx=_dp_ctx(), strategy="allreduce")
    b = TrainEngine(cfg, dataset, device="cuda:0", backend="hip", use_graph=False, ctx=_dp_ctx(), strategy="allreduce")
    assert a.program.carry is not None
    for i in range(6):
        a.step()
        b.step()
        b.flush_params()
        if i == 2:
            a.flush_params()                      # one flush mid-run
    a.sync_device(); b.sync_device()
    assert {"csa_conv_pair_fwd_carry", "csa_opt_carry_flush"} <= launches
    # the two differ only in which launch applied the update (same arithmetic per element)
    offs = a.model.state.offsets
    lo = min(offs[n] for n in offs if n.endswith(".weight") and a.model.state.shapes[n][0] > 100)
    torch.testing.assert_close(a.flat, b.flat, rtol=1e-5, atol=1e-7)
    assert lo in a.program.carry_offsets


# ------------------------------------------------------------------------------ 3. / 4. graphs, deterministic
SCHED_G = {"type": "exponential", "decay_steps": 3, "decay_rate": 0.5, "staircase": True, "warmup_steps": 2}


def _det_engine(dataset, opt="AdagradOptimizer", use_graph=True, sched=SCHED_G, **kw):
    cfg = XS.make_cfg(XS.SAMPLE128, opt, X.LRS[opt], sched)
    eng = TrainEngine(cfg, dataset, device="cuda:0", backend="hip", use_graph=use_graph, **kw)
    assert eng.backend == "hip" and eng.program.det, eng.fallback_reason
    return eng


@pytest.mark.parametrize("opt", ["AdagradOptimizer", "AdamOptimizer"], ids=lambda o: X.SHORT[o])
def test_multi_step_graphs_equal_single_steps(opt, dataset, monkeypatch):
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    monkeypatch.setenv("CSA_GRAPH_STEPS", "4")
    try:
        a, b, c = _det_engine(dataset, opt), _det_engine(dataset, opt), _det_engine(dataset, opt, use_graph=False)
        a.step(); b.step(); c.step()
        a.run_steps(8)
        assert a.graph_k is not None and a.group_steps() == 4
        for _ in range(8):
            b.step(); c.step()
        for e in (a, b, c):
            e.sync_device()
        assert a.host_step == b.host_step == 9 and int(a.dstep.item()) == 9
        assert torch.equal(a.flat, b.flat) and torch.equal(a.slots, b.slots)          # 4-step graphs
        assert torch.equal(c.flat, b.flat) and torch.equal(c.slots, b.slots)          # eager HIP run
        # and the schedule acted: the constant-rate run ends elsewhere
        d = _det_engine(dataset, opt, sched=None)
        for _ in range(9):
            d.step()
        d.sync_device()
        assert (d.flat - b.flat).abs().max().item() > 1e-4
    finally:
        torch.use_deterministic_algorithms(False)


# ------------------------------------------------------------------------------ 5. packed jobs
def test_packed_jobs_keep_their_own_schedules(dataset, monkeypatch):
    from cloud_server_amd.runtime.multijob import PackedJobs
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    scheds = (XS.STAIR_HALF, XS.COSINE_WARM)
    try:
        def eng(i):
            cfg = XS.make_cfg(XS.SAMPLE128, "AdagradOptimizer", 0.01, scheds[i], seed=i)
            e = TrainEngine(cfg, dataset, device="cuda:0", backend="hip", packed=True)
            assert e.backend == "hip" and e.program.packed, e.fallback_reason
            return e
        packed = [eng(0), eng(1)]
        pack = PackedJobs(packed)
        for _ in range(4):
            pack.step()
        pack.sync_device()
        for i, b in enumerate(packed):
            a = eng(i)                       # the same launch profile, alone
            for _ in range(4):
                a.step()
            a.sync_device()
            # (test_multitenant's tolerance: exact)
            torch.testing.assert_close(b.flat, a.flat, rtol=0, atol=0)
            torch.testing.assert_close(b.slots, a.slots, rtol=0, atol=0)
        assert not torch.equal(packed[0].slots, packed[1].slots)
    finally:
        torch.use_deterministic_algorithms(False)


# ------------------------------------------------------------------------------ 6. async_ps, world 2
APS_STEPS = 12
APS_SCHED = {"type": "exponential", "decay_steps": 4, "decay_rate": 0.5, "staircase": True}


def _worker_aps(rank: int, world: int, port: int, q) -> None:
    import torch.distributed as dist
    from cloud_server_amd.parallel.xgmi import shared_gpu_block_cap
    os.environ.update(LOCAL_WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0",
                      CSA_XGMI_BLOCKS=str(shared_gpu_block_cap(world)))     # one GPU: co-resident
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        from cloud_server_amd.parallel.dist import DistContext
        # (Adagrad 0.003: the eager engine's loss falls from 3.6 to 2.0 over these 24 applies; 0.05
        # diverges on this net with or without a schedule)
        cfg = XS.make_cfg(XS.SAMPLE128, "AdagradOptimizer", 0.003, APS_SCHED, batch=20, staleness=2)
        ds = synthetic_mnist(400, seed=3)
        ctx = DistContext(rank=rank, world=world, local_rank=0, backend="nccl", device=dev)
        eng = TrainEngine(cfg, ds, device="cuda:0", ctx=ctx, backend="hip", strategy="async_ps")
        assert eng.backend == "hip", eng.fallback_reason
        assert type(eng.aps).__name__ == "AsyncPSDevice" and eng.aps.sched_c is not None
        for i in range(APS_STEPS):
            eng.step()
            torch.cuda.synchronize()
            q.put((rank, {"step": i}))                    # the parent times every step
        eng.sync_device()
        eng.aps.check()
        losses = [float(eng.ring_loss[i].item()) for i in range(APS_STEPS)]
        eng.finish_async()
        health = [int(w.item()) for w in eng.health_words()]
        q.put((rank, {"done": True, "losses": losses, "stale": eng.staleness(), "applied": eng.aps.applied,
                      "t": eng.aps.t, "health": health, "flat": eng.flat.cpu().numpy().copy()}))
        eng.aps.close()
        dist.destroy_process_group()
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, {"exception": traceback.format_exc()}))


def test_async_ps_device_world2_with_a_schedule():
    world = 2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker_aps, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res, errs = {}, {}
    try:
        first = True
        while len(res) + len(errs) < world:
            # engine construction (warm-up, capture) comes before the first step's message
            r, d = q.get(timeout=180 if first else 60)
            first = False
            if "exception" in d:
                errs[r] = d["exception"].strip().splitlines()[-1]
            elif d.get("done"):
                res[r] = d
    finally:
        for p in ps:
            p.join(timeout=20)
            if p.is_alive():
                p.kill()
    assert not errs, errs
    assert len(res) == world, f"workers died: exit codes {[p.exitcode for p in ps]}"
    for r in range(world):
        d = res[r]
        assert d["stale"] <= 2 * 2, d["stale"]                         # max_staleness <= 2s
        assert d["applied"] == world * APS_STEPS and d["t"] == APS_STEPS
        assert not any(d["health"]), d["health"]
        assert all(np.isfinite(d["losses"]))
        assert np.mean(d["losses"][-4:]) < np.mean(d["losses"][:4]), d["losses"]      # it converges
        assert np.array_equal(d["flat"], res[0]["flat"]), r              # replicas agree after the drain


# ------------------------------------------------------------------------------ 7. resume
def test_resume_is_exact_on_the_hip_backend(dataset, monkeypatch):
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    try:
        a = _det_engine(dataset, "AdamOptimizer")
        for _ in range(6):
            a.step()
        a.sync_device()
        b = _det_engine(dataset, "AdamOptimizer")
        for _ in range(3):
            b.step()
        b.sync_device()
        obj = ckpt.engine_state(b)
        c = _det_engine(dataset, "AdamOptimizer")
        ckpt.restore_engine(c, obj)
        for _ in range(3):
            c.step()
        c.sync_device()
        assert int(c.dstep.item()) == 6
        assert torch.equal(a.flat, c.flat) and torch.equal(a.slots, c.slots)
    finally:
        torch.use_deterministic_algorithms(False)
