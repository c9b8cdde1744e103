"""Held-out validation on the GPU: ``csa_eval_rows`` / ``csa_eval_finish`` (eval.hip) against
fp64 NumPy, the device-resident sweep (``runtime.validation.HipValidator``) against the
eager ``TorchValidator`` on the same engine, the training state a sweep must leave alone,
and the job loop's ``validation.jsonl`` on the HIP backend."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, parse_train_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = {"none": 0, "sigmoid": 1, "relu": 2}
SENT = -7


def _bound(ref):
    """The project's HIP-vs-reference tolerance (tests/test_gpu_serving.py ``_close``)."""
    return 1e-4 + 1e-4 * float(np.abs(ref).max())


def _act64(x, act):
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if act == "relu":
        return np.maximum(x, 0.0)
    return x


def _reference(K, n, act, loss):
    """Seeded h / Wh / bh / labels (all ten classes) and their fp64 logits, predictions and
    loss terms; the seed is the first whose rows ALL have a top-two logit gap above
    1e-3 * max|logit| (searched on the CPU, asserted by the caller)."""
    for seed in range(64):
        rng = np.random.default_rng(1000 * K + seed)
        h = rng.standard_normal((n, K)).astype(np.float32)
        w = (rng.standard_normal((K, 10)) / np.sqrt(K)).astype(np.float32) * 2.0
        b = (rng.standard_normal(10) * 0.1).astype(np.float32)
        y = rng.permutation(np.arange(n) % 10).astype(np.int64)
        z = _act64(h.astype(np.float64), act) @ w.astype(np.float64) + b.astype(np.float64)
        top = np.sort(z, axis=1)
        gap = (top[:, -1] - top[:, -2]).min()
        if gap > 1e-3 * np.abs(z).max():
            break
    if loss == "mse":
        terms = ((z - np.eye(10)[y]) ** 2).sum(1)
    else:
        mx = z.max(1, keepdims=True)
        terms = mx[:, 0] + np.log(np.exp(z - mx).sum(1)) - z[np.arange(n), y]
    return h, w, b, y, z, gap, terms


def _sweep(lib, K_, bufs, M, Kdim, n_total, act, loss):
    """memset, one csa_eval_rows per batch, csa_eval_finish: what HipValidator.issue does."""
    from cloud_server_amd.ops import fused as F
    rows = bufs["rows"]
    nb = rows.shape[0]
    bufs["ctl"].zero_()
    cursor, counter, record = bufs["cursor"], bufs["counter"], bufs["record"]
    fused = bool(lib.csa_eval_rows_fused_ok(M, Kdim))
    for bi in range(nb):
        hb = bufs["h"].index_select(0, rows[bi]).contiguous()
        if fused:
            rc = lib.csa_eval_rows(F.ptr(hb), M, Kdim, ACTS[act], 0.0, F.ptr(bufs["w"]), F.ptr(bufs["b"]), None,
                                   F.ptr(bufs["labels"]), F.ptr(rows), F.ptr(cursor), int(loss == "mse"), n_total, nb,
                                   F.ptr(bufs["row_pred"]), F.ptr(bufs["row_loss"]), F.ptr(counter), F.stream())
        else:
            # logits mode: the kernel's INPUT is the [M, 10] logits csa_dense_fwd wrote (as in
            # HipProgram._predict_logits_into); formed once per batch and kept, since that
            # GEMM's split-K atomics are not what the second sweep's bit-equality is about
            logits = bufs.setdefault("logits", {}).get(bi)
            if logits is None:
                logits = bufs["logits"][bi] = torch.zeros(M, 10, device=DEV)
                rc = lib.csa_dense_fwd(F.ptr(hb), F.ptr(bufs["w"]), F.ptr(bufs["b"]), F.ptr(logits), M, 10, Kdim,
                                       None, 0, 0, 0.0, 0.0, None, None, ACTS[act], 0.0, F.stream())
                assert rc == 0
            rc = lib.csa_eval_rows(None, M, Kdim, 0, 0.0, None, None, F.ptr(logits),
                                   F.ptr(bufs["labels"]), F.ptr(rows), F.ptr(cursor), int(loss == "mse"), n_total, nb,
                                   F.ptr(bufs["row_pred"]), F.ptr(bufs["row_loss"]), F.ptr(counter), F.stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert int(cursor.item()) == (bi + 1) % nb and int(counter.item()) == 0
    rc = lib.csa_eval_finish(F.ptr(bufs["row_pred"]), F.ptr(bufs["row_loss"]), F.ptr(bufs["labels"]), F.ptr(rows),
                             n_total, F.ptr(record), F.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return fused, record.clone()


@pytest.mark.parametrize("loss", ["entropy", "mse"])
@pytest.mark.parametrize("act", ["none", "relu", "sigmoid"])
@pytest.mark.parametrize("Kdim", [4, 256, 260, 512, 1000, 1024, 1028])
def test_eval_kernels_match_fp64(Kdim, act, loss):
    from cloud_server_amd.ops import fused as F
    from cloud_server_amd.runtime.validation import row_table
    lib = F.load(required=True)
    h, w, b, y, z, gap, terms = _reference(Kdim, 100, act, loss)
    assert gap > 1e-3 * np.abs(z).max(), "no seed with every row's top-two gap above 1e-3 * max|logit|"
    assert set(y.tolist()) == set(range(10))
    pred64 = z.argmax(1)
    # (M = 64, n = 100): two batches, the second with 36 valid and 28 wrapped rows; (M = 1, n = 3)
    for M, n_total in ((64, 100), (1, 3)):
        rows = torch.from_numpy(row_table(n_total, M)).to(DEV)
        nb = rows.shape[0]
        ctl = torch.zeros(56, dtype=torch.int64, device=DEV)
        ctl32 = ctl.view(torch.int32)
        nrec = int(lib.csa_eval_record_ints())
        bufs = dict(h=torch.from_numpy(h).to(DEV), w=torch.from_numpy(w).to(DEV), b=torch.from_numpy(b).to(DEV),
                    labels=torch.from_numpy(y).to(DEV), rows=rows, ctl=ctl, cursor=ctl[0:1], counter=ctl32[2:3],
                    record=ctl32[4:4 + nrec],
                    row_pred=torch.full((nb * M,), SENT, dtype=torch.int32, device=DEV),
                    row_loss=torch.full((nb * M,), float(SENT), dtype=torch.float32, device=DEV))
        fused, rec = _sweep(lib, F, bufs, M, Kdim, n_total, act, loss)
        assert fused == (Kdim <= 1024)
        rp, rl = bufs["row_pred"].cpu().numpy(), bufs["row_loss"].cpu().numpy()
        # wrapped rows (and nothing else beyond n_total) were left alone
        assert (rp[n_total:] == SENT).all() and (rl[n_total:] == float(SENT)).all()
        assert nb * M > n_total or M == 1
        assert (rp[:n_total] == pred64[:n_total]).all()
        t = terms[:n_total]
        err = np.abs(rl[:n_total] - t).max()
        print(f"K={Kdim} M={M} {act}/{loss}: row-loss err {err:.3e} (bound {_bound(t):.3e})")
        assert err <= _bound(t), (err, _bound(t))
        r = rec.cpu().numpy()
        conf = np.zeros((10, 10), np.int64)
        np.add.at(conf, (y[:n_total], pred64[:n_total]), 1)
        assert r[0] == n_total and r[1] == np.trace(conf)
        assert (r[2:102].reshape(10, 10) == conf).all()
        loss_sum = float(r[102:104].view(np.float64)[0])
        denom = n_total * 10 if loss == "mse" else n_total
        mean_ref = t.sum() / denom
        assert abs(loss_sum / denom - mean_ref) <= _bound(np.asarray([mean_ref]))
        # fixed-order double sum of the fp32 row terms: exactly what NumPy gives in any order
        # up to double rounding; and bit-identical on a second sweep (with the re-armed state)
        assert int(bufs["cursor"].item()) == 0 and int(bufs["counter"].item()) == 0
        _, rec2 = _sweep(lib, F, bufs, M, Kdim, n_total, act, loss)
        assert torch.equal(rec, rec2)


# ----------------------------------------------------------------------------- end to end
NETS = {
    "sample": (None, "running"),
    "norm_batch": (None, "batch"),
    "conv_pool": ([{"layer": "conv", "filter": [2, 2, 10]}, {"layer": "conv", "filter": [2, 2, 20]},
                   {"layer": "pool"}], "running"),
}


def _config(net="sample", iters=20, **options):
    layers, bn_mode = NETS[net]
    c = copy.deepcopy(SAMPLE_CONFIG)
    if layers is not None:
        c["net_config"]["middle_layer"] = copy.deepcopy(layers)
    c.update(iter=iters, learning_rate=1e-3, optimizer_name="AdamOptimizer")
    c["options"] = dict(batch_size=50, bn_mode=bn_mode, log_every=100, ckpt_every=0, **options)
    return c


@pytest.fixture(scope="module")
def data():
    return synthetic_mnist(1500, seed=0).split(0.8)


def _engine(net, data, steps=20):
    from cloud_server_amd.runtime.engine import TrainEngine
    eng = TrainEngine(parse_train_config(_config(net)), data[0], device=DEV, backend="hip")
    assert eng.backend == "hip", eng.fallback_reason
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    return eng


def _state(eng):
    return ([eng.flat.clone(), eng.slots.clone(), eng.stream.cursor.clone(), eng.dstep.clone(),
             eng.ring_loss.clone(), eng.ring_correct.clone()] + [b.clone() for b in eng.model.buffers()])


@pytest.mark.parametrize("net", list(NETS))
def test_sweep_matches_torch_validator(net, data):
    from cloud_server_amd.runtime.validation import HipValidator, TorchValidator
    test = data[1]
    eng = _engine(net, data)
    before = _state(eng)
    for eb in (256, 64):
        val = eng.validator(test, eb, True)
        assert isinstance(val, HipValidator) and val.program.forward_only
        assert val.fwd.flat.data_ptr() == eng.flat.data_ptr()
        if net == "conv_pool":
            assert val.Kh == 3920 and not val.fused
        else:
            assert val.Kh <= 1024 and val.fused
        res = eng.validate(test, eb, True)
        tv = TorchValidator(eng, test, eb, predictions=True)
        tv.issue()
        ref = tv.wait()[1]
        z = tv.logits().double().cpu().numpy()
        assert res.n == ref.n == len(test)
        lb = _bound(np.asarray([ref.loss]))
        print(f"{net} eval_batch={eb}: loss {res.loss:.6f} vs {ref.loss:.6f}, acc {res.accuracy:.4f} vs {ref.accuracy:.4f}")
        assert abs(res.loss - ref.loss) <= lb, (res.loss, ref.loss, lb)
        # rows whose reference top-two gap is within twice the logit bound may flip (with the
        # eager model alone on the CPU, this seed excludes 0 of 300 rows on all three nets)
        top = np.sort(z, axis=1)
        sure = (top[:, -1] - top[:, -2]) > 2 * _bound(z)
        excluded = int((~sure).sum())
        same = res.predictions == ref.predictions
        assert same[sure].all(), f"{int((~same[sure]).sum())} confident rows differ ({excluded} gap-excluded rows)"
        assert same.mean() >= 0.99, f"agreement {same.mean():.4f} ({excluded} gap-excluded rows of {len(same)})"
        assert np.asarray(res.confusion).sum() == res.n
        assert res.accuracy == np.trace(np.asarray(res.confusion)) / res.n
        # a second sweep over the same parameters (the forward's split-K / statistic atomics
        # may reorder fp32 sums between sweeps; the fused head itself is fixed-order)
        again = eng.validate(test, eb, True)
        assert again.n == res.n and abs(again.loss - res.loss) <= lb
        assert (again.predictions == res.predictions)[sure].all()
    eng.check_health()
    after = _state(eng)
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))


def test_sweep_then_training_continues_identically(tmp_path, data, monkeypatch):
    """CSA_DETERMINISTIC=1: 12 steps with a sweep every 4 == 12 steps without."""
    from cloud_server_amd.runtime.trainer import JobRun
    monkeypatch.setenv("CSA_DETERMINISTIC", "1")
    ends = []
    for k, sub in ((4, "a"), (0, "b")):
        mdir = str(tmp_path / sub)
        os.makedirs(mdir)
        job = JobRun(mdir, _config("sample", 12, eval_every=k), device=DEV, backend="hip", data=data)
        while job.pending():
            job.before_step()
            job.step()
            if job.after_step():
                break
        out = job.finish()
        assert out["backend"] == "hip" and out["step"] == 12
        eng = job.eng
        ends.append([eng.flat.clone(), eng.slots.clone()] + [b.clone() for b in eng.model.buffers()])
        if k:
            with open(os.path.join(mdir, "validation.jsonl")) as f:
                assert [json.loads(l)["step"] for l in f] == [4, 8, 12]
    assert all(torch.equal(x, y) for x, y in zip(*ends))


def test_job_loop_hip(tmp_path, data):
    from cloud_server_amd.runtime.trainer import JobRun
    from cloud_server_amd.runtime.validation import HipValidator
    mdir = str(tmp_path / "m")
    os.makedirs(mdir)
    c = _config("sample", 96, eval_every=48)
    c["options"]["log_every"] = 32
    job = JobRun(mdir, c, device=DEV, backend="hip", data=data)
    while job.pending():
        job.before_step()
        job.step()
        if job.after_step():
            break
    out = job.finish()
    eng, val = job.eng, job.vlog.val
    assert out["backend"] == "hip" and out["step"] == 96
    with open(os.path.join(mdir, "validation.jsonl")) as f:
        rows = [json.loads(l) for l in f]
    assert [r["step"] for r in rows] == [48, 96]
    for r in rows:
        assert r["n"] == len(data[1]) and np.asarray(r["confusion"]).sum() == r["n"]
    assert eng.graphs_k, "multi-step graphs were not used"
    assert isinstance(val, HipValidator) and val.program.forward_only
    assert val.fwd.flat.data_ptr() == eng.flat.data_ptr()
    st = json.load(open(os.path.join(mdir, "status.json")))
    assert st["val_step"] == 96 and st["validation"] == "in_loop"
