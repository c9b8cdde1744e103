"""The classifier head's entry points, one launch each, against fp64 NumPy: ``csa_head_row``,
``csa_head_dgrad``, ``csa_head_part2`` and ``csa_head`` (head.hip, head_dgrad.h).  The shapes
are the smallest at which each kernel's index arithmetic can go wrong (every KPT at its edge
and with a clamped tail, partial row groups, both block orders of head_dgrad, both ``csa_head``
kernels); the inputs follow tests/test_gpu_validation.py ``_reference``."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = {"none": 0, "sigmoid": 1, "relu": 2, "leaky": 3}
IN_ACTS = ["none", "relu", "sigmoid"]
LOSSES = ["entropy", "mse"]
GS = 0.5            # grad_scale
LEAKY = 0.2
SENT = -7.0
STEP0 = 6           # device step counter before the launch

ROW_K, ROW_M = [2, 256, 258, 512, 514, 1024], [1, 5]
DG_KH, DG_K1, DG_M = [64, 320, 1024], [1, 17, 128], [1, 4, 5]
PART_K, PART_M = [4, 260], [1, 5, 17, 65]
HEAD_PATHS = {"rows": (8, [1, 16, 17], 0), "generic": (6, [1, 17], 0), "det": (8, [1, 16, 17], 1)}


def _bound(ref):
    """The project's HIP-vs-reference tolerance (tests/test_gpu_serving.py ``_close``)."""
    return 1e-4 + 1e-4 * float(np.abs(ref).max())


def _act64(x, act):
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if act == "relu":
        return np.maximum(x, 0.0)
    if act == "leaky":
        return np.maximum(x, LEAKY * x)
    return x


def _dact64(g, x, act):
    """g * act'(x), the kernels' conventions (common.h act_bwd)."""
    if act == "sigmoid":
        y = _act64(x, act)
        return g * y * (1.0 - y)
    if act == "relu":
        return np.where(x > 0.0, g, 0.0)
    if act == "leaky":
        return np.where(x >= LEAKY * x, g, g * LEAKY)
    return g


@functools.lru_cache(maxsize=None)
def _inputs(K, M, act):
    """Seeded h / Wh / bh and their fp64 logits; the seed is the first whose rows ALL have a
    top-two logit gap above 1e-3 * max|logit| (searched on the CPU, asserted by the caller).
    Cached and shared: callers do not write to the arrays."""
    for seed in range(64):
        rng = np.random.default_rng(1000 * K + seed)
        h = rng.standard_normal((M, K)).astype(np.float32)
        w = (rng.standard_normal((K, 10)) / np.sqrt(K)).astype(np.float32) * 2.0
        b = (rng.standard_normal(10) * 0.1).astype(np.float32)
        z = _act64(h.astype(np.float64), act) @ w.astype(np.float64) + b.astype(np.float64)
        top = np.sort(z, axis=1)
        gap = (top[:, -1] - top[:, -2]).min()
        if gap > 1e-3 * np.abs(z).max():
            break
    return h, w, b, z, gap


@functools.lru_cache(maxsize=None)
def _label_data(M):
    """Dataset labels covering all ten classes and a [2, M] row table into them."""
    n = 10 * max(1, -(-2 * M // 10))
    rng = np.random.default_rng(77 + M)
    lab = rng.permutation(np.arange(n) % 10).astype(np.int64)
    rows = rng.permutation(n)[:2 * M].reshape(2, M).astype(np.int64)
    assert set(lab.tolist()) == set(range(10))
    return lab, rows


def _labels(M, mode):
    """(labels, idx, cursor) device arguments of a label mode and the rows' labels y."""
    lab, rows = _label_data(M)
    if mode == "staged":
        y = lab[rows[1]]
        return torch.from_numpy(y).to(DEV), None, None, y
    idx = torch.from_numpy(rows.reshape(-1)).to(DEV)
    if mode == "idx":
        return torch.from_numpy(lab).to(DEV), idx, None, lab[rows[0]]
    return torch.from_numpy(lab).to(DEV), idx, torch.ones(1, dtype=torch.int64, device=DEV), lab[rows[1]]


def _head64(h, w, b, z, y, act, loss):
    """fp64 head: row loss terms, dlogits, dh, dWh, dbh, predictions."""
    M = h.shape[0]
    h64, w64 = h.astype(np.float64), w.astype(np.float64)
    onehot = np.eye(10)[y]
    if loss == "mse":
        t = z - onehot
        terms = (t ** 2).sum(1)
        dl = t * (2.0 * GS / (M * 10))
    else:
        mx = z.max(1, keepdims=True)
        lse = mx + np.log(np.exp(z - mx).sum(1, keepdims=True))
        terms = lse[:, 0] - z[np.arange(M), y]
        dl = (np.exp(z - lse) - onehot) * (GS / M)
    a = _act64(h64, act)
    dh = _dact64(dl @ w64.T, h64, act)
    return dict(terms=terms, dl=dl, dh=dh, dw=a.T @ dl, db=dl.sum(0), pred=z.argmax(1),
                corr=(z.argmax(1) == y).astype(np.int64))


def _close(what, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = float(np.abs(got - ref).max()), _bound(ref)
    print(f"  {what}: err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (what, err, bound)


def _checked_inputs(K, M, act):
    h, w, b, z, gap = _inputs(K, M, act)
    assert gap > 1e-3 * np.abs(z).max(), "no seed with every row's top-two gap above 1e-3 * max|logit|"
    return h, w, b, z


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _advance(mode):
    """(adv_cursor tensor or None, wrap, expected value after the launch)."""
    if mode == "none":
        return None, 0, None
    adv = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    return (adv, 3, 0) if mode == "wrap" else (adv, 9, 3)


def _lib():
    from cloud_server_amd.ops import fused as F
    return F, F.load(required=True)


# ------------------------------------------------------------------------------ csa_head_row
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("act", IN_ACTS)
@pytest.mark.parametrize("K", ROW_K)
def test_head_row_matches_fp64(K, act, loss):
    F, lib = _lib()
    for M in ROW_M:
        assert lib.csa_head_row_ok(M, K) == 1
        h, w, b, z = _checked_inputs(K, M, act)
        hd, wd, bd = _dev(h, w, b)
        for lmode in ("staged", "idx", "idx+cursor"):
            labels, idx, cursor, y = _labels(M, lmode)
            ref = _head64(h, w, b, z, y, act, loss)
            for amode in ("none", "keep", "wrap"):
                adv, wrap, adv_after = _advance(amode)
                dh = torch.full((M, K), SENT, device=DEV)
                dl = torch.full((M, 10), SENT, device=DEV)
                rloss = torch.full((M,), SENT, device=DEV)
                rcorr = torch.full((M,), int(SENT), dtype=torch.int32, device=DEV)
                step = torch.full((1,), STEP0, dtype=torch.int64, device=DEV)
                rc = lib.csa_head_row(F.ptr(hd), M, K, ACTS[act], 0.0, F.ptr(wd), F.ptr(bd), F.ptr(labels), F.ptr(idx),
                                      F.ptr(cursor), int(loss == "mse"), GS, F.ptr(dh), F.ptr(dl), F.ptr(rloss),
                                      F.ptr(rcorr), F.ptr(step), F.ptr(adv), wrap, F.stream())
                assert rc == 0
                torch.cuda.synchronize()
                print(f"head_row K={K} M={M} {act}/{loss} labels={lmode} advance={amode}")
                _close("dh", dh.cpu().numpy(), ref["dh"])
                _close("dl", dl.cpu().numpy(), ref["dl"])
                _close("rloss", rloss.cpu().numpy(), ref["terms"])
                assert (rcorr.cpu().numpy() == ref["corr"]).all()
                assert int(step.item()) == STEP0 + 1
                if adv is not None:
                    assert int(adv.item()) == adv_after
                if cursor is not None:
                    assert int(cursor.item()) == 1


def test_head_row_refuses_odd_k():
    F, lib = _lib()
    M, K = 5, 7
    assert lib.csa_head_row_ok(M, K) == 0
    hd = torch.zeros(M, K, device=DEV)
    wd, bd = torch.zeros(K, 10, device=DEV), torch.zeros(10, device=DEV)
    labels = torch.zeros(M, dtype=torch.int64, device=DEV)
    out = torch.full((M * K + M * 10 + M,), SENT, device=DEV)
    rcorr = torch.full((M,), int(SENT), dtype=torch.int32, device=DEV)
    step = torch.full((1,), STEP0, dtype=torch.int64, device=DEV)
    rc = lib.csa_head_row(F.ptr(hd), M, K, 0, 0.0, F.ptr(wd), F.ptr(bd), F.ptr(labels), None, None, 0, GS,
                          F.ptr(out), F.ptr(out[M * K:]), F.ptr(out[M * K + M * 10:]), F.ptr(rcorr), F.ptr(step),
                          None, 0, F.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert (out == SENT).all() and (rcorr == int(SENT)).all() and int(step.item()) == STEP0


# ---------------------------------------------------------------------------- csa_head_dgrad
@functools.lru_cache(maxsize=None)
def _dense_inputs(Kh, K1, M):
    """The last dense layer's weight [K1][Kh] and its pre-transform input [M][K1]."""
    rng = np.random.default_rng(500000 + 1000 * Kh + 10 * K1 + M)
    W = (rng.standard_normal((K1, Kh)) / np.sqrt(Kh)).astype(np.float32)
    x = rng.standard_normal((M, K1)).astype(np.float32)
    return W, x


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("act", IN_ACTS)
@pytest.mark.parametrize("Kh", DG_KH)
def test_head_dgrad_matches_fp64(Kh, act, loss):
    F, lib = _lib()
    for M in DG_M:
        h, w, b, z = _checked_inputs(Kh, M, act)
        hd, wd, bd = _dev(h, w, b)
        # the label and advance modes rotate over the (K1, dense act) grid
        modes = [(lm, am) for lm in ("staged", "idx", "idx+cursor") for am in ("none", "keep", "wrap")]
        for n, (K1, dact) in enumerate((k1, da) for k1 in DG_K1 for da in ("none", "relu", "leaky")):
            assert lib.csa_head_dgrad_ok(M, Kh, K1) == 1
            lmode, amode = modes[n % len(modes)]
            labels, idx, cursor, y = _labels(M, lmode)
            adv, wrap, adv_after = _advance(amode)
            ref = _head64(h, w, b, z, y, act, loss)
            W, x = _dense_inputs(Kh, K1, M)
            dX64 = _dact64(ref["dh"] @ W.astype(np.float64).T, x.astype(np.float64), dact)
            Wd, xd = _dev(W, x)
            dh = torch.full((M, Kh), SENT, device=DEV)
            dl = torch.full((M, 10), SENT, device=DEV)
            rloss = torch.full((M,), SENT, device=DEV)
            rcorr = torch.full((M,), int(SENT), dtype=torch.int32, device=DEV)
            dX = torch.full((M, K1), SENT, device=DEV)
            step = torch.full((1,), STEP0, dtype=torch.int64, device=DEV)
            rc = lib.csa_head_dgrad(F.ptr(hd), M, Kh, ACTS[act], 0.0, F.ptr(wd), F.ptr(bd), F.ptr(labels), F.ptr(idx),
                                    F.ptr(cursor), int(loss == "mse"), GS, F.ptr(dh), F.ptr(dl), F.ptr(rloss),
                                    F.ptr(rcorr), F.ptr(step), F.ptr(adv), wrap, F.ptr(Wd), K1, F.ptr(xd),
                                    ACTS[dact], LEAKY if dact == "leaky" else 0.0, F.ptr(dX), F.stream())
            assert rc == 0
            torch.cuda.synchronize()
            print(f"head_dgrad Kh={Kh} K1={K1} M={M} {act}/{loss} dense={dact} labels={lmode} advance={amode}")
            _close("dh", dh.cpu().numpy(), ref["dh"])
            _close("dl", dl.cpu().numpy(), ref["dl"])
            _close("rloss", rloss.cpu().numpy(), ref["terms"])
            _close("dX", dX.cpu().numpy(), dX64)
            assert (rcorr.cpu().numpy() == ref["corr"]).all()
            assert int(step.item()) == STEP0 + 1
            if adv is not None:
                assert int(adv.item()) == adv_after


def test_head_dgrad_refuses_kh_not_multiple_of_64():
    F, lib = _lib()
    M, Kh, K1 = 4, 100, 17
    assert lib.csa_head_dgrad_ok(M, Kh, K1) == 0
    hd, wd, bd = torch.zeros(M, Kh, device=DEV), torch.zeros(Kh, 10, device=DEV), torch.zeros(10, device=DEV)
    Wd, xd = torch.zeros(K1, Kh, device=DEV), torch.zeros(M, K1, device=DEV)
    labels = torch.zeros(M, dtype=torch.int64, device=DEV)
    outs = [torch.full(s, SENT, device=DEV) for s in ((M, Kh), (M, 10), (M,), (M, K1))]
    rcorr = torch.full((M,), int(SENT), dtype=torch.int32, device=DEV)
    step = torch.full((1,), STEP0, dtype=torch.int64, device=DEV)
    rc = lib.csa_head_dgrad(F.ptr(hd), M, Kh, 0, 0.0, F.ptr(wd), F.ptr(bd), F.ptr(labels), None, None, 0, GS,
                            F.ptr(outs[0]), F.ptr(outs[1]), F.ptr(outs[2]), F.ptr(rcorr), F.ptr(step), None, 0,
                            F.ptr(Wd), K1, F.ptr(xd), 0, 0.0, F.ptr(outs[3]), F.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert all(bool((o == SENT).all()) for o in outs) and (rcorr == int(SENT)).all() and int(step.item()) == STEP0


# ---------------------------------------------------------------------------- csa_head_part2
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("act", IN_ACTS)
@pytest.mark.parametrize("K", PART_K)
def test_head_part2_matches_fp64(K, act, loss):
    F, lib = _lib()
    stride = (K * 10 + 10 + 3) & ~3
    for M, lmode, amode in zip(PART_M, ("staged", "idx+cursor", "idx", "staged"), ("wrap", "none", "keep", "keep")):
        rg = int(lib.csa_head_part_rows(M, K))
        assert rg == (8 if M == 65 else 4)
        G = (M + rg - 1) // rg
        h, w, b, z = _checked_inputs(K, M, act)
        hd, wd, bd = _dev(h, w, b)
        labels, idx, cursor, y = _labels(M, lmode)
        adv, wrap, adv_after = _advance(amode)
        ref = _head64(h, w, b, z, y, act, loss)
        dh = torch.full((M, K), SENT, device=DEV)
        part = torch.full((G, stride), SENT, device=DEV)
        mpart = torch.full((G,), SENT, device=DEV)
        mcorr = torch.full((G,), int(SENT), dtype=torch.int32, device=DEV)
        logits = torch.full((M, 10), SENT, device=DEV)
        step = torch.full((1,), STEP0, dtype=torch.int64, device=DEV)
        rc = lib.csa_head_part2(F.ptr(hd), M, K, ACTS[act], 0.0, F.ptr(wd), F.ptr(bd), F.ptr(labels), F.ptr(idx),
                                F.ptr(cursor), int(loss == "mse"), GS, F.ptr(dh), F.ptr(part), F.ptr(mpart),
                                F.ptr(mcorr), F.ptr(logits), F.ptr(step), F.ptr(adv), wrap, F.stream())
        assert rc == 0
        torch.cuda.synchronize()
        print(f"head_part2 K={K} M={M} (groups of {rg}) {act}/{loss} labels={lmode} advance={amode}")
        _close("dh", dh.cpu().numpy(), ref["dh"])
        _close("logits_out", logits.cpu().numpy(), z)
        p = part.cpu().numpy().astype(np.float64)
        assert (p[:, K * 10 + 10:] == SENT).all()            # the padding of a part row is nobody's
        _close("dWh (part rows summed)", p[:, :K * 10].sum(0).reshape(K, 10), ref["dw"])
        _close("dbh (part rows summed)", p[:, K * 10:K * 10 + 10].sum(0), ref["db"])
        grp = np.arange(M) // rg
        _close("mpart", mpart.cpu().numpy(), np.bincount(grp, ref["terms"], G))
        assert (mcorr.cpu().numpy() == np.bincount(grp, ref["corr"], G)).all()
        assert int(step.item()) == STEP0 + 1
        if adv is not None:
            assert int(adv.item()) == adv_after


# ---------------------------------------------------------------------------------- csa_head
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("act", IN_ACTS)
@pytest.mark.parametrize("path", list(HEAD_PATHS))
def test_head_matches_fp64(path, act, loss):
    """The row-group MFMA kernel, and the generic kernel by shape (K % 4) and by the
    deterministic flag.  The generic kernel stores dw / db, the row-group kernel accumulates
    into them: a second launch onto the first's results tells which one ran."""
    F, lib = _lib()
    K, Ms, det = HEAD_PATHS[path]
    RING = 4
    prev = int(lib.csa_deterministic())
    lib.csa_set_deterministic(det)
    try:
        for M, lmode in zip(Ms, ("idx+cursor", "idx", "idx+cursor")):
            h, w, b, z = _checked_inputs(K, M, act)
            hd, wd, bd = _dev(h, w, b)
            labels, idx, cursor, y = _labels(M, lmode)
            ref = _head64(h, w, b, z, y, act, loss)
            dw, db = torch.zeros(K, 10, device=DEV), torch.zeros(10, device=DEV)
            dh = torch.full((M, K), SENT, device=DEV)
            logits = torch.full((M, 10), SENT, device=DEV)
            ring_loss = torch.full((RING,), SENT, device=DEV)
            ring_correct = torch.full((RING,), int(SENT), dtype=torch.int32, device=DEV)
            step = torch.full((1,), STEP0, dtype=torch.int64, device=DEV)
            ws = torch.zeros(4, dtype=torch.int32, device=DEV)

            def launch():
                rc = lib.csa_head(F.ptr(hd), M, K, ACTS[act], 0.0, F.ptr(wd), F.ptr(bd), F.ptr(labels), F.ptr(idx),
                                  int(loss == "mse"), GS, F.ptr(dw), F.ptr(db), F.ptr(dh), F.ptr(logits), F.ptr(step),
                                  F.ptr(ring_loss), F.ptr(ring_correct), RING, F.ptr(cursor), F.ptr(ws), F.stream())
                assert rc == 0
                torch.cuda.synchronize()

            launch()
            print(f"head[{path}] K={K} M={M} {act}/{loss} labels={lmode}")
            dw1, db1 = dw.clone(), db.clone()
            _close("dw", dw.cpu().numpy(), ref["dw"])
            _close("db", db.cpu().numpy(), ref["db"])
            _close("dh", dh.cpu().numpy(), ref["dh"])
            _close("logits_out", logits.cpu().numpy(), z)
            pos = STEP0 % RING
            mean = ref["terms"].sum() / (M * 10 if loss == "mse" else M)
            _close("ring_loss", ring_loss[pos:pos + 1].cpu().numpy(), np.asarray([mean]))
            assert int(ring_correct[pos].item()) == int(ref["corr"].sum())
            keep = [i for i in range(RING) if i != pos]
            assert (ring_loss[keep] == SENT).all() and (ring_correct[keep] == int(SENT)).all()
            assert int(step.item()) == STEP0 + 1
            assert (ws == 0).all()
            launch()
            assert int(step.item()) == STEP0 + 2
            if path == "rows":
                _close("dw accumulated twice", dw.cpu().numpy(), 2.0 * ref["dw"])
                _close("db accumulated twice", db.cpu().numpy(), 2.0 * ref["db"])
            else:
                assert torch.equal(dw, dw1) and torch.equal(db, db1)
    finally:
        lib.csa_set_deterministic(prev)
