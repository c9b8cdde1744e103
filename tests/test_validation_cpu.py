"""Held-out validation during training (CPU, ``backend="torch"``): the DSL options, the
job loop's ``validation.jsonl`` against an independent NumPy fp64 computation, training
left unperturbed, the wrapped tail batch, resume, and the API route."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from cloud_server_amd.data.datasets import synthetic_mnist
from cloud_server_amd.models.dsl import SAMPLE_CONFIG, ConfigError, parse_train_config
from cloud_server_amd.runtime.trainer import RESULT, STATUS, JobRun, run_job

VALIDATION = "validation.jsonl"


def _cfg(iters=10, **options):
    c = copy.deepcopy(SAMPLE_CONFIG)
    c.update(iter=iters, learning_rate=0.01, optimizer_name="AdamOptimizer")
    c["options"] = dict(log_every=5, ckpt_every=0, **options)
    return c


@pytest.fixture(scope="module")
def data():
    return synthetic_mnist(600, seed=0).split(0.8)


def _rows(mdir):
    with open(os.path.join(mdir, VALIDATION)) as f:
        return [json.loads(line) for line in f]


def _numpy_reference(eng, test, loss_name="entropy"):
    """Loss / accuracy / confusion in NumPy fp64 from the eager model's eval-mode logits."""
    model = eng.model
    model.eval()
    with torch.no_grad():
        z = model(torch.from_numpy(test.images.astype(np.float32) / 255.0)).double().numpy()
    model.train()
    y = test.labels.astype(np.int64)
    n = len(y)
    if loss_name == "mse":
        loss = float(((z - np.eye(10)[y]) ** 2).sum() / (n * 10))
    else:
        mx = z.max(1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(z - mx).sum(1))
        loss = float((lse - z[np.arange(n), y]).sum() / n)
    pred = z.argmax(1)
    conf = np.zeros((10, 10), np.int64)
    np.add.at(conf, (y, pred), 1)
    return {"n": n, "loss": loss, "accuracy": float((pred == y).mean()), "confusion": conf.tolist()}


def _drive(job, at_steps, test):
    """run_job's loop, taking the NumPy reference whenever host_step reaches one of
    ``at_steps`` (the parameters after that many updates)."""
    refs = {}
    while job.pending():
        job.before_step()
        job.step()
        end = job.after_step()
        if job.eng.host_step in at_steps:
            refs[job.eng.host_step] = _numpy_reference(job.eng, test)
        if end:
            break
    return job.finish(), refs


def test_parse_options():
    tc = parse_train_config(_cfg())
    assert tc.eval_every == 0 and tc.eval_batch == 256
    tc = parse_train_config(_cfg(eval_every="5", eval_batch="50"))
    assert tc.eval_every == 5 and tc.eval_batch == 50
    with pytest.raises(ConfigError):
        parse_train_config(_cfg(eval_every=-1))
    for bad in (0, -3):
        with pytest.raises(ConfigError):
            parse_train_config(_cfg(eval_batch=bad))


def test_job_validation_matches_numpy(tmp_path, data):
    train, test = data
    assert len(test) == 120
    mdir = str(tmp_path / "m")
    os.makedirs(mdir)
    job = JobRun(mdir, _cfg(10, eval_every=5), device="cpu", backend="torch", data=data)
    out, refs = _drive(job, (5, 10), test)
    assert out["state"] == "done" and sorted(refs) == [5, 10]
    rows = _rows(mdir)
    assert [r["step"] for r in rows] == [5, 10]
    for r in rows:
        conf = np.asarray(r["confusion"])
        assert conf.shape == (10, 10) and conf.sum() == r["n"] == 120
        assert r["accuracy"] == np.trace(conf) / r["n"]
        ref = refs[r["step"]]
        assert r["confusion"] == ref["confusion"]
        assert r["accuracy"] == pytest.approx(ref["accuracy"], rel=1e-6)
        assert r["loss"] == pytest.approx(ref["loss"], rel=1e-6)
        assert set(r) == {"step", "n", "loss", "accuracy", "confusion", "time"}
    st = json.load(open(os.path.join(mdir, STATUS)))
    assert st["val_step"] == 10 and st["val_accuracy"] == rows[-1]["accuracy"] and st["val_loss"] == rows[-1]["loss"]


def _final_state(mdir, cfg, data):
    job = JobRun(mdir, cfg, device="cpu", backend="torch", data=data)
    out, _ = _drive(job, (), data[1])
    eng = job.eng
    return (out, eng.flat.clone(), eng.slots.clone(), [b.clone() for b in eng.model.buffers()],
            open(os.path.join(mdir, RESULT)).read())


def _step_acc(result_txt):
    out = []
    for line in result_txt.splitlines():
        if line.startswith("step"):
            parts = dict(p.split(":", 1) for p in line.split(","))
            out.append((parts["step"], parts["accuracy"]))
    return out


def test_training_not_perturbed(tmp_path, data):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(a); os.makedirs(b)
    o1, flat1, slots1, bufs1, res1 = _final_state(a, _cfg(10, eval_every=5), data)
    o2, flat2, slots2, bufs2, res2 = _final_state(b, _cfg(10), data)
    assert torch.equal(flat1, flat2) and torch.equal(slots1, slots2)
    assert len(bufs1) == len(bufs2) > 0 and all(torch.equal(x, y) for x, y in zip(bufs1, bufs2))
    assert _step_acc(res1) == _step_acc(res2) and len(_step_acc(res1)) >= 2
    assert o1["final_accuracy"] == o2["final_accuracy"]
    assert not os.path.exists(os.path.join(b, VALIDATION))


def test_tail_batch_same_result(tmp_path, data):
    """120 rows in batches of 50: the last batch holds 20 valid rows and 30 wrapped ones."""
    rows = {}
    for eb in (50, 120):
        mdir = str(tmp_path / f"m{eb}")
        os.makedirs(mdir)
        run_job(mdir, _cfg(10, eval_every=5, eval_batch=eb), device="cpu", backend="torch", data=data)
        rows[eb] = _rows(mdir)
    assert [r["step"] for r in rows[50]] == [5, 10]
    for r50, r120 in zip(rows[50], rows[120]):
        assert r50["n"] == r120["n"] == 120
        assert r50["confusion"] == r120["confusion"] and r50["accuracy"] == r120["accuracy"]
        assert r50["loss"] == pytest.approx(r120["loss"], rel=1e-6)


def test_validator_direct_and_per_class(data):
    from cloud_server_amd.runtime.engine import TrainEngine
    from cloud_server_amd.runtime.validation import TorchValidator
    train, test = data
    eng = TrainEngine(parse_train_config(_cfg(10)), train, device="cpu", backend="torch")
    for _ in range(3):
        eng.step()
    res = eng.validate(test, batch=50, predictions=True)
    assert isinstance(eng.validator(test, 50, True), TorchValidator)
    ref = _numpy_reference(eng, test)
    assert res.n == 120 and res.confusion == ref["confusion"]
    assert res.loss == pytest.approx(ref["loss"], rel=1e-6)
    conf = np.asarray(res.confusion)
    assert res.predictions.shape == (120,)
    assert (np.bincount(test.labels * 10 + res.predictions, minlength=100).reshape(10, 10) == conf).all()
    for i in range(10):
        rec, prec = res.per_class["recall"][i], res.per_class["precision"][i]
        assert rec == (conf[i, i] / conf[i].sum() if conf[i].sum() else None)
        assert prec == (conf[i, i] / conf[:, i].sum() if conf[:, i].sum() else None)


def test_resume_rows_once(tmp_path, data):
    mdir = str(tmp_path / "m")
    os.makedirs(mdir)
    run_job(mdir, _cfg(10, eval_every=5), device="cpu", backend="torch", data=data)
    first = _rows(mdir)
    assert [r["step"] for r in first] == [5, 10]
    out = run_job(mdir, _cfg(20, eval_every=5), device="cpu", backend="torch", data=data)
    assert out["step"] == 20
    rows = _rows(mdir)
    assert [r["step"] for r in rows] == [5, 10, 15, 20]
    # the re-logged row at the resume step is the same parameters: the same numbers
    assert rows[1]["confusion"] == first[1]["confusion"] and rows[1]["loss"] == first[1]["loss"]


def test_api_validation_route(tmp_path):
    from fastapi.testclient import TestClient
    from cloud_server_amd.api.app import create_app
    from cloud_server_amd.config import Settings
    pw = "Str0ng-pass-42"
    s = Settings(storage_root=str(tmp_path / "store"), db_path=str(tmp_path / "db.sqlite3"),
                 executor="inline", train_backend="torch", allow_url_fetch=True)
    app = create_app(s, executor="inline", ngpu=0, inference_device="cpu")

    def auth(c, name):
        r = c.post("/rest-auth/registration/", json={"username": name, "email": f"{name}@x.org",
                                                       "password1": pw, "password2": pw})
        assert r.status_code == 201, r.text
        r = c.post("/rest-auth/login/", json={"username": name, "password": pw})
        h = {"Authorization": "Token " + r.json()["key"]}
        return h, c.get("/rest-auth/user/", headers=h).json()["pk"]

    with TestClient(app) as c:
        ha, uid = auth(c, "alice")
        hb, _ = auth(c, "bob")
        mdir = s.model_dir(uid, "digits")
        os.makedirs(mdir)
        run_job(mdir, _cfg(10, eval_every=5), device="cpu", backend="torch",
                data=synthetic_mnist(300, seed=1).split(0.8))
        rows = _rows(mdir)
        r = c.get("/runtime/validation/digits/", headers=ha)
        assert r.status_code == 200
        body = r.json()
        assert body["every_result"] == [{"step": x["step"], "accuracy": x["accuracy"], "loss": x["loss"]}
                                        for x in rows]
        latest = body["latest"]
        assert latest["step"] == 10 and latest["n"] == 60 and latest["confusion"] == rows[-1]["confusion"]
        assert set(latest) == {"step", "n", "accuracy", "loss", "confusion", "per_class"}
        assert len(latest["per_class"]["recall"]) == len(latest["per_class"]["precision"]) == 10
        # another user's namespace holds no such model: nothing of alice's leaks
        assert c.get("/runtime/validation/digits/", headers=hb).json() == {"every_result": []}
        assert c.get("/runtime/validation/digits/").status_code == 401
        # a model without validation: the empty shape
        os.makedirs(s.model_dir(uid, "plain"))
        assert c.get("/runtime/validation/plain/", headers=ha).json() == {"every_result": []}
