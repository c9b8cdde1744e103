"""Held-out validation during training: accuracy, loss and the confusion matrix of a test
set under the CURRENT parameters, without perturbing the training state.

Two validators produce the same ``EvalResult``:

* ``HipValidator`` — the device-resident sweep.  The test set lives in HBM as uint8 rows
  (uploaded once), a ``[n_batches, batch]`` row table addresses it (the tail wraps to the
  first rows of the set: real samples, so batch statistics under ``bn_mode == "batch"``
  never see zeros; wrapped rows are masked out of every count by ``n_total``), and a
  ``HipProgram(forward_only=True)`` built over the training engine's OWN model and flat
  parameters runs the forward.  One batch is one captured graph: the forward up to the
  head's input, then ``csa_eval_rows`` (eval.hip), which forms each row's prediction and
  loss term and advances the batch cursor.  A sweep is

      memset {cursor, arrival counter, record} -> n_batches replays -> csa_eval_finish
      -> non-blocking D2H of the record into pinned memory -> event

  with no host synchronisation inside it; ``poll()`` / ``wait()`` hand back the result.
  The head, the per-row terms and the sweep's sums are fixed-order (identical row terms
  give an identical record); the forward in front of them may still reorder fp32 sums
  between sweeps where it uses split-K or atomic statistic rows.
  The forward-only program owns its activations, statistic slabs and split-K
  accumulators, so nothing the training step expects zeroed is touched; the parameters,
  optimizer slots, BatchNorm running statistics, the training stream's cursor, ``dstep``
  and the metric rings are only ever read (or not referenced at all).
* ``TorchValidator`` — the same numbers with torch ops over the eager ``DigitNet``: the
  ``torch`` backend, CPU, data-parallel ranks, nets outside the HIP family, and the
  in-repo reference for the tests.

``make_validator`` picks between them; ``TrainEngine.validate`` is the one-call form.
"""
from __future__ import annotations

import dataclasses
from collections import deque
from types import SimpleNamespace
from typing import Any, Deque, Dict, List, Optional, Tuple

import numpy as np
import torch

from ..data.datasets import ArrayDataset

NCLS = 10


def per_class(confusion: List[List[int]]) -> Dict[str, List[Optional[float]]]:
    """Recall (row-wise) and precision (column-wise) per digit of ``conf[true][pred]``;
    ``None`` where the denominator is 0."""
    c = np.asarray(confusion, dtype=np.int64).reshape(NCLS, NCLS)
    rows, cols, diag = c.sum(1), c.sum(0), np.diag(c)
    return {"recall": [float(diag[i]) / int(rows[i]) if rows[i] else None for i in range(NCLS)],
            "precision": [float(diag[i]) / int(cols[i]) if cols[i] else None for i in range(NCLS)]}


@dataclasses.dataclass
class EvalResult:
    n: int
    accuracy: float
    loss: float                      # mean over rows (entropy) or over n * 10 (mse): models/cnn.py loss_fn
    confusion: List[List[int]]       # conf[true][pred]
    per_class: Dict[str, List[Optional[float]]]
    predictions: Optional[np.ndarray] = None

    @staticmethod
    def from_counts(n: int, confusion: np.ndarray, loss_sum: float, loss_name: str,
                    predictions: Optional[np.ndarray] = None) -> "EvalResult":
        conf = [[int(v) for v in row] for row in np.asarray(confusion).reshape(NCLS, NCLS)]
        correct = sum(conf[i][i] for i in range(NCLS))
        denom = n * NCLS if loss_name == "mse" else n
        return EvalResult(n=int(n), accuracy=correct / n if n else float("nan"),
                          loss=float(loss_sum) / denom if n else float("nan"),
                          confusion=conf, per_class=per_class(conf), predictions=predictions)


def row_table(n: int, batch: int) -> np.ndarray:
    """``[n_batches, batch]`` row indices covering 0..n-1 in order; the tail wraps to the
    first rows of the set."""
    nb = (n + batch - 1) // batch
    return (np.arange(nb * batch, dtype=np.int64) % n).reshape(nb, batch)


class _Validator:
    """Sweeps are issued with a caller's tag and handed back in issue order."""

    def __init__(self, eng, ds: ArrayDataset, batch: int, predictions: bool):
        if len(ds) == 0:
            raise ValueError("empty validation set")
        self.eng, self.n = eng, len(ds)
        self.batch = max(1, min(int(batch), self.n))
        self.loss_name = eng.cfg.loss_name
        self.want_predictions = predictions
        self.pending: Deque[Tuple[Any, ...]] = deque()

    def poll(self) -> Optional[Tuple[Any, EvalResult]]:
        """The oldest issued sweep's ``(tag, result)`` if it has finished, else None."""
        return self._pop(block=False)

    def wait(self) -> Optional[Tuple[Any, EvalResult]]:
        """Block for the oldest issued sweep; None when nothing is pending."""
        return self._pop(block=True)


class TorchValidator(_Validator):
    """The eager reference: ``DigitNet`` in eval mode over the same batches (wrapped tail
    included, so batch-statistics BatchNorm sees what the HIP sweep sees), loss terms and
    sums in float64."""

    def __init__(self, eng, ds: ArrayDataset, batch: int = 256, predictions: bool = False):
        super().__init__(eng, ds, batch, predictions)
        dev = eng.device
        self.images = torch.from_numpy(np.ascontiguousarray(ds.images)).to(dev)
        self.labels = torch.from_numpy(np.ascontiguousarray(ds.labels)).to(dev)
        self.rows = torch.from_numpy(row_table(self.n, self.batch)).to(dev)

    @torch.no_grad()
    def logits(self) -> torch.Tensor:
        """[n, 10] fp32 eval-mode logits of the set's rows, in order."""
        eng = self.eng
        eng.flush_params()
        model = eng.model
        was_training = model.training
        model.eval()
        try:
            out = []
            for b in range(self.rows.shape[0]):
                x = self.images.index_select(0, self.rows[b]).to(torch.float32).mul_(1.0 / 255.0)
                out.append(model(x))
        finally:
            model.train(was_training)
        return torch.cat(out)[:self.n]

    @torch.no_grad()
    def issue(self, tag: Any = None) -> None:
        z = self.logits().double()
        y = self.labels[:self.n].long()
        if self.loss_name == "mse":
            terms = ((z - torch.nn.functional.one_hot(y, NCLS).double()) ** 2).sum(1)
        else:
            terms = torch.logsumexp(z, dim=1) - z.gather(1, y.view(-1, 1)).view(-1)
        pred = z.argmax(1)               # first index attaining the max
        conf = torch.bincount(y * NCLS + pred, minlength=NCLS * NCLS).view(NCLS, NCLS)
        res = EvalResult.from_counts(self.n, conf.cpu().numpy(), float(terms.sum().item()), self.loss_name,
                                     pred.cpu().numpy().astype(np.int32) if self.want_predictions else None)
        self.pending.append((tag, res))

    def _pop(self, block: bool):
        return self.pending.popleft() if self.pending else None


class _FwdEngine:
    """The engine surface ``HipProgram(forward_only=True)`` reads (cf. ``serve.hip_infer``):
    the TRAINING engine's model and flat parameters (no copy), a disabled distributed
    context, and the validation set with its own row table and cursor."""

    def __init__(self, eng, B: int, images, labels, rows, cursor):
        from ..parallel.dist import DistContext
        self.cfg = dataclasses.replace(eng.cfg, batch_size=B)
        self.device, self.model, self.flat = eng.device, eng.model, eng.flat
        self.flat_grad = None
        self.ctx = DistContext(device=eng.device)
        self.data = SimpleNamespace(images=images, labels=labels)
        self.stream = SimpleNamespace(rows=rows, cursor=cursor, wrap=int(rows.shape[0]))


class HipValidator(_Validator):
    # control block, zeroed by ONE memset node per sweep: int64 cursor | int32 arrival
    # counter (+ pad) | result record {int32 n, correct, conf[100], double loss_sum}
    CTL_WORDS = 56                       # int64 words: 448 bytes, a multiple of 16

    def __init__(self, eng, ds: ArrayDataset, batch: int = 256, predictions: bool = False):
        from ..ops import fused as K
        from .hip_program import HipProgram
        super().__init__(eng, ds, batch, predictions)
        if eng.device.type != "cuda":
            raise RuntimeError("HipValidator needs a GPU device")
        dev = eng.device
        self._K = K
        with torch.cuda.device(dev):
            self.images = torch.from_numpy(np.ascontiguousarray(ds.images)).to(dev)     # uint8, uploaded once
            self.labels = torch.from_numpy(np.ascontiguousarray(ds.labels).astype(np.int64)).to(dev)
            self.rows = torch.from_numpy(row_table(self.n, self.batch)).to(dev)
            self.n_batches = int(self.rows.shape[0])
            self.ctl = torch.zeros(self.CTL_WORDS, dtype=torch.int64, device=dev)
            ctl32 = self.ctl.view(torch.int32)
            self.cursor, self.counter = self.ctl[0:1], ctl32[2:3]
            self.lib = K.load(required=True)
            self.rec_ints = int(self.lib.csa_eval_record_ints())
            assert 4 + self.rec_ints <= 2 * self.CTL_WORDS
            self.record = ctl32[4:4 + self.rec_ints]
            self.row_pred = torch.zeros(self.n, dtype=torch.int32, device=dev)
            self.row_loss = torch.zeros(self.n, dtype=torch.float32, device=dev)
            self.fwd = _FwdEngine(eng, self.batch, self.images, self.labels, self.rows, self.cursor)
            self.program = HipProgram(self.fwd, forward_only=True)          # may raise Unsupported
            hin = self.program.units[-1].y.view(self.batch, -1)
            self.Kh = int(hin.shape[1])
            wh = self.program.views["head.weight"]
            self.fused = bool(self.lib.csa_eval_rows_fused_ok(self.batch, self.Kh)) and wh.data_ptr() % 8 == 0
            self.logits = None if self.fused else torch.zeros(self.batch, NCLS, device=dev)
            self.loss_id = 1 if self.loss_name == "mse" else 0
            self.graph: Optional[torch.cuda.CUDAGraph] = None
            self._capture()

    # ---- one batch: the forward up to the head's input, then csa_eval_rows ----
    def _body(self) -> None:
        from .hip_program import _act_id, _alpha
        K, p = self._K, self.program
        with p._det_scope():
            if self.fused:
                hin = p._predict_head_input()
                rc = self.lib.csa_eval_rows(
                    K.ptr(hin), self.batch, self.Kh, _act_id(p.head_tf.act), _alpha(p.head_tf.act),
                    K.ptr(p.views["head.weight"]), K.ptr(p.views["head.bias"]), None,
                    K.ptr(self.labels), K.ptr(self.rows), K.ptr(self.cursor), self.loss_id, self.n,
                    self.n_batches, K.ptr(self.row_pred), K.ptr(self.row_loss), K.ptr(self.counter), K.stream())
            else:
                p._predict_logits_into(self.logits)
                rc = self.lib.csa_eval_rows(
                    None, self.batch, self.Kh, 0, 0.0, None, None, K.ptr(self.logits),
                    K.ptr(self.labels), K.ptr(self.rows), K.ptr(self.cursor), self.loss_id, self.n,
                    self.n_batches, K.ptr(self.row_pred), K.ptr(self.row_loss), K.ptr(self.counter), K.stream())
        if rc != 0:
            raise RuntimeError(f"csa_eval_rows failed: {rc}")

    def _capture(self) -> None:
        from ..serve.hip_infer import CAPTURE_LOCK
        from ..utils.graphs import capture
        dev = self.eng.device
        with CAPTURE_LOCK:
            s = torch.cuda.Stream(dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                self._body()                      # warm-up (lazy buffers); the sweep re-zeroes the cursor
            torch.cuda.current_stream(dev).wait_stream(s)
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with capture(g):
                self._body()
            self.graph = g

    def __del__(self):
        g, self.graph = getattr(self, "graph", None), None
        if g is not None:
            from ..serve.hip_infer import CAPTURE_LOCK
            with CAPTURE_LOCK:          # never destroyed while another thread captures
                del g

    def issue(self, tag: Any = None) -> None:
        """Enqueue one sweep on the current stream (no host synchronisation)."""
        K = self._K
        dev = self.eng.device
        with torch.cuda.device(dev):
            self.eng.flush_params()     # a carried dense update lands before the forward reads W
            self.ctl.zero_()
            for _ in range(self.n_batches):
                self.graph.replay()
            rc = self.lib.csa_eval_finish(K.ptr(self.row_pred), K.ptr(self.row_loss), K.ptr(self.labels),
                                          K.ptr(self.rows), self.n, K.ptr(self.record), K.stream())
            if rc != 0:
                raise RuntimeError(f"csa_eval_finish failed: {rc}")
            h_rec = torch.empty(self.rec_ints, dtype=torch.int32, pin_memory=True)
            h_rec.copy_(self.record, non_blocking=True)
            h_pred = None
            if self.want_predictions:
                h_pred = torch.empty(self.n, dtype=torch.int32, pin_memory=True)
                h_pred.copy_(self.row_pred, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
        self.pending.append((tag, ev, h_rec, h_pred))

    def _pop(self, block: bool):
        if not self.pending:
            return None
        tag, ev, h_rec, h_pred = self.pending[0]
        if not block and not ev.query():
            return None
        self.pending.popleft()
        ev.synchronize()
        rec = h_rec.numpy()
        n, correct = int(rec[0]), int(rec[1])
        conf = rec[2:2 + NCLS * NCLS].reshape(NCLS, NCLS)
        loss_sum = float(rec[2 + NCLS * NCLS:].view(np.float64)[0])
        if n != self.n or correct != int(np.trace(conf)):
            raise RuntimeError(f"validation record inconsistent: n={n} (expected {self.n}), correct={correct}")
        return tag, EvalResult.from_counts(n, conf, loss_sum, self.loss_name,
                                           h_pred.numpy().copy() if h_pred is not None else None)


def make_validator(eng, ds: ArrayDataset, batch: int = 256, predictions: bool = False) -> _Validator:
    """The HIP sweep for a one-process job on the HIP backend; the eager validator for the
    ``torch`` backend (requested, or fallen back to because the net is outside the HIP
    family), CPU, and for data-parallel ranks and packed hosts, which run only the final
    sweep (their final evaluation already runs eagerly; no capture beside the host's)."""
    if (eng.backend == "hip" and eng.device.type == "cuda" and not eng.ctx.enabled
            and not getattr(eng, "packed", False)):
        from .hip_program import Unsupported
        try:
            return HipValidator(eng, ds, batch, predictions)
        except Unsupported:
            pass
    return TorchValidator(eng, ds, batch, predictions)
