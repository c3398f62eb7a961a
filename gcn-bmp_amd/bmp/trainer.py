"""Minimal trainer / evaluator counterpart of what the reference's scripts wire up around the
hot path with chainer.training (train_binary.py:530-665, train_ddi_modify.py:280-380):

* ``evaluate``: BatchEvaluator semantics (training/extensions/batch_evaluator.py:49-100): logits of the whole
  iterator under no-backprop, sigmoid, then ROC-AUC / PRC-AUC / accuracy / F1 on the host with the definitions of
  training/extensions/{roc_auc,prc_auc,acc,f1}_evaluator.py (labels equal to ``ignore_label`` are left out);
* ``ExponentialShift`` of Adam's alpha at manually scheduled epochs (train_binary.py:636-646);
* ``EarlyStopping`` = triggers.EarlyStoppingTrigger(monitor='validation/main/loss', patients=50,
  max_trigger=(500, 'epoch')) (train_binary.py:558);
* ``augment_pairs``: the pair swap of augment_dataset (train_binary.py:285-294) on index arrays;
* ``PairBatches``: SerialIterator + the converter concat_mols (train_binary.py:520-528, 551) over a pair list and a drug store
  resident in HBM: every batch collated on the device, in the per-instance layout or in the encoder layout (optionally with
  every distinct molecule of the batch encoded once), this rank's share of each global batch;
* ``fit``: StandardUpdater + the extensions above as one loop over packed batches, log entries named as the
  reference's PrintReport columns (train_binary.py:650-658).  The reference's optimizer hooks (GradientClipping, WeightDecay,
  Lasso: train_binary.py:538-543) belong to the optimizer: ``opt.add_hook(...)`` on the FlatAdam handed to ``fit``.

Metrics are plain numpy (no sklearn at run time); tests/test_trainer.py checks them against sklearn.
"""
from __future__ import annotations

import math
import time
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

SHIFT_SCHEDULES = {1: (10, 20, 30, 40, 50, 60), 2: (5, 10, 15, 20, 25, 30),
                   3: (5, 10, 15, 20, 25, 30, 40, 50, 60, 70)}          # train_binary.py:638-646


# ---- metrics (one column = one class; averaged over columns like the reference's evaluators) -------------------
def _valid(y: np.ndarray, t: np.ndarray, ignore_label):
    m = np.ones(len(t), dtype=bool) if ignore_label is None else (t != ignore_label)
    return y[m], t[m]


def roc_auc_binary(score: np.ndarray, t: np.ndarray) -> float:
    """Area under the ROC curve = Mann-Whitney statistic with average ranks for ties (sklearn.metrics.roc_auc_score)."""
    pos = t == 1
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    order = np.argsort(score, kind="mergesort")
    s = score[order]
    ranks = np.empty(len(s), dtype=np.float64)
    i = 0
    while i < len(s):                      # average ranks over runs of equal scores
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[i:j + 1] = 0.5 * (i + j) + 1.0
        i = j + 1
    r = np.empty(len(s), dtype=np.float64)
    r[order] = ranks
    return float((r[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def prc_auc_binary(score: np.ndarray, t: np.ndarray) -> float:
    """metrics.auc(recall, precision) over metrics.precision_recall_curve (prc_auc_evaluator.py:111-117): one point
    per distinct score threshold, trapezoid rule, plus the (recall 0, precision 1) end point."""
    n_pos = int((t == 1).sum())
    if n_pos == 0:
        return float("nan")
    order = np.argsort(-score, kind="mergesort")
    s, tt = score[order], (t[order] == 1).astype(np.float64)
    distinct = np.nonzero(np.diff(s))[0]
    idx = np.r_[distinct, len(s) - 1]
    tps = np.cumsum(tt)[idx]
    fps = 1 + idx - tps
    precision = tps / (tps + fps)
    recall = tps / n_pos
    last = int(np.searchsorted(tps, tps[-1]))          # sklearn stops at the first threshold with full recall
    precision = np.r_[precision[:last + 1][::-1], 1.0]
    recall = np.r_[recall[:last + 1][::-1], 0.0]
    return float(-np.trapezoid(precision, recall))


def f1_binary(pred: np.ndarray, t: np.ndarray) -> float:
    tp = float(((pred == 1) & (t == 1)).sum())
    fp = float(((pred == 1) & (t != 1)).sum())
    fn = float(((pred != 1) & (t == 1)).sum())
    return 0.0 if 2 * tp + fp + fn == 0 else 2 * tp / (2 * tp + fp + fn)


def classification_metrics(prob: np.ndarray, t: np.ndarray, ignore_label: Optional[int] = -1) -> Dict[str, float]:
    """prob = sigmoid(logits) (B, C), t (B, C) in {0, 1, ignore_label}.  Means over the classes."""
    prob = np.asarray(prob, dtype=np.float64).reshape(len(prob), -1)
    t = np.asarray(t).reshape(len(t), -1)
    roc, prc, acc, f1 = [], [], [], []
    for c in range(prob.shape[1]):
        y, tc = _valid(prob[:, c], t[:, c], ignore_label)
        pred = np.round(y)                                   # acc_evaluator.py:66
        roc.append(roc_auc_binary(y, tc)); prc.append(prc_auc_binary(y, tc))
        acc.append(float((pred == tc).mean()) if len(tc) else float("nan")); f1.append(f1_binary(pred, tc))
    return {"roc_auc": float(np.mean(roc)), "prc_auc": float(np.mean(prc)), "accuracy": float(np.mean(acc)),
            "f1": float(np.mean(f1))}


# ---- evaluation / schedule / stopping -------------------------------------------------------------------------------
# What ``evaluate(..., graphed=None, on_device=None)`` and ``fit`` do on a GPU, set by tools/eval_probe.py's figures
# (profiles/eval_probe.json): True only for what passed the adoption rule there.
# EVAL_GRAPH_DEFAULT: a set of fixed-shape batches (PairBatches(layout="static")) replays one recorded forward pass per batch
# (bmp.dp.GraphedPredict) with its scores kept on the device (ScoreSink; the pass's short remainder is appended launch by launch)
# and comes to the host in one copy.  Adopted: 0.58 -> 0.23 ms per batch of 32 on the reference's published model, 0.64 -> 0.40
# on C2, passing in four runs of four on both.
# EVAL_ON_DEVICE_DEFAULT: every other set on a GPU keeps its scores in a ScoreSink too, launch by launch.  NOT adopted: at 32
# pairs it gained less than the spreads on the published model (0.58 -> 0.56 ms) and LOST on C2 (0.64 -> 0.84 ms, in four runs of
# four); at 1024 pairs per batch it gained.  Reachable with ``on_device=True``.
EVAL_GRAPH_DEFAULT = True
EVAL_ON_DEVICE_DEFAULT = False
UNSIZED_START = (1024, 64)      # rows, batches of the sink of a set whose size nobody told; doubled between batches as needed


class ScoreSink:
    """Where the batches of one evaluated set leave their scores ON THE DEVICE: logits and int32 labels [cap_rows x label_cols],
    one float32 loss per batch [cap_batches] and, with ``widths`` = (g1 columns, g2 columns), the two molecule vectors handed to
    the link predictor.  ``append`` is one bmp_eval_append on the current stream: the rows go behind the rows appended before,
    at a cursor the kernel reads from device memory -- so an append recorded in a HIP graph (bmp.dp.GraphedPredict) lands in
    the right place at every replay.  ``finish`` is the set's ONE synchronisation and ONE copy to the host.

    The host knows the cursor without asking -- it is the sum of the batch sizes it appended -- and refuses a batch that does
    not fit before any launch; the kernel's own guard (the overflow word, which ``finish`` checks) is the second line.
    ``words`` = {rows appended, batches appended, overflow}: ``reset`` zeroes them (``words.zero_()`` is the whole reset of the
    device side)."""

    def __init__(self, device, cap_rows: int, cap_batches: int, label_cols: int, widths: Sequence[int] = ()):
        import ctypes
        if cap_rows <= 0 or cap_batches <= 0 or label_cols <= 0:
            raise ValueError("ScoreSink: cap_rows, cap_batches and label_cols must be positive")
        if len(widths) > 3 or any(int(w) <= 0 for w in widths):
            raise ValueError("ScoreSink: up to three further row blocks of positive width")
        self.device = torch.device(device)
        self.cap_rows, self.cap_batches, self.label_cols = int(cap_rows), int(cap_batches), int(label_cols)
        self.widths = tuple(int(w) for w in widths)
        kw = dict(device=self.device)
        self.logits = torch.empty(self.cap_rows, self.label_cols, dtype=torch.float32, **kw)
        self.labels = torch.empty(self.cap_rows, self.label_cols, dtype=torch.int32, **kw)
        self.loss = torch.empty(self.cap_batches, dtype=torch.float32, **kw)
        self.reps = [torch.empty(self.cap_rows, w, dtype=torch.float32, **kw) for w in self.widths]
        self.words = torch.zeros(3, dtype=torch.int32, **kw)
        blocks = [self.logits] + self.reps
        self._dst = (ctypes.c_void_p * 4)(*[b.data_ptr() for b in blocks] + [None] * (4 - len(blocks)))
        self._width = (ctypes.c_int * 4)(*[b.shape[1] for b in blocks] + [0] * (4 - len(blocks)))
        self.rows = self.batches = 0
        self.with_loss: Optional[bool] = None

    def reset(self) -> None:
        self.words.zero_()
        self.rows = self.batches = 0
        self.with_loss = None

    def fits(self, cap_rows: int, cap_batches: int, label_cols: int, representations: bool) -> bool:
        return (self.cap_rows >= cap_rows and self.cap_batches >= cap_batches and self.label_cols == label_cols
                and bool(self.widths) == bool(representations))

    def reserve(self, B: int, with_loss: bool) -> None:
        """The host's count of one more batch of ``B`` rows -- before its launch (or the replay that holds its launch)."""
        if B <= 0:
            raise ValueError("ScoreSink: an empty batch")
        if self.rows + B > self.cap_rows or self.batches + 1 > self.cap_batches:
            raise RuntimeError(f"ScoreSink: {self.rows} + {B} rows / {self.batches} + 1 batches do not fit "
                               f"{self.cap_rows} rows / {self.cap_batches} batches")
        if self.with_loss is not None and self.with_loss != with_loss:
            raise ValueError("ScoreSink: every batch of a set comes with a loss, or none does")
        self.with_loss = with_loss
        self.rows += B
        self.batches += 1

    def _block(self, x, cols: int, dtype, name: str) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.device.type != self.device.type or \
                (self.device.index is not None and x.device.index != self.device.index):
            raise ValueError(f"ScoreSink: {name} must be a tensor on {self.device}")
        x = x.reshape(len(x), -1)
        if x.shape[1] != cols:
            raise ValueError(f"ScoreSink: {name} has {x.shape[1]} columns, the sink {cols}")
        return x.to(dtype).contiguous()

    def launch(self, y, t, loss=None, g1=None, g2=None) -> None:
        """bmp_eval_append without the host's count (``reserve``): what a recording holds."""
        import ctypes
        from . import _lib
        if self.device.type != "cuda":
            raise ValueError("ScoreSink: appending needs the sink on a GPU")
        y = self._block(y, self.label_cols, torch.float32, "logits")
        B = len(y)
        t = self._block(torch.as_tensor(t), self.label_cols, torch.int32, "labels")
        reps = [g for g in (g1, g2) if g is not None]
        if len(reps) != len(self.widths) or len(t) != B:
            raise ValueError(f"ScoreSink: {len(reps)} representation blocks for a sink of {len(self.widths)}, {len(t)} label rows for {B}")
        reps = [self._block(g, w, torch.float32, "representation") for g, w in zip(reps, self.widths)]
        if any(len(g) != B for g in reps):
            raise ValueError("ScoreSink: one representation row per pair")
        if loss is not None:
            loss = self._block(loss.reshape(1, 1), 1, torch.float32, "loss")
        src = (ctypes.c_void_p * 4)(*[b.data_ptr() for b in [y] + reps] + [None] * (3 - len(reps)))
        w = self.words
        _lib.check(_lib.lib().bmp_eval_append(src, self._width, _lib.ptr(t), self.label_cols, _lib.ptr(loss), B, self._dst,
                                              _lib.ptr(self.labels), _lib.ptr(self.loss), w.data_ptr(), self.cap_rows,
                                              self.cap_batches, w.data_ptr() + 8, _lib.stream()), "bmp_eval_append")

    def append(self, y, t, loss=None, g1=None, g2=None) -> None:
        self.reserve(len(y), loss is not None)
        self.launch(y, t, loss, g1, g2)

    def grown(self, cap_rows: int, cap_batches: int) -> "ScoreSink":
        """A larger sink with this one's contents (device copies, no synchronisation): for a set whose size nobody told."""
        new = ScoreSink(self.device, max(cap_rows, self.cap_rows), max(cap_batches, self.cap_batches), self.label_cols, self.widths)
        n, nb = self.rows, self.batches
        new.logits[:n].copy_(self.logits[:n]); new.labels[:n].copy_(self.labels[:n]); new.loss[:nb].copy_(self.loss[:nb])
        for a, b in zip(new.reps, self.reps):
            a[:n].copy_(b[:n])
        new.words.copy_(self.words)
        new.rows, new.batches, new.with_loss = n, nb, self.with_loss
        return new

    def finish(self) -> Dict[str, Optional[np.ndarray]]:
        """Host arrays cut to the rows appended: logits, prob = sigmoid(logits) (taken once, on the device, over the whole
        buffer: elementwise, so a pair's probability does not depend on the batch it came in), labels, loss (one per batch, or
        None) and g1 / g2.  Everything travels as ONE tensor in ONE copy, which is the set's only synchronisation."""
        n, nb, C = self.rows, self.batches, self.label_cols
        logits = self.logits[:n]
        parts = [self.words.view(torch.float32), logits.reshape(-1), torch.sigmoid(logits).reshape(-1),
                 self.labels[:n].reshape(-1).view(torch.float32), self.loss[:nb]] + [r[:n].reshape(-1) for r in self.reps]
        host = torch.cat(parts).cpu().numpy()
        words = host[:3].view(np.int32)
        if words[2] != 0:
            raise RuntimeError("ScoreSink: a batch did not fit the buffers on the device (overflow word set)")
        if (int(words[0]), int(words[1])) != (n, nb):
            raise RuntimeError(f"ScoreSink: the device appended {int(words[0])} rows / {int(words[1])} batches, the host counted {n} / {nb}")
        out, o = {}, 3
        for name, size, shape in (("logits", n * C, (n, C)), ("prob", n * C, (n, C)), ("labels", n * C, (n, C)), ("loss", nb, (nb,))):
            out[name] = host[o:o + size].reshape(shape)
            o += size
        out["labels"] = out["labels"].view(np.int32)
        if not self.with_loss:
            out["loss"] = None
        for name, w in zip(("g1", "g2"), self.widths):
            out[name] = host[o:o + n * w].reshape(n, w)
            o += n * w
        return out


def _on_gpu(predictor, opt) -> bool:
    if opt is not None:
        return bool(opt.flat.is_cuda)
    p = next(iter(predictor.parameters()), None) if callable(getattr(predictor, "parameters", None)) else None
    return p is not None and p.is_cuda


def _set_size(batches):
    """(rows, batches) of a sized set -- a PairBatches: this rank's share is at most len(lab) -- or None."""
    lab = getattr(batches, "lab", None)
    if lab is None or not callable(getattr(batches, "__len__", None)):
        return None
    return max(len(lab), 1), max(len(batches), 1)


def _eager_scores(predictor, inputs, opt):
    """Logits and the two molecule vectors of one batch, launch by launch (a fixed-shape batch writes its arrays first)."""
    if callable(getattr(inputs, "emit", None)):
        inputs.reset_derived(); inputs.emit()
        inputs = inputs.pb
    args = tuple(inputs) if isinstance(inputs, (tuple, list)) else (inputs,)
    if opt is not None:
        y, (g1, g2) = opt.functional_predict(*args)
        return y, g1, g2
    y = predictor(*args)
    return y, getattr(predictor, "g1", None), getattr(predictor, "g2", None)


def _scores_on_device(predictor, batches: Iterable, lossfun, opt, graphed, representations: bool):
    """One pass over ``batches`` with every score left in a ScoreSink: (finish()'s dict, the batch sizes).  ``graphed``: a
    bmp.dp.GraphedPredict for the fixed-shape batches (its sink is used, or replaced by one that fits), or None."""
    size = _set_size(batches)
    sink, lens = None, []
    was_training = predictor.training
    predictor.eval()
    try:
        with torch.no_grad():
            for inputs, t in batches:
                B = len(t)
                static = callable(getattr(inputs, "emit", None))
                C = int(torch.as_tensor(t).reshape(B, -1).shape[1])
                if sink is None and graphed is not None:
                    need = size or (B, 1)
                    if graphed.sink is not None and graphed.sink.fits(need[0], need[1], C, representations):
                        sink = graphed.sink
                        sink.reset()
                if sink is not None and graphed is not None and static and sink is graphed.sink:
                    graphed(inputs, lossfun=lossfun, representations=representations)      # one replay, the append in it
                    lens.append(B)
                    continue
                y, g1, g2 = _eager_scores(predictor, inputs, opt)
                if not representations:
                    g1 = g2 = None
                elif g1 is None or g2 is None:
                    raise ValueError("representations: the model leaves no g1 / g2")
                if sink is None:             # the first batch says what a row holds
                    rows, nb = size or (max(UNSIZED_START[0], B), UNSIZED_START[1])
                    hint = getattr(graphed, "capacity_hint", None)
                    if hint is not None:
                        rows, nb = max(rows, hint[0]), max(nb, hint[1])
                    sink = ScoreSink(y.device, rows, nb, C, () if g1 is None else (g1.shape[1], g2.shape[1]))
                    if graphed is not None:
                        graphed.set_sink(sink)
                elif sink.rows + B > sink.cap_rows or sink.batches + 1 > sink.cap_batches:
                    if size is not None:
                        raise RuntimeError(f"the set yields more than its {size[0]} pairs / {size[1]} batches")
                    sink = sink.grown(2 * max(sink.cap_rows, B), 2 * sink.cap_batches)
                    if graphed is not None:
                        graphed.set_sink(sink)
                sink.append(y, t, None if lossfun is None else lossfun(y, t), g1, g2)
                lens.append(B)
    finally:
        predictor.train(was_training)
    if sink is None:
        raise ValueError("no batches")
    return sink.finish(), lens


def _graph_by_default(batches, opt, predictor) -> bool:
    """EVAL_GRAPH_DEFAULT speaks for the sets that yield fixed-shape batches, evaluated through an optimizer's flat buffer --
    unless the set itself refuses the model on that layout (``PairBatches.check_encoder``): nothing is recorded then."""
    if not (EVAL_GRAPH_DEFAULT and opt is not None and getattr(batches, "layout", None) == "static"):
        return False
    try:
        if callable(getattr(batches, "check_encoder", None)):
            batches.check_encoder(predictor)
    except NotImplementedError:
        return False
    return True


def _graphed_for(graphed, predictor, opt, batches):
    """The GraphedPredict a pass with its scores on the device runs its fixed-shape batches through, or None.  Asked for by
    keyword, what ``PairBatches.check_encoder`` refuses for the set's layout is refused here with the same reason."""
    if graphed is None:
        graphed = _graph_by_default(batches, opt, predictor)
    elif graphed is not False and callable(getattr(batches, "check_encoder", None)):
        batches.check_encoder(predictor)
    if graphed is True:
        if opt is None:
            raise ValueError("graphed evaluation runs opt.functional_predict: pass opt")
        from .dp import GraphedPredict
        return GraphedPredict(predictor, opt)
    return graphed or None


def predict_pairs(model, batches: Iterable, opt=None, representations: bool = False, graphed=None) -> Dict[str, np.ndarray]:
    """The evaluation scripts' ``predict`` over a whole set (eval_coattention.py:103-124; with ``representations`` also their
    generate_representations / add_representations: every pair's two molecule vectors, as handed to the link predictor):
    dict(logits, prob, labels[, g1, g2]) of host arrays in pair order.  On a GPU the set is ONE pass with its scores kept on the
    device (ScoreSink) and one copy to the host; fixed-shape batches replay a recorded forward pass (``graphed``: None follows
    EVAL_GRAPH_DEFAULT, a bmp.dp.GraphedPredict is reused)."""
    if _on_gpu(model, opt):
        res, _lens = _scores_on_device(model, batches, None, opt, _graphed_for(graphed, model, opt, batches), representations)
        res.pop("loss")
        return res
    if graphed is not None and graphed is not False:
        raise ValueError("graphed prediction needs a GPU")
    cols: Dict[str, list] = {"logits": [], "labels": [], "g1": [], "g2": []}
    was_training = model.training
    model.eval()
    with torch.no_grad():
        for inputs, t in batches:
            y, g1, g2 = _eager_scores(model, inputs, opt)
            cols["logits"].append(y.float().reshape(len(y), -1)); cols["labels"].append(torch.as_tensor(t).reshape(len(y), -1))
            if representations:
                cols["g1"].append(g1); cols["g2"].append(g2)
    model.train(was_training)
    out = {k: torch.cat(v).cpu().numpy() for k, v in cols.items() if v}
    out["prob"] = torch.sigmoid(torch.cat(cols["logits"])).cpu().numpy()
    return out


def evaluate(predictor, batches: Iterable, lossfun: Optional[Callable] = None, ignore_label: int = -1, opt=None, *,
             graphed=None, on_device=None) -> Dict[str, float]:
    """``batches`` yields (inputs, labels) with inputs a packed batch or the reference's tuple of four arrays.  With ``opt``
    (bmp.dp.FlatAdam) the logits come from ``opt.functional_predict``: the planned forward-only path on the flat buffer.

    ``on_device``: on a GPU, logits, labels and the per-batch losses stay on the device (ScoreSink) until ONE copy at the end of
    the set; ``graphed`` (True, or a bmp.dp.GraphedPredict to reuse: its recordings are made once) then replays one recorded
    forward pass for every fixed-shape batch.  Left at None they follow the module's switches: EVAL_GRAPH_DEFAULT sends a
    ``PairBatches(layout="static")`` through both, EVAL_ON_DEVICE_DEFAULT every other set through the sink.  The result is the
    same dict either way: the same float32 probabilities reach the metrics and the per-batch float32 losses are combined in
    batch order as before.  On CPU tensors, or with ``on_device`` off, the batches go one by one through the host as they always
    did."""
    asked = graphed is not None and graphed is not False
    if on_device is None:
        on_device = EVAL_ON_DEVICE_DEFAULT or asked or _graph_by_default(batches, opt, predictor)
    if on_device and _on_gpu(predictor, opt):
        res, lens = _scores_on_device(predictor, batches, lossfun, opt, _graphed_for(graphed, predictor, opt, batches), False)
        out = classification_metrics(res["prob"], res["labels"], ignore_label)
        if lossfun is not None:
            losses, n = 0.0, 0
            for loss_b, len_b in zip(res["loss"], lens):
                losses += float(loss_b) * len_b; n += len_b
            out["loss"] = losses / max(n, 1)
        return out
    if asked:
        raise ValueError("graphed evaluation needs a GPU and leaves its scores on the device (on_device)")
    ys, ts, losses, n = [], [], 0.0, 0
    was_training = predictor.training
    predictor.eval()
    with torch.no_grad():
        for inputs, t in batches:
            if callable(getattr(inputs, "emit", None)):          # a fixed-shape batch (PairBatches(layout="static")): write its arrays
                inputs.reset_derived(); inputs.emit()
                inputs = inputs.pb
            if opt is not None:
                y = opt.functional_predict(*inputs)[0] if isinstance(inputs, (tuple, list)) else opt.functional_predict(inputs)[0]
            else:
                y = predictor(*inputs) if isinstance(inputs, (tuple, list)) else predictor(inputs)
            if lossfun is not None:
                losses += float(lossfun(y, t)) * len(t); n += len(t)
            ys.append(torch.sigmoid(y).float().cpu().numpy()); ts.append(torch.as_tensor(t).cpu().numpy())
    predictor.train(was_training)
    out = classification_metrics(np.concatenate(ys), np.concatenate(ts), ignore_label)
    if lossfun is not None:
        out["loss"] = losses / max(n, 1)
    return out


class ExponentialShift:
    """extensions.ExponentialShift('alpha', rate) fired by a ManualScheduleTrigger: alpha *= rate at the listed epochs."""

    def __init__(self, optimizer, rate: float, epochs: Sequence[int], attr: str = "alpha"):
        self.opt, self.rate, self.epochs, self.attr = optimizer, rate, set(epochs), attr

    def __call__(self, epoch: int) -> float:
        if epoch in self.epochs:
            setattr(self.opt, self.attr, getattr(self.opt, self.attr) * self.rate)
        return getattr(self.opt, self.attr)


class EarlyStopping:
    """chainer.training.triggers.EarlyStoppingTrigger in 'min' mode: stop after ``patients`` checks without a new best
    value of the monitored entry, or at ``max_epoch``."""

    def __init__(self, monitor: str = "validation/main/loss", patients: int = 50, max_epoch: int = 500):
        self.monitor, self.patients, self.max_epoch = monitor, patients, max_epoch
        self.best, self.count = math.inf, 0

    def __call__(self, epoch: int, log: Dict[str, float]) -> bool:
        if epoch >= self.max_epoch:
            return True
        v = log.get(self.monitor)
        if v is None:
            return False
        if v < self.best:
            self.best, self.count = v, 0
        else:
            self.count += 1
        return self.count >= self.patients


def augment_pairs(idx1: np.ndarray, idx2: np.ndarray, label: np.ndarray):
    """augment_dataset (train_binary.py:285-294): every pair once in each order, labels repeated."""
    return np.concatenate((idx1, idx2)), np.concatenate((idx2, idx1)), np.concatenate((label, label))


class PairBatches:
    """The reference's SerialIterator(dataset, batchsize, shuffle=...) + converter concat_mols for one rank: an iterable of
    (batch, labels on the device), re-collated from the store in HBM on every pass (a new order per pass when ``shuffle``,
    like SerialIterator's per-epoch permutation; the last batch of a pass is the short remainder, as with repeat=False).

    ``layout`` "instance": bmp.packed.pack_from_store_device.  "encoder": bmp.enclayout.encode_from_store_device (encoder
    tiles balanced over the CUs); with ``dedup`` every distinct molecule of this rank's share is encoded once and its atom
    states are copied to the instances -- the same logits and gradients, fewer encoder rows.  "static": every full batch is
    loaded into ONE fixed-shape batch (bmp.packed.StaticPairBatch: the same object is yielded every time, its contents change),
    on which ``fit`` replays one recorded HIP graph per step -- the way to run small batches such as the reference's default of
    32 pairs (train_ddi_modify.py:196), where a step is ~55 launches of one workgroup round each; the short remainder of a pass
    comes as a usual packed batch.

    With ``world`` > 1 a global batch is ``batch_size * world`` pairs and this rank takes its share of it (a remainder smaller
    than ``world`` is left out, so that no rank steps on an empty batch): ``share`` "contiguous" is the slice
    [r * batch_size, (r + 1) * batch_size); "strided" is ``sel[r::world]``, the share Chainer's ``ParallelUpdater`` gives
    device r (recalled third-party behaviour).  Every full global batch gives each rank exactly
    ``batch_size`` pairs either way, so "static" serves any ``world``: ``fit`` then replays the step recorded as two graphs
    with the gradient all-reduce between them (bmp.dp.GraphedTrainStep).  The reference's ``--multi-gpu=True --batchsize 32``
    is ``batch_size=16, world=2, share="strided"`` with ``FlatAdam(..., grad_reduce="sum")``."""

    def __init__(self, dstore, idx1: np.ndarray, idx2: np.ndarray, labels: np.ndarray, batch_size: int, shuffle: bool = False,
                 seed: int = 0, layout: str = "instance", dedup: bool = False, rank: int = 0, world: int = 1,
                 share: str = "contiguous"):
        if layout not in ("instance", "encoder", "static"):
            raise ValueError(f"layout {layout!r}: 'instance', 'encoder' or 'static'")
        if share not in ("contiguous", "strided"):
            raise ValueError(f"share {share!r}: 'contiguous' or 'strided'")
        if dedup and layout != "encoder":
            raise ValueError("dedup needs layout='encoder'")
        if not (len(idx1) == len(idx2) == len(labels)):
            raise ValueError("idx1, idx2 and labels must have one entry per pair")
        self.dstore, self.i1, self.i2, self.lab = dstore, np.asarray(idx1), np.asarray(idx2), np.asarray(labels)
        self.B, self.shuffle, self.seed, self.layout, self.dedup = int(batch_size), shuffle, seed, layout, dedup
        self.rank, self.world, self.share, self.epoch = rank, world, share, 0

    def check_encoder(self, model) -> None:
        """Refuse a layout the model's encoder cannot take: with message_function='edge_network' a molecule's atom states depend
        on the padded atom count of its batch side, which the encoder layout and ``dedup`` give up (``fit`` asks before the first
        batch)."""
        enc = getattr(model, "graph_conv", model)
        reason = getattr(enc, "layout_reason", None)     # bmp.ggnn_jk: layer_aggr='attn' couples the molecules of a batch side
        if reason and self.layout in ("encoder", "static"):
            raise NotImplementedError(f"PairBatches(layout={self.layout!r}, dedup={self.dedup}): " + reason)
        reason = getattr(enc, "encoder_layout_reason", None)     # bmp.ggnn_gate: concat_hidden has no encode_rows
        if reason and self.layout == "encoder":
            raise NotImplementedError(f"PairBatches(layout='encoder', dedup={self.dedup}): " + reason)
        if getattr(enc, "message_function", None) != "edge_network":
            return
        if self.layout == "encoder":
            from .ggnn import EDGE_NETWORK_LAYOUT_REASON
            raise NotImplementedError(f"PairBatches(layout='encoder', dedup={self.dedup}): " + EDGE_NETWORK_LAYOUT_REASON)
        if self.layout == "static":
            raise NotImplementedError("PairBatches(layout='static'): the recorded step is not built for message_function='edge_network'")

    def __len__(self) -> int:
        g = self.B * self.world
        full, rem = divmod(len(self.lab), g)
        return full + (1 if rem >= self.world else 0)

    def selections(self):
        """This pass's pair indices, one array per batch of this rank (advances the pass counter)."""
        n, g = len(self.lab), self.B * self.world
        order = np.random.RandomState(self.seed + self.epoch).permutation(n) if self.shuffle else np.arange(n)
        self.epoch += 1
        for lo in range(0, n, g):
            sel = order[lo:lo + g]
            if len(sel) < self.world:
                break
            if self.share == "strided":
                yield sel[self.rank::self.world]
                continue
            q, r = divmod(len(sel), self.world)          # ranks 0..r-1 take one pair more: no rank is left without pairs
            a = self.rank * q + min(self.rank, r)
            yield sel[a:a + q + (1 if self.rank < r else 0)]

    def __iter__(self):
        from . import enclayout, packed
        for sel in self.selections():
            sides, lab = [self.i1[sel], self.i2[sel]], self.lab[sel]
            if self.layout == "static" and len(sel) == self.B:
                if getattr(self, "_static", None) is None:
                    self._static = packed.StaticPairBatch(self.dstore, self.B, label_cols=int(np.asarray(lab).reshape(len(sel), -1).shape[1]))
                self._static.load(sides, lab)
                yield self._static, self._static.t
            elif self.layout == "encoder":
                yield enclayout.encode_from_store_device(self.dstore, sides, labels=lab, dedup=self.dedup)
            else:
                yield packed.pack_from_store_device(self.dstore, sides, labels=lab)


def fit(model, opt, train_batches: Sequence, valid_batches: Sequence = (), epochs: int = 1,
        shift: Optional[ExponentialShift] = None, stopper: Optional[EarlyStopping] = None, eval_train: bool = False,
        report: Optional[Callable[[Dict[str, float]], None]] = None) -> List[Dict[str, float]]:
    """One StandardUpdater loop (train_binary.py:551-553) with bmp.dp.FlatAdam ``opt``: per batch forward, loss,
    backward, one gradient all-reduce, Adam; per epoch the evaluators, the alpha shift and the stop trigger."""
    if callable(getattr(train_batches, "check_encoder", None)):
        train_batches.check_encoder(model)
    logs: List[Dict[str, float]] = []
    t0 = time.time()
    stepper = None
    # ONE recorded forward pass per fixed-shape batch object (the train set's and the validation set's: two recordings, each
    # made once) and one score sink for all the evaluations of this call, where the module's switches allow
    replayer = None
    static = [b for b in ((train_batches,) if eval_train else ()) + (valid_batches,) if _graph_by_default(b, opt, model)]
    if static and opt.flat.is_cuda:
        from .dp import GraphedPredict
        sizes = [s for s in map(_set_size, static) if s is not None]
        replayer = GraphedPredict(model, opt)
        replayer.capacity_hint = (max(s[0] for s in sizes), max(s[1] for s in sizes)) if sizes else None     # one sink fits both sets
    replay_for = lambda b: replayer if replayer is not None and any(b is s for s in static) else None
    for epoch in range(1, epochs + 1):
        tot, n = None, 0
        for pb, t in train_batches:
            if callable(getattr(pb, "emit", None)):                 # a fixed-shape batch: the whole step is one graph replay
                if stepper is None:
                    from .dp import GraphedTrainStep
                    stepper = GraphedTrainStep(model, opt)
                loss = stepper(pb)
                tot = loss.detach() * len(t) if tot is None else tot + loss.detach() * len(t)
                n += len(t)
                continue
            if callable(getattr(model, "forward_loss", None)):      # the reference's Classifier: link predictor + loss together
                loss = opt.functional_loss(*(pb if isinstance(pb, (tuple, list)) else (pb,)), t=t)
            else:
                loss = model.loss(opt.functional_forward(pb), t)
            loss.backward()
            opt.collect_grads()
            opt.all_reduce_grads()
            opt.step()
            tot = loss.detach() * len(t) if tot is None else tot + loss.detach() * len(t)
            n += len(t)
        log = {"epoch": epoch, "main/loss": float(tot) / max(n, 1) if tot is not None else float("nan")}
        if eval_train:
            m = evaluate(model, train_batches, opt=opt, graphed=replay_for(train_batches))
            log.update({"train_acc/main/accuracy": m["accuracy"], "train_roc/main/roc_auc": m["roc_auc"],
                        "train_prc/main/prc_auc": m["prc_auc"], "train_f/main/f1": m["f1"]})
        if len(valid_batches):
            m = evaluate(model, valid_batches, lossfun=model.loss, opt=opt, graphed=replay_for(valid_batches))
            log.update({"validation/main/loss": m["loss"], "val_acc/main/accuracy": m["accuracy"],
                        "val_roc/main/roc_auc": m["roc_auc"], "val_prc/main/prc_auc": m["prc_auc"], "val_f/main/f1": m["f1"]})
        log["lr"] = shift(epoch) if shift is not None else opt.alpha
        log["elapsed_time"] = time.time() - t0
        logs.append(log)
        if report is not None:
            report(log)
        if stopper is not None and stopper(epoch, log):
            break
    return logs
