"""CPU checks of the on-device evaluation plumbing: bmp_eval_append in the header, the ctypes table and the gfx950-only library,
its argument checks, the host-side capacity check of ScoreSink, and evaluate / predict_pairs on CPU tensors (today's path)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bmp_eval_append",)


def test_header_and_ctypes_table_declare_the_entry_point():
    from bmp import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmp.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, f"{name} is not declared in include/bmp.h"
        assert name in _lib.SIGNATURES
        assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SIGNATURES[name][1]) == 14, name


def test_library_exports_it_and_is_gfx950_only():
    import __graft_entry__ as g
    g.build()
    from bmp import _lib
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name)
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx90a", b"gfx942", b"sm_"):
        assert other not in blob


def test_entry_point_checks_its_arguments_without_a_launch():
    """B <= 0, a negative width, a present source without its destination, a missing cursor or overflow word and cap_rows <= 0
    come back as argument-check codes (< -1000) -- on host pointers, so a launch would have been an error of another kind."""
    import __graft_entry__ as g
    g.build()
    from bmp import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    words = (ctypes.c_int * 3)()
    p, w = ctypes.addressof(buf), ctypes.addressof(words)
    P4, I4 = ctypes.c_void_p * 4, ctypes.c_int * 4
    src, dst, width = P4(p, None, None, None), P4(p, None, None, None), I4(1, 0, 0, 0)

    def call(src=src, width=width, B=2, dst=dst, cursor=w, cap_rows=8, cap_batches=4, overflow=w + 8, lab=None, lab_dst=None):
        return L.bmp_eval_append(src, width, lab, 1, None, B, dst, lab_dst, None, cursor, cap_rows, cap_batches, overflow, None)

    assert call(B=0) < -1000 and call(B=-3) < -1000
    assert call(width=I4(1, -1, 0, 0)) < -1000
    assert call(src=P4(p, p, None, None), width=I4(1, 4, 0, 0)) < -1000          # block 1 present, dst[1] absent
    assert call(cursor=None) < -1000 and call(overflow=None) < -1000
    assert call(cap_rows=0) < -1000 and call(cap_rows=-1) < -1000
    assert call(lab=p, lab_dst=None) < -1000                                      # labels without a place for them
    assert list(words) == [0, 0, 0]
    with pytest.raises(ValueError):
        _lib.check(call(B=0), "bmp_eval_append")


def test_score_sink_refuses_a_batch_beyond_capacity_on_the_host():
    """The host counts what it appended and refuses before any launch: on CPU tensors a launch could not even be made."""
    from bmp.trainer import ScoreSink
    sink = ScoreSink("cpu", cap_rows=4, cap_batches=2, label_cols=1)
    with pytest.raises(RuntimeError, match="do not fit"):
        sink.append(torch.zeros(5, 1), torch.zeros(5, 1, dtype=torch.int32))
    assert (sink.rows, sink.batches) == (0, 0)
    sink.reserve(3, False); sink.reserve(1, False)
    with pytest.raises(RuntimeError, match="do not fit"):                     # rows fit no longer, and neither does a third batch
        sink.reserve(1, False)
    assert (sink.rows, sink.batches) == (4, 2) and sink.words.tolist() == [0, 0, 0]
    sink.reset()
    assert (sink.rows, sink.batches) == (0, 0)
    with pytest.raises(ValueError, match="GPU"):                               # within capacity: still no launch on host memory
        sink.append(torch.zeros(2, 1), torch.zeros(2, 1, dtype=torch.int32))


class _StandIn(torch.nn.Module):
    """logits = x @ w, and the two halves of x as g1 / g2."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([[0.5], [-1.0], [0.25], [2.0]]))

    def forward(self, x):
        self.g1, self.g2 = x[:, :2], x[:, 2:]
        return x @ self.w


def _two_batches():
    rs = np.random.RandomState(4)
    x = torch.from_numpy(rs.normal(size=(5, 4)).astype(np.float32))
    t = torch.tensor([[1], [0], [-1], [1], [0]], dtype=torch.int32)
    return x, t, [((x[:3],), t[:3]), ((x[3:],), t[3:])]


def test_evaluate_on_cpu_tensors_is_todays_result():
    from bmp import trainer
    from bmp.mlp import sigmoid_cross_entropy
    x, t, batches = _two_batches()
    m = _StandIn()
    m.train()
    with torch.no_grad():
        y = torch.cat([x[:3] @ m.w, x[3:] @ m.w])        # (batch by batch, as the passes under test run it)
    want = trainer.classification_metrics(torch.sigmoid(y).numpy(), t.numpy(), -1)
    want["loss"] = (float(sigmoid_cross_entropy(y[:3], t[:3])) * 3 + float(sigmoid_cross_entropy(y[3:], t[3:])) * 2) / 5
    for kw in ({}, dict(on_device=True), dict(graphed=False, on_device=False)):       # CPU tensors: the host path whatever is asked
        got = trainer.evaluate(m, batches, lossfun=sigmoid_cross_entropy, **kw)
        assert got == want and list(got) == list(want), kw
        assert m.training
    with pytest.raises(ValueError, match="GPU"):
        trainer.evaluate(m, batches, graphed=True)
    assert trainer.EVAL_GRAPH_DEFAULT in (True, False) and trainer.EVAL_ON_DEVICE_DEFAULT in (True, False)


def test_predict_pairs_on_cpu_tensors():
    from bmp import trainer
    x, t, batches = _two_batches()
    m = _StandIn()
    with torch.no_grad():
        y = torch.cat([x[:3] @ m.w, x[3:] @ m.w])        # (batch by batch, as the passes under test run it)
    out = trainer.predict_pairs(m, batches)
    assert sorted(out) == ["labels", "logits", "prob"]
    assert np.array_equal(out["logits"], y.numpy()) and np.array_equal(out["labels"], t.numpy())
    assert np.array_equal(out["prob"], torch.sigmoid(y).numpy())
    out = trainer.predict_pairs(m, batches, representations=True)
    assert np.array_equal(out["g1"], x[:, :2].numpy()) and np.array_equal(out["g2"], x[:, 2:].numpy())
