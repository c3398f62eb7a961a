"""bmp_eval_append on the GPU: batches appended at the device-side cursor equal torch.cat of their sources bit for bit (dword and
16-byte paths, aligned and not), a batch that does not fit sets the overflow word and writes nothing, and ONE captured launch
lands one block behind the other over three replays."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_ops import dev               # noqa: E402

SENTINEL = -12345.0


def _bits(x):
    return x.contiguous().view(torch.int32)


def _append_c(srcs, lab, loss, dsts, lab_dst, loss_slots, words, cap_rows, cap_batches, B):
    """The C entry directly: srcs / dsts lists of up to 4 tensors (None: absent), words = {rows, batches, overflow}."""
    from bmp import _lib
    P4, I4 = ctypes.c_void_p * 4, ctypes.c_int * 4
    pad = lambda xs: list(xs) + [None] * (4 - len(xs))
    src = P4(*[None if s is None else s.data_ptr() for s in pad(srcs)])
    dst = P4(*[None if d is None else d.data_ptr() for d in pad(dsts)])
    width = I4(*[0 if s is None else s.shape[1] for s in pad(srcs)])
    rc = _lib.lib().bmp_eval_append(src, width, _lib.ptr(lab), 0 if lab is None else lab.shape[1], _lib.ptr(loss), B, dst,
                                    _lib.ptr(lab_dst), _lib.ptr(loss_slots), words.data_ptr(), cap_rows, cap_batches,
                                    words.data_ptr() + 8, _lib.stream())
    _lib.check(rc, "bmp_eval_append")


def _batches(C, sizes=(5, 1, 4), seed=0):
    g = torch.Generator().manual_seed(seed + C)
    out = []
    for B in sizes:
        y = torch.randn(B, C, generator=g)
        y.view(-1)[0] = -0.0                       # (bit for bit: a copy that went through arithmetic would lose the sign)
        out.append(dict(y=y.to(dev()), t=torch.randint(-1, 2, (B, C), generator=g, dtype=torch.int32).to(dev()),
                        loss=torch.randn((), generator=g).to(dev()), g1=torch.randn(B, 4, generator=g).to(dev()),
                        g2=torch.randn(B, 20, generator=g).to(dev())))
    return out


@pytest.mark.parametrize("C", [1, 3, 37])
def test_appended_batches_equal_the_concatenation(C):
    """C = 1, 3 and 37 (the multi-class label count): dword copies, and a destination offset that is no multiple of 16 bytes
    after the first batch of 5 rows; the representation blocks of 4 and 20 columns: 16-byte copies, aligned at every cursor."""
    from bmp.trainer import ScoreSink
    bs = _batches(C)
    sink = ScoreSink(dev(), cap_rows=10, cap_batches=3, label_cols=C, widths=(4, 20))
    for b in bs:
        sink.append(b["y"], b["t"], b["loss"], b["g1"], b["g2"])
    cat = lambda k: torch.cat([b[k] for b in bs])
    assert sink.words.tolist() == [10, 3, 0]
    assert torch.equal(_bits(sink.logits), _bits(cat("y"))) and torch.equal(sink.labels, cat("t"))
    assert torch.equal(_bits(sink.reps[0]), _bits(cat("g1"))) and torch.equal(_bits(sink.reps[1]), _bits(cat("g2")))
    assert torch.equal(sink.loss, torch.stack([b["loss"] for b in bs]))
    res = sink.finish()
    assert np.array_equal(res["logits"], cat("y").cpu().numpy()) and np.array_equal(res["labels"], cat("t").cpu().numpy())
    assert np.array_equal(res["prob"], torch.sigmoid(cat("y")).cpu().numpy())
    assert np.array_equal(res["loss"], torch.stack([b["loss"] for b in bs]).cpu().numpy())
    assert np.array_equal(res["g1"], cat("g1").cpu().numpy()) and np.array_equal(res["g2"], cat("g2").cpu().numpy())
    sink.reset()
    assert sink.words.tolist() == [0, 0, 0] and (sink.rows, sink.batches) == (0, 0)


def test_a_source_or_destination_off_16_bytes_takes_the_dword_path():
    """A width of 4 with the source one float into its allocation, and with the destination one float into its own: neither
    may be copied 16 bytes at a time.  Guard floats around the destination stay as they were."""
    B, w = 6, 4
    store = torch.randn(B * w + 1, device=dev())
    src_off = store[1:].view(B, w)
    src_al = torch.randn(B, w, device=dev())
    room = torch.full((1 + 2 * B * w + 8,), SENTINEL, device=dev())
    dst_off = room[1:1 + 2 * B * w].view(2 * B, w)
    assert src_off.data_ptr() % 16 == 4 and dst_off.data_ptr() % 16 == 4 and src_al.data_ptr() % 16 == 0
    words = torch.zeros(3, dtype=torch.int32, device=dev())
    _append_c([src_off], None, None, [dst_off], None, None, words, 2 * B, 2, B)
    _append_c([src_al], None, None, [dst_off], None, None, words, 2 * B, 2, B)
    assert words.tolist() == [2 * B, 2, 0]
    assert torch.equal(_bits(dst_off), _bits(torch.cat([src_off, src_al])))
    assert float(room[0]) == SENTINEL and bool((room[1 + 2 * B * w:] == SENTINEL).all())


def test_a_batch_that_does_not_fit_sets_the_overflow_word_and_writes_nothing():
    """cap_rows = 9 inside buffers of 9 + 7 rows filled with a sentinel: 5 and 1 rows fit, 4 more do not.  Through the C entry,
    since ScoreSink refuses on the host first.  Everything happens inside the test's own allocations."""
    C, cap, guard = 3, 9, 7
    bs = _batches(C)
    mk = lambda w, dt=torch.float32: torch.full((cap + guard, w), SENTINEL, dtype=dt, device=dev())
    dsts, lab_dst, slots = [mk(C), mk(4), mk(20)], mk(C, torch.int32), torch.full((3 + guard,), SENTINEL, device=dev())
    words = torch.zeros(3, dtype=torch.int32, device=dev())
    for b in bs:
        _append_c([b["y"], b["g1"], b["g2"]], b["t"], b["loss"], dsts, lab_dst, slots, words, cap, 3, len(b["y"]))
    assert words.tolist() == [6, 2, 1]
    for d, k in zip(dsts, ("y", "g1", "g2")):
        assert torch.equal(_bits(d[:6]), _bits(torch.cat([b[k] for b in bs[:2]])))
        assert bool((d[6:] == SENTINEL).all())
    assert torch.equal(lab_dst[:6], torch.cat([b["t"] for b in bs[:2]])) and bool((lab_dst[6:] == int(SENTINEL)).all())
    assert torch.equal(slots[:2], torch.stack([b["loss"] for b in bs[:2]])) and bool((slots[2:] == SENTINEL).all())
    # the batch count has a guard of its own: rows would fit, a third batch would not
    words.zero_()
    for b in bs[:2] + bs[1:2]:
        _append_c([b["y"]], None, b["loss"], dsts[:1], None, slots, words, cap + guard, 2, len(b["y"]))
    assert words.tolist() == [6, 2, 1] and bool((dsts[0][6:] == SENTINEL).all()) and bool((slots[2:] == SENTINEL).all())


def test_finish_raises_on_the_overflow_word():
    from bmp.trainer import ScoreSink
    sink = ScoreSink(dev(), cap_rows=4, cap_batches=2, label_cols=1)
    sink.append(torch.zeros(2, 1, device=dev()), torch.zeros(2, 1, dtype=torch.int32, device=dev()))
    sink.words[2] = 1
    with pytest.raises(RuntimeError, match="overflow"):
        sink.finish()


def test_one_captured_append_lands_block_after_block():
    """The launch is recorded once from fixed source tensors; the sources are overwritten between three replays."""
    from bmp.trainer import ScoreSink
    B, C = 5, 3
    y, t = torch.zeros(B, C, device=dev()), torch.zeros(B, C, dtype=torch.int32, device=dev())
    g1, g2, loss = torch.zeros(B, 4, device=dev()), torch.zeros(B, 20, device=dev()), torch.zeros((), device=dev())
    sink = ScoreSink(dev(), cap_rows=3 * B, cap_batches=3, label_cols=C, widths=(4, 20))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sink.launch(y, t, loss, g1, g2)                                   # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(s)
    sink.words.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sink.launch(y, t, loss, g1, g2)
    bs = _batches(C, sizes=(B, B, B), seed=9)
    for b in bs:
        y.copy_(b["y"]); t.copy_(b["t"]); g1.copy_(b["g1"]); g2.copy_(b["g2"]); loss.copy_(b["loss"])
        sink.reserve(B, True)
        graph.replay()
    res = sink.finish()
    cat = lambda k: torch.cat([b[k] for b in bs]).cpu().numpy()
    assert np.array_equal(res["logits"], cat("y")) and np.array_equal(res["labels"], cat("t"))
    assert np.array_equal(res["g1"], cat("g1")) and np.array_equal(res["g2"], cat("g2"))
    assert np.array_equal(res["loss"], torch.stack([b["loss"] for b in bs]).cpu().numpy())
