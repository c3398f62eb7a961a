"""The weight-gradient GEMM family (csrc/bmp_gemm.hip: k_wgrad<MB,NB>, k_wgrad_lds with its one-hot form, wgrad_dma_body under
the three grid mappings of k_wgrad_dma_multi, the two slab reductions; the d = 32 step kernel, the NFP row-wise kernel and the
embedding table kernels next to them) at its edges, through the C ABI, against the float64 restatements of tests/wgrad_ref.py.

Every case runs twice.  INTEGER operands (entries in [-4, 4], rz and wdeg in {0, 1, 2}, integer prefills): every product and
partial sum stays below 2^24, float32 is exact in any summation order, and the result must EQUAL the reference -- a dropped
or doubled row, a wrong column skip or a wrong tile-to-problem map cannot hide in a tolerance.  GAUSSIAN operands (gda scaled
by 1e-2): within 2e-5 of the tensor's max-abs, the bound tests/test_gpu_type_rows.py and tests/test_gpu_fullsize_backward.py
already assert for these outputs, and a second call on the same inputs bit-identical (fixed-order reductions).

Every case also holds: outputs written with accumulate = 0 start as NaN; every output sits between two 64-float sentinel
borders that must survive; the workspace has exactly the size the entry's *_ws_floats reports and is followed, in the same
allocation, by a 4096-float sentinel tail that must survive; what the contract says is not read holds NaN (the G_e blocks of
rows off list e when lists are passed, the da_r columns on the first call, the columns next to a strided operand, fv in the
rows of no class), and the list entries past a count name rows off the list -- rows whose blocks are NaN."""
import pytest
import torch

import wgrad_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-5
SENT = 12345.0
BORDER, TAIL = 64, 4096
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from bmp import _lib
    return _lib.lib()


def _dev():
    return torch.device("cuda:0")


class Guarded:
    """A device tensor inside a larger allocation with a sentinel border of BORDER floats on each side."""

    def __init__(self, init):
        n = init.numel()
        self.buf = torch.full((n + 2 * BORDER,), SENT, dtype=torch.float32, device=_dev())
        self.t = self.buf[BORDER:BORDER + n].view(init.shape)
        self.t.copy_(init)

    def intact(self):
        return bool((self.buf[:BORDER] == SENT).all()) and bool((self.buf[BORDER + self.t.numel():] == SENT).all())


class Workspace:
    """Exactly `floats` floats of NaN followed, in the same allocation, by TAIL sentinel floats."""

    def __init__(self, floats):
        self.floats = int(floats)
        self.buf = torch.full((self.floats + TAIL,), SENT, dtype=torch.float32, device=_dev())
        self.buf[:self.floats] = NAN

    def intact(self):
        return bool((self.buf[self.floats:] == SENT).all())


def _operand(gen, integer, *shape, lo=-4, hi=4, scale=1.0, unit=False):
    if integer:
        return torch.randint(lo, hi + 1, shape, generator=gen).float()
    return torch.rand(*shape, generator=gen) if unit else torch.randn(*shape, generator=gen) * scale


def _prefill(gen, integer, accumulate, *shape):
    """what an output holds before the call: NaN when it is to be written, numbers when it is to be added to"""
    if not accumulate:
        return torch.full(shape, NAN)
    return _operand(gen, integer, *shape)


def _compare(got, want, integer, name):
    from parity_util import close
    got = got.detach().cpu()
    if integer:
        if not torch.equal(got.double(), want):
            bad = torch.nonzero(got.double() != want)
            raise AssertionError(f"{name}: {bad.shape[0]} of {want.numel()} elements differ from the integer reference; first at "
                                 f"{bad[0].tolist()}: got {got[tuple(bad[0])].item()}, want {want[tuple(bad[0])].item()}; "
                                 f"rows {sorted(set(bad[:, 0].tolist()))[:8]} cols {sorted(set(bad[:, -1].tolist()))[:8]}")
    else:
        close(got, want, name, tol=TOL)


def _guards_ok(outs, ws, name):
    for k, o in enumerate(outs):
        assert o.intact(), f"{name}: the border of output {k} was written"
    assert ws.intact(), f"{name}: the tail behind the workspace was written"


# ---- (a) bmp_linear_wgrad -------------------------------------------------------------------------------------------------
def _linear_once(L, N, K, Nn, integer, want_db, strided, offset=0, seed=0):
    from bmp._lib import check, ptr, stream
    g = torch.Generator().manual_seed(1000 * K + 10 * Nn + N + seed)
    ldx, c0 = (K + 12, 4 * K) if strided else (K, 0)
    ldy = c0 + Nn
    # the operands' buffers: NaN wherever the [N x K] / [N x Nn] views do not reach
    Xb = torch.full((offset + N * ldx,), NAN)
    Yb = torch.full((offset + N * ldy,), NAN)
    R.rows_view(Xb, N, K, ldx, offset).copy_(_operand(g, integer, N, K))
    R.rows_view(Yb, N, Nn, ldy, offset + c0).copy_(_operand(g, integer, N, Nn, scale=1e-2))
    want_w, want_b = R.linear_wgrad(Xb[offset:], ldx, Yb[offset + c0:], ldy, N, K, Nn, want_db)
    Xd, Yd = Xb.to(_dev()), Yb.to(_dev())
    xp, yp = Xd[offset:], Yd[offset + c0:]
    assert (xp.data_ptr() % 16 == 0) == (offset % 4 == 0)
    name = f"linear_wgrad K {K} Nn {Nn} N {N} {'int' if integer else 'gauss'} db {want_db} strided {strided} offset {offset}"
    nws = L.bmp_wgrad_ws_floats_c(N, K, Nn)
    res = []
    for _ in range(1 if integer else 2):
        dWT, db, ws = Guarded(torch.full((K, Nn), NAN)), Guarded(torch.full((Nn,), NAN)), Workspace(nws)
        check(L.bmp_linear_wgrad(ptr(xp), ldx, ptr(yp), ldy, N, K, Nn, ptr(dWT.t), ptr(db.t) if want_db else None, ptr(ws.buf), nws,
                                 stream()), "linear_wgrad")
        torch.cuda.synchronize()
        _guards_ok((dWT, db), ws, name)
        res.append((dWT.t.cpu(), db.t.cpu()))
    _compare(res[0][0], want_w, integer, name + ": dWT")
    if want_db:
        _compare(res[0][1], want_b, integer, name + ": db")
    else:
        assert bool(torch.isnan(res[0][1]).all()), name + ": a null db was written"
    if not integer:
        assert torch.equal(res[0][0], res[1][0]) and (not want_db or torch.equal(res[0][1], res[1][1])), name + ": two calls differ"


# (128, 128) is an LDS-kernel shape: N = 136, a multiple of 8 but not of 32, forces it onto the direct kernel
@pytest.mark.parametrize("K, Nn, N", [(K, Nn, N) for K, Nn in R.LINEAR_DIRECT for N in R.LINEAR_DIRECT_N] + [(128, 128, 136)])
def test_linear_wgrad_direct_kernel(L, K, Nn, N):
    for integer in (True, False):
        for want_db in (True, False):
            for strided in (False, True):
                _linear_once(L, N, K, Nn, integer, want_db, strided)


@pytest.mark.parametrize("N", R.LINEAR_LDS_N)
@pytest.mark.parametrize("K, Nn", R.LINEAR_LDS)
def test_linear_wgrad_lds_kernel(L, K, Nn, N):
    for integer in (True, False):
        for want_db in (True, False):
            for strided in (False, True):
                _linear_once(L, N, K, Nn, integer, want_db, strided)


@pytest.mark.parametrize("offset", [0, 1])
def test_linear_wgrad_same_operands_aligned_and_one_float_off(L, offset):
    """(128, 128) at N = 160: aligned the LDS kernel runs, as a one-float-offset view the direct one; both match."""
    assert R.linear_kernel(160, 128, 128, 128, 128, x_aligned=offset == 0, dy_aligned=offset == 0) == ("k_wgrad<2,2>" if offset else "k_wgrad_lds")
    for integer in (True, False):
        _linear_once(L, 160, 128, 128, integer, True, False, offset=offset, seed=7)      # the same seed: the same operands


# ---- (b) bmp_ggnn_step_wgrad ------------------------------------------------------------------------------------------------
def _step_operands(gen, integer, N, d, first, mode, rot):
    """h, m, rz, gda as the kernel gets them (NaN where the contract says unread) and the lists"""
    h, m = _operand(gen, integer, N, d), _operand(gen, integer, N, d)
    rz = _operand(gen, integer, N, 2 * d, lo=0, hi=2, unit=True)
    gda = _operand(gen, integer, N, 7 * d, scale=1e-2)
    idx = cnt = lvi = lvc = None
    counts = [min(c, N) for c in R.list_counts(N, rot)]
    # the G_e block of a row without a bond of type e: an exact zero, read as such without lists, never read with them
    tidx, tcnt = R.make_row_lists(N, counts, gen)
    for e in range(4):
        gda[~R.list_mask(tidx, tcnt, e, N), e * d:(e + 1) * d] = 0.0 if mode == "none" else NAN
    if mode != "none":
        idx, cnt = tidx, tcnt
    if mode == "type+live":
        lvi, lvc = R.make_row_lists(N, [N if rot % 2 else max(int(0.3 * N + 0.5), 1)], gen)
        off = ~R.list_mask(lvi, lvc, 0, N)
        gda[off] = torch.where(torch.isnan(gda[off]), gda[off], torch.zeros(()))      # rows of no molecule: zeros; h, m, rz finite
    if first:
        gda[:, 4 * d:5 * d] = NAN                                     # da_r: not written by the first step's backward
    return h, m, rz, gda, idx, cnt, lvi, lvc


def _step_once(L, N, d, first, accumulate, mode, integer):
    from bmp._lib import check, ptr, stream
    rot = R.case_rotation(d, first, accumulate, N, mode) if d != 32 else 0
    g = torch.Generator().manual_seed(N + 7 * d + first + 2 * accumulate + 4 * R.LIST_MODES.index(mode) + 100 * integer)
    h, m, rz, gda, idx, cnt, lvi, lvc = _step_operands(g, integer, N, d, first, mode, rot)
    shapes = ((d, 7 * d), (d, 3 * d), (d, d), (7 * d,))
    prev = tuple(_prefill(g, integer, accumulate, *s) for s in shapes)
    want = R.ggnn_step_wgrad(h, m, rz, gda, N, d, first, accumulate, prev, idx, cnt, lvi, lvc)
    if accumulate:                                                    # two accumulating calls: prefill + 2 x the sums
        want = tuple(2.0 * w - p.double() for w, p in zip(want, prev))
    dv = lambda t: None if t is None else t.to(_dev())
    hd, md, rzd, gd, idxd, cntd, lvid, lvcd = (dv(t) for t in (h, m, rz, gda, idx, cnt, lvi, lvc))
    nws = L.bmp_ggnn_step_wgrad_ws_floats(N, d)
    name = f"step_wgrad d {d} N {N} first {first} acc {accumulate} lists {mode} rot {rot} {'int' if integer else 'gauss'}"
    res = []
    for _ in range(1 if integer else 2):
        outs = [Guarded(p) for p in prev]
        ws = Workspace(nws)
        for _call in range(2 if accumulate else 1):
            check(L.bmp_ggnn_step_wgrad(ptr(hd), ptr(md), ptr(rzd), ptr(gd), N, d, first, *(ptr(o.t) for o in outs), accumulate,
                                        ptr(idxd), ptr(cntd), ptr(lvid), ptr(lvcd), ptr(ws.buf), nws, stream()), "step_wgrad")
        torch.cuda.synchronize()
        _guards_ok(outs, ws, name)
        res.append([o.t.cpu() for o in outs])
    for k, nm in enumerate(("o1", "o2", "dUcT", "cs")):
        _compare(res[0][k], want[k], integer, f"{name}: {nm}")
        if not integer:
            assert torch.equal(res[0][k], res[1][k]), f"{name}: {nm} differs between two calls"
    if first:                                                         # zeros when written, untouched when accumulating
        keep = prev if accumulate else tuple(torch.zeros(s) for s in shapes)
        o1, o2, dU, cs = res[0]
        assert torch.equal(o1[:, 4 * d:5 * d], keep[0][:, 4 * d:5 * d]) and torch.equal(o2[:, :d], keep[1][:, :d]), name
        assert torch.equal(dU, keep[2]) and torch.equal(cs[4 * d:5 * d], keep[3][4 * d:5 * d]), name


@pytest.mark.parametrize("mode", R.LIST_MODES)
@pytest.mark.parametrize("N", R.STEP_N)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("d", [64, 128])
def test_ggnn_step_wgrad(L, d, first, accumulate, N, mode):
    assert L.bmp_step_wgrad_lists_used(N, d) == 1
    for integer in (True, False):
        _step_once(L, N, d, first, accumulate, mode, integer)


@pytest.mark.parametrize("N", [8, 40, 520])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("first", [0, 1])
def test_ggnn_step_wgrad_small_kernel(L, first, accumulate, N):
    for integer in (True, False):
        _step_once(L, N, 32, first, accumulate, "none", integer)


# ---- (c) bmp_relgcn_layer_wgrad ---------------------------------------------------------------------------------------------
def _rel_once(L, N, d, accumulate, lists, integer):
    from bmp._lib import check, ptr, stream
    mode = "type" if lists else "none"
    rot = (R.case_rotation(d, 0, accumulate, N, mode) + 3 * int(integer)) % 7       # four cases per (N, mode): both runs rotate
    g = torch.Generator().manual_seed(3 * N + d + accumulate + 2 * lists + 100 * integer)
    h = _operand(g, integer, N, d)
    wdeg = _operand(g, integer, N, 4, lo=0, hi=2, unit=True)
    gda = _operand(g, integer, N, 5 * d, scale=1e-2)
    tidx, tcnt = R.make_row_lists(N, R.list_counts(N, rot), g)
    for e in range(4):
        gda[~R.list_mask(tidx, tcnt, e, N), e * d:(e + 1) * d] = NAN if lists else 0.0
    idx, cnt = (tidx, tcnt) if lists else (None, None)
    shapes = ((d, 5 * d), (4, d), (5 * d,))
    prev = tuple(_prefill(g, integer, accumulate, *s) for s in shapes)
    want = R.relgcn_layer_wgrad(h, wdeg, gda, N, d, accumulate, prev, idx, cnt)
    if accumulate:
        want = tuple(2.0 * w - p.double() for w, p in zip(want, prev))
    dv = lambda t: None if t is None else t.to(_dev())
    hd, wd, gd, idxd, cntd = (dv(t) for t in (h, wdeg, gda, idx, cnt))
    nws = L.bmp_relgcn_layer_wgrad_ws_floats(N, d)
    name = f"relgcn_wgrad d {d} N {N} acc {accumulate} lists {lists} rot {rot} {'int' if integer else 'gauss'}"
    res = []
    for _ in range(1 if integer else 2):
        outs = [Guarded(p) for p in prev]
        ws = Workspace(nws)
        for _call in range(2 if accumulate else 1):
            check(L.bmp_relgcn_layer_wgrad(ptr(hd), ptr(wd), ptr(gd), N, d, *(ptr(o.t) for o in outs), accumulate, ptr(idxd), ptr(cntd),
                                           ptr(ws.buf), nws, stream()), "relgcn_wgrad")
        torch.cuda.synchronize()
        _guards_ok(outs, ws, name)
        res.append([o.t.cpu() for o in outs])
    for k, nm in enumerate(("o1", "dbE", "cs")):
        _compare(res[0][k], want[k], integer, f"{name}: {nm}")
        if not integer:
            assert torch.equal(res[0][k], res[1][k]), f"{name}: {nm} differs between two calls"


@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("N", R.STEP_N)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("d", [64, 128])
def test_relgcn_layer_wgrad(L, d, accumulate, N, lists):
    for integer in (True, False):
        _rel_once(L, N, d, accumulate, lists, integer)


# ---- (d) bmp_nfp_layer_wgrad ------------------------------------------------------------------------------------------------
NFP_COUNTS = {
    (32, "mixed"): [1, 0, 16, 0, 1, 0, 0],
    (40, "mixed"): [0, 17, 1, 0, 16, 0, 1],
    (544, "mixed"): [0, 1, 16, 17, 33, 200, 15],
    (544, "one"): [544, 0, 0, 0, 0, 0, 0],                            # all rows in the class planned at 2 %
    (2080, "mixed"): [17, 0, 1, 1000, 16, 31, 500],
}


@pytest.mark.parametrize("N, variant, listed", [(32, "mixed", 1), (32, "mixed", 0), (544, "mixed", 1), (544, "mixed", 0), (544, "one", 1),
                                                (544, "one", 0), (2080, "mixed", 1), (2080, "mixed", 0), (40, "mixed", 1)])
@pytest.mark.parametrize("d_in, d_out", [(64, 64), (96, 72), (128, 132), (128, 256)])
def test_nfp_layer_wgrad(L, d_in, d_out, N, variant, listed):
    from bmp._lib import check, ptr, stream
    counts = NFP_COUNTS[(N, variant)]
    assert sum(counts) <= N
    for integer in (True, False):
        g = torch.Generator().manual_seed(N + d_in + d_out + listed + 100 * integer)
        fv, dpre = _operand(g, integer, N, d_in), _operand(g, integer, N, d_out, scale=1e-2)
        idx, cnt = R.make_class_lists(N, counts, g)
        on = torch.zeros(N, dtype=torch.bool)
        for k in range(R.NFP_NCLS):
            on |= R.list_mask(idx, cnt, k, N)
        fv[~on] = NAN                                                 # class-0 rows: on no list, fv never read (dpre is: dB)
        want_w, want_b = R.nfp_layer_wgrad(fv, dpre, N, d_in, d_out, idx, cnt)
        fd, pd, idxd, cntd = (t.to(_dev()) for t in (fv, dpre, idx, cnt))
        nws = L.bmp_nfp_layer_wgrad_ws_floats(N, d_in, d_out)
        name = f"nfp_wgrad {d_in}x{d_out} N {N} {variant} listed {listed} {'int' if integer else 'gauss'}"
        res = []
        for _ in range(1 if integer else 2):
            dWT, dB, ws = Guarded(torch.full((R.NFP_NCLS, d_in, d_out), NAN)), Guarded(torch.full((d_out,), NAN)), Workspace(nws)
            check(L.bmp_nfp_layer_wgrad(ptr(fd), ptr(pd), N, d_in, d_out, ptr(idxd), ptr(cntd), ptr(dWT.t), ptr(dB.t), listed, ptr(ws.buf),
                                        nws, stream()), "nfp_wgrad")
            torch.cuda.synchronize()
            _guards_ok((dWT, dB), ws, name)
            res.append((dWT.t.cpu(), dB.t.cpu()))
        _compare(res[0][0], want_w, integer, name + ": dWT")
        _compare(res[0][1], want_b, integer, name + ": dB")
        if not integer:
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), name + ": two calls differ"


# ---- (e) bmp_embed_bwd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids_kind", ["zeros", "last", "mixed"])
@pytest.mark.parametrize("N", [32, 416, 40])
@pytest.mark.parametrize("d", [4, 24, 128])
@pytest.mark.parametrize("V", [117, 130])
def test_embed_bwd(L, V, d, N, ids_kind):
    from bmp._lib import check, ptr, stream
    for integer in (True, False):
        g = torch.Generator().manual_seed(V + d + N + 100 * integer)
        ids = {"zeros": torch.zeros(N, dtype=torch.int32), "last": torch.full((N,), V - 1, dtype=torch.int32),
               "mixed": torch.randint(0, V, (N,), generator=g).int()}[ids_kind]
        assert int(ids.min()) >= 0 and int(ids.max()) < V
        dout = _operand(g, integer, N, d, scale=1e-2)
        want = R.embed_bwd(ids, dout, N, d, V)
        idsd, doutd = ids.to(_dev()), dout.to(_dev())
        nws = L.bmp_embed_bwd_ws_floats(N, d, V)
        name = f"embed_bwd V {V} d {d} N {N} ids {ids_kind} {'int' if integer else 'gauss'}"
        res = []
        for _ in range(1 if integer else 2):
            dW, ws = Guarded(torch.full((V, d), NAN)), Workspace(nws)
            check(L.bmp_embed_bwd(ptr(idsd), ptr(doutd), N, d, V, ptr(dW.t), ptr(ws.buf), nws, stream()), "embed_bwd")
            torch.cuda.synchronize()
            _guards_ok((dW,), ws, name)
            res.append(dW.t.cpu())
        _compare(res[0], want, integer, name)
        if not integer:
            assert torch.equal(res[0], res[1]), name + ": two calls differ"
