"""The row GEMM's forms must agree.  The launcher picks them for big launches only (n_tiles x column tiles > 256), which the
operator tests (a handful of tiles) never reach, and by operand layout, so one problem reaches each of them:
  (A) aligned operands: k_rowgemm_db (weights staged through LDS), its tile crossing to row-major for the epilogue;
  (B) as (A) with the row GEMMs' outputs at a one-float offset: k_rowgemm_db, the epilogue in accumulator layout;
  (C) as (A) with the weights at a one-float offset: the 64-row direct form (weights straight from L2).
The problem: GRU (both epilogue kinds, first and later call) and a message layer with self connection, forward and backward,
through the C ABI.  Only outputs that no later GEMM of the same call reads back are offset (the launcher rejects an unaligned
X / X2); the backward's GRU_DRH epilogue writes the library's workspace, so (B) reaches its accumulator-layout form through
its operand r instead.  Every offset operand is a view into a real allocation one 16-byte piece larger than it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
D = 72


def _at(t, off):
    """The values of ``t`` in a fresh allocation, ``off`` floats into it."""
    buf = torch.full((t.numel() + 4,), 7.0, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _run(pb, p, y_off, w_off):
    """{"gru0" | "gru1" | "msg": every output of the forward and of the backward call}.  y_off: the offset of the outputs the
    row GEMMs' epilogues write, w_off: that of the weights.  Each backward reads aligned copies of its forward's results."""
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    L = _lib.lib()
    dev = pb.device
    N, d, nt = pb.n_rows, D, pb.n_tiles
    full = lambda *s: torch.full(s, 7.0, device=dev)
    out = lambda *s: _at(full(*s), y_off)
    w = lambda t: _at(t.contiguous(), w_off)
    h, m, dy = p["h"], p["m"], p["dy"]
    # (every operand is held by a name until the calls are enqueued: a temporary freed inside an argument list could hand its
    #  block to the next argument's copy, which the stream runs BEFORE the launch that reads it)
    AT, UcT, A, Uc = w(p["AT"]), w(p["UcT"]), w(p["AT"].t()), w(p["UcT"].t())
    WT, WsT, Wnat, Ws = w(p["WT"]), w(p["WsT"]), w(p["WT"].t()), w(p["WsT"].t())
    res = {}
    for first in (True, False):
        rz = out(N, 2 * d) if first else full(N, 2 * d)        # (later calls: the candidate's GEMM reads r as X)
        c, hout = out(N, d), out(N, d)
        check(L.bmp_gru_fwd(ptr(h), ptr(m), nt, d, int(first), ptr(AT), ptr(UcT), ptr(p["b"]), ptr(rz), ptr(c), ptr(hout),
                            stream()), "bmp_gru_fwd")
        rz_a, c_a = rz.clone(), c.clone()

        def gru_bwd(rz_in):
            dh, dm = out(N, d), out(N, d)
            dAT, dUcT, db = full(2 * d, 3 * d), full(d, d), full(3 * d)
            nws = L.bmp_gru_bwd_ws_floats(nt, d)
            ws = torch.empty(nws, device=dev)
            check(L.bmp_gru_bwd(ptr(dy), ptr(h), ptr(m), ptr(rz_in), ptr(c_a), nt, d, int(first), ptr(A), ptr(Uc), ptr(dh),
                                ptr(dm), ptr(dAT), ptr(dUcT), ptr(db), 0, ptr(ws), nws, stream(), None), "bmp_gru_bwd")
            return dh, dm, dAT, dUcT, db
        dh, dm, dAT, dUcT, db = gru_bwd(rz_a)
        res[f"gru{int(first)}"] = [hout, rz, c, dh, dm, dAT, dUcT, db]
        if not first:
            # r at the offset too: the d(r*h) GEMM (GRU_DRH epilogue, writing the library's workspace) reads it in its
            # epilogue, so that epilogue leaves the row-major form as well.  (Not this call's dUcT: r is also its X, and an
            # unaligned X takes the weight-gradient kernel that reads global memory directly, another summation order.)
            rz_r = _at(rz_a, y_off)
            dh, dm, dAT, _, db = gru_bwd(rz_r)
            res["gru0_r"] = [dh, dm, dAT, db]
    agg, wdeg, y = full(N, 4 * d), full(N, 4), out(N, d)      # (agg: the GEMM's X; wdeg: read in 16-byte pieces)
    check(L.bmp_msg_fwd(ptr(h), d, nt, d, d, ptr(pb.csr_ptr), ptr(pb.csr_col), ptr(pb.csr_val), ptr(WT), ptr(p["bE"]), ptr(WsT),
                        ptr(p["bs"]), 2, ptr(agg), ptr(wdeg), ptr(y), d, stream()), "bmp_msg_fwd")
    y_a = y.clone()
    dx = full(N, d)                                            # (also written by the transposed gather, in 16-byte pieces)
    dWT, dbE, dWsT, dbs = full(4 * d, d), full(4, d), full(d, d), full(d)
    trf, trc = pb.type_rows_T(forward=True)
    nws = L.bmp_msg_bwd_ws_floats(nt, d, d)
    ws = torch.empty(nws, device=dev)
    check(L.bmp_msg_bwd(ptr(dy), d, ptr(y_a), d, 2, ptr(h), d, nt, d, d, ptr(pb.csrT_ptr), ptr(pb.csrT_col), ptr(pb.csrT_val),
                        ptr(Wnat), ptr(Ws), ptr(agg), ptr(wdeg), ptr(dx), ptr(dWT), ptr(dbE), ptr(dWsT), ptr(dbs), 0, ptr(trf),
                        ptr(trc), ptr(ws), nws, stream(), None), "bmp_msg_bwd")
    res["msg"] = [y, agg, wdeg, dx, dWT, dbE, dWsT, dbs]
    torch.cuda.synchronize()
    return {k: [t.clone() for t in v] for k, v in res.items()}


@pytest.fixture(scope="module")
def case():
    from bmp import packed, synth
    dev = torch.device("cuda:0")
    store = synth.make_store(400, seed=3, n_lo=20, n_hi=90, n_mean=60)
    rs = np.random.RandomState(0)
    pb = packed.pack_from_store(packed.MolStore(store), [rs.randint(0, 400, 330), rs.randint(0, 400, 330)], device=dev)
    assert pb.n_tiles > 256, pb.n_tiles
    N, d = pb.n_rows, D
    g = torch.Generator().manual_seed(1)
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.2).to(dev)
    p = dict(h=mk(N, d), m=mk(N, d), AT=mk(2 * d, 3 * d), UcT=mk(d, d), b=mk(3 * d), WT=mk(4 * d, d), bE=mk(4, d), WsT=mk(d, d),
             bs=mk(d), dy=torch.randn(N, d, generator=g).to(dev))
    return pb, p, _run(pb, p, 0, 0)


def test_lds_forms_equal_direct_form(case):
    pb, p, a = case
    b = _run(pb, p, 0, 1)
    assert set(a) == set(b)
    for key in a:
        for k, (x, y) in enumerate(zip(b[key], a[key])):
            scale = max(float(y.abs().max()), 1e-6)
            err = float((x - y).abs().max())
            assert err <= 2e-5 * scale, f"direct {key}[{k}]: {err:.3e} vs scale {scale:.3e}"


def test_row_major_epilogue_equals_the_accumulator_layout_one(case):
    """The same products in the same order and the same arithmetic per element: every output of the GRU (both epilogue kinds,
    first and later call), forward and backward, is IDENTICAL; the message layer's (per-bond-type bias: a sum of four products
    per element that the compiler contracts into fused multiply-adds differently in the two forms) within 1e-6 of the tensor's
    scale -- one unit in the last place."""
    pb, p, a = case
    b = _run(pb, p, 1, 0)
    assert set(a) == set(b)
    for key in a:
        for k, (x, y) in enumerate(zip(b[key], a[key])):
            if key.startswith("gru"):
                assert torch.equal(x, y), f"{key}[{k}]: max diff {float((x - y).abs().max()):.3e}"
            else:
                scale = max(float(y.abs().max()), 1e-6)
                assert float((x - y).abs().max()) <= 1e-6 * scale, f"{key}[{k}]"
