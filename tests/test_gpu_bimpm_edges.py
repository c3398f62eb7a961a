"""k_bimpm (csrc/bmp_bimpm.hip) at its edges, against tests/bimpm_ref.py: the float64 packed-row reference FORCED to the
selections the kernel itself made (read back from the workspace of a forward launch through the C ABI,
bmp_bimpm_ws_layout), each selection first held to lie within tau of the float64 maximum (bimpm_ref.py's derivation).  A
near-tie that float32 resolves the other way is then no longer an error source, and values AND every gradient are
asserted at the project's 1e-4 -- the large molecules included.

Every case compares mol_1, mol_2, dX1, dX2, dP, dQ, dR."""
import ctypes

import numpy as np
import pytest
import torch

import bimpm_ref as BR
from parity_util import close as _close      # asserts AND logs the achieved relative error

pytestmark = pytest.mark.gpu
GRID_MAX = 512                               # bm_grid: workgroup g walks pairs g, g + 512, ...


# ------------------------------------------------------------------ cases ------------------------------------------------------------------ #
class Case:
    """host-side float32 inputs of one call: X1 / X2 [N, d] (one tensor when ``shared``), w1 / w2 [N], pair ranges, P Q R,
    cotangents c1 / c2 [B, 3H]"""

    def __init__(self, X1, X2, w1, w2, r1, n1, r2, n2, W, seed=0, maxn=None):
        self.shared = X2 is X1
        self.X1, self.X2, self.w1, self.w2 = X1, X2, w1, w2
        self.r1, self.n1, self.r2, self.n2 = (list(map(int, v)) for v in (r1, n1, r2, n2))
        self.W = W
        self.B, self.d, self.H = len(self.r1), X1.shape[1], W[0].shape[0]
        self.maxn = max(self.n1 + self.n2) if maxn is None else maxn
        g = torch.Generator().manual_seed(1000 + seed)
        self.c1, self.c2 = torch.randn(self.B, 3 * self.H, generator=g), torch.randn(self.B, 3 * self.H, generator=g)
        # the launch reads rows r .. r + n of X and w and writes the same rows of dX: hold the ranges inside the buffers here
        assert self.maxn >= max(self.n1 + self.n2) and min(self.n1 + self.n2) >= 1
        for r, n, X, w in ((self.r1, self.n1, X1, w1), (self.r2, self.n2, X2, w2)):
            assert w.shape[0] == X.shape[0] and all(0 <= a and a + b <= X.shape[0] for a, b in zip(r, n))

    def pairs(self, lo, hi):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.r1, c.n1, c.r2, c.n2 = self.r1[lo:hi], self.n1[lo:hi], self.r2[lo:hi], self.n2[lo:hi]
        c.c1, c.c2, c.B = self.c1[lo:hi], self.c2[lo:hi], hi - lo
        return c


def _weights(d, H, g, scale=None):
    s = (2.0 / d) ** 0.5 if scale is None else scale
    return [torch.randn(H, d, generator=g) * s for _ in range(3)]


def dense_case(d, H, mb, N1, N2, seed, x1=None, x2=None):
    """mb pairs of N1 x N2 rows, w = 1, contiguous ranges, separate buffers"""
    g = torch.Generator().manual_seed(seed)
    X1 = torch.randn(mb * N1, d, generator=g) if x1 is None else x1
    X2 = torch.randn(mb * N2, d, generator=g) if x2 is None else x2
    return Case(X1, X2, torch.ones(mb * N1), torch.ones(mb * N2), [p * N1 for p in range(mb)], [N1] * mb,
                [p * N2 for p in range(mb)], [N2] * mb, _weights(d, H, g), seed=seed)


# ------------------------------------------------------------------ the kernel ------------------------------------------------------------------ #
def _dev(c):
    dev = torch.device("cuda:0")
    X1 = c.X1.to(dev)
    X2 = X1 if c.shared else c.X2.to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    meta = dict(B=c.B, r1=i32(c.r1), n1=i32(c.n1), r2=i32(c.r2), n2=i32(c.n2))
    return X1, X2, c.w1.to(dev), c.w2.to(dev), meta, [w.to(dev) for w in c.W]


def run_fn(c, maxn=None):
    """BiMPMFn forward + backward -> (mol_1, mol_2, dX1, dX2, dP, dQ, dR); dX2 is dX1 when the buffer is shared"""
    from bmp.bimpm import BiMPMFn
    X1, X2, w1, w2, meta, W = _dev(c)
    X1.requires_grad_()
    if not c.shared:
        X2.requires_grad_()
    W = [w.requires_grad_() for w in W]
    o1, o2 = BiMPMFn.apply(X1, X2, W[0], W[1], W[2], w1, w2, meta, c.maxn if maxn is None else maxn)
    ((o1 * c.c1.to(o1.device)).sum() + (o2 * c.c2.to(o1.device)).sum()).backward()
    return [o1.detach(), o2.detach(), X1.grad, X2.grad] + [w.grad for w in W]


def kernel_selections(c):
    """forward launches through the C ABI into a workspace this test owns, at most 512 pairs each (workgroup pr then
    handles pair pr only); returns mol_1, mol_2 and per pair the kernel's four selection arrays"""
    from bmp import _lib
    L = _lib.lib()
    lay = (ctypes.c_size_t * 5)()
    _lib.check(L.bmp_bimpm_ws_layout(c.d, c.H, c.maxn, 0, lay), "bmp_bimpm_ws_layout")
    stride, offs = lay[0], dict(zip(BR.SEL_NAMES, list(lay)[1:]))
    o1s, o2s, sels = [], [], []
    for lo in range(0, c.B, GRID_MAX):
        s = c.pairs(lo, min(lo + GRID_MAX, c.B))
        X1, X2, w1, w2, meta, W = _dev(s)
        nws = L.bmp_bimpm_ws_floats(s.d, s.H, s.maxn, s.B, 0)
        assert nws >= s.B * stride
        ws = torch.zeros(nws, dtype=torch.float32, device=X1.device)
        o1 = torch.empty(s.B, 3 * s.H, dtype=torch.float32, device=X1.device); o2 = torch.empty_like(o1)
        p = _lib.ptr
        _lib.check(L.bmp_bimpm_fwd(p(X1), p(X2), s.d, s.H, p(w1), p(meta["r1"]), p(meta["n1"]), p(w2), p(meta["r2"]), p(meta["n2"]),
                                   s.B, s.maxn, p(W[0]), p(W[1]), p(W[2]), p(o1), p(o2), p(ws), nws, _lib.stream()), "bmp_bimpm_fwd")
        torch.cuda.synchronize()
        wsi = ws.view(torch.int32).cpu()
        for q in range(s.B):
            n1, n2, base = s.n1[q], s.n2[q], q * stride
            take = lambda name, n, cols: wsi[base + offs[name]: base + offs[name] + n * cols].view(n, cols).long()
            sels.append(dict(jT2=take("jT2", n1, s.d), iT1=take("iT1", n2, s.d), j1s=take("j1s", n1, s.H), i2s=take("i2s", n2, s.H)))
        o1s.append(o1); o2s.append(o2)
    return torch.cat(o1s), torch.cat(o2s), sels


# ------------------------------------------------------------------ the reference ------------------------------------------------------------------ #
def reference(c, sels, validate=True):
    """float64 reference forced to ``sels`` -> the same seven tensors; with ``validate`` every selection is first held to tau"""
    X1 = c.X1.double().requires_grad_()
    X2 = X1 if c.shared else c.X2.double().requires_grad_()
    W = [w.double().requires_grad_() for w in c.W]
    if validate:
        gaps = BR.packed_selection_gaps(c.X1.double(), c.X2.double(), c.w1, c.w2, c.r1, c.n1, c.r2, c.n2, c.W[0], sels)
        print(f"[selections] worst (float64 maximum - selected score) / tau over {c.B} pairs: {gaps.max().item():.2e}")
        assert gaps.max() <= 1.0, f"pair {int(gaps.max(1).values.argmax())}: a kernel selection lies more than tau below the float64 maximum"
    o1, o2, res = BR.bimpm_packed(X1, X2, c.w1.double(), c.w2.double(), c.r1, c.n1, c.r2, c.n2, *W, sels=sels)
    ((o1 * c.c1.double()).sum() + (o2 * c.c2.double()).sum()).backward()
    gX1 = X1.grad if X1.grad is not None else torch.zeros_like(X1)
    gX2 = gX1 if c.shared else (X2.grad if X2.grad is not None else torch.zeros_like(X2))
    return [o1.detach(), o2.detach(), gX1, gX2] + [w.grad for w in W], res


NAMES = ("mol_1", "mol_2", "dX1", "dX2", "dP", "dQ", "dR")


def compare(got, want, tol=1e-4):
    for n, a, b in zip(NAMES, got, want):
        _close(a, b, n, tol=tol)


def check(c, validate=True):
    """the whole comparison of one case; returns (kernel results, reference results, selections, per-pair reference records)"""
    o1a, o2a, sels = kernel_selections(c)
    got = run_fn(c)
    assert torch.equal(got[0], o1a) and torch.equal(got[1], o2a)          # the launch the selections were read from
    want, res = reference(c, sels, validate)
    compare(got, want)
    return got, want, sels, res


# ------------------------------------------------------------------ a. gradients under the kernel's own selections ------------------------------------------------------------------ #
@pytest.mark.parametrize("d,H,mb,N1,N2", [(128, 16, 2, 200, 150), (128, 8, 2, 300, 40), (64, 16, 1, 330, 310), (32, 8, 5, 9, 13)])
def test_gradients_under_the_kernels_own_selections(d, H, mb, N1, N2):
    """Thousands of maxima per pair: against the unforced oracle a float32 near-tie that picks the other atom moves a
    gradient by the difference of two candidates (test_gpu_bimpm.py states 2e-3 for that).  Here the reference takes the
    kernel's selections, each validated against tau, and every gradient is held to 1e-4."""
    check(dense_case(d, H, mb, N1, N2, seed=d + H))


# ------------------------------------------------------------------ b. persistent grid ------------------------------------------------------------------ #
def test_persistent_grid_walks_three_pairs_per_workgroup():
    """B = 1100 > 512 workgroups: a workgroup's second and third pair reuse its scratch slice (arg-max arrays, head / next
    lists) at another size -- side 1 grows while side 2 shrinks through 1..7 -- and its weight-gradient slab accumulates."""
    B, d, H = 1100, 16, 4
    n1 = [1 + p % 7 for p in range(B)]
    n2 = [7 - p % 7 for p in range(B)]
    assert {n1[g + 512] - n1[g] for g in range(512)} == {1, -6} and {n2[g + 512] - n2[g] for g in range(512)} == {-1, 6}
    r1 = np.concatenate([[0], np.cumsum(n1)[:-1]]); r2 = np.concatenate([[0], np.cumsum(n2)[:-1]])
    g = torch.Generator().manual_seed(21)
    c = Case(torch.randn(sum(n1), d, generator=g), torch.randn(sum(n2), d, generator=g), torch.ones(sum(n1)), torch.ones(sum(n2)),
             r1, n1, r2, n2, _weights(d, H, g), seed=21)
    o1a, o2a, sels = kernel_selections(c)                              # three launches of <= 512 pairs
    got = run_fn(c)                                                   # forward-only path and backward at B = 1100
    parts = [run_fn(c.pairs(lo, min(lo + GRID_MAX, B))) for lo in range(0, B, GRID_MAX)]
    assert len(parts) == 3
    assert torch.equal(got[0], torch.cat([p[0] for p in parts])) and torch.equal(got[1], torch.cat([p[1] for p in parts]))
    assert torch.equal(got[0], o1a) and torch.equal(got[1], o2a)
    assert torch.equal(got[2], parts[0][2] + parts[1][2] + parts[2][2])            # disjoint rows: the sum is exact
    assert torch.equal(got[3], parts[0][3] + parts[1][3] + parts[2][3])
    for k in (4, 5, 6):
        _close(got[k], parts[0][k].double() + parts[1][k].double() + parts[2][k].double(), NAMES[k] + " vs three calls", tol=1e-5)
    want, _ = reference(c, sels)
    compare(got, want)


# ------------------------------------------------------------------ c. hand-built layouts ------------------------------------------------------------------ #
def _layout_case(shared):
    d, H = 16, 4
    g = torch.Generator().manual_seed(33)
    #            side 1 ranges (first row, rows)      side 2 ranges: gaps before, between and behind them
    r1, n1 = [2, 9, 20], [5, 7, 3]
    r2, n2 = ([30, 41, 47], [6, 4, 8]) if shared else ([1, 12, 18], [6, 4, 8])
    N1, N2 = (58, 58) if shared else (25, 29)
    X1 = torch.full((N1, d), float("nan"))
    X2 = X1 if shared else torch.full((N2, d), float("nan"))
    w1 = torch.ones(N1); w2 = w1 if shared else torch.ones(N2)
    for r, n, X in ((r1, n1, X1), (r2, n2, X2)):
        for a, b in zip(r, n):
            X[a:a + b] = torch.randn(b, d, generator=g)
    # multiplicities 3 and 2; w = 0 rows inside a range holding large finite values that any maximum would pick
    w1[3] = 3; w1[11] = 3; w2[r2[0] + 1] = 3; w2[r2[2] + 7] = 2
    for X, w, row in ((X1, w1, 4), (X1, w1, 9), (X1, w1, 15), (X2, w2, r2[1] + 2), (X2, w2, r2[2])):
        w[row] = 0
        X[row] = 1.0e4 * torch.sign(torch.randn(d, generator=g))
    return Case(X1, X2, w1, w2, r1, n1, r2, n2, _weights(d, H, g), seed=33), (r1, n1, r2, n2)


@pytest.mark.parametrize("shared", [False, True], ids=["separate-buffers", "one-buffer"])
def test_hand_built_layouts(shared):
    c, (r1, n1, r2, n2) = _layout_case(shared)
    got, want, sels, _ = check(c)
    in1 = torch.zeros(c.X1.shape[0], dtype=torch.bool); in2 = torch.zeros(c.X2.shape[0], dtype=torch.bool)
    for a, b in zip(r1, n1):
        in1[a:a + b] = True
    for a, b in zip(r2, n2):
        in2[a:a + b] = True
    if shared:
        in1 = in2 = in1 | in2
    assert torch.isnan(c.X1[~in1]).all() and (~in1).sum() >= 5
    for t in got:
        assert torch.isfinite(t).all()
    assert (got[2].cpu()[~in1] == 0).all() and (got[3].cpu()[~in2] == 0).all()       # rows of no pair: exactly zero
    dead1, dead2 = (c.w1 == 0) & in1, (c.w2 == 0) & in2
    assert dead1.sum() >= 2 and (got[2].cpu()[dead1] == 0).all() and (got[3].cpu()[dead2] == 0).all()
    for p, s in enumerate(sels):                                       # no maximum of a live row picked a w = 0 row
        lw1, lw2 = c.w1[r1[p]:r1[p] + n1[p]], c.w2[r2[p]:r2[p] + n2[p]]
        assert (lw2[s["jT2"]] > 0).all() and (lw2[s["j1s"]] > 0).all() and (lw1[s["iT1"]] > 0).all() and (lw1[s["i2s"]] > 0).all()


# ------------------------------------------------------------------ d. degenerate shapes ------------------------------------------------------------------ #
@pytest.mark.parametrize("d", [5, 32])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("n1,n2", [(1, 1), (1, 7), (7, 1), (5, 4), (6, 9)])
def test_degenerate_shapes(n1, n2, H, d):
    """single rows, one perspective, widths and heads that are no power of two, every tail of bm_maxpool's four-row unroll"""
    check(dense_case(d, H, 2, n1, n2, seed=100 * n1 + 10 * n2 + H + d))


# ------------------------------------------------------------------ e. LDS boundary ------------------------------------------------------------------ #
def test_lds_boundary_157_158():
    """bm_lds_bytes = (2 maxn (d + 1) + 2 maxn + 16) * 4 <= 160 KiB: at d = 128 the last in-LDS maxn is 157 (163,344 of
    163,840 bytes of dynamic LDS requested), 158 stages in global memory.  The small pairs of the bit-for-bit test on both
    sides of the switch and at their true size."""
    from bmp import packed, synth
    from bmp.bimpm import BiMPMFn
    from bmp.coattention import pair_rows
    from bmp.ggnn import PackedAtoms
    d, H = 128, 16
    fits = lambda n: (2 * n * (d + 1) + 2 * n + 16) * 4 <= 160 * 1024
    last = max(n for n in range(1, 1000) if fits(n))
    assert last == 157 and (2 * 157 * (d + 1) + 2 * 157 + 16) * 4 == 163344
    dev = torch.device("cuda:0")
    store = synth.make_store(20, seed=3, n_lo=3, n_hi=40, n_mean=14)
    ms = packed.MolStore(store)
    rs = np.random.RandomState(2)
    i1, i2 = rs.randint(0, 20, 11), rs.randint(0, 20, 11)
    pb = packed.pack_from_store(ms, [i1, i2], device=dev)
    g = torch.Generator().manual_seed(1)
    rows = torch.randn(pb.n_rows, d, generator=g).to(dev)
    W = [(torch.randn(H, d, generator=g) * 0.1).to(dev) for _ in range(3)]
    c1, c2 = torch.randn(11, 3 * H, generator=g).to(dev), torch.randn(11, 3 * H, generator=g).to(dev)
    assert pb.max_rows_per_mol < last
    res = []
    for maxn in (pb.max_rows_per_mol, last, last + 1):
        x = rows.clone().requires_grad_()
        Ws = [w.clone().requires_grad_() for w in W]
        at = PackedAtoms(x, pb, None)
        X1, X2, w1, w2, meta, _ = pair_rows(at, at)
        o1, o2 = BiMPMFn.apply(X1, X2, Ws[0], Ws[1], Ws[2], w1, w2, meta, maxn)
        ((o1 * c1).sum() + (o2 * c2).sum()).backward()
        res.append((o1.detach(), o2.detach(), x.grad, Ws[0].grad, Ws[1].grad, Ws[2].grad))
    assert torch.isfinite(res[0][0]).all() and res[0][2].abs().max() > 0
    for other in res[1:]:
        for a_, b_ in zip(res[0], other):
            assert torch.equal(a_, b_)


# ------------------------------------------------------------------ f. clamp branches ------------------------------------------------------------------ #
def _clamp_case(clamped):
    d, H, mb, n = 16, 4, 3, 6
    g = torch.Generator().manual_seed(55)
    x1 = torch.randn(mb * n, d, generator=g).abs() + 0.05            # non-negative features: every cosine positive
    x2 = -x1.clone() if clamped else torch.randn(mb * n, d, generator=g).abs() + 0.05
    c = dense_case(d, H, mb, n, n, seed=55, x1=x1, x2=x2)
    c.w1[2] = 3; c.w2[7] = 2
    return c


@pytest.mark.parametrize("clamped", [False, True], ids=["above", "clamped"])
def test_div_eps_clamp_branches(clamped):
    """both sides of max(sum_j w_j att_ij, BM_DIV_EPS), hit on purpose: the reference's float64 sums put EVERY row of the
    input on the intended side, a hundred times the threshold away from it, before anything is compared"""
    c = _clamp_case(clamped)
    _, _, _, res = check(c)
    for r in res:
        D = torch.cat([r["D2"], r["D1"]])
        assert (D <= -100 * BR.DIV_EPS).all() if clamped else (D >= 100 * BR.DIV_EPS).all()


# ------------------------------------------------------------------ g. exact ties and zero rows ------------------------------------------------------------------ #
def test_exact_ties_go_to_the_lowest_index():
    """symmetric atoms give bit-identical rows: x2 rows 1, 4 and 6 of every pair are one row, x1 rows 0 and 2 another.  The
    strict `>` keeps the first; the gradient goes to that one winner (the forced reference)."""
    d, H, mb, N1, N2 = 16, 4, 2, 5, 7
    c = dense_case(d, H, mb, N1, N2, seed=77)
    for p in range(mb):
        c.X2[p * N2 + 4] = c.X2[p * N2 + 1]; c.X2[p * N2 + 6] = c.X2[p * N2 + 1]
        c.X1[p * N1 + 2] = c.X1[p * N1 + 0]
    got, want, sels, _ = check(c)
    picked = 0
    for s in sels:
        for name in ("jT2", "j1s"):
            assert (s[name] != 4).all() and (s[name] != 6).all(), name
            picked += int((s[name] == 1).sum())
        for name in ("iT1", "i2s"):
            assert (s[name] != 2).all(), name
            picked += int((s[name] == 0).sum())
    assert picked > 0                                                  # the tied rows did win maxima
    # the later copies win nothing, so all they receive is the smooth part -- not the same gradient as the first copy
    assert not torch.equal(got[3][1], got[3][4])


def test_all_zero_row_with_multiplicity():
    """an all-zero row with w = 2 (a zero pad row): |u| = 0 in every matching of that row -- the `nu > 0` guard of bm_dmatch,
    subgradient 0 -- and its attention sum is 0, clamped.  Its own gradient is of the order 1 / eps = 1e5 (d att / d x at
    x = 0), so it is compared apart from the other rows, each at 1e-4 of its own scale."""
    d, H, mb, N1, N2 = 16, 4, 2, 5, 6
    c = dense_case(d, H, mb, N1, N2, seed=88)
    zrow = N1 + 3                                                      # pair 1, row 3 of side 1
    c.X1[zrow] = 0; c.w1[zrow] = 2
    o1a, o2a, sels = kernel_selections(c)
    got = run_fn(c)
    want, res = reference(c, sels)
    for t in got:
        assert torch.isfinite(t).all()
    assert (res[1]["D2"][3] == 0).all()
    keep = torch.ones(mb * N1, dtype=torch.bool); keep[zrow] = False
    for n, a, b in zip(NAMES, got, want):
        if n == "dX1":
            _close(a.cpu()[keep], b[keep], "dX1 (other rows)")
            _close(a.cpu()[zrow], b[zrow], "dX1 (the zero row)")
        else:
            _close(a, b, n)
    assert (sels[1]["jT2"][3] == 0).all() and (sels[1]["j1s"][3] == 0).all()      # all scores 0: the first row wins
