"""CPU tests of tests/wgrad_ref.py: every float64 restatement against an explicit loop over rows, the restated launch plans
against the sizes the library reports (host arithmetic, no GPU call), the cases of tests/test_gpu_wgrad_edges.py against the
kernel and grid forms they are named for, and the float32 error of the reference operation itself."""
import pytest
import torch

import wgrad_ref as R


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from bmp import _lib
    return _lib.lib()


def _ints(gen, *shape, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


# ---- the restatements against plain loops (N = 8, d = 4) --------------------------------------------------------------
def test_linear_wgrad_is_the_row_loop():
    g = torch.Generator().manual_seed(1)
    N, K, Nn, ldx, ldy = 8, 3, 5, 7, 9
    X, dY = _ints(g, N * ldx), _ints(g, N * ldy + 2)
    dWT, db = R.linear_wgrad(X, ldx, dY[2:], ldy, N, K, Nn)
    want, wb = torch.zeros(K, Nn, dtype=torch.float64), torch.zeros(Nn, dtype=torch.float64)
    for r in range(N):
        for j in range(Nn):
            wb[j] += float(dY[2 + r * ldy + j])
            for i in range(K):
                want[i, j] += float(X[r * ldx + i]) * float(dY[2 + r * ldy + j])
    assert torch.equal(dWT, want) and torch.equal(db, wb)
    assert R.linear_wgrad(X, ldx, dY, ldy, N, K, Nn, want_db=False)[1] is None


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("mode", R.LIST_MODES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_ggnn_step_wgrad_is_the_row_loop(first, mode, accumulate):
    g = torch.Generator().manual_seed(2 + first)
    N, d = 8, 4
    h, m, rz, gda = _ints(g, N, d), _ints(g, N, d), _ints(g, N, 2 * d, lo=0, hi=2), _ints(g, N, 7 * d)
    idx = cnt = lvi = lvc = None
    on = torch.ones(4, N, dtype=torch.bool)
    live = torch.ones(N, dtype=torch.bool)
    if mode != "none":
        idx, cnt = R.make_row_lists(N, [0, 1, 5, N], g)
        on = torch.stack([R.list_mask(idx, cnt, e, N) for e in range(4)])
        for e in range(4):
            gda[~on[e], e * d:(e + 1) * d] = float("nan")            # never read
    if mode == "type+live":
        lvi, lvc = R.make_row_lists(N, [3], g)
        live = R.list_mask(lvi, lvc, 0, N)
        gda[~live, 4 * d:] = 0.0
    if first:
        gda[:, 4 * d:5 * d] = float("nan")                            # never read
    prev = tuple(_ints(g, *s) for s in ((d, 7 * d), (d, 3 * d), (d, d), (7 * d,)))
    got = R.ggnn_step_wgrad(h, m, rz, gda, N, d, first, accumulate, prev, idx, cnt, lvi, lvc)
    o1, o2, dU, cs = (p.double().clone() if accumulate else torch.zeros_like(p, dtype=torch.float64) for p in prev)
    for r in range(N):
        for j in range(7 * d):
            e = j // d
            if (e < 4 and not on[e, r]) or (first and e == 4):
                continue
            if e >= 4 and not first and not live[r]:
                assert float(gda[r, j]) == 0.0
            cs[j] += float(gda[r, j])
            for i in range(d):
                o1[i, j] += float(h[r, i]) * float(gda[r, j])
                if e >= 4:
                    o2[i, j - 4 * d] += float(m[r, i]) * float(gda[r, j])
                if e == 6 and not first:
                    dU[i, j - 6 * d] += float(rz[r, i]) * float(h[r, i]) * float(gda[r, j])
    for name, a, b in zip(("o1", "o2", "dUcT", "cs"), got, (o1, o2, dU, cs)):
        assert torch.equal(a, b), name
    if first:                                                         # the skipped columns: zeros, or left as they were
        keep = prev if accumulate else tuple(torch.zeros_like(p) for p in prev)
        assert torch.equal(got[0][:, 4 * d:5 * d], keep[0][:, 4 * d:5 * d].double()) and torch.equal(got[1][:, :d], keep[1][:, :d].double())
        assert torch.equal(got[2], keep[2].double()) and torch.equal(got[3][4 * d:5 * d], keep[3][4 * d:5 * d].double())


@pytest.mark.parametrize("lists", [False, True])
def test_relgcn_layer_wgrad_is_the_row_loop(lists):
    g = torch.Generator().manual_seed(4)
    N, d = 8, 4
    h, wdeg, gda = _ints(g, N, d), _ints(g, N, 4, lo=0, hi=2), _ints(g, N, 5 * d)
    idx = cnt = None
    on = torch.ones(4, N, dtype=torch.bool)
    if lists:
        idx, cnt = R.make_row_lists(N, [N, 0, 1, 6], g)
        on = torch.stack([R.list_mask(idx, cnt, e, N) for e in range(4)])
        for e in range(4):
            gda[~on[e], e * d:(e + 1) * d] = float("nan")
    prev = tuple(_ints(g, *s) for s in ((d, 5 * d), (4, d), (5 * d,)))
    got = R.relgcn_layer_wgrad(h, wdeg, gda, N, d, 1, prev, idx, cnt)
    o1, dbE, cs = (p.double().clone() for p in prev)
    for r in range(N):
        for j in range(5 * d):
            e = j // d
            if e < 4 and not on[e, r]:
                continue
            cs[j] += float(gda[r, j])
            for i in range(d):
                o1[i, j] += float(h[r, i]) * float(gda[r, j])
            if e == 4:
                for t in range(4):
                    dbE[t, j - 4 * d] += float(wdeg[r, t]) * float(gda[r, j])
    for name, a, b in zip(("o1", "dbE", "cs"), got, (o1, dbE, cs)):
        assert torch.equal(a, b), name


def test_nfp_layer_wgrad_and_embed_bwd_are_the_row_loops():
    g = torch.Generator().manual_seed(5)
    N, d_in, d_out = 8, 4, 3
    fv, dpre = _ints(g, N, d_in), _ints(g, N, d_out)
    idx, cnt = R.make_class_lists(N, [0, 1, 2, 0, 3, 0, 1], g)
    cls = torch.zeros(N, dtype=torch.long)
    for k in range(7):
        assert int(cls[R.list_mask(idx, cnt, k, N)].sum()) == 0      # disjoint
        cls[R.list_mask(idx, cnt, k, N)] = k + 1
    fv[cls == 0] = float("nan")                                       # rows of no class: fv is never read
    dWT, dB = R.nfp_layer_wgrad(fv, dpre, N, d_in, d_out, idx, cnt)
    want, wb = torch.zeros(7, d_in, d_out, dtype=torch.float64), torch.zeros(d_out, dtype=torch.float64)
    for r in range(N):
        for j in range(d_out):
            wb[j] += float(dpre[r, j])
            for i in range(d_in):
                if cls[r] > 0:
                    want[cls[r] - 1, i, j] += float(fv[r, i]) * float(dpre[r, j])
    assert torch.equal(dWT, want) and torch.equal(dB, wb)
    V, d = 5, 4
    ids, dout = torch.randint(0, V, (N,), generator=g).int(), _ints(g, N, d)
    want = torch.zeros(V, d, dtype=torch.float64)
    for r in range(N):
        for c in range(d):
            want[int(ids[r]), c] += float(dout[r, c])
    assert torch.equal(R.embed_bwd(ids, dout, N, d, V), want)


@pytest.mark.parametrize("N, counts", [(32, [0, 1, 31, 32]), (288, [15, 16, 17, 288]), (16, [16])])
def test_row_lists_are_ascending_distinct_and_their_tails_valid_rows_off_the_list(N, counts):
    g = torch.Generator().manual_seed(6)
    for make in (R.make_row_lists, R.make_class_lists):
        if make is R.make_class_lists and sum(counts) > N:
            continue
        idx, cnt = make(N, counts, g)
        assert idx.dtype == torch.int32 and cnt.dtype == torch.int32 and idx.numel() == len(counts) * N and cnt.tolist() == counts
        assert int(idx.min()) >= 0 and int(idx.max()) < N            # every entry a valid row, past the count too
        for l, c in enumerate(counts):
            rows = idx[l * N:(l + 1) * N]
            assert bool((rows[1:c] > rows[:max(c - 1, 0)]).all())
            on = R.list_mask(idx, cnt, l, N)
            assert int(on.sum()) == c and not bool(on[rows[c:].long()].any())


# ---- the restated plans are the library's -----------------------------------------------------------------------------
def test_fused_workspace_sizes_are_the_library_ones(L):
    for d in (64, 128):
        for N in range(32, 128 * 640 + 1, 352):
            want = max(R.fused_ws_floats(R.step_problems(d, first, lists, live), N)
                       for first in (0, 1) for lists, live in ((False, False), (True, False), (True, True)))
            assert L.bmp_ggnn_step_wgrad_ws_floats(N, d) == want, (N, d)
            want = max(R.fused_ws_floats(R.rel_problems(d, lists), N) for lists in (False, True))
            assert L.bmp_relgcn_layer_wgrad_ws_floats(N, d) == want, (N, d)


def test_single_problem_workspace_size_is_the_library_one(L):
    shapes = R.LINEAR_DIRECT + R.LINEAR_LDS + ((128, 128), (128, 896), (117, 4), (132, 128), (256, 768), (4, 64))
    for K, Nn in shapes:
        for N in list(range(8, 1300, 8)) + [2848, 81920]:
            assert L.bmp_wgrad_ws_floats_c(N, K, Nn) == R.wgrad_ws_floats(N, K, Nn), (N, K, Nn)


@pytest.mark.parametrize("d_in", [64, 96, 128])
@pytest.mark.parametrize("d_out", [64, 72, 132, 256])
def test_nfp_workspace_is_the_restated_one_and_covers_the_listed_slabs(L, d_in, d_out):
    probs = R.nfp_listed_problems(d_in, d_out)
    for N in range(32, 81920 + 1, 32):
        ws = L.bmp_nfp_layer_wgrad_ws_floats(N, d_in, d_out)
        assert R.nfp_listed_ok(N, d_in, d_out)
        assert ws - R.colsum_ws_floats(N, d_out) >= R.slab_floats(probs, N), (N, d_in, d_out)       # the column sums own the tail
        if N % 352 == 0 or N < 4096:
            assert ws == R.nfp_layer_wgrad_ws_floats(N, d_in, d_out), (N, d_in, d_out)
    for N in (8, 40, 520):                                            # the row-wise kernel's slabs
        assert not R.nfp_listed_ok(N, d_in, d_out)
        assert L.bmp_nfp_layer_wgrad_ws_floats(N, d_in, d_out) == R.nfp_layer_wgrad_ws_floats(N, d_in, d_out)


def test_a_listed_part_holds_the_whole_list_whatever_its_count():
    """nsplit parts of listed_part_rows rows cover any count up to N (the kernel cuts the list by the count it finds)."""
    for count in (0, 1, 15, 16, 17, 287, 288, 2847, 2848):
        for nsplit in (1, 2, 3, 6, 8):
            rows = R.listed_part_rows(count, nsplit)
            assert rows % R.WD_RS == 0 and rows * nsplit >= count and (count == 0) == (rows == 0)


# ---- the GPU cases take the forms they are named for --------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_step_cases_take_the_named_grid_forms(d):
    table = {32: (32, 1, "plain", "plain"), 288: (288, 1, "plain", "plain"), 544: (288, 2, "plain", "flat"),
             2848: (288, 10, "xcd", "flat")}
    assert tuple(table) == R.STEP_N
    for N, (rps, S, no_lists, with_lists) in table.items():
        for first in (0, 1):
            probs = R.step_problems(d, first, False, False)
            Sp, rp, _ = R.fused_plan(probs, N)
            assert set(rp) == {rps} and {s for s in Sp if s} == {S}, (N, first)
            assert R.grouped_grid(probs, N)[0] == no_lists, (N, first)
            for live in (False, True):
                assert R.grouped_grid(R.step_problems(d, first, True, live), N)[0] == with_lists, (N, first, live)
        assert R.grouped_grid(R.rel_problems(d, True), N)[0] == with_lists
    assert 544 - 288 == 256                                           # the ragged second split
    # N = 2848: one whole split per XCD and two remainder splits; the lists' parts
    for first in (0, 1):
        assert R.grouped_grid(R.step_problems(d, first, False, False), 2848)[:2] == ("xcd", 2)
    assert R.fused_plan(R.step_problems(d, 0, True, False), 2848)[0] == [10, 10, 10, 8, 2, 1, 6]
    assert R.fused_plan(R.step_problems(d, 0, True, True), 2848)[0] == [3, 3, 10, 8, 2, 1, 6]
    assert R.fused_plan(R.rel_problems(d, True), 2848)[0] == [10, 8, 2, 1, 6]
    assert R.grouped_grid(R.step_problems(d, 0, False, False), 2080)[:2] == ("xcd", 0)          # no remainder there
    # the single RelGCN problem without lists: d = 128 has five column tiles (XCD-grouped), d = 64 three
    assert R.grouped_grid(R.rel_problems(d, False), 2848)[:2] == ("xcd", 2)


def test_the_later_call_at_2848_rows_and_d_128():
    assert R.grouped_grid(R.step_problems(128, 0, True, False), 2848) == ("flat", 87)
    assert R.grouped_grid(R.step_problems(128, 0, False, False), 2848) == ("xcd", 2, 112)


def test_case_rotations_give_every_type_every_count():
    for N in R.STEP_N:
        for mode in R.LIST_MODES[1:]:
            seen = [set() for _ in range(4)]
            for d in (64, 128):
                for first in (0, 1):
                    for acc in (0, 1):
                        for e, c in enumerate(R.list_counts(N, R.case_rotation(d, first, acc, N, mode))):
                            seen[e].add(c)
            for e in range(4):
                assert seen[e] == {0, 1, 15, 16, 17, N - 1, N}, (N, mode, e)


def test_linear_cases_take_the_named_kernels():
    seen = set()
    for K, Nn in R.LINEAR_DIRECT:
        for N in R.LINEAR_DIRECT_N:
            for strided in (False, True):
                ldx, ldy = (K + 12, 4 * K + Nn) if strided else (K, Nn)
                k = R.linear_kernel(N, K, Nn, ldx, ldy)
                assert k.startswith("k_wgrad<"), (K, Nn, N)
                seen.add(k)
    assert seen == {"k_wgrad<1,1>", "k_wgrad<2,1>", "k_wgrad<1,2>", "k_wgrad<2,2>"}
    for K, Nn in R.LINEAR_LDS:
        for N in R.LINEAR_LDS_N:
            assert R.linear_kernel(N, K, Nn, K, Nn) == "k_wgrad_lds" and R.linear_kernel(N, K, Nn, K + 12, 4 * K + Nn) == "k_wgrad_lds"
        assert R.linear_kernel(136, K, Nn, K, Nn) == "k_wgrad<2,2>"
    assert R.linear_kernel(136, 128, 128, 128, 128) == "k_wgrad<2,2>"                   # 8 | N, 32 does not
    assert R.linear_kernel(160, 128, 128, 128, 128) == "k_wgrad_lds"
    assert R.linear_kernel(160, 128, 128, 128, 128, x_aligned=False) == "k_wgrad<2,2>"
    assert R.wgrad_plan(1160, 130, 66)[2:] == (9, 136) and 1160 % 136 != 0              # a ragged last split
    assert R.wgrad_lds_plan(1056, 136, 136) == (4, 288) and 1056 % 288 != 0


def test_nfp_and_embed_cases_take_the_named_paths():
    for d_in, d_out in ((64, 64), (96, 72), (128, 132), (128, 256)):
        for N in (32, 544, 2080):
            assert R.nfp_listed_ok(N, d_in, d_out)
        assert not R.nfp_listed_ok(40, d_in, d_out)
    _, _, ty0 = R.fused_plan(R.nfp_listed_problems(128, 132), 544)
    assert ty0[-1] == 14 and 132 % 128 == 4                           # two column tiles per class, the second four columns wide
    for N, onehot in ((32, True), (416, True), (40, False)):
        for d in (4, 24, 128):
            assert R.wgrad_use_lds(N, 117, d, 0, d, onehot=True) == onehot


# ---- the reference operation in float32 ----------------------------------------------------------------------------------
def test_float32_matmul_of_the_largest_case_stays_within_a_tenth_of_the_tolerance():
    """The GPU tests allow 2e-5 of the tensor's max-abs against float64; torch's own float32 product of the same kind of
    operands (N = 2848, d = 128, gda scaled by 1e-2) is within 2e-6: the reference operation does not use up the margin."""
    g = torch.Generator().manual_seed(7)
    N, d = 2848, 128
    h, gda = torch.randn(N, d, generator=g), torch.randn(N, 7 * d, generator=g) * 1e-2
    want = h.double().t() @ gda.double()
    rel = float((h.t() @ gda - want).abs().max() / want.abs().max())
    assert rel <= 2e-6, rel
    cs = gda.double().sum(0)
    assert float((gda.sum(0) - cs).abs().max() / cs.abs().max()) <= 2e-6
