"""The weight-gradient GEMM family of csrc/bmp_gemm.hip, restated for the tests (no GPU, no library call):

* float64 references of what every entry point of the family writes -- bmp_linear_wgrad, bmp_ggnn_step_wgrad,
  bmp_relgcn_layer_wgrad, bmp_nfp_layer_wgrad, bmp_embed_bwd -- from the operands the C ABI gets.  A reference reads exactly
  what the entry point's contract lets it read: with row lists only the listed rows of a per-type block, on the first call
  never the da_r columns.  Whatever else the operands hold (the tests put NaN there) cannot reach the result;
* the launch plans: wgrad_fused_plan, the slab offsets of bmp_launch_wgrad_fused and the grid choice of wgrad_grouped_grid
  (fused launches), wgrad_plan / wgrad_lds_plan / wgrad_use_lds (single-problem launch), the problem sets of
  step_wgrad_problems / rel_wgrad_problem (bmp_fused.hip) and nfp_listed_problems (bmp_nfp.hip), and the *_ws_floats sizes;
* a builder of synthetic row lists laid out as bmp_type_rows lays them out.

tests/test_wgrad_ref.py pins all of it on the CPU; tests/test_gpu_wgrad_edges.py runs the kernels against it."""
import numpy as np
import torch

TYPE_FRAC = [float(np.float32(f)) for f in (0.78, 0.24, 0.05, 0.58)]                  # kTypeFrac (bmp_fused.hip)
LIVE_FRAC = float(np.float32(0.3))
NFP_CLASS_FRAC = [float(np.float32(f)) for f in (0.02, 0.25, 0.40, 0.25, 0.05, 0.02, 0.02)]      # kNfpClassFrac (bmp_nfp.hip)
NFP_NCLS = 7
WD_RS = 16                          # rows of one stage of the LDS-DMA body
WG_MAXT = 32                        # BMP_WG_MAXT: column tiles the flat grid can describe


# ---------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------
def rows_view(flat, N, cols, ld, off=0):
    """[N x cols] view of a flat buffer: element (r, c) at flat[off + r * ld + c] (what a pointer + leading dimension name)."""
    return torch.as_strided(flat, (N, cols), (ld, 1), flat.storage_offset() + off)


def _tn(a, b):
    return a.double().t() @ b.double()


def _listed(rows, cnt, l, N):
    return rows[l * N: l * N + int(cnt[l])].long()


def linear_wgrad(X, ldx, dY, ldy, N, K, Nn, want_db=True):
    """bmp_linear_wgrad: dWT [K x Nn] = X^T dY, db [Nn] = column sums of dY (X, dY flat, rows ldx / ldy apart)."""
    x, y = rows_view(X, N, K, ldx), rows_view(dY, N, Nn, ldy)
    return _tn(x, y), (y.double().sum(0) if want_db else None)


def ggnn_step_wgrad(h, m, rz, gda, N, d, first, accumulate=0, prev=None, type_rows=None, type_cnt=None, live_rows=None,
                    live_cnt=None):
    """bmp_ggnn_step_wgrad: (o1 [d x 7d], o2 [d x 3d], dUcT [d x d], cs [7d]).  h, m [N x d], rz [N x 2d], gda [N x 7d] =
    [G_0..G_3 | da_r | da_z | da_c].  first: the da_r columns are not read; o1[:, 4d:5d], o2[:, :d], cs[4d:5d] and dUcT get no
    sum -- zeros when written, left as they were when accumulating.  type_rows / type_cnt: block G_e is read in the rows of
    list e only; live_rows / live_cnt (later calls, with type lists): the da columns of o1, o2 and cs are summed over that list
    only; dUcT always walks every row.  prev: the outputs before the call (accumulate != 0)."""
    o1, o2, dU, cs = (torch.zeros(s, dtype=torch.float64) for s in ((d, 7 * d), (d, 3 * d), (d, d), (7 * d,)))
    lists = type_rows is not None and type_cnt is not None
    every = torch.arange(N)
    for e in range(4):
        r = _listed(type_rows, type_cnt, e, N) if lists else every
        g = gda[r, e * d:(e + 1) * d]
        o1[:, e * d:(e + 1) * d] = _tn(h[r], g)
        cs[e * d:(e + 1) * d] = g.double().sum(0)
    r = _listed(live_rows, live_cnt, 0, N) if (lists and live_rows is not None and not first) else every
    c0 = 5 * d if first else 4 * d
    da = gda[r, c0:]
    o1[:, c0:] = _tn(h[r], da)
    o2[:, c0 - 4 * d:] = _tn(m[r], da)
    cs[c0:] = da.double().sum(0)
    if not first:
        dU = _tn(rz[:, :d] * h, gda[:, 6 * d:])
    out = (o1, o2, dU, cs)
    if accumulate:
        out = tuple(p.double() + o for p, o in zip(prev, out))
    return out


def relgcn_layer_wgrad(h, wdeg, gda, N, d, accumulate=0, prev=None, type_rows=None, type_cnt=None):
    """bmp_relgcn_layer_wgrad: (o1 [d x 5d] = h^T gda, dbE [4 x d] = wdeg^T dpre, cs [5d]); gda [N x 5d] = [G_0..G_3 | dpre],
    block G_e read in the rows of list e only when lists are passed."""
    o1, cs = torch.zeros(d, 5 * d, dtype=torch.float64), torch.zeros(5 * d, dtype=torch.float64)
    lists = type_rows is not None and type_cnt is not None
    for e in range(5):
        r = _listed(type_rows, type_cnt, e, N) if (lists and e < 4) else torch.arange(N)
        g = gda[r, e * d:(e + 1) * d]
        o1[:, e * d:(e + 1) * d] = _tn(h[r], g)
        cs[e * d:(e + 1) * d] = g.double().sum(0)
    out = (o1, _tn(wdeg, gda[:, 4 * d:]), cs)
    if accumulate:
        out = tuple(p.double() + o for p, o in zip(prev, out))
    return out


def nfp_layer_wgrad(fv, dpre, N, d_in, d_out, deg_rows, deg_cnt):
    """bmp_nfp_layer_wgrad: dWT [7 x d_in x d_out], dW_k over the rows of list k; dB [d_out] over all rows."""
    dWT = torch.zeros(NFP_NCLS, d_in, d_out, dtype=torch.float64)
    for k in range(NFP_NCLS):
        r = _listed(deg_rows, deg_cnt, k, N)
        dWT[k] = _tn(fv[r], dpre[r])
    return dWT, dpre.double().sum(0)


def embed_bwd(ids, dout, N, d, V):
    """bmp_embed_bwd: dW [V x d], dW[id] = sum of dout over the rows with that id (ids in [0, V))."""
    dW = torch.zeros(V, d, dtype=torch.float64)
    dW.index_add_(0, ids.long(), dout.double())
    return dW


# ---------------------------------------------------------------------------------------------------------------------
# synthetic row lists
# ---------------------------------------------------------------------------------------------------------------------
def _with_tail(on, N, gen):
    """N entries: the listed rows ascending, then rows that are NOT on the list (valid row numbers: an entry past the count
    that a kernel wrongly used gives a wrong number, not an address outside the operands)."""
    on = torch.sort(on).values
    mask = torch.ones(N, dtype=torch.bool)
    mask[on] = False
    off = torch.nonzero(mask).flatten()
    if off.numel() == 0:
        return on
    pick = off[torch.randint(0, off.numel(), (N - on.numel(),), generator=gen)]
    return torch.cat([on, pick])


def make_row_lists(N, counts, gen):
    """Independent lists (bmp_type_rows): (idx int32 [len(counts) * N], cnt int32 [len(counts)]); list l holds counts[l]
    distinct rows in ascending order."""
    idx = [_with_tail(torch.randperm(N, generator=gen)[:c], N, gen) for c in counts]
    return torch.cat(idx).int(), torch.tensor(list(counts), dtype=torch.int32)


def make_class_lists(N, counts, gen):
    """Disjoint lists (bmp_nfp_deg_rows: a row has one class): as make_row_lists; rows on no list are class-0 rows."""
    assert sum(counts) <= N
    perm = torch.randperm(N, generator=gen)
    idx, at = [], 0
    for c in counts:
        idx.append(_with_tail(perm[at:at + c], N, gen))
        at += c
    return torch.cat(idx).int(), torch.tensor(list(counts), dtype=torch.int32)


def list_mask(idx, cnt, l, N):
    m = torch.zeros(N, dtype=torch.bool)
    m[_listed(idx, cnt, l, N)] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the fused launch (bmp_launch_wgrad_fused): problem sets, plan, slabs, grid
# ---------------------------------------------------------------------------------------------------------------------
def prob(K, Nn, cs=False, zero_only=False, rfrac=None, wrow=False):
    return dict(K=K, Nn=Nn, cs=cs, zero_only=zero_only, rfrac=rfrac, wrow=wrow)


def step_problems(d, first, lists, live):
    """step_wgrad_problems (bmp_fused.hip)"""
    g1 = prob(d, 2 * d if first else 3 * d)
    g2 = prob(d, d, zero_only=bool(first))
    if not lists:
        return [prob(d, 6 * d if first else 7 * d, cs=True), g1, g2]
    g0 = prob(d, 2 * d if first else 3 * d, cs=True)
    if live and not first:
        g0["rfrac"] = g1["rfrac"] = LIVE_FRAC
    return [g0, g1, g2] + [prob(d, d, cs=True, rfrac=f) for f in TYPE_FRAC]


def rel_problems(d, lists):
    """rel_wgrad_problem (bmp_fused.hip)"""
    if not lists:
        return [prob(d, 5 * d, cs=True, wrow=True)]
    return [prob(d, d, cs=True, wrow=True)] + [prob(d, d, cs=True, rfrac=f) for f in TYPE_FRAC]


def nfp_listed_problems(d_in, d_out):
    """nfp_listed_problems (bmp_nfp.hip): one listed problem per degree class"""
    return [prob(d_in, d_out, rfrac=f) for f in NFP_CLASS_FRAC]


def nfp_listed_ok(N, d_in, d_out):
    return 64 <= d_in <= 128 and d_out >= 64 and d_in % 4 == 0 and d_out % 4 == 0 and N % 32 == 0 and N % WD_RS == 0


def fused_plan(probs, N):
    """wgrad_fused_plan: (S, rps, ty0) -- parts and rows per part of every problem, first column tile of every problem (one
    entry more than problems: the launch's tile count)."""
    tiles = [0 if p["zero_only"] else (p["Nn"] + 127) // 128 for p in probs]
    wtiles = sum(t * (p["rfrac"] if p["rfrac"] is not None else 1.0) for t, p in zip(tiles, probs))
    S, rps, ty0 = [], [], [0]
    for t, p in zip(tiles, probs):
        ty0.append(ty0[-1] + t)
        s = int(512.0 / (wtiles if wtiles > 0.0 else 1.0))
        s = max(min(s, max(N // 256, 1)), 1)
        r = (N + s - 1) // s
        r = (r + 31) & ~31
        sfull = (N + r - 1) // r
        if p["zero_only"]:
            S.append(0)
        elif p["rfrac"] is not None:
            S.append(min(max(int(sfull * p["rfrac"] + 0.5), 1), sfull))
        else:
            S.append(sfull)
        rps.append(r)
    return S, rps, ty0


def slab_floats(probs, N):
    """Floats of ws that bmp_launch_wgrad_fused reaches: the zero row, then S x Krows x Nn per problem."""
    S, _, _ = fused_plan(probs, N)
    end = 128
    for s, p in zip(S, probs):
        want_cs = p["cs"] and not p["zero_only"]
        krows = p["K"] + want_cs + (4 if (p["wrow"] and want_cs) else 0)
        end += s * krows * p["Nn"]
    return end


def fused_ws_floats(probs, N):
    """bmp_wgrad_fused_ws_floats: K + 5 rows reserved per problem whatever it carries"""
    return slab_floats([dict(p, K=p["K"] + 5, cs=False, wrow=False) for p in probs], N)


def grouped_grid(probs, N):
    """wgrad_grouped_grid for the plan of (probs, N): ("plain", T, smax) | ("xcd", remainder splits, workgroups) |
    ("flat", work items)."""
    S, _, ty0 = fused_plan(probs, N)
    T, smax = ty0[-1], max(S)
    if any(s not in (0, smax) for s in S) and T <= WG_MAXT:
        return ("flat", sum(s * (ty0[p + 1] - ty0[p]) for p, s in enumerate(S)))
    if T > 1 and smax >= 8:
        G = smax >> 3
        slots = G * T + ((smax - 8 * G) * T + 7) // 8
        if slots <= 64:
            return ("xcd", smax - 8 * G, 8 * slots)
    return ("plain", T, smax)


def listed_part_rows(count, nsplit):
    """rows of one part of a list of `count` rows cut into nsplit parts (wgrad_dma_body): whole stages"""
    return (((count + nsplit - 1) // nsplit) + WD_RS - 1) // WD_RS * WD_RS


# ---------------------------------------------------------------------------------------------------------------------
# the single-problem launch (bmp_launch_wgrad) and the sizes built on it
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_plan(N, K, Nn):
    """wgrad_plan: (mb, nb, S, rps) of the direct kernel k_wgrad<mb, nb>"""
    mb, nb = (2 if K > 32 else 1), (2 if Nn > 32 else 1)
    tiles = ((K + 64 * mb - 1) // (64 * mb)) * ((Nn + 64 * nb - 1) // (64 * nb))
    S = max(min((512 + tiles - 1) // tiles, max(N // 128, 1)), 1)
    rps = ((N + S - 1) // S + 7) & ~7
    return mb, nb, (N + rps - 1) // rps, rps


def wgrad_lds_plan(N, K, Nn):
    """wgrad_lds_plan: (S, rps) of k_wgrad_lds"""
    tiles = ((K + 127) // 128) * ((Nn + 127) // 128)
    S = max(min(max(512 // tiles, 1), max(N // (128 if tiles == 1 else 256), 1)), 1)
    rps = ((N + S - 1) // S + 31) & ~31
    return (N + rps - 1) // rps, rps


def wgrad_use_lds(N, K, Nn, ldx, ldy, x_aligned=True, dy_aligned=True, onehot=False):
    """wgrad_use_lds: does the problem take the register-staged LDS kernel (else the direct one)?"""
    if onehot:
        return Nn % 4 == 0 and ldy % 4 == 0 and N % 32 == 0 and dy_aligned
    return (K >= 64 and Nn >= 64 and K % 4 == 0 and Nn % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and N % 32 == 0 and
            x_aligned and dy_aligned)


def linear_kernel(N, K, Nn, ldx, ldy, x_aligned=True, dy_aligned=True):
    """name of the GEMM kernel bmp_linear_wgrad launches"""
    if wgrad_use_lds(N, K, Nn, ldx, ldy, x_aligned, dy_aligned):
        return "k_wgrad_lds"
    mb, nb, _, _ = wgrad_plan(N, K, Nn)
    return f"k_wgrad<{mb},{nb}>"


def colsum_ws_floats(N, Nn):
    S = min(max(N // 64, 1), 256)
    rps = (N + S - 1) // S
    return (N + rps - 1) // rps * Nn


def wgrad_ws_floats(N, K, Nn):
    """bmp_wgrad_ws_floats = bmp_wgrad_ws_floats_c: the larger of the two kernels' slabs and the column sums' slab"""
    _, _, S, _ = wgrad_plan(N, K, Nn)
    S2, _ = wgrad_lds_plan(N, K, Nn)
    return max(S * K * Nn, S2 * (K + 1) * Nn, colsum_ws_floats(N, Nn))


def nfp_wgrad_parts(N):
    return min(max(N // 512, 1), 32)


def nfp_layer_wgrad_ws_floats(N, d_in, d_out):
    """bmp_nfp_layer_wgrad_ws_floats"""
    a = nfp_wgrad_parts(N) * NFP_NCLS * d_in * d_out
    if nfp_listed_ok(N, d_in, d_out):
        a = max(a, fused_ws_floats(nfp_listed_problems(d_in, d_out), N))
    return a + colsum_ws_floats(N, d_out)


# ---------------------------------------------------------------------------------------------------------------------
# the cases tests/test_gpu_wgrad_edges.py runs, kept here so that the CPU tests can hold them to the forms they are named for
# ---------------------------------------------------------------------------------------------------------------------
STEP_N = (32, 288, 544, 2848)
LIST_MODES = ("none", "type", "type+live")


def list_counts(N, rot):
    """counts of the four type lists: {0, 1, 15, 16, 17, N - 1, N} rotated over the types"""
    pool = (0, 1, 15, 16, 17, N - 1, N)
    return [pool[(e + rot) % 7] for e in range(4)]


def case_rotation(d, first, accumulate, N, mode):
    """rotation of a (d, first, accumulate, N, lists) case: for every N and mode the 8 (d, first, accumulate) cases reach all 7"""
    return (STEP_N.index(N) + 4 * (int(bool(first)) + 2 * int(bool(accumulate)) + 4 * int(d == 128)) + 32 * LIST_MODES.index(mode)) % 7


LINEAR_DIRECT = ((8, 8), (24, 1), (1, 24), (33, 65), (72, 20), (20, 72), (130, 66))
LINEAR_LDS = ((64, 64), (72, 64), (64, 68), (136, 136), (260, 132))
LINEAR_DIRECT_N = (8, 136, 384, 1160)
LINEAR_LDS_N = (32, 160, 384, 1056)
