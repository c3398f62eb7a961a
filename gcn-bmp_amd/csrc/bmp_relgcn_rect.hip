// Fused RelGCN layer for unequal widths (models/update/relgcn_update.py:24-44 + the tanh of models/relgcn.py:71):
//   out = act(h W_s^T + b_s + sum_e adj'_e (W_e h + b_e)),   h [N x DI] -> out [N x DO],  DI != DO
// -- the default stack of models/relgcn.py:37, ch_list = [16, 128, 64], is two such layers.  The square kernels of bmp_fused.hip
// (DI == DO in {64, 128}) stay as they are; this file is the same arithmetic on the whole-tile machinery of bmp_wtile.h:
//
//   workgroup = 512 threads = 8 waves per 128-row tile, two [128 x (W + 4)] f32 tiles in LDS (W = DI forward, DO backward:
//   the width of the GATHERED operand) + the tile's CSR entries (stage_csr, bmp_tile.h), 147 KB at W = 128;
//   wave w owns the 32-row block w >> 1 and the column half w & 1 of the [128 x DO] (forward) / [128 x DI] (backward)
//   product; exact-f32 MFMA 32x32x2 (tile_mma, bmp_tile.h), weights K4-packed and streamed from L2 two k-steps ahead;
//   gather first, then multiply: per bond type the tile-local typed gather (wt_tile_gather_typed) fills the second tile,
//   and the 32-row blocks without a row of that type skip the type's product.
//
// The rows of block b are gathered by waves 2 b, 2 b + 1 (4 threads per row) and multiplied by the same two waves.
// A product narrower than 64 columns (DO = 32 forward; DI = 16 / 32 backward) is ONE 32-column block per row block: the
// waves with w & 1 == 1 have no product there (they still gather).  DI = 16 in the backward: Ws_p / Wnat_p come zero-padded
// to 32 output columns per block (bmp/functional.py: rel_rect_pack_bwd) and 16 columns of the product are stored.
// VAR: the tile is an entry of a tile table (mt_row0 / mt_nblk, 1..4 live 32-row blocks): no global access goes to a tile row
// >= nrows, the waves of a dead block skip their products and still reach every barrier.  No atomics on floats, every sum in
// a fixed order: two runs are bit-identical.  No kernel of this file spills.
#include "bmp_kernels.h"
#include "bmp_wtile_gru.h"

struct RectArgs {
    const int* ptr; const int* col; const float* val;      // CSR (fwd) or transposed CSR (bwd)
    int tile0;                      // the launch covers tiles tile0 .. tile0 + gridDim.x - 1 (all arrays whole)
    int act;
    const int* mt_row0; const int* mt_nblk;     // optional tile table (already advanced by tile0)
    int mt_rows;
    // forward
    const float* h;                 // [N x DI]
    const float* WT;                // [4 DI x DO]  K4-packed, rows e * DI + k
    const float* bE;                // [4 x DO]
    const float* WsT;               // [DI x DO]    K4-packed
    const float* bs;                // [DO]
    float* out;                     // [N x DO]
    float* wdeg;                    // [N x 4] or null (forward-only evaluation)
    // backward
    const float* dout; const float* y;          // [N x DO]
    const float* Wnat;              // [DO x 4 DIP] (= WT^T, DIP = max(DI, 32) columns per type) K4-packed
    const float* Ws;                // [DO x DIP]   (= WsT^T) K4-packed
    float* dh;                      // [N x DI]
    float* gda;                     // [N x 5 DO]: G_0..G_3 | dpre
    int skip_zero_g;
};

#define RR_CSR_INTS (132 + 2 * FZ_ECAP + WT_R + 8)          // row pointers, entries, values, row type masks, block type masks
static inline size_t rr_lds_bytes(int W) { return ((size_t)2 * WT_R * (W + 4) + 4 * WT_R + RR_CSR_INTS) * sizeof(float); }

// The LDS behind the two operand tiles and the tile's graph in it.
struct RectLds {
    float* wds;         // [128 x 4] weighted degree per bond type (forward)
    int* rptr;          // [132] tile-relative row pointers
    int* ecol;          // [FZ_ECAP] entries, columns tile-relative (type in the low two bits)
    float* evalv;       // [FZ_ECAP]
    int* rmask;         // [128] bit e: the row has an entry of type e
    int* bmask;         // [4]   ... some row of the 32-row block has
    bool staged;        // the tile's entries fit FZ_ECAP; else the gathers walk the global arrays
};

template <bool VAR>
__device__ __forceinline__ void rr_tile(const RectArgs& a, int& row0, int& nblk, int& nrows) {
    if constexpr (VAR) {
        wg_tile_rows<true>(WgTable{a.mt_row0, a.mt_nblk, a.mt_rows, 0}, row0, nblk, nrows);
    } else {
        row0 = (blockIdx.x + a.tile0) * WT_R; nblk = WT_R / 32; nrows = WT_R;
    }
}

// Stage the tile's CSR (columns made tile-relative by the threads that staged them).  The caller's barrier follows.
__device__ __forceinline__ RectLds rr_stage(float* behind_tiles, const RectArgs& a, int row0, int nrows, int tid) {
    RectLds g;
    g.wds = behind_tiles;
    g.rptr = (int*)(g.wds + 4 * WT_R);
    g.ecol = g.rptr + 132;
    g.evalv = (float*)(g.ecol + FZ_ECAP);
    g.rmask = (int*)(g.evalv + FZ_ECAP);
    g.bmask = g.rmask + WT_R;
    g.staged = stage_csr(a.ptr, a.col, a.val, row0, g.rptr, g.ecol, g.evalv, nrows);
    if (g.staged) {
        const int ne = a.ptr[row0 + nrows] - a.ptr[row0];
        for (int i = tid; i < ne; i += 512) g.ecol[i] -= 4 * row0;
    }
    return g;
}

// After the barrier behind rr_stage: which bond types every row and every 32-row block has (waves 0 and 1, a row per lane).
// Visible to all after the caller's next barrier.
__device__ __forceinline__ void rr_type_masks(const RectLds& g, const RectArgs& a, int row0, int nrows, int tid) {
    if (tid >= WT_R) return;
    int m = 0;
    if (tid < nrows) {
        if (g.staged) { for (int ed = g.rptr[tid]; ed < g.rptr[tid + 1]; ++ed) m |= 1 << (g.ecol[ed] & 3); }
        else { for (int ed = a.ptr[row0 + tid]; ed < a.ptr[row0 + tid + 1]; ++ed) m |= 1 << (a.col[ed] & 3); }
    }
    g.rmask[tid] = m;
    int lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned long long bal = __ballot((m >> e) & 1);
        lo |= ((unsigned)bal != 0u) << e;
        hi |= ((unsigned)(bal >> 32) != 0u) << e;
    }
    if ((tid & 63) == 0) { g.bmask[2 * (tid >> 6)] = lo; g.bmask[2 * (tid >> 6) + 1] = hi; }
}

// one row's quarter of the type-e gather over the tile `src` ([128 x (D + 4)])
template <int D, bool VAR>
__device__ __forceinline__ float rr_gather(f32x4 (&acc)[D / 16], const float* src, int row, int q, const RectLds& g, const RectArgs& a,
                                           int row0, int e, int nrows) {
    return g.staged ? wt_tile_gather_typed<D, VAR>(acc, src, row, q, 0, g.rptr, g.ecol, g.evalv, e, nrows)
                    : wt_tile_gather_typed<D, VAR>(acc, src, row, q, row0, a.ptr, a.col, a.val, e, nrows);
}

// acc += (this wave's 32 rows of an LDS tile, K wide) . (NB 32-column blocks from column c0 of a K4-packed [K x N] matrix), on
// tile_mma (bmp_tile.h): the B fragments come from L2 two k-steps ahead of the MFMAs that use them.
template <int NB>
__device__ __forceinline__ void rr_mma(f32x16 (&acc)[NB][1], const float* As_wave, int LD, const float* Wp, int N, int c0, int K, int rot) {
    const float* Bp[NB];
    int ldw[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { Bp[nb] = Wp + (size_t)(4 * (threadIdx.x >> 5 & 1)) * N + 4 * (c0 + nb * 32); ldw[nb] = N; }
    tile_mma<NB, 1, 1>(acc, As_wave, LD, Bp, ldw, K, rot);
}

template <int DI, int DO, bool VAR>
__global__ __launch_bounds__(512) void k_relgcn_rect_fwd(RectArgs a) {
    constexpr int LD = DI + 4, F = DI / 16;
    constexpr int NB = DO >= 64 ? DO / 64 : 1;               // 32-column blocks of the product per wave
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* ta = sm;                          // [128 x LD]  h tile
    float* tb = sm + WT_R * LD;              // [128 x LD]  A_e, one bond type at a time
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    int row0, nblk, nrows;
    rr_tile<VAR>(a, row0, nblk, nrows);
    if (VAR && nrows <= 0) return;           // (uniform: before any barrier)
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) < nblk;           // this wave's block has rows
    const bool wmma = blive && (DO >= 64 || __builtin_amdgcn_readfirstlane(wv.ch) == 0);     // ... and this wave a product
    wt_load_tile<DI, VAR>(ta, a.h, row0, tid, nrows);
    const RectLds g = rr_stage(tb + WT_R * LD, a, row0, nrows, tid);
    __syncthreads();
    rr_type_masks(g, a, row0, nrows, tid);

    const int l31 = wv.lane & 31, hi = wv.lane >> 5;
    const int aoff = (wv.b * 32 + l31) * LD + 4 * hi;                                 // this lane's A rows in a tile
    const int c0 = wv.ch * NB * 32 + l31;                                             // its first output column
    const int rot = ((blockIdx.x + a.tile0) * 8) % DI;                                // (tile_mma: where this tile's K loops start)
    f32x16 acc[NB][1];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) zero_acc(acc[nb]);
    if (wmma) rr_mma<NB>(acc, ta + aoff, LD, a.WsT, DO, c0, DI, rot);                 // self connection: h . W_s^T
    const int row = tid >> 2, q = tid & 3;
    const bool rlive = !VAR || row < nrows;
    for (int e = 0; e < 4; ++e) {
        if (rlive) {
            f32x4 ga[F];
            const float wd = rr_gather<DI, VAR>(ga, ta, row, q, g, a, row0, e, nrows);
            float* d = tb + row * LD + q * (DI / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) *(f32x4*)(d + 4 * f) = ga[f];
            if (q == 0) g.wds[row * 4 + e] = wd;
        }
        __syncthreads();
        if (wmma && ((g.bmask[wv.b] >> e) & 1)) rr_mma<NB>(acc, tb + aoff, LD, a.WT + (size_t)e * DI * DO, DO, c0, DI, rot);
        if (e < 3) __syncthreads();          // tb is free for the next type
    }
    if (wmma) {
        const int act = a.act;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = c0 + nb * 32;
            float be[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) be[e] = a.bE[e * DO + c];
            const float bsv = a.bs ? a.bs[c] : 0.f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = wt_row(wv, reg);
                if (VAR && r >= nrows) continue;
                const f32x4 wd4 = *(const f32x4*)(g.wds + r * 4);
                const float v = acc[nb][0][reg] + bsv + wd4[0] * be[0] + wd4[1] * be[1] + wd4[2] * be[2] + wd4[3] * be[3];
                a.out[(size_t)(row0 + r) * DO + c] = bmp_act(act, v);
            }
        }
    }
    // the backward's operand: not written in forward-only evaluation (the wds rows were complete at the last barrier)
    if (a.wdeg != nullptr && tid < WT_R && tid < nrows) *(f32x4*)(a.wdeg + (size_t)(row0 + tid) * 4) = *(const f32x4*)(g.wds + tid * 4);
}

template <int DI, int DO, bool VAR>
__global__ __launch_bounds__(512) void k_relgcn_rect_bwd(RectArgs a) {
    constexpr int LD = DO + 4, F = DO / 16;
    constexpr int DIP = DI < 32 ? 32 : DI;                   // columns per block of the packed Ws_p / Wnat_p
    constexpr int NB = DIP >= 64 ? DIP / 64 : 1;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* tx = sm;                          // [128 x LD]  dpre (read-only after the prologue)
    float* ty = sm + WT_R * LD;              // [128 x LD]  G_e, one bond type at a time
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    int row0, nblk, nrows;
    rr_tile<VAR>(a, row0, nblk, nrows);
    if (VAR && nrows <= 0) return;
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) < nblk;
    const bool wmma = blive && (DIP >= 64 || __builtin_amdgcn_readfirstlane(wv.ch) == 0);
    {   // dpre = dout * act'(out) -> tx and gda[:, 4 DO:]
        const int act = a.act;
        for (int i = tid; i < (VAR ? nrows : WT_R) * (DO / 4); i += 512) {
            const int r = i / (DO / 4), c4 = i % (DO / 4);
            const size_t go = (size_t)(row0 + r) * DO + 4 * c4;
            const f32x4 g4 = *(const f32x4*)(a.dout + go), y4 = *(const f32x4*)(a.y + go);
            f32x4 dp;
#pragma unroll
            for (int t = 0; t < 4; ++t) dp[t] = g4[t] * bmp_dact(act, y4[t]);
            *(f32x4*)(tx + r * LD + 4 * c4) = dp;
            *(f32x4*)(a.gda + (size_t)(row0 + r) * 5 * DO + 4 * DO + 4 * c4) = dp;
        }
    }
    const RectLds g = rr_stage(ty + WT_R * LD, a, row0, nrows, tid);
    __syncthreads();
    rr_type_masks(g, a, row0, nrows, tid);

    const int l31 = wv.lane & 31, hi = wv.lane >> 5;
    const int aoff = (wv.b * 32 + l31) * LD + 4 * hi;
    const int c0 = wv.ch * NB * 32 + l31;                     // this lane's first column of dh
    const int rot = (blockIdx.x * 8) % DO;
    f32x16 acc[NB][1];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) zero_acc(acc[nb]);
    if (wmma) rr_mma<NB>(acc, tx + aoff, LD, a.Ws, DIP, c0, DO, rot);                 // dh = dpre . W_s
    const int row = tid >> 2, q = tid & 3;
    const bool rlive = !VAR || row < nrows;
    const int skip = a.skip_zero_g;
    for (int e = 0; e < 4; ++e) {
        if (rlive) {
            f32x4 ga[F];
            rr_gather<DO, VAR>(ga, tx, row, q, g, a, row0, e, nrows);
            float* d = ty + row * LD + q * (DO / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) *(f32x4*)(d + 4 * f) = ga[f];
        }
        __syncthreads();                     // (the first one also publishes the type masks)
        // G_e -> gda[:, e DO:] from the tile, row-major: a row's DO / 4 lanes write DO * 4 contiguous bytes (from the gather's
        // registers every lane of a store would touch a 128-byte line of its own)
        for (int i = tid; i < (VAR ? nrows : WT_R) * (DO / 4); i += 512) {
            const int r = i / (DO / 4), q4 = i % (DO / 4);
            if (skip && !((g.rmask[r] >> e) & 1)) continue;
            *(f32x4*)(a.gda + (size_t)(row0 + r) * 5 * DO + e * DO + 4 * q4) = *(const f32x4*)(ty + r * LD + 4 * q4);
        }
        if (wmma && ((g.bmask[wv.b] >> e) & 1)) rr_mma<NB>(acc, ty + aoff, LD, a.Wnat, 4 * DIP, e * DIP + c0, DO, rot);
        if (e < 3) __syncthreads();
    }
    if (wmma) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = c0 + nb * 32;
            if (DI < 32 && c >= DI) continue;                 // the zero-padded columns
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = wt_row(wv, reg);
                if (VAR && r >= nrows) continue;
                a.dh[(size_t)(row0 + r) * DI + c] = acc[nb][0][reg];
            }
        }
    }
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------
#define RR_PAIRS(X) X(16, 32) X(16, 64) X(16, 128) X(32, 64) X(32, 128) X(64, 32) X(64, 128) X(128, 32) X(128, 64)

extern "C" int bmp_relgcn_rect_supported(int d_in, int d_out) {
#define RR_IS(di, dn) if (d_in == di && d_out == dn) return 1;
    RR_PAIRS(RR_IS)
#undef RR_IS
    return 0;
}

template <int DI, int DO, bool VAR>
static int rr_launch2(bool bwd, const RectArgs& a, int n_tiles, hipStream_t st) {
    const void* fn = bwd ? (const void*)k_relgcn_rect_bwd<DI, DO, VAR> : (const void*)k_relgcn_rect_fwd<DI, DO, VAR>;
    const size_t lds = rr_lds_bytes(bwd ? DO : DI);
    if (int rc = bmp_lds_attr(fn, lds)) return rc;
    const double rows = VAR ? (double)a.mt_rows : (double)n_tiles * WT_R;
    BmpProfScope prof(bwd ? BMP_KCLS_STEP_BWD : BMP_KCLS_STEP_FWD, 2.0 * rows * 5.0 * DI * DO, 4.0 * rows * (bwd ? 7.0 * DO + DI : DI + DO), st,
                      BMP_KID_RELGCN);
    if (bwd) hipLaunchKernelGGL((k_relgcn_rect_bwd<DI, DO, VAR>), dim3(n_tiles), dim3(512), lds, st, a);
    else hipLaunchKernelGGL((k_relgcn_rect_fwd<DI, DO, VAR>), dim3(n_tiles), dim3(512), lds, st, a);
    BMP_LAUNCH_CHECK();
    return 0;
}

static int rr_launch(bool bwd, int d_in, int d_out, const RectArgs& a, int n_tiles, hipStream_t st) {
#define RR_GO(di, dn)                                                                                                       \
    if (d_in == di && d_out == dn)                                                                                          \
        return a.mt_row0 ? rr_launch2<di, dn, true>(bwd, a, n_tiles, st) : rr_launch2<di, dn, false>(bwd, a, n_tiles, st);
    RR_PAIRS(RR_GO)
#undef RR_GO
    return -1;
}

// a table comes whole (both arrays, rows in them) or not at all
static inline bool rr_table_ok(const int* mt_row0, const int* mt_nblk, int mt_rows) {
    return (mt_row0 == nullptr && mt_nblk == nullptr) || bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, 0, WT_R);
}
static inline bool rr_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// out = act(h . WsT + bs + sum_e gather_e(h) . WT_e + wdeg_e * bE_e); WT [4 d_in x d_out] and WsT [d_in x d_out] K4-packed
// (bmp/functional.py: pack_k4).  Saves wdeg [N x 4] unless it is null.
extern "C" int bmp_relgcn_rect_fwd(const float* h, int tile0, int n_tiles, int d_in, int d_out, const int* csr_ptr, const int* csr_col,
                                   const float* csr_val, const float* WT, const float* bE, const float* WsT, const float* bs, int act,
                                   float* out, float* wdeg, const int* mt_row0, const int* mt_nblk, int mt_rows, hipStream_t st) {
    BMP_REQUIRE(tile0 >= 0 && n_tiles > 0 && bmp_relgcn_rect_supported(d_in, d_out) && rr_table_ok(mt_row0, mt_nblk, mt_rows));
    BMP_REQUIRE(h && csr_ptr && WT && bE && WsT && out);        // (a batch without a bond has no csr_col / csr_val)
    BMP_REQUIRE(rr_al16(h) && rr_al16(WT) && rr_al16(WsT) && rr_al16(out) && rr_al16(wdeg));
    RectArgs a; memset(&a, 0, sizeof(a));
    a.ptr = csr_ptr; a.col = csr_col; a.val = csr_val; a.act = act; a.tile0 = tile0; a.mt_rows = mt_rows;
    a.mt_row0 = mt_row0 ? mt_row0 + tile0 : nullptr; a.mt_nblk = mt_nblk ? mt_nblk + tile0 : nullptr;
    a.h = h; a.WT = WT; a.bE = bE; a.WsT = WsT; a.bs = bs; a.out = out; a.wdeg = wdeg;
    return rr_launch(false, d_in, d_out, a, n_tiles, st);
}

// The weight gradients of the pairs with d_in >= 64 and d_out >= 64 come from ONE bmp_launch_wgrad_fused call, which walks the
// per-type row lists; every other pair's from the all-rows launches, which read every row of gda.
static bool rr_wgrad_fused(int d_in, int d_out) { return d_in >= 64 && d_out >= 64; }
extern "C" int bmp_relgcn_rect_lists_used(int N, int d_in, int d_out) {
    return bmp_relgcn_rect_supported(d_in, d_out) && rr_wgrad_fused(d_in, d_out) && N > 0 && (N & 31) == 0 && bmp_wgrad_fused_lists_ok(N);
}

// dh [N x d_in] and gda [N x 5 d_out] = [G_0..G_3 | dpre] for bmp_relgcn_rect_wgrad.  Wnat [d_out x 4 dip] = WT^T and
// Ws [d_out x dip] = WsT^T, K4-packed, dip = max(d_in, 32) columns per block (the columns behind d_in zeros).
// skip_zero_g != 0 needs a pair whose weight-gradient launch reads gda through the row lists (bmp_relgcn_rect_lists_used):
// for any other pair it is an error, nothing is launched.
extern "C" int bmp_relgcn_rect_bwd(const float* dout, const float* out, int act, int n_tiles, int d_in, int d_out, const int* csrT_ptr,
                                   const int* csrT_col, const float* csrT_val, const float* Wnat, const float* Ws, float* dh, float* gda,
                                   const int* mt_row0, const int* mt_nblk, int mt_rows, int skip_zero_g, hipStream_t st) {
    BMP_REQUIRE(n_tiles > 0 && bmp_relgcn_rect_supported(d_in, d_out) && rr_table_ok(mt_row0, mt_nblk, mt_rows));
    BMP_REQUIRE(!skip_zero_g || rr_wgrad_fused(d_in, d_out));
    BMP_REQUIRE(dout && out && csrT_ptr && Wnat && Ws && dh && gda);
    BMP_REQUIRE(rr_al16(dout) && rr_al16(out) && rr_al16(Wnat) && rr_al16(Ws) && rr_al16(dh) && rr_al16(gda));
    RectArgs a; memset(&a, 0, sizeof(a));
    a.ptr = csrT_ptr; a.col = csrT_col; a.val = csrT_val; a.act = act; a.mt_row0 = mt_row0; a.mt_nblk = mt_nblk; a.mt_rows = mt_rows;
    a.dout = dout; a.y = out; a.Wnat = Wnat; a.Ws = Ws; a.dh = dh; a.gda = gda; a.skip_zero_g = skip_zero_g;
    return rr_launch(true, d_in, d_out, a, n_tiles, st);
}

// rel_wgrad_problem of bmp_fused.hip with K = d_in and d_out-wide blocks
static const float kRectTypeFrac[4] = {0.78f, 0.24f, 0.05f, 0.58f};       // expected shares of listed rows: balance only
static int rr_wgrad_problem(WGArgs* g, const float* h, const float* wdeg, const float* gda, int N, int di, int dn, float* o1, float* dbE,
                            float* cs, int accumulate, const int* type_rows = nullptr, const int* type_cnt = nullptr) {
    if (type_rows == nullptr) {
        g[0] = WGArgs{h, nullptr, di, 0, gda, 5 * dn, di, 5 * dn, N, o1, 5 * dn, accumulate, cs};
        g[0].wrow = wdeg; g[0].w_col0 = 4 * dn; g[0].wout = dbE; g[0].ldwo = dn;      // dbE = wdeg^T . dpre rides along
        return 1;
    }
    g[0] = WGArgs{h, nullptr, di, 0, gda + 4 * dn, 5 * dn, di, dn, N, o1 + 4 * dn, 5 * dn, accumulate, cs + 4 * dn};
    g[0].wrow = wdeg; g[0].w_col0 = 0; g[0].wout = dbE; g[0].ldwo = dn;
    for (int e = 0; e < 4; ++e) {
        g[1 + e] = WGArgs{h, nullptr, di, 0, gda + e * dn, 5 * dn, di, dn, N, o1 + e * dn, 5 * dn, accumulate, cs + e * dn};
        g[1 + e].ridx = type_rows + (size_t)e * N; g[1 + e].rcnt = type_cnt + e; g[1 + e].rfrac = kRectTypeFrac[e];
    }
    return 5;
}

static inline size_t rr_max(size_t a, size_t b) { return a > b ? a : b; }

extern "C" size_t bmp_relgcn_rect_wgrad_ws_floats(int N, int d_in, int d_out) {
    if (N <= 0 || !bmp_relgcn_rect_supported(d_in, d_out)) return 0;
    if (rr_wgrad_fused(d_in, d_out)) {
        if (N & 31) return 0;
        WGArgs g[BMP_WG_MAXP];
        int n = rr_wgrad_problem(g, nullptr, (const float*)16, nullptr, N, d_in, d_out, nullptr, (float*)16, (float*)16, 0);
        const size_t a = bmp_wgrad_fused_ws_floats(g, n);
        n = rr_wgrad_problem(g, nullptr, (const float*)16, nullptr, N, d_in, d_out, nullptr, (float*)16, (float*)16, 0, (const int*)16,
                             (const int*)16);
        return rr_max(a, bmp_wgrad_fused_ws_floats(g, n));
    }
    return rr_max(rr_max(bmp_wgrad_ws_floats(N, d_in, 5 * d_out), bmp_wgrad_ws_floats(N, 4, d_out)), bmp_colsum_ws_floats(N, 5 * d_out));
}

// Weight gradients of one layer (reduction over all N rows), from the existing weight-gradient GEMM family:
//   o1 [d_in x 5 d_out] = h^T . gda     cols [0, 4 d_out): dWT as [k][e * d_out + c];  cols [4 d_out, 5 d_out): dWsT
//   dbE [4 x d_out]     = wdeg^T . dpre
//   cs [5 d_out]        = column sums of gda; cs[4 d_out:] = dbs
// d_in >= 64 and d_out >= 64: one fused launch + one reduction, through type_rows / type_cnt (as bmp_ggnn_step_wgrad) when
// bmp_relgcn_rect_lists_used; N a multiple of 32.  Every other pair: the all-rows launches (o1 with its column sums, then dbE as
// a K = 4 problem on wdeg), which read every row of gda -- the lists are not used; N a multiple of 8.
extern "C" int bmp_relgcn_rect_wgrad(const float* h, const float* wdeg, const float* gda, int N, int d_in, int d_out, float* o1,
                                     float* dbE, float* cs, int accumulate, const int* type_rows, const int* type_cnt, float* ws,
                                     size_t ws_floats, hipStream_t st) {
    BMP_REQUIRE(N > 0 && bmp_relgcn_rect_supported(d_in, d_out) && ws_floats >= bmp_relgcn_rect_wgrad_ws_floats(N, d_in, d_out));
    BMP_REQUIRE(h && wdeg && gda && o1 && dbE && cs && ws);
    BMP_REQUIRE(rr_al16(h) && rr_al16(gda) && rr_al16(wdeg));
    const int acc = accumulate ? 1 : 0;
    if (rr_wgrad_fused(d_in, d_out)) {
        BMP_REQUIRE((N & 31) == 0);
        WGArgs g[BMP_WG_MAXP];
        const bool lists = type_rows != nullptr && type_cnt != nullptr && bmp_relgcn_rect_lists_used(N, d_in, d_out);
        const int n = rr_wgrad_problem(g, h, wdeg, gda, N, d_in, d_out, o1, dbE, cs, acc, lists ? type_rows : nullptr,
                                       lists ? type_cnt : nullptr);
        return bmp_launch_wgrad_fused(g, n, ws, st, BMP_KID_WGRAD_STEP);
    }
    BMP_REQUIRE((N & 7) == 0);
    const WGArgs g1{h, nullptr, d_in, 0, gda, 5 * d_out, d_in, 5 * d_out, N, o1, 5 * d_out, acc, cs};
    if (int rc = bmp_launch_wgrad(g1, ws, st)) return rc;
    const WGArgs g2{wdeg, nullptr, 4, 0, gda + 4 * d_out, 5 * d_out, 4, d_out, N, dbE, d_out, acc};
    return bmp_launch_wgrad(g2, ws, st);
}
