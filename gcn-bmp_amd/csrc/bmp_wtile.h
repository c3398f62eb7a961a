// Whole-tile machinery shared by the fused per-tile kernels of the GIN, NFP, gated-GGNN, self-loop and edge-network GGNN encoders
// (bmp_gin.hip, bmp_nfp.hip, bmp_gate.hip, bmp_loop.hip, bmp_edge.hip): one workgroup of 512 threads (8 waves) per 128-row tile, d in {64, 128}, exact-f32 MFMA 32x32x2, two
// [128][d + 4] tiles in LDS used in turn; wave w owns the 32-row block w >> 1 of the operand tile and the column half w & 1 of
// the product.
// Weights are K4-packed ([K/4][N][4], as for bmp_ggnn_step_*): a lane's four k values are one 16-byte load.
// The GRU step that the self-loop and edge-network kernels share is one body on this machinery, in bmp_wtile_gru.h.
// (The half-tile-group kernels of bmp_fused*.hip keep their own loop and gather in bmp_tile.h: tile_mma, tile_gather.)
#pragma once
#include "bmp_tile.h"

#define WT_R 128
static inline size_t wt_lds_bytes(int d) { return (size_t)2 * WT_R * (d + 4) * sizeof(float); }

// a wave's place in the tile and the (row, column) of its accumulator registers: NB column blocks of 32 per wave
struct WtWave { int lane, b, ch; };
__device__ __forceinline__ int wt_row(WtWave wv, int reg) { return wv.b * 32 + bmp_acc_row(reg, wv.lane); }
__device__ __forceinline__ int wt_col(WtWave wv, int NB, int nb) { return (wv.ch * NB + nb) * 32 + (wv.lane & 31); }
__device__ __forceinline__ WtWave wt_wave(int tid) {
    const int w = tid >> 6;
    return WtWave{tid & 63, w >> 1, w & 1};
}

// The VAR form of a primitive serves a tile of a tile table (bmp_tile.h: mt_row0 / mt_nblk), whose rows behind its `nrows` =
// 32 * nblk live rows belong to the next tile or lie past the arrays: no global access goes to a row >= nrows.  Without VAR
// `nrows` is not read and the code is the whole-tile one.
// rows [row0, row0 + 128) of the row-major g [.. x D] -> tile [128][D + 4], 16 bytes per lane
template <int D, bool VAR = false>
__device__ __forceinline__ void wt_load_tile(float* tile, const float* __restrict__ g, int row0, int tid, int nrows = WT_R) {
    for (int i = tid; i < (VAR ? nrows : WT_R) * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        *(f32x4*)(tile + r * (D + 4) + 4 * q4) = *(const f32x4*)(g + (size_t)(row0 + r) * D + 4 * q4);
    }
}

// rows [row0, row0 + 128) of the row-major g [.. x ldg], columns [coff, coff + D) := tile, 16 bytes per lane
template <int D, bool VAR = false>
__device__ __forceinline__ void wt_store_tile(const float* tile, float* __restrict__ g, int ldg, int coff, int row0, int tid,
                                              int nrows = WT_R) {
    for (int i = tid; i < (VAR ? nrows : WT_R) * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        *(f32x4*)(g + (size_t)(row0 + r) * ldg + coff + 4 * q4) = *(const f32x4*)(tile + r * (D + 4) + 4 * q4);
    }
}

// tile := a wave's accumulators, each lane its own (row, column) elements
template <int D>
__device__ __forceinline__ void wt_acc_to_tile(float* tile, const f32x16 (&acc)[D / 64], WtWave wv) {
#pragma unroll
    for (int nb = 0; nb < D / 64; ++nb) {
        const int c = wt_col(wv, D / 64, nb);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) tile[wt_row(wv, reg) * (D + 4) + c] = acc[nb][reg];
    }
}

// acc[nb] += A(32 rows x K) . B(K x 32 cols per nb);  Ar = this lane's A row + 4 * (lane >> 5),
// Bp = packed matrix + ((lane >> 5) * Nw + first column + (lane & 31)) * 4, column blocks 32 apart.
// MASKED: the A rows of the lanes with mine == false count as zeros (rows of another class, nfp_class_walk).
template <int NB, bool MASKED>
__device__ __forceinline__ void wt_block_mma(f32x16 (&acc)[NB], const float* Ar, const float* __restrict__ Bp, int Nw, int K,
                                             bool mine = true) {
    const f32x4 z4 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int k0 = 0; k0 < K; k0 += 8) {
        f32x4 a = *(const f32x4*)(Ar + k0);
        if constexpr (MASKED) a = mine ? a : z4;
        f32x4 b[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) b[nb] = *(const f32x4*)(Bp + ((size_t)(k0 >> 2) * Nw + nb * 32) * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = bmp_mfma(a[t], b[nb][t], acc[nb]);
    }
}

// The same for NG groups of output columns that share the A rows (the gates of one update, the two halves of its transpose):
// acc[g][nb] += A(32 rows x K) . B(K x 32 cols), the column of (g, nb) = first column + g * gs + nb * 32 of a packed matrix
// Nw columns wide.  One A fragment feeds NG * NB MFMAs.
template <int NG, int NB>
__device__ __forceinline__ void wt_block_mma_g(f32x16 (&acc)[NG][NB], const float* Ar, const float* __restrict__ Bp, int Nw, int gs,
                                               int K) {
#pragma unroll 2
    for (int k0 = 0; k0 < K; k0 += 8) {
        const f32x4 a = *(const f32x4*)(Ar + k0);
        f32x4 b[NG][NB];
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) b[g][nb] = *(const f32x4*)(Bp + ((size_t)(k0 >> 2) * Nw + g * gs + nb * 32) * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[g][nb] = bmp_mfma(a[t], b[g][nb][t], acc[g][nb]);
    }
}

// One wave's product, opened: acc = 0, and this lane's addresses into rows [32 b, 32 b + 32) of `opnd` (row stride lda) and
// into the columns of half ch of a packed [K x D] matrix (boff: floats from the matrix's base).
struct WtLane { const float* Ar; size_t boff; };
template <int D>
__device__ __forceinline__ WtLane wt_wave_open(f32x16 (&acc)[D / 64], const float* opnd, int lda, WtWave wv) {
    zero_acc(acc);
    return WtLane{opnd + (wv.b * 32 + (wv.lane & 31)) * lda + 4 * (wv.lane >> 5),
                  ((size_t)(wv.lane >> 5) * D + wv.ch * (D / 64) * 32 + (wv.lane & 31)) * 4};
}
// ... and run: acc = those rows (K wide) times the packed K x D matrix Wp
template <int D>
__device__ __forceinline__ void wt_wave_mma(f32x16 (&acc)[D / 64], const float* opnd, int lda, const float* __restrict__ Wp, int K,
                                            WtWave wv) {
    const WtLane p = wt_wave_open<D>(acc, opnd, lda, wv);
    wt_block_mma<D / 64, false>(acc, p.Ar, Wp + p.boff, D, K);
}

// tile-local gather of one row's quarter (4 threads per row), type-blind: src[row] (SELF: times self) + the sum over the
// row's entries of val * src[col - row0].  VAR: called for rows < nrows only (the walk reads ptr[row0 + row + 1]); an entry that
// points at or behind tile row nrows is skipped.
template <int D, bool SELF, bool VAR = false>
__device__ __forceinline__ void wt_tile_gather(f32x4 (&acc)[D / 16], const float* src, int row, int q, int row0,
                                               const int* __restrict__ ptr, const int* __restrict__ col, const float* __restrict__ val,
                                               float self = 1.f, int nrows = WT_R) {
    constexpr int LD = D + 4, F = D / 16;
    const float* s0 = src + row * LD + q * (D / 4);
#pragma unroll
    for (int f = 0; f < F; ++f) {
        acc[f] = *(const f32x4*)(s0 + 4 * f);
        if constexpr (SELF) acc[f] = acc[f] * self;
    }
    for (int e = ptr[row0 + row]; e < ptr[row0 + row + 1]; ++e) {
        const int j = (col[e] >> 2) - row0;
        if ((unsigned)j >= (unsigned)(VAR ? nrows : WT_R)) continue;      // (molecules never straddle a tile on this path: never taken)
        const float v = val[e];
        const float* s = src + j * LD + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] += *(const f32x4*)(s + 4 * f) * v;
    }
}

// ... and filtered by bond type: the sum over the row's entries of type e (col & 3) of val * src[col - row0], no self term.
// Returns the row's weighted degree for the type (the sum of those entries' values).  VAR: called for rows < nrows only (the
// walk reads ptr[row0 + row + 1]); an entry that points at or behind tile row nrows is skipped.
template <int D, bool VAR = false>
__device__ __forceinline__ float wt_tile_gather_typed(f32x4 (&acc)[D / 16], const float* src, int row, int q, int row0,
                                                      const int* __restrict__ ptr, const int* __restrict__ col,
                                                      const float* __restrict__ val, int e, int nrows = WT_R) {
    constexpr int LD = D + 4, F = D / 16;
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float wd = 0.f;
    for (int ed = ptr[row0 + row]; ed < ptr[row0 + row + 1]; ++ed) {
        const int cv = col[ed];
        if ((cv & 3) != e) continue;
        const int j = (cv >> 2) - row0;
        if ((unsigned)j >= (unsigned)(VAR ? nrows : WT_R)) continue;      // (molecules never straddle a tile on this path: never taken)
        const float v = val[ed];
        const float* s = src + j * LD + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] += *(const f32x4*)(s + 4 * f) * v;
        wd += v;
    }
    return wd;
}

// Pick the <64> / <128> instance of a tile kernel, set its LDS attribute (once per device), launch one workgroup per tile,
// check.  Returns from the calling function on an error.
#define WT_LAUNCH(KERNEL, d, n_tiles, lds_bytes, st, ...)                                                                   \
    do {                                                                                                                    \
        const size_t lds__ = (lds_bytes);                                                                                   \
        const void* fn__ = (d) == 128 ? (const void*)KERNEL<128> : (const void*)KERNEL<64>;                                 \
        if (int rc__ = bmp_lds_attr(fn__, lds__)) return rc__;                                                              \
        if ((d) == 128) hipLaunchKernelGGL(KERNEL<128>, dim3(n_tiles), dim3(512), lds__, st, __VA_ARGS__);                  \
        else hipLaunchKernelGGL(KERNEL<64>, dim3(n_tiles), dim3(512), lds__, st, __VA_ARGS__);                              \
        BMP_LAUNCH_CHECK();                                                                                                 \
    } while (0)
