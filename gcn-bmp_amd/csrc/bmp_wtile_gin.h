// The GIN layer on whole tiles (see bmp_gin.hip for the arithmetic), ONE body per direction for the whole-tile kernels
// (bmp_gin.hip) and the tile-table kernels (bmp_gin_table.hip).  D and VAR are template parameters.
//
// VAR: the contract of the self loop's table kernels (bmp_wtile_gru.h).  The tile is entry blockIdx.x of a tile table, rows
// [row0, row0 + nrows), nrows = 32 nblk, 1..4 live blocks (clipped to the arrays' mt_rows).  No global access goes to a tile row
// >= nrows, the waves of a dead block skip their MFMA loops and epilogues and still reach every barrier, and with a fixed stride
// > nrows the rows [row0 + nrows, row0 + stride) are written as zeros in every array the kernel writes (relu(b1) of a dead row is
// not zero: the clear is explicit).  The LDS rows of a dead block hold whatever was there: no live row reads them (the gathers
// skip entries >= nrows, an MFMA row reads its own A row only).  The VAR forward takes s == t == nullptr and then stores neither
// (forward-only evaluation).  Without VAR the table is not read, s and t are always stored and the code is the whole-tile one.
#pragma once
#include "bmp_wtile_gru.h"

// this workgroup's tile and its live rows
template <bool VAR>
__device__ __forceinline__ void gin_tile(WgTable tt, int& row0, int& nblk, int& nrows) {
    wg_tile_rows<VAR>(tt, row0, nblk, nrows);
}

template <int D, bool VAR = false>
__device__ __forceinline__ void gin_layer_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                              const float* __restrict__ val, const float* __restrict__ W1p,
                                              const float* __restrict__ b1, const float* __restrict__ W2p,
                                              const float* __restrict__ b2, const float* __restrict__ keep,
                                              float* __restrict__ s, float* __restrict__ t, float* __restrict__ out,
                                              WgTable tt = WgTable{}) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16;
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    int row0, nblk, nrows;
    gin_tile<VAR>(tt, row0, nblk, nrows);
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) < nblk;           // this wave's block has rows
    const bool save = !VAR || s != nullptr;                                           // s and t are kept for a backward
    if constexpr (VAR) {                                      // fixed stride: the rows behind the live ones, in every array written
        const int e = wg_dead_end(tt, row0, nrows);
        fz_clear_rows<512>(s, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(t, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(out, D, row0 + nrows, e, tid);
    }
    wt_load_tile<D, VAR>(ta, h, row0, tid, nrows);
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
        if (!VAR || row < nrows) {
            f32x4 acc[F];
            wt_tile_gather<D, false, VAR>(acc, ta, row, q, row0, ptr, col, val, 1.f, nrows);
            float* d = tb + row * LD + q * (D / 4);
            float* gq = s + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                *(f32x4*)(d + 4 * f) = acc[f];
                if (save) *(f32x4*)(gq + 4 * f) = acc[f];
            }
        }
    }
    __syncthreads();
    f32x16 acc[NB];
    if (blive) {
        wt_wave_mma<D>(acc, tb, LD, W1p, D, wv);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = wt_col(wv, NB, nb);
            const float bc = b1[c];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float v = acc[nb][reg] + bc;
                ta[wt_row(wv, reg) * LD + c] = v > 0.f ? v : 0.f;
            }
        }
    }
    __syncthreads();
    if (blive) {
        wt_wave_mma<D>(acc, ta, LD, W2p, D, wv);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = wt_col(wv, NB, nb);
            const float bc = b2[c];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) tb[wt_row(wv, reg) * LD + c] = acc[nb][reg] + bc;
        }
    }
    __syncthreads();
    const f32x4 z4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < (VAR ? nrows : WT_R) * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        const size_t g = (size_t)(row0 + r) * D + 4 * q4;
        if (save) *(f32x4*)(t + g) = *(const f32x4*)(ta + r * LD + 4 * q4);
        f32x4 p = *(const f32x4*)(tb + r * LD + 4 * q4);
        if (keep) p = p * *(const f32x4*)(keep + g);
        *(f32x4*)(out + g) = __builtin_elementwise_max(p, z4);
    }
}

template <int D, bool VAR = false>
__device__ __forceinline__ void gin_layer_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                              const float* __restrict__ keep, const float* __restrict__ t,
                                              const int* __restrict__ ptrT, const int* __restrict__ colT,
                                              const float* __restrict__ valT, const float* __restrict__ W2np,
                                              const float* __restrict__ W1np, float* __restrict__ dp2,
                                              float* __restrict__ dp1, float* __restrict__ dh, WgTable tt = WgTable{}) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16;
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    int row0, nblk, nrows;
    gin_tile<VAR>(tt, row0, nblk, nrows);
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) < nblk;           // this wave's block has rows
    if constexpr (VAR) {                                      // fixed stride: the rows behind the live ones read as zeros to the
        const int e = wg_dead_end(tt, row0, nrows);           // weight-gradient GEMMs and to the layer below
        fz_clear_rows<512>(dp2, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(dp1, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(dh, D, row0 + nrows, e, tid);
    }
    for (int i = tid; i < (VAR ? nrows : WT_R) * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        const size_t g = (size_t)(row0 + r) * D + 4 * q4;
        const f32x4 ov = *(const f32x4*)(out + g);
        f32x4 v = *(const f32x4*)(dout + g);
        if (keep) v = v * *(const f32x4*)(keep + g);
#pragma unroll
        for (int x = 0; x < 4; ++x) v[x] = ov[x] > 0.f ? v[x] : 0.f;
        *(f32x4*)(dp2 + g) = v;
        *(f32x4*)(ta + r * LD + 4 * q4) = v;
        *(f32x4*)(tb + r * LD + 4 * q4) = *(const f32x4*)(t + g);
    }
    __syncthreads();
    f32x16 acc[NB];
    if (blive) {
        wt_wave_mma<D>(acc, ta, LD, W2np, D, wv);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = wt_col(wv, NB, nb);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {             // every (row, column) of B belongs to one lane: in place
                float* p = tb + wt_row(wv, reg) * LD + c;
                *p = *p > 0.f ? acc[nb][reg] : 0.f;
            }
        }
    }
    __syncthreads();
    if (blive) {
        wt_wave_mma<D>(acc, tb, LD, W1np, D, wv);
        wt_acc_to_tile<D>(ta, acc, wv);
    }
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
        if (!VAR || row < nrows) {
            const float* pq = tb + row * LD + q * (D / 4);
            float* g1 = dp1 + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) *(f32x4*)(g1 + 4 * f) = *(const f32x4*)(pq + 4 * f);
            f32x4 a[F];
            wt_tile_gather<D, false, VAR>(a, ta, row, q, row0, ptrT, colT, valT, 1.f, nrows);
            float* gq = dh + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) *(f32x4*)(gq + 4 * f) = a[f];
        }
    }
}

// What every GIN entry refuses before its launch, one function per direction: the _tile_ entries (bmp_gin.hip) and the _table_
// entries (bmp_gin_table.hip, behind their table's own check) call it.  save_ok: what the entry asks of s and t.
static inline int gin_fwd_check(bool d_ok, bool save_ok, const float* h, int n_tiles, const int* csr_ptr, const float* W1p,
                                const float* b1, const float* W2p, const float* b2, const float* keep, const float* s, const float* t,
                                const float* out) {
    BMP_REQUIRE(h && n_tiles > 0 && d_ok && csr_ptr && W1p && b1 && W2p && b2 && save_ok && out);
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)W1p | (uintptr_t)W2p | (uintptr_t)keep | (uintptr_t)s | (uintptr_t)t | (uintptr_t)out) & 15) == 0);
    return 0;
}
static inline int gin_bwd_check(bool d_ok, const float* dout, const float* out, const float* keep, const float* t, int n_tiles,
                                const int* csrT_ptr, const float* W2np, const float* W1np, const float* dp2, const float* dp1,
                                const float* dh) {
    BMP_REQUIRE(dout && out && t && n_tiles > 0 && d_ok && csrT_ptr && W2np && W1np && dp2 && dp1 && dh);
    BMP_REQUIRE((((uintptr_t)dout | (uintptr_t)out | (uintptr_t)keep | (uintptr_t)t | (uintptr_t)W2np | (uintptr_t)W1np | (uintptr_t)dp2 |
                  (uintptr_t)dp1 | (uintptr_t)dh) & 15) == 0);
    return 0;
}
