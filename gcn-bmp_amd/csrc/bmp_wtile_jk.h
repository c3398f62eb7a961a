// The jumping-knowledge step on whole tiles (see bmp_jk.hip for the arithmetic), ONE body per direction for the whole-tile
// kernels (bmp_jk.hip) and the tile-table kernels (bmp_jk_table.hip).  D, NG (Nu = NG d) and VAR are template parameters.
//
// VAR: the contract of the self loop's table kernels (bmp_wtile_gru.h).  The tile is entry blockIdx.x of a tile table, rows
// [row0, row0 + nrows), nrows = 32 nblk, 1..4 live blocks.  No global access goes to a tile row >= nrows, the waves of a dead
// block skip their MFMA loops, accumulator-to-tile writes and epilogues and still reach every barrier, and with a fixed stride
// > nrows the rows [row0 + nrows, row0 + stride) are written as zeros in every array the kernel writes (relu(bU) of a dead row is
// not zero: the clear is explicit).  The LDS rows of a dead block hold whatever was there: no live row reads them (the gathers
// skip entries >= nrows, an MFMA row reads its own A row only).  Without VAR the table is not read and the code is the
// whole-tile one.
#pragma once
#include "bmp_wtile_gru.h"

template <int D, int NG, bool VAR = false>
__device__ __forceinline__ void jk_step_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                            const float* __restrict__ val, const float* __restrict__ WTp,
                                            const float* __restrict__ bE, const float* __restrict__ WsTp,
                                            const float* __restrict__ bs, const float* __restrict__ AUp,
                                            const float* __restrict__ bU, float* __restrict__ m, float* __restrict__ out,
                                            WgTable tt = WgTable{}) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16, NU = NG * D;
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    int row0, nblk;
    wg_tile<VAR>(tt, row0, nblk);
    const int nrows = 32 * nblk;
    const WtWave wv = wt_wave(tid);
    const int row = tid >> 2, q = tid & 3;                    // the gather's and the bias's (row, quarter) of this thread
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) < nblk;           // this wave's block has rows
    const bool rlive = !VAR || row < nrows;                                           // this thread's gather row is one
    if constexpr (VAR) {                                      // fixed stride: the rows behind the live ones, in every array written
        const int e = wg_dead_end(tt, row0, nrows);
        fz_clear_rows<512>(m, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(out, NU, row0 + nrows, e, tid);
    }
    const int aoff = (wv.b * 32 + (wv.lane & 31)) * LD + 4 * (wv.lane >> 5);          // this lane's A rows in a tile
    const size_t bcol = wv.ch * NB * 32 + (wv.lane & 31);                             // its first output column
    wt_load_tile<D, VAR>(ta, h, row0, tid, nrows);
    __syncthreads();
    float wd[4];
    {
        f32x16 am[NB];
        zero_acc(am);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            wd[e] = 0.f;
            if (rlive) {
                f32x4 g[F];
                wd[e] = wt_tile_gather_typed<D, VAR>(g, ta, row, q, row0, ptr, col, val, e, nrows);
                float* d = tb + row * LD + q * (D / 4);
#pragma unroll
                for (int f = 0; f < F; ++f) *(f32x4*)(d + 4 * f) = g[f];
            }
            __syncthreads();
            if (blive) wt_block_mma<NB, false>(am, tb + aoff, WTp + (size_t)e * D * D + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);
            __syncthreads();
        }
        if (WsTp && blive) wt_block_mma<NB, false>(am, ta + aoff, WsTp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);   // the self loop
        if (blive) wt_acc_to_tile<D>(tb, am, wv);
    }
    __syncthreads();
    if (rlive) {   // + sum_e wdeg_e b_e (+ b_s), by the thread that took the row's weighted degrees
        float* d = tb + row * LD + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const int c = q * (D / 4) + 4 * f;
            f32x4 v = *(const f32x4*)(d + 4 * f);
            if (WsTp) v += *(const f32x4*)(bs + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v += *(const f32x4*)(bE + e * D + c) * wd[e];
            *(f32x4*)(d + 4 * f) = v;
            if (m) *(f32x4*)(m + (size_t)(row0 + row) * D + c) = v;
        }
    }
    __syncthreads();
    f32x16 au[NG][NB];
#pragma unroll
    for (int g = 0; g < NG; ++g) zero_acc(au[g]);
    const float* Bu = AUp + ((size_t)(wv.lane >> 5) * NU + bcol) * 4;
    if (blive) {
        wt_block_mma_g<NG, NB>(au, ta + aoff, Bu, NU, D, D);
        wt_block_mma_g<NG, NB>(au, tb + aoff, Bu + (size_t)D * NU, NU, D, D);
    }
    // A wave's products read all d columns of its rows of A and B: nobody writes into A or B before every wave has left them.
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (!blive) continue;
        float* t = (g & 1) ? tb : ta;                         // block 0 -> A, block 1 -> B: one barrier for both
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = wt_col(wv, NB, nb);
            const float bu = bU[g * D + c];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) t[wt_row(wv, reg) * LD + c] = fmaxf(au[g][nb][reg] + bu, 0.f);
        }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NG; ++g) wt_store_tile<D, VAR>((g & 1) ? tb : ta, out, NU, g * D, row0, tid, nrows);
}

template <int D, int NG, bool VAR = false>
__device__ __forceinline__ void jk_step_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                            const int* __restrict__ ptrT, const int* __restrict__ colT,
                                            const float* __restrict__ valT, const float* __restrict__ Wnp,
                                            const float* __restrict__ Wsp, const float* __restrict__ Unp, float* __restrict__ dh,
                                            float* __restrict__ gda, WgTable tt = WgTable{}) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16, NU = NG * D;
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    int row0, nblk;
    wg_tile<VAR>(tt, row0, nblk);
    const int nrows = 32 * nblk;
    const WtWave wv = wt_wave(tid);
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) < nblk;           // this wave's block has rows
    const int aoff = (wv.b * 32 + (wv.lane & 31)) * LD + 4 * (wv.lane >> 5);
    const size_t bcol = wv.ch * NB * 32 + (wv.lane & 31);
    const int pre0 = (Wsp ? 5 : 4) * D, ldg = pre0 + NU;      // gda's dpre columns and its row stride
    if constexpr (VAR) {                                      // fixed stride: the rows behind the live ones read as zeros to the
        const int e = wg_dead_end(tt, row0, nrows);           // weight-gradient GEMMs and to the step below
        fz_clear_rows<512>(dh, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(gda, ldg, row0 + nrows, e, tid);
    }
    f32x16 ad[2][NB];                                         // [0]: dh, [1]: dm
    zero_acc(ad[0]);
    zero_acc(ad[1]);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        float* t = (g & 1) ? tb : ta;                         // in turn: the fill of block g + 1 needs no barrier of its own
        for (int i = tid; i < (VAR ? nrows : WT_R) * (D / 4); i += 512) {
            const int r = i / (D / 4), q4 = i % (D / 4);
            const size_t x = (size_t)(row0 + r) * NU + g * D + 4 * q4;
            const f32x4 dv = *(const f32x4*)(dout + x), ov = *(const f32x4*)(out + x);
            f32x4 dp;
#pragma unroll
            for (int j = 0; j < 4; ++j) dp[j] = ov[j] > 0.f ? dv[j] : 0.f;
            *(f32x4*)(t + r * LD + 4 * q4) = dp;
            *(f32x4*)(gda + (size_t)(row0 + r) * ldg + pre0 + g * D + 4 * q4) = dp;
        }
        __syncthreads();
        if (blive) wt_block_mma_g<2, NB>(ad, t + aoff, Unp + (size_t)g * D * 2 * D + ((size_t)(wv.lane >> 5) * 2 * D + bcol) * 4, 2 * D, D, D);
    }
    // dm -> X, the tile the last product did not read: B for one block (nothing read it), A for two (block 0's product read
    // it, and every wave left that product before the barrier of block 1).  Y, the other tile, is written behind the next barrier.
    float* tx = (NG & 1) ? tb : ta;
    float* ty = (NG & 1) ? ta : tb;
    if (blive) wt_acc_to_tile<D>(tx, ad[1], wv);
    __syncthreads();
    if (Wsp) {                                                // the self loop: dh += dm . Ws, dm into gda
        if (blive) wt_block_mma<NB, false>(ad[0], tx + aoff, Wsp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);
        wt_store_tile<D, VAR>(tx, gda, ldg, 4 * D, row0, tid, nrows);
    }
    {
        const int row = tid >> 2, q = tid & 3;
        const bool rlive = !VAR || row < nrows;               // this thread's gather row is a row of the tile
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (rlive) {
                f32x4 g[F];
                wt_tile_gather_typed<D, VAR>(g, tx, row, q, row0, ptrT, colT, valT, e, nrows);
                float* d = ty + row * LD + q * (D / 4);
                float* gq = gda + (size_t)(row0 + row) * ldg + e * D + q * (D / 4);
#pragma unroll
                for (int f = 0; f < F; ++f) { *(f32x4*)(d + 4 * f) = g[f]; *(f32x4*)(gq + 4 * f) = g[f]; }
            }
            __syncthreads();
            if (blive) wt_block_mma<NB, false>(ad[0], ty + aoff, Wnp + ((size_t)(wv.lane >> 5) * 4 * D + e * D + bcol) * 4, 4 * D, D);
            __syncthreads();
        }
    }
    if (blive) wt_acc_to_tile<D>(ty, ad[0], wv);              // (behind the loop's last barrier)
    __syncthreads();
    wt_store_tile<D, VAR>(ty, dh, D, 0, row0, tid, nrows);
}

// ---------------------------------------------------------------------------------------------------------
// What the aggregators of bmp_jk.hip and the row-count 'mean' of bmp_jk_table.hip share: the T step tensors BY VALUE in the kernel
// arguments (as bmp_agg.hip's AggIn), the launch shape of the elementwise kernels and their per-unit bodies.
// ---------------------------------------------------------------------------------------------------------
#define JK_MAXT BMP_AGG_MAXT
#define JK_TPB 256
#define JK_MAX_BLOCKS 1024

struct JkIn { const float* p[JK_MAXT]; };
struct JkOut { float* p[JK_MAXT]; };

// unit u of sum_t c[t] H_t
template <int T>
__device__ __forceinline__ f32x4 jk_comb_unit(const JkIn& h, size_t u, const float* c) {
    f32x4 o = reinterpret_cast<const f32x4*>(h.p[0])[u] * c[0];
#pragma unroll
    for (int t = 1; t < T; ++t) o += reinterpret_cast<const f32x4*>(h.p[t])[u] * c[t];
    return o;
}
// unit u of dH_t = c[t] dy, every t
template <int T>
__device__ __forceinline__ void jk_scale_unit(const JkOut& dh, size_t u, f32x4 g, const float* c) {
#pragma unroll
    for (int t = 0; t < T; ++t) reinterpret_cast<f32x4*>(dh.p[t])[u] = g * c[t];
}

static inline int jk_blocks(size_t n4) {
    const size_t b = (n4 + JK_TPB - 1) / JK_TPB;
    return (int)(b < 1 ? 1 : (b > JK_MAX_BLOCKS ? JK_MAX_BLOCKS : b));
}

#define JK_T_SWITCH(T, CASE)                                                                          \
    switch (T) {                                                                                      \
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)                               \
        default: return -1000 - __LINE__;                                                             \
    }

static inline bool jk_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// What every step entry refuses before its launch, one function per direction: the _tile_ entries (bmp_jk.hip) and the _table_
// entries (bmp_jk_table.hip, behind their table's own check) call it.  d_ok: the entry's bmp_jk_step_*supported(d).
static inline int jk_fwd_check(bool d_ok, int ng, const float* h, int n_tiles, const int* csr_ptr, const float* WTp, const float* bE,
                               const float* WsTp, const float* bs, const float* AUp, const float* bU, const float* m, const float* out) {
    BMP_REQUIRE((ng == 1 || ng == 2) && h && n_tiles > 0 && d_ok);
    BMP_REQUIRE(csr_ptr && WTp && bE && AUp && bU && out && (WsTp == nullptr) == (bs == nullptr));
    BMP_REQUIRE(jk_aligned(h) && jk_aligned(WTp) && jk_aligned(bE) && jk_aligned(WsTp) && jk_aligned(bs) && jk_aligned(AUp) &&
                jk_aligned(m) && jk_aligned(out));
    return 0;
}
static inline int jk_bwd_check(bool d_ok, int ng, const float* dout, const float* out, int n_tiles, const int* csrT_ptr,
                               const float* Wnat_p, const float* Ws_p, const float* Unat_p, const float* dh, const float* gda) {
    BMP_REQUIRE((ng == 1 || ng == 2) && dout && out && n_tiles > 0 && d_ok);
    BMP_REQUIRE(csrT_ptr && Wnat_p && Unat_p && dh && gda);
    BMP_REQUIRE(jk_aligned(dout) && jk_aligned(out) && jk_aligned(Wnat_p) && jk_aligned(Ws_p) && jk_aligned(Unat_p) && jk_aligned(dh) &&
                jk_aligned(gda));
    return 0;
}
