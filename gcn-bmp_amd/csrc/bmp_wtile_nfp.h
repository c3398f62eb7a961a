// The NFP layer and its softmax readout on whole tiles (see bmp_nfp.hip for the arithmetic), ONE body per kernel for the
// whole-tile kernels (bmp_nfp.hip) and the tile-table kernels (bmp_nfp_table.hip).  D and VAR are template parameters.
//
// Degree-class walk: the tile's rows are ranked by (class 1..7, then class 0; row) -- a fixed order, computed from the
// classes alone -- and the operand rows (fv forward, dpre backward) are laid into LDS at their ranks.  A 32-row block of
// the ranked tile then holds a contiguous run of classes; for every class present in the block the wave runs the MFMAs of
// that class's matrix over the block with the other rows zeroed in the A operand.  Every row belongs to one class, so its
// accumulators receive its product once plus exact zeros; blocks of class-0 rows (pad rows, dead rows at the tile's end,
// hubs) run no MFMA at all.  Work = (block, class) pairs present: at most blocks + classes - 1 block passes per tile.
// Weights are K4-packed per class ([K/4][N][4], as for bmp_ggnn_step_*): a lane's four k values are one 16-byte load.
//
// VAR: the contract of the GIN layer's table kernels (bmp_wtile_gin.h).  The tile is entry blockIdx.x of a tile table, rows
// [row0, row0 + nrows), nrows = 32 nblk, 1..4 live blocks (clipped to the arrays' mt_rows).  No global access goes to a tile
// row >= nrows -- not h, not the classes, not self_w, not row_mol: the ranking counts those rows as class 0 without loading
// them, so they rank behind every live row and the ranked blocks [0, nblk) hold exactly the live rows.  The waves of the other
// blocks skip their products and epilogues and still reach every barrier.  With a fixed stride > nrows the rows [row0 + nrows,
// row0 + stride) are written as zeros in every row array the kernel writes (sigmoid(B) of a dead row is not zero: the clear is
// explicit).  The VAR layer forward takes fv == nullptr and then stores none (forward-only evaluation).  Without VAR the table
// is not read and the code is the whole-tile one.
#pragma once
#include "bmp_wtile_gru.h"

#define NFP_NCLS 7          // degree classes 1..7 (max_degree 6 + 1, nfp.py:26,111); class 0 = none of them
#define NFP_LDZ 132         // row stride of the readout's z / dz tile (o <= 128)

struct NfpOrder { int scl[WT_R]; int skey[WT_R]; unsigned char inv[WT_R]; unsigned char perm[WT_R]; };
// rank of every tile row in the order (class 1..7, class 0; row); ends with a workgroup barrier
template <bool VAR>
__device__ __forceinline__ void nfp_rank_rows(NfpOrder& o, const int* __restrict__ cls, int row0, int nrows) {
    const int tid = threadIdx.x;
    if (tid < WT_R) o.scl[tid] = (!VAR || tid < nrows) ? cls[row0 + tid] : 0;
    __syncthreads();
    if (tid < WT_R) {
        const int c = o.scl[tid], key = c ? c : 8;
        int pos = 0;
        for (int j = 0; j < WT_R; ++j) {
            const int cj = o.scl[j], kj = cj ? cj : 8;
            pos += (kj < key || (kj == key && j < tid)) ? 1 : 0;
        }
        o.inv[tid] = (unsigned char)pos;
        o.perm[pos] = (unsigned char)tid;
        o.skey[pos] = c;
    }
    __syncthreads();
}
// the class walk of one wave: acc = ranked block wv.b of `opnd` times the class matrices Wp [7][D x D packed]
template <int D>
__device__ __forceinline__ void nfp_class_walk(f32x16 (&acc)[D / 64], const float* opnd, const NfpOrder& o, const float* __restrict__ Wp,
                                               WtWave wv) {
    const int c_l = o.skey[wv.b * 32 + (wv.lane & 31)];
    const WtLane p = wt_wave_open<D>(acc, opnd, D + 4, wv);
    for (int k = 1; k <= NFP_NCLS; ++k)
        if (__ballot(c_l == k)) wt_block_mma<D / 64, true>(acc, p.Ar, Wp + (size_t)(k - 1) * D * D + p.boff, D, D, c_l == k);
}

template <int D, bool VAR = false>
__device__ __forceinline__ void nfp_layer_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                              const float* __restrict__ val, const float* __restrict__ self_w,
                                              const int* __restrict__ cls, const float* __restrict__ WTp,
                                              const float* __restrict__ B, float* __restrict__ fv, float* __restrict__ out,
                                              WgTable tt = WgTable{}) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16;
    extern __shared__ float sm[];
    float* ht = sm;                        // h tile, tile-row order
    float* ft = sm + WT_R * LD;            // fv tile, ranked order
    __shared__ NfpOrder o;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    int row0, nblk, nrows;
    wg_tile_rows<VAR>(tt, row0, nblk, nrows);
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) * 32 < nrows;     // this wave's ranked block has rows
    const bool save = !VAR || fv != nullptr;                                          // fv is kept for a backward
    if constexpr (VAR) {                                      // fixed stride: the rows behind the live ones, in every array written
        const int e = wg_dead_end(tt, row0, nrows);
        fz_clear_rows<512>(fv, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(out, D, row0 + nrows, e, tid);
    }
    wt_load_tile<D, VAR>(ht, h, row0, tid, nrows);
    nfp_rank_rows<VAR>(o, cls, row0, nrows);                  // (its barriers also publish the h tile)
    {
        const int row = tid >> 2, q = tid & 3;
        if (!VAR || row < nrows) {
            f32x4 acc[F];
            wt_tile_gather<D, true, VAR>(acc, ht, row, q, row0, ptr, col, val, self_w[row0 + row], nrows);
            float* d = ft + o.inv[row] * LD + q * (D / 4);
            float* gq = fv + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                *(f32x4*)(d + 4 * f) = acc[f];
                if (save) *(f32x4*)(gq + 4 * f) = acc[f];
            }
        }
    }
    __syncthreads();
    if (blive) {
        f32x16 acc[NB];
        nfp_class_walk<D>(acc, ft, o, WTp, wv);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = wt_col(wv, NB, nb);
            const float bc = B[c];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = o.perm[wt_row(wv, reg)];
                out[(size_t)(row0 + row) * D + c] = bmp_sigmoid(acc[nb][reg] + bc);
            }
        }
    }
}

// live [N]: a row of weight 0 leaves with dpre == 0 (row_w of a per-instance batch; the liveness weight of the encoder layout,
// whose pad rows have row_w == 0 and still carry gradient)
template <int D, bool VAR = false>
__device__ __forceinline__ void nfp_layer_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                              const int* __restrict__ ptrT, const int* __restrict__ colT,
                                              const float* __restrict__ valT, const float* __restrict__ self_w,
                                              const int* __restrict__ cls, const float* __restrict__ live,
                                              const float* __restrict__ Wnp, float* __restrict__ dpre, float* __restrict__ dh,
                                              WgTable tt = WgTable{}) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16;
    extern __shared__ float sm[];
    float* dt = sm;                        // dpre tile, ranked order
    float* gt = sm + WT_R * LD;            // dfv tile, tile-row order
    __shared__ NfpOrder o;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    int row0, nblk, nrows;
    wg_tile_rows<VAR>(tt, row0, nblk, nrows);
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) * 32 < nrows;     // this wave's ranked block has rows
    if constexpr (VAR) {                                      // fixed stride: the rows behind the live ones read as zeros to the
        const int e = wg_dead_end(tt, row0, nrows);           // weight-gradient GEMM, the column sums and the layer below
        fz_clear_rows<512>(dpre, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(dh, D, row0 + nrows, e, tid);
    }
    nfp_rank_rows<VAR>(o, cls, row0, nrows);
    for (int i = tid; i < (VAR ? nrows : WT_R) * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        const size_t g = (size_t)(row0 + r) * D + 4 * q4;
        const f32x4 ov = *(const f32x4*)(out + g), gv = *(const f32x4*)(dout + g);
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (live[row0 + r] != 0.f) v = gv * ov * ((f32x4){1.f, 1.f, 1.f, 1.f} - ov);
        *(f32x4*)(dpre + g) = v;
        *(f32x4*)(dt + o.inv[r] * LD + 4 * q4) = v;
    }
    __syncthreads();
    if (blive) {
        f32x16 acc[NB];
        nfp_class_walk<D>(acc, dt, o, Wnp, wv);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = wt_col(wv, NB, nb);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) gt[o.perm[wt_row(wv, reg)] * LD + c] = acc[nb][reg];
        }
    }
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
        if (!VAR || row < nrows) {
            f32x4 a[F];
            wt_tile_gather<D, true, VAR>(a, gt, row, q, row0, ptrT, colT, valT, self_w[row0 + row], nrows);
            float* gq = dh + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) *(f32x4*)(gq + 4 * f) = a[f];
        }
    }
}

// ---- the readout per tile: z = h . W_o + b_o on MFMA (column blocks of 32, o a multiple of 8 up to 128), softmax per row
// (4 threads per row), the tile's molecules summed in row order by one thread per channel.  VAR: the dead rows count as rows
// of no molecule and of weight 0 without being loaded; with a fixed stride they are zeros in s (forward), dz and dh (backward).
template <int D, bool VAR = false>
__device__ __forceinline__ void nfp_readout_fwd(const float* __restrict__ h, int o, const float* __restrict__ WoTp,
                                                const float* __restrict__ bo, const float* __restrict__ row_w,
                                                const int* __restrict__ row_mol, float* __restrict__ sout, float* __restrict__ g,
                                                int accumulate, WgTable tt = WgTable{}) {
    constexpr int LD = D + 4;
    extern __shared__ float sm[];
    float* ht = sm;
    float* zt = sm + WT_R * LD;            // [128][NFP_LDZ]
    __shared__ int rmol[WT_R];
    __shared__ float rw[WT_R];
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int lane = wv.lane;
    int row0, nblk, nrows;
    wg_tile_rows<VAR>(tt, row0, nblk, nrows);
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) * 32 < nrows;     // this wave's block has rows
    if constexpr (VAR) fz_clear_rows<512>(sout, o, row0 + nrows, wg_dead_end(tt, row0, nrows), tid);
    wt_load_tile<D, VAR>(ht, h, row0, tid, nrows);
    if (tid < WT_R) {
        const bool rl = !VAR || tid < nrows;
        rmol[tid] = rl ? row_mol[row0 + tid] : -1;
        rw[tid] = rl ? row_w[row0 + tid] : 0.f;
    }
    __syncthreads();
    if (blive) {
        for (int cb = wv.ch; cb * 32 < o; cb += 2) {
            const int c = cb * 32 + (lane & 31);
            const bool valid = c < o;
            f32x16 acc[1];
            zero_acc(acc);
            // (a column past o multiplies column 0's weights; its results are not stored)
            wt_block_mma<1, false>(acc, ht + (wv.b * 32 + (lane & 31)) * LD + 4 * (lane >> 5),
                                   WoTp + ((size_t)(lane >> 5) * o + (valid ? c : 0)) * 4, o, D);
            if (valid) {
                const float bc = bo[c];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) zt[wt_row(wv, reg) * NFP_LDZ + c] = acc[0][reg] + bc;
            }
        }
    }
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
        if (!VAR || row < nrows) {         // (the four threads of a row share one quad: the shuffles stay inside a live row)
            float* z = zt + row * NFP_LDZ;
            float mx = -3.0e38f;
            for (int c = q; c < o; c += 4) mx = fmaxf(mx, z[c]);
            mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2));
            float sum = 0.f;
            for (int c = q; c < o; c += 4) { const float e = bmp_exp(z[c] - mx); z[c] = e; sum += e; }
            sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2);
            const float inv = 1.0f / sum;
            for (int c = q; c < o; c += 4) { const float s = z[c] * inv; z[c] = s; sout[(size_t)(row0 + row) * o + c] = s; }
        }
    }
    __syncthreads();
    if (tid < o) {
        float acc = 0.f;
        int cur = -1;
        for (int r = 0; r <= WT_R; ++r) {
            const int m = r < WT_R ? rmol[r] : -1;
            if (m != cur) {
                if (cur >= 0) { float* p = g + (size_t)cur * o + tid; *p = accumulate ? (*p + acc) : acc; }
                cur = m; acc = 0.f;
            }
            if (m >= 0) acc = fmaf(rw[r], zt[r * NFP_LDZ + tid], acc);
        }
    }
}

template <int D, bool VAR = false>
__device__ __forceinline__ void nfp_readout_bwd(const float* __restrict__ dg, const float* __restrict__ s, int o,
                                                const float* __restrict__ Wnp, const float* __restrict__ row_w,
                                                const int* __restrict__ row_mol, float* __restrict__ dz, float* __restrict__ dh,
                                                WgTable tt = WgTable{}) {
    constexpr int NB = D / 64;
    extern __shared__ float sm[];
    float* zt = sm;                        // dz tile [128][NFP_LDZ]
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    int row0, nblk, nrows;
    wg_tile_rows<VAR>(tt, row0, nblk, nrows);
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) * 32 < nrows;     // this wave's block has rows
    if constexpr (VAR) {
        const int e = wg_dead_end(tt, row0, nrows);
        fz_clear_rows<512>(dz, o, row0 + nrows, e, tid);
        fz_clear_rows<512>(dh, D, row0 + nrows, e, tid);
    }
    {
        const int row = tid >> 2, q = tid & 3, gr = row0 + row;
        if (!VAR || row < nrows) {
            const int m = row_mol[gr];
            const float rwv = m >= 0 ? row_w[gr] : 0.f;
            const bool on = rwv != 0.f;
            float dot = 0.f;
            if (on) for (int c = q; c < o; c += 4) dot = fmaf(dg[(size_t)m * o + c], s[(size_t)gr * o + c], dot);
            dot += __shfl_xor(dot, 1); dot += __shfl_xor(dot, 2);
            for (int c = q; c < o; c += 4) {
                const float v = on ? rwv * s[(size_t)gr * o + c] * (dg[(size_t)m * o + c] - dot) : 0.f;
                zt[row * NFP_LDZ + c] = v;
                dz[(size_t)gr * o + c] = v;
            }
        }
    }
    __syncthreads();
    if (blive) {
        f32x16 acc[NB];
        wt_wave_mma<D>(acc, zt, NFP_LDZ, Wnp, o, wv);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = wt_col(wv, NB, nb);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) dh[(size_t)(row0 + wt_row(wv, reg)) * D + c] = acc[nb][reg];
        }
    }
}

// What the _tile_ entries (bmp_nfp.hip) and the _table_ entries (bmp_nfp_table.hip, behind their table's own check) refuse
// before their launch.  save_ok: what the entry asks of fv.
static inline int nfp_layer_fwd_check(bool d_ok, bool save_ok, const float* h, int n_tiles, const int* csr_ptr, const float* self_w,
                                      const int* deg_class, const float* WTp, const float* B, const float* fv, const float* out) {
    BMP_REQUIRE(h && n_tiles > 0 && d_ok && csr_ptr && self_w && deg_class && WTp && B && save_ok && out);
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)WTp | (uintptr_t)fv) & 15) == 0);
    return 0;
}
static inline int nfp_layer_bwd_check(bool d_ok, const float* dout, const float* out, int n_tiles, const int* csrT_ptr,
                                      const float* self_w, const int* deg_class, const float* row_w, const float* Wnp,
                                      const float* dpre, const float* dh) {
    BMP_REQUIRE(dout && out && n_tiles > 0 && d_ok && csrT_ptr && self_w && deg_class && row_w && Wnp && dpre && dh);
    BMP_REQUIRE((((uintptr_t)dout | (uintptr_t)out | (uintptr_t)Wnp | (uintptr_t)dpre | (uintptr_t)dh) & 15) == 0);
    return 0;
}
static inline int nfp_readout_fwd_check(bool ok, const float* h, int n_tiles, const float* WoTp, const float* b, const float* row_w,
                                        const int* row_mol, const float* s, const float* g) {
    BMP_REQUIRE(h && n_tiles > 0 && ok && WoTp && b && row_w && row_mol && s && g);
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)WoTp) & 15) == 0);
    return 0;
}
static inline int nfp_readout_bwd_check(bool ok, const float* dg, const float* h, const float* s, int n_tiles, const float* Wnp,
                                        const float* row_w, const int* row_mol, const float* dh, const float* dWT, const float* db,
                                        const float* ws) {
    BMP_REQUIRE(dg && h && s && n_tiles > 0 && ok && Wnp && row_w && row_mol && dh && dWT && db && ws);
    BMP_REQUIRE(((uintptr_t)Wnp & 15) == 0);
    return 0;
}

// The readout backward's weight gradients behind its tile kernel, dW_o [d x o] = h^T dz and db [o] = column sums of dz over all N
// rows (bmp_nfp.hip): ws as bmp_nfp_readout_bwd, whose first N x o floats are dz.
int nfp_readout_wgrad(const float* h, int N, int d, int o, float* dWT, float* db, float* ws, hipStream_t st);
