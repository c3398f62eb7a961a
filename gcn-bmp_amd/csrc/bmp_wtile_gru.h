// The GRU propagation step on whole tiles, ONE body per direction for the self-loop kernels (bmp_loop.hip) and the edge-network
// kernels (bmp_edge.hip): the typed GGNN message with a fifth operand MSG, then, with a = [h, m] . AT + b, columns [r | z | c],
//   later calls       r = sigmoid(a_r), z = sigmoid(a_z), c = tanh(a_c + (r * h) . UcT);  out = z * c + (1 - z) * h
//   first after reset z = sigmoid(a_z), c = tanh(a_c);  out = z * c          (no r gate, no U term: GRU.kernel_weights)
// One workgroup of 512 threads per 128-row tile, two [128][d + 4] tiles in LDS, A and B, the machinery of bmp_wtile.h.  D, FIRST and
// MSG are template parameters; what MSG changes sits behind `if constexpr`, the rest is one text.  (One body and not per-phase
// functions: split into message / GRU / epilogue functions, the later-call backward at d = 128 spills; DESIGN.md.)
//   forward   h -> A;  per bond type: agg_e = typed gather(A) -> B, acc_m += B . W_e;  the fifth operand
//               self loop     acc_m += A . WsT (it reads A itself, no gather);  m = acc_m + sum_e wdeg_e b_e + b_s -> B (and global)
//               edge network  S -> B, acc_m += B . B^T;  m = acc_m -> B (and global): no bias
//             acc[r|z|c] = A . AT[:d] + B . AT[d:];  later calls: r * A[i] over the lane's own elements of B (m is no longer
//             needed), acc_c += B . UcT;  out in the accumulators, each lane overwriting its own elements of A;  then r, z, c
//             through the tiles to global, row-major with 16-byte accesses.
//   backward  da_c -> A, da_z -> B (and into gda);  acc_dh | acc_dm += A . A_c + B . A_z;  later calls: d(r h) = A . Uc -> A,
//             da_r = d(r h) h r (1 - r) -> A in place (and into gda, r h into rh), acc_dh | acc_dm += A . A_r;  dm = acc_dm -> B;
//               self loop     acc_dh += B . W_s;  dm into gda
//               edge network  Q -> A (and into gda, where the self loop has dm);  acc_dh += A . B
//             per bond type: G_e = typed transposed-CSR gather(B) -> A (and into gda), acc_dh += A . W_e^T;
//             dh = acc_dh + the direct term dout (1 - z) + d(r h) r.     gda [N x 8d] = [G_0 .. G_3 | dm or Q | da_r | da_z | da_c]
// Every term of the backward carries a factor dout or is a gather or a sum of dm: a zero dout row leaves with zero dh and gda rows.
//
// VAR (self loop only): the tile is entry blockIdx.x of a tile table, rows [row0, row0 + nrows), nrows = 32 nblk, 1..4 live blocks.
// No global access goes to a tile row >= nrows (in the dense encoder layout those rows are the next tile's, or lie past the
// arrays), the waves of a dead block (wave w owns block w >> 1) skip their MFMA loops and accumulator-to-tile writes and still
// reach every barrier, and with a fixed stride > nrows the rows [row0 + nrows, row0 + stride) are written as zeros in every array
// the kernel writes.  The LDS rows of a dead block hold whatever was there: no live row reads them (the gathers skip entries
// >= nrows, an MFMA row reads its own A row only).  Without VAR the table is not read and the code is the whole-tile one.
#pragma once
#include "bmp_wtile.h"

enum { WG_SELF_LOOP = 0, WG_EDGE_NET = 1 };                   // MSG: the message's fifth operand

// The tile table of the VAR form (bmp_tile.h: StepArgs' mt_row0 / mt_nblk / tile_stride); mt_rows: the arrays' rows.
struct WgTable { const int* mt_row0; const int* mt_nblk; int mt_rows; int tile_stride; };

// this workgroup's tile: first row, live blocks (a table entry's count is clipped to the 4 the LDS tiles hold)
template <bool VAR>
__device__ __forceinline__ void wg_tile(WgTable tt, int& row0, int& nblk) {
    if constexpr (VAR) {
        row0 = tt.mt_row0[blockIdx.x];
        const int n = tt.mt_nblk[blockIdx.x];
        nblk = n < 0 ? 0 : (n > WT_R / 32 ? WT_R / 32 : n);
    } else {
        row0 = blockIdx.x * WT_R;
        nblk = WT_R / 32;
    }
}
// ... and its live rows, clipped to the arrays (the GIN and NFP kernels)
template <bool VAR>
__device__ __forceinline__ void wg_tile_rows(WgTable tt, int& row0, int& nblk, int& nrows) {
    wg_tile<VAR>(tt, row0, nblk);
    nrows = 32 * nblk;
    if constexpr (VAR) {
        const int left = tt.mt_rows - row0;
        nrows = nrows < left ? nrows : (left > 0 ? left : 0);
    }
}
// the end of the rows a fixed-stride table's tile clears behind its live rows (none: row0 + nrows), clipped to the arrays
__device__ __forceinline__ int wg_dead_end(WgTable tt, int row0, int nrows) {
    const int e = row0 + (tt.tile_stride > nrows ? tt.tile_stride : nrows);
    return e < tt.mt_rows ? e : tt.mt_rows;
}

// The molecules of a tile as segments of its rows (edge network; the self loop passes an empty one).
struct EdgeSeg { const float* row_w; const int* row_mol; const int* mol_row0; const int* mol_nrows; int n_mols; };

// the tile-local first row of the molecule of tile row `row`, -1 for a row of no molecule
__device__ __forceinline__ int edge_seg_first(EdgeSeg sg, int row0, int row) {
    const int mol = sg.row_mol[row0 + row];
    if ((unsigned)mol >= (unsigned)sg.n_mols) return -1;
    const int first = sg.mol_row0[mol] - row0;
    return (unsigned)first < (unsigned)WT_R ? first : -1;
}

// By the four threads (quarters q) of a molecule's first row: dst[row] := the sum over the molecule's rows r of (WEIGHTED ?
// row_w[r] : 1) * src[r], clipped to the tile (a table with a straddling molecule cannot send an LDS access out of the tiles).
template <int D, bool WEIGHTED>
__device__ __forceinline__ void edge_seg_sum(float* dst, const float* src, EdgeSeg sg, int row0, int row, int q) {
    constexpr int LD = D + 4, F = D / 16;
    if (edge_seg_first(sg, row0, row) != row) return;
    int nr = sg.mol_nrows[sg.row_mol[row0 + row]];
    nr = nr < WT_R - row ? nr : WT_R - row;
    f32x4 acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int r = row; r < row + nr; ++r) {
        const float w = WEIGHTED ? sg.row_w[row0 + r] : 1.f;
        const float* s = src + r * LD + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] += *(const f32x4*)(s + 4 * f) * w;
    }
    float* d = dst + row * LD + q * (D / 4);
#pragma unroll
    for (int f = 0; f < F; ++f) *(f32x4*)(d + 4 * f) = acc[f];
}

// v := this thread's quarter of the sum its molecule's first row holds in `t`; zeros on a row of no molecule
template <int D>
__device__ __forceinline__ void edge_seg_fetch(f32x4 (&v)[D / 16], const float* t, int first, int q) {
    constexpr int LD = D + 4, F = D / 16;
#pragma unroll
    for (int f = 0; f < F; ++f) v[f] = first < 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : *(const f32x4*)(t + first * LD + q * (D / 4) + 4 * f);
}

// W5p: WsTp (self loop) or BTp (edge network);  bE, bs: the self loop's biases (edge network: not read);  sg: edge network only.
template <int D, bool FIRST, int MSG, bool VAR = false>
__device__ __forceinline__ void wg_step_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                            const float* __restrict__ val, EdgeSeg sg, const float* __restrict__ WTp,
                                            const float* __restrict__ bE, const float* __restrict__ W5p, const float* __restrict__ bs,
                                            const float* __restrict__ ATp, const float* __restrict__ UcTp, const float* __restrict__ b,
                                            float* __restrict__ m, float* __restrict__ rz, float* __restrict__ c,
                                            float* __restrict__ hout, WgTable tt = WgTable{}) {
    static_assert(!VAR || MSG == WG_SELF_LOOP, "the edge network takes whole tiles only");
    constexpr int LD = D + 4, NB = D / 64, F = D / 16, NG = FIRST ? 2 : 3, G0 = 3 - NG;       // gates computed: G0 .. 2 of r, z, c
    extern __shared__ float sm[];
    float *ta = sm, *tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    int row0, nblk;
    wg_tile<VAR>(tt, row0, nblk);
    const int nrows = 32 * nblk;
    const WtWave wv = wt_wave(tid);
    const int row = tid >> 2, q = tid & 3;                    // the gather's, the bias's and the segment sum's (row, quarter)
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) < nblk;           // this wave's block has rows
    const bool rlive = !VAR || row < nrows;                                           // this thread's gather row is one
    if constexpr (VAR) {                                      // fixed stride: the rows behind the live ones, in every array written
        const int e = wg_dead_end(tt, row0, nrows);
        fz_clear_rows<512>(hout, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(m, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(rz, 2 * D, row0 + nrows, e, tid);
        fz_clear_rows<512>(c, D, row0 + nrows, e, tid);
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
        if constexpr (MSG == WG_SELF_LOOP) {
            if (blive) wt_block_mma<NB, false>(am, ta + aoff, W5p + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);   // the self loop
        } else {
            // S (a molecule's rows: the row_w-weighted sum of its rows of h; rows of no molecule: zeros) into B: summed by each
            // molecule's first row, then copied by its other rows (a first row keeps what it wrote: no row is written and read)
            edge_seg_sum<D, true>(tb, ta, sg, row0, row, q);
            __syncthreads();
            const int first = edge_seg_first(sg, row0, row);
            if (first != row) {
                f32x4 v[F];
                edge_seg_fetch<D>(v, tb, first, q);
                float* d = tb + row * LD + q * (D / 4);
#pragma unroll
                for (int f = 0; f < F; ++f) *(f32x4*)(d + 4 * f) = v[f];
            }
            __syncthreads();
            wt_block_mma<NB, false>(am, tb + aoff, W5p + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);   // + S . B^T
            __syncthreads();                                  // every wave has left the product on B
        }
        if (blive) wt_acc_to_tile<D>(tb, am, wv);             // m -> B (self loop: before its biases)
    }
    __syncthreads();
    if constexpr (MSG == WG_SELF_LOOP) {   // + sum_e wdeg_e b_e + b_s, by the thread that took the row's weighted degrees
        if (rlive) {
            float* d = tb + row * LD + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const int cc = q * (D / 4) + 4 * f;
                f32x4 v = *(const f32x4*)(d + 4 * f) + *(const f32x4*)(bs + cc);
#pragma unroll
                for (int e = 0; e < 4; ++e) v += *(const f32x4*)(bE + e * D + cc) * wd[e];
                *(f32x4*)(d + 4 * f) = v;
                if (m) *(f32x4*)(m + (size_t)(row0 + row) * D + cc) = v;
            }
        }
        __syncthreads();
    } else if (m) wt_store_tile<D>(tb, m, D, 0, row0, tid);
    f32x16 au[NG][NB];                                        // later calls r, z, c; first call z, c
#pragma unroll
    for (int g = 0; g < NG; ++g) zero_acc(au[g]);
    const float* Bu = ATp + ((size_t)(wv.lane >> 5) * 3 * D + G0 * D + bcol) * 4;
    if (blive) {
        wt_block_mma_g<NG, NB>(au, ta + aoff, Bu, 3 * D, D, D);
        wt_block_mma_g<NG, NB>(au, tb + aoff, Bu + (size_t)D * 3 * D, 3 * D, D, D);
    }
    // A wave's products read all d columns of its rows of A and B, the column half of its sibling wave included: nobody
    // writes into A or B before every wave has left the products.  Behind the barrier each (row, column) is read and
    // written by the one lane that holds its accumulator element: in place.
    __syncthreads();
    if constexpr (!FIRST) {
        if (blive) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int cc = wt_col(wv, NB, nb);
                const float br = b[cc];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int i = wt_row(wv, reg) * LD + cc;
                    const float r = bmp_sigmoid(au[0][nb][reg] + br);
                    au[0][nb][reg] = r;
                    tb[i] = r * ta[i];
                }
            }
        }
        __syncthreads();
        if (blive) wt_block_mma<NB, false>(au[2], tb + aoff, UcTp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);
        __syncthreads();                                      // (B is overwritten with r below)
    }
    if (blive) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int cc = wt_col(wv, NB, nb);
            const float bz = b[D + cc], bc = b[2 * D + cc];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i = wt_row(wv, reg) * LD + cc;
                const float z = bmp_sigmoid(au[NG - 2][nb][reg] + bz), cv = bmp_tanh(au[NG - 1][nb][reg] + bc);
                au[NG - 2][nb][reg] = z; au[NG - 1][nb][reg] = cv;
                ta[i] = FIRST ? z * cv : z * cv + (1.f - z) * ta[i];
                if constexpr (!FIRST) tb[i] = au[0][nb][reg];
            }
        }
    }
    __syncthreads();
    wt_store_tile<D, VAR>(ta, hout, D, 0, row0, tid, nrows);
    if (rz == nullptr) return;
    if constexpr (!FIRST) wt_store_tile<D, VAR>(tb, rz, 2 * D, 0, row0, tid, nrows);  // (first call: no r, its half of rz is not written)
    __syncthreads();
    if (blive) {
        wt_acc_to_tile<D>(ta, au[NG - 2], wv);
        wt_acc_to_tile<D>(tb, au[NG - 1], wv);
    }
    __syncthreads();
    wt_store_tile<D, VAR>(ta, rz, 2 * D, D, row0, tid, nrows);
    wt_store_tile<D, VAR>(tb, c, D, 0, row0, tid, nrows);
}

// W5p: Ws_p (self loop) or B_p (edge network), in the reference layout [out x in];  sg: edge network only.
template <int D, bool FIRST, int MSG, bool VAR = false>
__device__ __forceinline__ void wg_step_bwd(const float* __restrict__ dhout, const float* __restrict__ h, const float* __restrict__ rz,
                                            const float* __restrict__ c, const int* __restrict__ ptrT, const int* __restrict__ colT,
                                            const float* __restrict__ valT, EdgeSeg sg, const float* __restrict__ Wnp,
                                            const float* __restrict__ W5p, const float* __restrict__ Anp, const float* __restrict__ Ucp,
                                            float* __restrict__ dh, float* __restrict__ gda, float* __restrict__ rh,
                                            WgTable tt = WgTable{}) {
    static_assert(!VAR || MSG == WG_SELF_LOOP, "the edge network takes whole tiles only");
    constexpr int LD = D + 4, NB = D / 64, F = D / 16, LDG = 8 * D;
    extern __shared__ float sm[];
    float *ta = sm, *tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    int row0, nblk;
    wg_tile<VAR>(tt, row0, nblk);
    const int nrows = 32 * nblk;
    const WtWave wv = wt_wave(tid);
    const bool blive = !VAR || __builtin_amdgcn_readfirstlane(wv.b) < nblk;           // this wave's block has rows
    if constexpr (VAR) {                                      // fixed stride: the rows behind the live ones read as zeros to the
        const int e = wg_dead_end(tt, row0, nrows);           // weight-gradient GEMMs and to the step below
        fz_clear_rows<512>(dh, D, row0 + nrows, e, tid);
        fz_clear_rows<512>(gda, LDG, row0 + nrows, e, tid);
        if constexpr (!FIRST) fz_clear_rows<512>(rh, D, row0 + nrows, e, tid);
    }
    const int aoff = (wv.b * 32 + (wv.lane & 31)) * LD + 4 * (wv.lane >> 5);
    const size_t bcol = wv.ch * NB * 32 + (wv.lane & 31);
    const f32x4 one4 = (f32x4){1.f, 1.f, 1.f, 1.f}, zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the row-major view: slot v of this thread = element tid + 512 v of the [128][D / 4] array of 16-byte groups
#pragma unroll
    for (int v = 0; v < F; ++v) {
        const int i = tid + 512 * v, r = i / (D / 4), q4 = i % (D / 4);
        if (VAR && r >= nrows) continue;
        const size_t x = (size_t)(row0 + r) * D + 4 * q4;
        float* go = gda + (size_t)(row0 + r) * LDG + 4 * q4;
        const f32x4 gv = *(const f32x4*)(dhout + x), zv = *(const f32x4*)(rz + (size_t)(row0 + r) * 2 * D + D + 4 * q4);
        const f32x4 cv = *(const f32x4*)(c + x);
        const f32x4 gz = gv * zv;
        const f32x4 dac = gz * (one4 - cv * cv);
        f32x4 daz = gz * (one4 - zv);
        if constexpr (FIRST) { daz = daz * cv; *(f32x4*)(go + 5 * D) = zero4; }
        else daz = daz * (cv - *(const f32x4*)(h + x));
        *(f32x4*)(ta + r * LD + 4 * q4) = dac;
        *(f32x4*)(tb + r * LD + 4 * q4) = daz;
        *(f32x4*)(go + 7 * D) = dac;
        *(f32x4*)(go + 6 * D) = daz;
    }
    __syncthreads();
    f32x16 ad[2][NB];                                         // [0]: dh, [1]: dm
    zero_acc(ad[0]); zero_acc(ad[1]);
    const float* Ab = Anp + ((size_t)(wv.lane >> 5) * 2 * D + bcol) * 4;              // A_p [3d x 2d], rows r | z | c
    if (blive) {
        wt_block_mma_g<2, NB>(ad, ta + aoff, Ab + (size_t)2 * D * 2 * D, 2 * D, D, D);
        wt_block_mma_g<2, NB>(ad, tb + aoff, Ab + (size_t)D * 2 * D, 2 * D, D, D);
    }
    if constexpr (!FIRST) {
        f32x16 adr[NB]; zero_acc(adr);                        // d(r h) = da_c . Uc
        if (blive) wt_block_mma<NB, false>(adr, ta + aoff, Ucp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);
        __syncthreads();                                      // every wave has left the products on A
        if (blive) wt_acc_to_tile<D>(ta, adr, wv);
        __syncthreads();
#pragma unroll
        for (int v = 0; v < F; ++v) {
            const int i = tid + 512 * v, r = i / (D / 4), q4 = i % (D / 4);
            if (VAR && r >= nrows) continue;
            const size_t x = (size_t)(row0 + r) * D + 4 * q4;
            const f32x4 rv = *(const f32x4*)(rz + (size_t)(row0 + r) * 2 * D + 4 * q4), hv = *(const f32x4*)(h + x);
            const f32x4 dr = *(const f32x4*)(ta + r * LD + 4 * q4) * rv;
            const f32x4 dar = dr * hv * (one4 - rv);
            *(f32x4*)(dh + x) = dr;                           // (waits in dh for the epilogue, which this thread runs too)
            *(f32x4*)(ta + r * LD + 4 * q4) = dar;            // (each 16-byte group its thread's own: in place)
            *(f32x4*)(gda + (size_t)(row0 + r) * LDG + 5 * D + 4 * q4) = dar;
            *(f32x4*)(rh + x) = rv * hv;
        }
        __syncthreads();
        if (blive) wt_block_mma_g<2, NB>(ad, ta + aoff, Ab, 2 * D, D, D);
    }
    __syncthreads();                                          // every wave has left the products on A and B
    if (blive) wt_acc_to_tile<D>(tb, ad[1], wv);              // dm -> B
    __syncthreads();
    const int row = tid >> 2, q = tid & 3;
    const bool rlive = !VAR || row < nrows;                   // this thread's gather row is a row of the tile
    float* g4 = gda + (size_t)(row0 + row) * LDG + 4 * D + q * (D / 4);
    if constexpr (MSG == WG_SELF_LOOP) {
        if (blive) wt_block_mma<NB, false>(ad[0], tb + aoff, W5p + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);    // the self loop
        if (rlive) {
            const float* s = tb + row * LD + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) *(f32x4*)(g4 + 4 * f) = *(const f32x4*)(s + 4 * f);
        }
    } else {
        // Q_r = row_w[r] T_mol(r) into A, T = the molecule's sum of dm by its first row;  every row takes T into registers;
        // only then does row_w T overwrite A.  X = h against Q is dB^T: dB[p, q] = sum_mol T[p] S[q] = sum_r Q_r[p] h_r[q].
        edge_seg_sum<D, false>(ta, tb, sg, row0, row, q);
        __syncthreads();
        f32x4 t[F];
        edge_seg_fetch<D>(t, ta, edge_seg_first(sg, row0, row), q);
        __syncthreads();
        const float w = sg.row_w[row0 + row];
        float* d = ta + row * LD + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) { const f32x4 v = t[f] * w; *(f32x4*)(d + 4 * f) = v; *(f32x4*)(g4 + 4 * f) = v; }
        __syncthreads();
        wt_block_mma<NB, false>(ad[0], ta + aoff, W5p + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);        // + Q . B
        __syncthreads();                                  // every wave has left the product on A
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (rlive) {
            f32x4 g[F];
            wt_tile_gather_typed<D, VAR>(g, tb, row, q, row0, ptrT, colT, valT, e, nrows);
            float* d = ta + row * LD + q * (D / 4);
            float* gq = gda + (size_t)(row0 + row) * LDG + e * D + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) { *(f32x4*)(d + 4 * f) = g[f]; *(f32x4*)(gq + 4 * f) = g[f]; }
        }
        __syncthreads();
        if (blive) wt_block_mma<NB, false>(ad[0], ta + aoff, Wnp + ((size_t)(wv.lane >> 5) * 4 * D + e * D + bcol) * 4, 4 * D, D);
        __syncthreads();
    }
    if (blive) wt_acc_to_tile<D>(ta, ad[0], wv);              // (behind the loop's last barrier)
    __syncthreads();
#pragma unroll
    for (int v = 0; v < F; ++v) {
        const int i = tid + 512 * v, r = i / (D / 4), q4 = i % (D / 4);
        if (VAR && r >= nrows) continue;
        const size_t x = (size_t)(row0 + r) * D + 4 * q4;
        f32x4 dv = *(const f32x4*)(ta + r * LD + 4 * q4);
        if constexpr (!FIRST)                                 // + the direct term dout (1 - z) + d(r h) r
            dv += *(const f32x4*)(dhout + x) * (one4 - *(const f32x4*)(rz + (size_t)(row0 + r) * 2 * D + D + 4 * q4)) + *(const f32x4*)(dh + x);
        *(f32x4*)(dh + x) = dv;
    }
}

// What every self-loop and edge-network entry refuses before its launch, one function per direction: the _tile_ and _table_
// entries of the self loop (bmp_loop.hip, bmp_loop_table.hip) and the edge network's (bmp_edge.hip) call it.  d_ok: the family's
// bmp_ggnn_*_step_supported(d); W5: WsT / BT.  The self loop's biases, the edge network's segments and the table are the entries' own.
static inline int wg_fwd_check(bool d_ok, const float* h, int n_tiles, int first, const int* csr_ptr, const float* WTp, const float* W5p,
                               const float* ATp, const float* UcTp, const float* b, const float* m, const float* rz, const float* c,
                               const float* hout) {
    BMP_REQUIRE(h && n_tiles > 0 && d_ok && csr_ptr && WTp && W5p && ATp && b && hout);
    BMP_REQUIRE((first || UcTp) && (m == nullptr) == (rz == nullptr) && (m == nullptr) == (c == nullptr));
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)WTp | (uintptr_t)W5p | (uintptr_t)ATp | (uintptr_t)UcTp | (uintptr_t)m | (uintptr_t)rz |
                  (uintptr_t)c | (uintptr_t)hout) & 15) == 0);
    return 0;
}
static inline int wg_bwd_check(bool d_ok, const float* dhout, const float* h, const float* rz, const float* c, int n_tiles, int first,
                               const int* csrT_ptr, const float* Wnat_p, const float* W5_p, const float* A_p, const float* Uc_p,
                               const float* dh, const float* gda, const float* rh) {
    BMP_REQUIRE(dhout && h && rz && c && n_tiles > 0 && d_ok && csrT_ptr && Wnat_p && W5_p && A_p && dh && gda);
    BMP_REQUIRE(first || (Uc_p && rh));
    BMP_REQUIRE((((uintptr_t)dhout | (uintptr_t)h | (uintptr_t)rz | (uintptr_t)c | (uintptr_t)Wnat_p | (uintptr_t)W5_p | (uintptr_t)A_p |
                  (uintptr_t)Uc_p | (uintptr_t)dh | (uintptr_t)gda | (uintptr_t)rh) & 15) == 0);
    return 0;
}
