// GGNN propagation step with the edge-network message -- EdgeNetwork of models/ggnn.py:657-720 behind GGNN.update's
// 'edge_network' branch (:245-248), always built without hidden layers (:95).  The network is affine in the adjacency vector of an
// atom pair, so with W_e[p, q] = output_layer.W[p d + q, e] and B[p, q] = output_layer.b[p d + q]
//   m_i = sum_e W_e . agg_e(i) + B . S,   agg_e = the neighbour sum over the bonds of type e,
//                                         S = the sum of h over ALL A padded positions of the atom's molecule
//       = the row_w-weighted sum over the molecule's rows (the virtual pad row with its multiplicity A - n),
//   out = GRU([h, m]) as in bmp_loop.hip (state folded into the h-part; `first`: no r gate, no U term).
// No bias enters the message: the per-edge bias of bmp_ggnn_step_* and the self loop's b_s have no counterpart here.
//
// The kernels are those of bmp_loop.hip with the fifth message operand changed: the tile of S rows (every row of a molecule
// holds the molecule's S; rows of no molecule hold zeros) in place of the tile of h.  Two [128][d + 4] tiles in LDS, A and B,
// and nothing else: S is built in tile B once the four typed products have left it --
//   the four threads of a molecule's FIRST row sum the molecule's rows of A, weighted, into that row of B (every h row is read
//   once);  a barrier;  the molecule's other rows copy it.
// The backward does the same on dm (unweighted: T = the sum of dm over the molecule's rows) and scales by the row's weight:
//   Q_r = row_w[r] T_mol(r) -> A (and into gda, where the self-loop kernel has dm);  acc_dh += A . B.
// gda [N x 8d] = [G_0 .. G_3 | Q | da_r | da_z | da_c]: X = h against the Q block is dB^T, since
//   dB[p, q] = sum_mol T[p] S[q] = sum_r Q_r[p] h_r[q].
// Whole tiles whose molecules never straddle a tile; a segment is clipped to its tile all the same, so that a table that breaks
// the rule cannot send an LDS access out of the tiles.
#include "bmp_wtile.h"

// rows [row0, row0 + 128) of the row-major g [.. x ldg], columns [coff, coff + D) := tile, 16 bytes per lane
template <int D>
__device__ __forceinline__ void edge_store_tile(const float* tile, float* __restrict__ g, int ldg, int coff, int row0, int tid) {
    for (int i = tid; i < WT_R * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        *(f32x4*)(g + (size_t)(row0 + r) * ldg + coff + 4 * q4) = *(const f32x4*)(tile + r * (D + 4) + 4 * q4);
    }
}

// tile := a wave's accumulators, each lane its own (row, column) elements
template <int D>
__device__ __forceinline__ void edge_acc_to_tile(float* tile, const f32x16 (&acc)[D / 64], WtWave wv) {
#pragma unroll
    for (int nb = 0; nb < D / 64; ++nb) {
        const int c = wt_col(wv, D / 64, nb);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) tile[wt_row(wv, reg) * (D + 4) + c] = acc[nb][reg];
    }
}

// The molecules of a tile as segments of its rows.
struct EdgeSeg { const float* row_w; const int* row_mol; const int* mol_row0; const int* mol_nrows; int n_mols; };

// the tile-local first row of the molecule of tile row `row`, -1 for a row of no molecule
__device__ __forceinline__ int edge_seg_first(EdgeSeg sg, int row0, int row) {
    const int mol = sg.row_mol[row0 + row];
    if ((unsigned)mol >= (unsigned)sg.n_mols) return -1;
    const int first = sg.mol_row0[mol] - row0;
    return (unsigned)first < (unsigned)WT_R ? first : -1;
}

// By the four threads (quarters q) of a molecule's first row: dst[row] := the sum over the molecule's rows r of
// (WEIGHTED ? row_w[r] : 1) * src[r].  Every other thread passes through.
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

#define EDGE_FWD_ARGS const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,                \
                      const float* __restrict__ val, EdgeSeg sg, const float* __restrict__ WTp,                             \
                      const float* __restrict__ BTp, const float* __restrict__ ATp, const float* __restrict__ UcTp,          \
                      const float* __restrict__ b, float* __restrict__ m, float* __restrict__ rz, float* __restrict__ c,     \
                      float* __restrict__ hout
#define EDGE_BWD_ARGS const float* __restrict__ dhout, const float* __restrict__ h, const float* __restrict__ rz,           \
                      const float* __restrict__ c, const int* __restrict__ ptrT, const int* __restrict__ colT,               \
                      const float* __restrict__ valT, EdgeSeg sg, const float* __restrict__ Wnp,                            \
                      const float* __restrict__ Bp, const float* __restrict__ Anp, const float* __restrict__ Ucp,            \
                      float* __restrict__ dh, float* __restrict__ gda, float* __restrict__ rh

template <int D, bool FIRST>
__device__ __forceinline__ void edge_step_fwd(EDGE_FWD_ARGS) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16, NG = FIRST ? 2 : 3, G0 = 3 - NG;       // gates computed: G0 .. 2 of r, z, c
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int row0 = blockIdx.x * WT_R;
    const int row = tid >> 2, q = tid & 3;                    // the gather's and the segment sum's (row, quarter) of this thread
    const int aoff = (wv.b * 32 + (wv.lane & 31)) * LD + 4 * (wv.lane >> 5);          // this lane's A rows in a tile
    const size_t bcol = wv.ch * NB * 32 + (wv.lane & 31);                             // its first output column
    wt_load_tile<D>(ta, h, row0, tid);
    __syncthreads();
    {
        f32x16 am[NB];
        zero_acc(am);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f32x4 g[F];
            wt_tile_gather_typed<D>(g, ta, row, q, row0, ptr, col, val, e);
            float* d = tb + row * LD + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) *(f32x4*)(d + 4 * f) = g[f];
            __syncthreads();
            wt_block_mma<NB, false>(am, tb + aoff, WTp + (size_t)e * D * D + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);
            __syncthreads();
        }
        // S into B: summed by each molecule's first row, then copied by its other rows (a first row keeps what it wrote, so
        // nobody writes a row that another thread reads)
        edge_seg_sum<D, true>(tb, ta, sg, row0, row, q);
        __syncthreads();
        {
            const int first = edge_seg_first(sg, row0, row);
            if (first != row) {
                f32x4 v[F];
                edge_seg_fetch<D>(v, tb, first, q);
                float* d = tb + row * LD + q * (D / 4);
#pragma unroll
                for (int f = 0; f < F; ++f) *(f32x4*)(d + 4 * f) = v[f];
            }
        }
        __syncthreads();
        wt_block_mma<NB, false>(am, tb + aoff, BTp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);      // + S . B^T
        __syncthreads();                                      // every wave has left the product on B
        edge_acc_to_tile<D>(tb, am, wv);                      // m -> B: no bias
    }
    __syncthreads();
    if (m) edge_store_tile<D>(tb, m, D, 0, row0, tid);
    f32x16 au[NG][NB];                                        // later calls r, z, c; first call z, c
#pragma unroll
    for (int g = 0; g < NG; ++g) zero_acc(au[g]);
    const float* Bu = ATp + ((size_t)(wv.lane >> 5) * 3 * D + G0 * D + bcol) * 4;
    wt_block_mma_g<NG, NB>(au, ta + aoff, Bu, 3 * D, D, D);
    wt_block_mma_g<NG, NB>(au, tb + aoff, Bu + (size_t)D * 3 * D, 3 * D, D, D);
    // A wave's products read all d columns of its rows of A and B, the column half of its sibling wave included: nobody
    // writes into A or B before every wave has left the products.  Behind the barrier each (row, column) is read and
    // written by the one lane that holds its accumulator element: in place.
    __syncthreads();
    if constexpr (!FIRST) {
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
        __syncthreads();
        wt_block_mma<NB, false>(au[2], tb + aoff, UcTp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);
        __syncthreads();                                      // (B is overwritten with r below)
    }
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
    __syncthreads();
    edge_store_tile<D>(ta, hout, D, 0, row0, tid);
    if (rz == nullptr) return;
    if constexpr (!FIRST) edge_store_tile<D>(tb, rz, 2 * D, 0, row0, tid);    // (first call: no r, its half of rz is not written)
    __syncthreads();
    edge_acc_to_tile<D>(ta, au[NG - 2], wv);
    edge_acc_to_tile<D>(tb, au[NG - 1], wv);
    __syncthreads();
    edge_store_tile<D>(ta, rz, 2 * D, D, row0, tid);
    edge_store_tile<D>(tb, c, D, 0, row0, tid);
}

template <int D, bool FIRST>
__device__ __forceinline__ void edge_step_bwd(EDGE_BWD_ARGS) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16, LDG = 8 * D;
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int row0 = blockIdx.x * WT_R;
    const int aoff = (wv.b * 32 + (wv.lane & 31)) * LD + 4 * (wv.lane >> 5);
    const size_t bcol = wv.ch * NB * 32 + (wv.lane & 31);
    const f32x4 one4 = (f32x4){1.f, 1.f, 1.f, 1.f}, zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the row-major view: slot v of this thread = element tid + 512 v of the [128][D / 4] array of 16-byte groups
#pragma unroll
    for (int v = 0; v < F; ++v) {
        const int i = tid + 512 * v, r = i / (D / 4), q4 = i % (D / 4);
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
    zero_acc(ad[0]);
    zero_acc(ad[1]);
    const float* Ab = Anp + ((size_t)(wv.lane >> 5) * 2 * D + bcol) * 4;              // A_p [3d x 2d], rows r | z | c
    wt_block_mma_g<2, NB>(ad, ta + aoff, Ab + (size_t)2 * D * 2 * D, 2 * D, D, D);
    wt_block_mma_g<2, NB>(ad, tb + aoff, Ab + (size_t)D * 2 * D, 2 * D, D, D);
    if constexpr (!FIRST) {
        f32x16 adr[NB];                                       // d(r h) = da_c . Uc
        zero_acc(adr);
        wt_block_mma<NB, false>(adr, ta + aoff, Ucp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);
        __syncthreads();                                      // every wave has left the products on A
        edge_acc_to_tile<D>(ta, adr, wv);
        __syncthreads();
#pragma unroll
        for (int v = 0; v < F; ++v) {
            const int i = tid + 512 * v, r = i / (D / 4), q4 = i % (D / 4);
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
        wt_block_mma_g<2, NB>(ad, ta + aoff, Ab, 2 * D, D, D);
    }
    __syncthreads();                                          // every wave has left the products on A and B
    edge_acc_to_tile<D>(tb, ad[1], wv);                       // dm -> B
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
        // Q into A: T = the molecule's sum of dm by its first row;  every row takes T into registers;  only then is A
        // overwritten with row_w T (a first row scales what the others have read)
        edge_seg_sum<D, false>(ta, tb, sg, row0, row, q);
        __syncthreads();
        {
            f32x4 t[F];
            edge_seg_fetch<D>(t, ta, edge_seg_first(sg, row0, row), q);
            __syncthreads();
            const float w = sg.row_w[row0 + row];
            float* d = ta + row * LD + q * (D / 4);
            float* gq = gda + (size_t)(row0 + row) * LDG + 4 * D + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) { const f32x4 v = t[f] * w; *(f32x4*)(d + 4 * f) = v; *(f32x4*)(gq + 4 * f) = v; }
        }
        __syncthreads();
        wt_block_mma<NB, false>(ad[0], ta + aoff, Bp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);    // + Q . B
        __syncthreads();                                      // every wave has left the product on A
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f32x4 g[F];
            wt_tile_gather_typed<D>(g, tb, row, q, row0, ptrT, colT, valT, e);
            float* d = ta + row * LD + q * (D / 4);
            float* gq = gda + (size_t)(row0 + row) * LDG + e * D + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) { *(f32x4*)(d + 4 * f) = g[f]; *(f32x4*)(gq + 4 * f) = g[f]; }
            __syncthreads();
            wt_block_mma<NB, false>(ad[0], ta + aoff, Wnp + ((size_t)(wv.lane >> 5) * 4 * D + e * D + bcol) * 4, 4 * D, D);
            __syncthreads();
        }
    }
    edge_acc_to_tile<D>(ta, ad[0], wv);                       // (behind the loop's last barrier)
    __syncthreads();
#pragma unroll
    for (int v = 0; v < F; ++v) {
        const int i = tid + 512 * v, r = i / (D / 4), q4 = i % (D / 4);
        const size_t x = (size_t)(row0 + r) * D + 4 * q4;
        f32x4 dv = *(const f32x4*)(ta + r * LD + 4 * q4);
        if constexpr (!FIRST)                                 // + the direct term dout (1 - z) + d(r h) r
            dv += *(const f32x4*)(dhout + x) * (one4 - *(const f32x4*)(rz + (size_t)(row0 + r) * 2 * D + D + 4 * q4)) + *(const f32x4*)(dh + x);
        *(f32x4*)(dh + x) = dv;
    }
}

template <int D>
__global__ __launch_bounds__(512) void k_edge_step_first_tile_fwd(EDGE_FWD_ARGS) {
    edge_step_fwd<D, true>(h, ptr, col, val, sg, WTp, BTp, ATp, UcTp, b, m, rz, c, hout);
}
template <int D>
__global__ __launch_bounds__(512) void k_edge_step_later_tile_fwd(EDGE_FWD_ARGS) {
    edge_step_fwd<D, false>(h, ptr, col, val, sg, WTp, BTp, ATp, UcTp, b, m, rz, c, hout);
}
template <int D>
__global__ __launch_bounds__(512) void k_edge_step_first_tile_bwd(EDGE_BWD_ARGS) {
    edge_step_bwd<D, true>(dhout, h, rz, c, ptrT, colT, valT, sg, Wnp, Bp, Anp, Ucp, dh, gda, rh);
}
template <int D>
__global__ __launch_bounds__(512) void k_edge_step_later_tile_bwd(EDGE_BWD_ARGS) {
    edge_step_bwd<D, false>(dhout, h, rz, c, ptrT, colT, valT, sg, Wnp, Bp, Anp, Ucp, dh, gda, rh);
}

extern "C" int bmp_ggnn_edge_step_supported(int d) { return d == 64 || d == 128; }

// WTp [4d x d] (row e d + q, column p: W_e[p, q]), ATp [2d x 3d], UcTp [d x d], b [3d]: as bmp_ggnn_step_fwd takes them;
// BTp [d x d] = B^T (K-major), K4-packed.  row_w [N], row_mol [N] (-1: a row of no molecule), mol_row0 / mol_nrows [n_mols]: the
// batch's segments.  Saves m [N x d], rz [N x 2d] and c [N x d], all three null for forward-only evaluation.  N = 128 n_tiles.
extern "C" int bmp_ggnn_edge_step_tile_fwd(const float* h, int n_tiles, int d, int first, const int* csr_ptr, const int* csr_col,
                                           const float* csr_val, const float* row_w, const int* row_mol, const int* mol_row0,
                                           const int* mol_nrows, int n_mols, const float* WTp, const float* BTp, const float* ATp,
                                           const float* UcTp, const float* b, float* m, float* rz, float* c, float* hout,
                                           hipStream_t st) {
    BMP_REQUIRE(h && n_tiles > 0 && bmp_ggnn_edge_step_supported(d) && csr_ptr && WTp && BTp && ATp && b && hout);
    BMP_REQUIRE(row_w && row_mol && mol_row0 && mol_nrows && n_mols > 0);
    BMP_REQUIRE((first || UcTp) && (m == nullptr) == (rz == nullptr) && (m == nullptr) == (c == nullptr));
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)WTp | (uintptr_t)BTp | (uintptr_t)ATp | (uintptr_t)UcTp | (uintptr_t)m | (uintptr_t)rz |
                  (uintptr_t)c | (uintptr_t)hout) & 15) == 0);
    const EdgeSeg sg{row_w, row_mol, mol_row0, mol_nrows, n_mols};
    if (first)
        WT_LAUNCH(k_edge_step_first_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, sg, WTp, BTp, ATp, UcTp, b, m, rz, c, hout);
    else
        WT_LAUNCH(k_edge_step_later_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, sg, WTp, BTp, ATp, UcTp, b, m, rz, c, hout);
    return 0;
}
// Wnat_p [d x 4d], A_p [3d x 2d], Uc_p [d x d]: as bmp_ggnn_step_bwd takes them; B_p [d x d] = B in the reference layout
// [out x in], K4-packed.  Writes dh [N x d], gda [N x 8d] = [G_0 .. G_3 | Q | da_r | da_z | da_c] and, for later calls,
// rh [N x d] = r * h; first != 0: the da_r block is written as zeros, rh is not written (and may be null).
extern "C" int bmp_ggnn_edge_step_tile_bwd(const float* dhout, const float* h, const float* rz, const float* c, int n_tiles, int d,
                                           int first, const int* csrT_ptr, const int* csrT_col, const float* csrT_val,
                                           const float* row_w, const int* row_mol, const int* mol_row0, const int* mol_nrows,
                                           int n_mols, const float* Wnat_p, const float* B_p, const float* A_p, const float* Uc_p,
                                           float* dh, float* gda, float* rh, hipStream_t st) {
    BMP_REQUIRE(dhout && h && rz && c && n_tiles > 0 && bmp_ggnn_edge_step_supported(d) && csrT_ptr && Wnat_p && B_p && A_p && dh && gda);
    BMP_REQUIRE(row_w && row_mol && mol_row0 && mol_nrows && n_mols > 0);
    BMP_REQUIRE(first || (Uc_p && rh));
    BMP_REQUIRE((((uintptr_t)dhout | (uintptr_t)h | (uintptr_t)rz | (uintptr_t)c | (uintptr_t)Wnat_p | (uintptr_t)B_p | (uintptr_t)A_p |
                  (uintptr_t)Uc_p | (uintptr_t)dh | (uintptr_t)gda | (uintptr_t)rh) & 15) == 0);
    const EdgeSeg sg{row_w, row_mol, mol_row0, mol_nrows, n_mols};
    if (first)
        WT_LAUNCH(k_edge_step_first_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, sg, Wnat_p, B_p, A_p, Uc_p, dh, gda, rh);
    else
        WT_LAUNCH(k_edge_step_later_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, sg, Wnat_p, B_p, A_p, Uc_p, dh, gda, rh);
    return 0;
}
