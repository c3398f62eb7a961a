// GGNN propagation step with a per-atom self loop in the message -- models/ggnn_dev_self_loop.py:67-110 (= models/ggnn_dev_edge.py)
// of the reference: the GRU step of bmp_ggnn_step_* with a fifth message operand,
//   m = sum_e (agg_e . W_e + wdeg_e b_e) + h . W_s^T + b_s,   agg_e = the neighbour sum over the bonds of type e,
//   out = GRU([h, m]) with the state folded into the h-part (GRU.kernel_weights):
//     later calls       r = sigmoid(a_r), z = sigmoid(a_z), c = tanh(a_c + (r * h) . UcT);  out = z * c + (1 - z) * h
//     first after reset z = sigmoid(a_z), c = tanh(a_c);  out = z * c                     (no r gate, no U term)
//   with a = [h, m] . AT + b, columns [r | z | c].
//
// One kernel per direction, one workgroup of 512 threads (8 waves) per 128-row tile, d in {64, 128}, exact-f32 MFMA 32x32x2, the
// machinery of bmp_wtile.h.  Two [128][d + 4] tiles in LDS, A and B (wave w owns the 32-row block w >> 1 and the column half w & 1).
// `first` is a TEMPLATE parameter of the kernels (the first call carries neither the r accumulators nor the U product) and an
// argument of the C entries, which pick the instance: 2 directions x 2 call forms x 2 widths = 8 kernels.
//   forward   h -> A;  per bond type: agg_e = typed gather(A) -> B, acc_m += B . W_e;  acc_m += A . WsT (the self loop reads A
//             itself, no gather);  m = acc_m + the biases -> B (and global);  acc[r|z|c] = A . AT[:d] + B . AT[d:];  a barrier;
//             later calls: r * A[i] over the lane's own elements of B (m is no longer needed), a barrier, acc_c += B . UcT, a
//             barrier;  out in the accumulators, each lane overwriting its own elements of A;  then r, z, c through the tiles
//             to global, row-major with 16-byte accesses.
//   backward  da_c -> A, da_z -> B (and into gda);  acc_dh | acc_dm += A . A_c + B . A_z;  later calls: d(r h) = A . Uc -> A,
//             da_r = d(r h) h r (1 - r) -> A in place (and into gda, r h into rh), acc_dh | acc_dm += A . A_r;  dm = acc_dm -> B
//             (and into gda);  acc_dh += B . W_s;  per bond type: G_e = typed transposed-CSR gather(B) -> A (and into gda),
//             acc_dh += A . W_e^T;  dh = acc_dh + the direct term dout (1 - z) + d(r h) r.
// Every term of the backward carries a factor dout or is a gather of dm: a row that enters with a zero dout leaves with zero dh
// and gda rows.  The weight gradients are the caller's calls of bmp_linear_wgrad on gda (include/bmp.h).
// Weights are K4-packed ([K/4][N][4], as for bmp_ggnn_step_*): a lane's four k values are one 16-byte load.
#include "bmp_wtile.h"

// rows [row0, row0 + 128) of the row-major g [.. x ldg], columns [coff, coff + D) := tile, 16 bytes per lane
template <int D>
__device__ __forceinline__ void loop_store_tile(const float* tile, float* __restrict__ g, int ldg, int coff, int row0, int tid) {
    for (int i = tid; i < WT_R * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        *(f32x4*)(g + (size_t)(row0 + r) * ldg + coff + 4 * q4) = *(const f32x4*)(tile + r * (D + 4) + 4 * q4);
    }
}

// tile := a wave's accumulators, each lane its own (row, column) elements
template <int D>
__device__ __forceinline__ void loop_acc_to_tile(float* tile, const f32x16 (&acc)[D / 64], WtWave wv) {
#pragma unroll
    for (int nb = 0; nb < D / 64; ++nb) {
        const int c = wt_col(wv, D / 64, nb);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) tile[wt_row(wv, reg) * (D + 4) + c] = acc[nb][reg];
    }
}

#define LOOP_FWD_ARGS const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,                \
                      const float* __restrict__ val, const float* __restrict__ WTp, const float* __restrict__ bE,            \
                      const float* __restrict__ WsTp, const float* __restrict__ bs, const float* __restrict__ ATp,           \
                      const float* __restrict__ UcTp, const float* __restrict__ b, float* __restrict__ m,                    \
                      float* __restrict__ rz, float* __restrict__ c, float* __restrict__ hout
#define LOOP_BWD_ARGS const float* __restrict__ dhout, const float* __restrict__ h, const float* __restrict__ rz,           \
                      const float* __restrict__ c, const int* __restrict__ ptrT, const int* __restrict__ colT,               \
                      const float* __restrict__ valT, const float* __restrict__ Wnp, const float* __restrict__ Wsp,          \
                      const float* __restrict__ Anp, const float* __restrict__ Ucp, float* __restrict__ dh,                  \
                      float* __restrict__ gda, float* __restrict__ rh

template <int D, bool FIRST>
__device__ __forceinline__ void loop_step_fwd(LOOP_FWD_ARGS) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16, NG = FIRST ? 2 : 3, G0 = 3 - NG;       // gates computed: G0 .. 2 of r, z, c
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int row0 = blockIdx.x * WT_R;
    const int row = tid >> 2, q = tid & 3;                    // the gather's and the bias's (row, quarter) of this thread
    const int aoff = (wv.b * 32 + (wv.lane & 31)) * LD + 4 * (wv.lane >> 5);          // this lane's A rows in a tile
    const size_t bcol = wv.ch * NB * 32 + (wv.lane & 31);                             // its first output column
    wt_load_tile<D>(ta, h, row0, tid);
    __syncthreads();
    float wd[4];
    {
        f32x16 am[NB];
        zero_acc(am);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f32x4 g[F];
            wd[e] = wt_tile_gather_typed<D>(g, ta, row, q, row0, ptr, col, val, e);
            float* d = tb + row * LD + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) *(f32x4*)(d + 4 * f) = g[f];
            __syncthreads();
            wt_block_mma<NB, false>(am, tb + aoff, WTp + (size_t)e * D * D + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);
            __syncthreads();
        }
        wt_block_mma<NB, false>(am, ta + aoff, WsTp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);      // the self loop
        loop_acc_to_tile<D>(tb, am, wv);
    }
    __syncthreads();
    {   // + sum_e wdeg_e b_e + b_s, by the thread that took the row's weighted degrees
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
    loop_store_tile<D>(ta, hout, D, 0, row0, tid);
    if (rz == nullptr) return;
    if constexpr (!FIRST) loop_store_tile<D>(tb, rz, 2 * D, 0, row0, tid);    // (first call: no r, its half of rz is not written)
    __syncthreads();
    loop_acc_to_tile<D>(ta, au[NG - 2], wv);
    loop_acc_to_tile<D>(tb, au[NG - 1], wv);
    __syncthreads();
    loop_store_tile<D>(ta, rz, 2 * D, D, row0, tid);
    loop_store_tile<D>(tb, c, D, 0, row0, tid);
}

template <int D, bool FIRST>
__device__ __forceinline__ void loop_step_bwd(LOOP_BWD_ARGS) {
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
        loop_acc_to_tile<D>(ta, adr, wv);
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
    loop_acc_to_tile<D>(tb, ad[1], wv);                       // dm -> B
    __syncthreads();
    wt_block_mma<NB, false>(ad[0], tb + aoff, Wsp + ((size_t)(wv.lane >> 5) * D + bcol) * 4, D, D);       // the self loop
    {
        const int row = tid >> 2, q = tid & 3;
        {
            const float* s = tb + row * LD + q * (D / 4);
            float* gq = gda + (size_t)(row0 + row) * LDG + 4 * D + q * (D / 4);
#pragma unroll
            for (int f = 0; f < F; ++f) *(f32x4*)(gq + 4 * f) = *(const f32x4*)(s + 4 * f);
        }
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
    loop_acc_to_tile<D>(ta, ad[0], wv);                       // (behind the loop's last barrier)
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
__global__ __launch_bounds__(512) void k_loop_step_first_tile_fwd(LOOP_FWD_ARGS) {
    loop_step_fwd<D, true>(h, ptr, col, val, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout);
}
template <int D>
__global__ __launch_bounds__(512) void k_loop_step_later_tile_fwd(LOOP_FWD_ARGS) {
    loop_step_fwd<D, false>(h, ptr, col, val, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout);
}
template <int D>
__global__ __launch_bounds__(512) void k_loop_step_first_tile_bwd(LOOP_BWD_ARGS) {
    loop_step_bwd<D, true>(dhout, h, rz, c, ptrT, colT, valT, Wnp, Wsp, Anp, Ucp, dh, gda, rh);
}
template <int D>
__global__ __launch_bounds__(512) void k_loop_step_later_tile_bwd(LOOP_BWD_ARGS) {
    loop_step_bwd<D, false>(dhout, h, rz, c, ptrT, colT, valT, Wnp, Wsp, Anp, Ucp, dh, gda, rh);
}

extern "C" int bmp_ggnn_loop_step_supported(int d) { return d == 64 || d == 128; }

// WTp [4d x d], bE [4 x d], ATp [2d x 3d], UcTp [d x d], b [3d]: as bmp_ggnn_step_fwd takes them; WsTp [d x d]: W_s^T (K-major),
// K4-packed; bs [d].  Saves m [N x d], rz [N x 2d] and c [N x d], all three null for forward-only evaluation.  N = 128 n_tiles.
extern "C" int bmp_ggnn_loop_step_tile_fwd(const float* h, int n_tiles, int d, int first, const int* csr_ptr, const int* csr_col,
                                           const float* csr_val, const float* WTp, const float* bE, const float* WsTp, const float* bs,
                                           const float* ATp, const float* UcTp, const float* b, float* m, float* rz, float* c,
                                           float* hout, hipStream_t st) {
    BMP_REQUIRE(h && n_tiles > 0 && bmp_ggnn_loop_step_supported(d) && csr_ptr && WTp && bE && WsTp && bs && ATp && b && hout);
    BMP_REQUIRE((first || UcTp) && (m == nullptr) == (rz == nullptr) && (m == nullptr) == (c == nullptr));
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)WTp | (uintptr_t)bE | (uintptr_t)WsTp | (uintptr_t)bs | (uintptr_t)ATp | (uintptr_t)UcTp |
                  (uintptr_t)m | (uintptr_t)rz | (uintptr_t)c | (uintptr_t)hout) & 15) == 0);
    if (first)
        WT_LAUNCH(k_loop_step_first_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout);
    else
        WT_LAUNCH(k_loop_step_later_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout);
    return 0;
}
// Wnat_p [d x 4d], A_p [3d x 2d], Uc_p [d x d]: as bmp_ggnn_step_bwd takes them; Ws_p [d x d]: W_s in the reference layout
// [out x in], K4-packed.  Writes dh [N x d], gda [N x 8d] = [G_0 .. G_3 | dm | da_r | da_z | da_c] and, for later calls,
// rh [N x d] = r * h; first != 0: the da_r block is written as zeros, rh is not written (and may be null).
extern "C" int bmp_ggnn_loop_step_tile_bwd(const float* dhout, const float* h, const float* rz, const float* c, int n_tiles, int d,
                                           int first, const int* csrT_ptr, const int* csrT_col, const float* csrT_val,
                                           const float* Wnat_p, const float* Ws_p, const float* A_p, const float* Uc_p, float* dh,
                                           float* gda, float* rh, hipStream_t st) {
    BMP_REQUIRE(dhout && h && rz && c && n_tiles > 0 && bmp_ggnn_loop_step_supported(d) && csrT_ptr && Wnat_p && Ws_p && A_p && dh && gda);
    BMP_REQUIRE(first || (Uc_p && rh));
    BMP_REQUIRE((((uintptr_t)dhout | (uintptr_t)h | (uintptr_t)rz | (uintptr_t)c | (uintptr_t)Wnat_p | (uintptr_t)Ws_p | (uintptr_t)A_p |
                  (uintptr_t)Uc_p | (uintptr_t)dh | (uintptr_t)gda | (uintptr_t)rh) & 15) == 0);
    if (first)
        WT_LAUNCH(k_loop_step_first_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, A_p, Uc_p, dh, gda, rh);
    else
        WT_LAUNCH(k_loop_step_later_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, A_p, Uc_p, dh, gda, rh);
    return 0;
}
