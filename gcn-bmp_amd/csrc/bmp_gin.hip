// Graph isomorphism network (GIN) layer on the packed layout -- models/gin.py of the reference:
//   GINUpdate.__call__ (:89-128):  s_i = h_i + sum_j adjsum[i, j] h_j, adjsum = the adjacency summed over the four bond types
//            (csr_col >> 2 is the source row, an entry counts with its value); t = relu(s . W1^T + b1);
//            out = relu(keep * (t . W2^T + b2)), keep = the dropout mask (0 or 1 / (1 - p)) between the second linear and its relu.
// Nothing is masked: a padded position has no neighbours and all of them share one trajectory, the layout's virtual pad row.
//
// One kernel per direction, one workgroup of 512 threads (8 waves) per 128-row tile, d in {64, 128}, exact-f32 MFMA 32x32x2.
// Two [128][d + 4] tiles in LDS, A and B, used in turn (wave w owns the 32-row block w >> 1 and the column half w & 1):
//   forward   h -> A;  s = gather(A) -> B (and global);  t = relu(B . W1 + b1) -> A;  p = A . W2 + b2 -> B;
//             row-major with 16-byte accesses: t from A to global, out = relu(keep * B) to global.
//   backward  dp2 = dout * [out > 0] * keep -> A (and global), t -> B;  dp1 = (A . W2) * [t > 0] in place in B;
//             ds = B . W1 -> A;  per row: dp1 from B to global, dh = ds + transposed-CSR gather of ds from A.
// h never leaves the CU between the gather and the second product.  The weight gradients dW2 = dp2^T t, dW1 = dp1^T s and the
// bias gradients are the caller's two calls of bmp_linear_wgrad on the saved s, t and the dp2, dp1 written here.
// Weights are K4-packed ([K/4][N][4], as for bmp_ggnn_step_*): a lane's four k values are one 16-byte load.
// The tile load, the MFMA loop, the wave product, the gather and the launch are the shared ones of bmp_wtile.h.
#include "bmp_wtile.h"

template <int D>
__global__ __launch_bounds__(512) void k_gin_tile_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                                      const float* __restrict__ val, const float* __restrict__ W1p,
                                                      const float* __restrict__ b1, const float* __restrict__ W2p,
                                                      const float* __restrict__ b2, const float* __restrict__ keep,
                                                      float* __restrict__ s, float* __restrict__ t, float* __restrict__ out) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16;
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int row0 = blockIdx.x * WT_R;
    wt_load_tile<D>(ta, h, row0, tid);
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
        f32x4 acc[F];
        wt_tile_gather<D, false>(acc, ta, row, q, row0, ptr, col, val);
        float* d = tb + row * LD + q * (D / 4);
        float* gq = s + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) { *(f32x4*)(d + 4 * f) = acc[f]; *(f32x4*)(gq + 4 * f) = acc[f]; }
    }
    __syncthreads();
    f32x16 acc[NB];
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
    __syncthreads();
    wt_wave_mma<D>(acc, ta, LD, W2p, D, wv);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int c = wt_col(wv, NB, nb);
        const float bc = b2[c];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) tb[wt_row(wv, reg) * LD + c] = acc[nb][reg] + bc;
    }
    __syncthreads();
    const f32x4 z4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < WT_R * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        const size_t g = (size_t)(row0 + r) * D + 4 * q4;
        *(f32x4*)(t + g) = *(const f32x4*)(ta + r * LD + 4 * q4);
        f32x4 p = *(const f32x4*)(tb + r * LD + 4 * q4);
        if (keep) p = p * *(const f32x4*)(keep + g);
        *(f32x4*)(out + g) = __builtin_elementwise_max(p, z4);
    }
}

template <int D>
__global__ __launch_bounds__(512) void k_gin_tile_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                                      const float* __restrict__ keep, const float* __restrict__ t,
                                                      const int* __restrict__ ptrT, const int* __restrict__ colT,
                                                      const float* __restrict__ valT, const float* __restrict__ W2np,
                                                      const float* __restrict__ W1np, float* __restrict__ dp2,
                                                      float* __restrict__ dp1, float* __restrict__ dh) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16;
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int row0 = blockIdx.x * WT_R;
    for (int i = tid; i < WT_R * (D / 4); i += 512) {
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
    __syncthreads();
    wt_wave_mma<D>(acc, tb, LD, W1np, D, wv);
    wt_acc_to_tile<D>(ta, acc, wv);
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
        const float* pq = tb + row * LD + q * (D / 4);
        float* g1 = dp1 + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) *(f32x4*)(g1 + 4 * f) = *(const f32x4*)(pq + 4 * f);
        f32x4 a[F];
        wt_tile_gather<D, false>(a, ta, row, q, row0, ptrT, colT, valT);
        float* gq = dh + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) *(f32x4*)(gq + 4 * f) = a[f];
    }
}

extern "C" int bmp_gin_layer_supported(int d) { return d == 64 || d == 128; }

// W1p / W2p [d x d]: W1^T / W2^T (K-major) K4-packed.  keep [N x d] or null (no dropout).  Saves s, t [N x d]; N = 128 n_tiles.
extern "C" int bmp_gin_layer_tile_fwd(const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col, const float* csr_val,
                                      const float* W1p, const float* b1, const float* W2p, const float* b2, const float* keep,
                                      float* s, float* t, float* out, hipStream_t st) {
    BMP_REQUIRE(h && n_tiles > 0 && bmp_gin_layer_supported(d) && csr_ptr && W1p && b1 && W2p && b2 && s && t && out);
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)W1p | (uintptr_t)W2p | (uintptr_t)keep | (uintptr_t)s | (uintptr_t)t | (uintptr_t)out) & 15) == 0);
    WT_LAUNCH(k_gin_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, W1p, b1, W2p, b2, keep, s, t, out);
    return 0;
}
// W2np / W1np [d x d]: W2 / W1 in the reference layout [out x in] (the K-major operands of dt = dp2 . W2, ds = dp1 . W1), K4-packed.
extern "C" int bmp_gin_layer_tile_bwd(const float* dout, const float* out, const float* keep, const float* t, int n_tiles, int d,
                                      const int* csrT_ptr, const int* csrT_col, const float* csrT_val, const float* W2np,
                                      const float* W1np, float* dp2, float* dp1, float* dh, hipStream_t st) {
    BMP_REQUIRE(dout && out && t && n_tiles > 0 && bmp_gin_layer_supported(d) && csrT_ptr && W2np && W1np && dp2 && dp1 && dh);
    BMP_REQUIRE((((uintptr_t)dout | (uintptr_t)out | (uintptr_t)keep | (uintptr_t)t | (uintptr_t)W2np | (uintptr_t)W1np | (uintptr_t)dp2 |
                  (uintptr_t)dp1 | (uintptr_t)dh) & 15) == 0);
    WT_LAUNCH(k_gin_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, keep, t, csrT_ptr, csrT_col, csrT_val, W2np, W1np, dp2, dp1, dh);
    return 0;
}
