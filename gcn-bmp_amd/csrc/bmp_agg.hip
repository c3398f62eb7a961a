// GGNN layer aggregators on packed rows -- models/ggnn.py:407-579 of the reference, the two closed-form ones that are an
// operator of their own ('concat' is a torch.cat in front of the readout):
//   max-pool (:424-432):  y = max_t x_t
//   attn     (:551-571):  z_s = sum_t W[s,t] x_t + b_s (attn_dense_layer = Linear(T, T) on the LAYER axis), p = softmax_s(z),
//                         y = sum_s p_s x_s
// with x_t = h_t[row, channel] the output of propagation step t, independently for every (row, channel).  The operator is
// elementwise over n_rows x d: a lane takes four consecutive channels (one 16-byte load per step tensor, T of them in
// registers), W and b are uniform, the grid strides over the float4 units.  No row weights: the virtual pad row is a row
// like any other here and its multiplicity enters in the readout.
//
// Backward of attn:  dz_s = p_s (x_s - y) dy;  dx_t = p_t dy + sum_s W[s,t] dz_s;  dW[s,t] = sum dz_s x_t,  db_s = sum dz_s
// over all rows and channels.  p is recomputed from x (aux == NULL) or read back from aux (T planes of n_rows x d floats
// the forward kept).  dW / db: per-lane accumulators, a butterfly over the wave, the four wave sums in wave order -> one
// partial per workgroup in ws, then one pass that adds the partials in a fixed order.  The grid is a function of
// (n_rows, d) alone, so two runs add the same numbers in the same order; no floating-point atomics.
// Backward of max: chainer's F.max hands the WHOLE upstream gradient to every position equal to the maximum (third-party
// behaviour restated from memory); aux holds the T-bit tie mask of each element, one byte per
// element, so the backward reads dy and the masks only and writes every dh_t, zeros included.
#include "bmp_kernels.h"

#define AGG_MAXT BMP_AGG_MAXT
#define AGG_TPB 256
#define AGG_MAX_BLOCKS 1024          // 256 CUs x 4 workgroups of 256 threads: every CU holds its share for the whole launch

// the T step tensors BY VALUE in the kernel arguments: nothing is staged through a device pointer array, a captured
// launch replays with the addresses it was recorded with
struct AggIn { const float* p[AGG_MAXT]; };
struct AggOut { float* p[AGG_MAXT]; };

static inline int agg_blocks(size_t n4) {
    const size_t b = (n4 + AGG_TPB - 1) / AGG_TPB;
    return (int)(b < 1 ? 1 : (b > AGG_MAX_BLOCKS ? AGG_MAX_BLOCKS : b));
}

template <int T>
__device__ __forceinline__ void agg_load_w(const float* __restrict__ W, const float* __restrict__ b, float (&w)[T * T], float (&bb)[T]) {
#pragma unroll
    for (int i = 0; i < T * T; ++i) w[i] = W[i];
#pragma unroll
    for (int s = 0; s < T; ++s) bb[s] = b ? b[s] : 0.f;
}

// p = softmax_s(W x + b) of one element (x: the T step values); returns y = sum_s p_s x_s
template <int T>
__device__ __forceinline__ float agg_attn_p(const float (&x)[T], const float (&w)[T * T], const float (&bb)[T], float (&p)[T]) {
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < T; ++s) {
        float z = bb[s];
#pragma unroll
        for (int t = 0; t < T; ++t) z = fmaf(w[s * T + t], x[t], z);
        p[s] = z;
        mx = fmaxf(mx, z);
    }
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < T; ++s) {
        p[s] = bmp_exp(p[s] - mx);
        sum += p[s];
    }
    const float inv = __fdividef(1.0f, sum);
    float y = 0.f;
#pragma unroll
    for (int s = 0; s < T; ++s) {
        p[s] *= inv;
        y = fmaf(p[s], x[s], y);
    }
    return y;
}

template <int T, int MODE>
__global__ __launch_bounds__(AGG_TPB) void k_agg_fwd(AggIn h, size_t n4, const float* __restrict__ W, const float* __restrict__ b,
                                                     float* __restrict__ y, void* __restrict__ aux) {
    float w[T * T], bb[T];
    if (MODE == BMP_AGG_ATTN) agg_load_w<T>(W, b, w, bb);
    const size_t stride = (size_t)gridDim.x * AGG_TPB;
    for (size_t u = (size_t)blockIdx.x * AGG_TPB + threadIdx.x; u < n4; u += stride) {
        f32x4 x[T];
#pragma unroll
        for (int t = 0; t < T; ++t) x[t] = reinterpret_cast<const f32x4*>(h.p[t])[u];
        f32x4 out;
        if (MODE == BMP_AGG_MAX) {
            out = x[0];
#pragma unroll
            for (int t = 1; t < T; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) out[j] = fmaxf(out[j], x[t][j]);
            if (aux) {
                unsigned mask = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int t = 0; t < T; ++t) mask |= (x[t][j] == out[j]) ? (1u << (8 * j + t)) : 0u;
                reinterpret_cast<unsigned*>(aux)[u] = mask;
            }
        } else {
            f32x4 pk[T];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float xe[T], p[T];
#pragma unroll
                for (int t = 0; t < T; ++t) xe[t] = x[t][j];
                out[j] = agg_attn_p<T>(xe, w, bb, p);
#pragma unroll
                for (int s = 0; s < T; ++s) pk[s][j] = p[s];
            }
            if (aux) {
#pragma unroll
                for (int s = 0; s < T; ++s) reinterpret_cast<f32x4*>(aux)[(size_t)s * n4 + u] = pk[s];
            }
        }
        reinterpret_cast<f32x4*>(y)[u] = out;
    }
}

template <int T>
__global__ __launch_bounds__(AGG_TPB) void k_agg_bwd_max(const float* __restrict__ dy, size_t n4, const unsigned* __restrict__ aux,
                                                         AggOut dh) {
    const size_t stride = (size_t)gridDim.x * AGG_TPB;
    for (size_t u = (size_t)blockIdx.x * AGG_TPB + threadIdx.x; u < n4; u += stride) {
        const f32x4 g = reinterpret_cast<const f32x4*>(dy)[u];
        const unsigned mask = aux[u];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = ((mask >> (8 * j + t)) & 1u) ? g[j] : 0.f;
            reinterpret_cast<f32x4*>(dh.p[t])[u] = o;
        }
    }
}

// KEPT: p comes from aux (the forward's T planes) instead of being recomputed from x
template <int T, bool KEPT>
__global__ __launch_bounds__(AGG_TPB) void k_agg_bwd_attn(const float* __restrict__ dy, AggIn h, size_t n4,
                                                          const float* __restrict__ W, const float* __restrict__ b,
                                                          const float* __restrict__ aux, AggOut dh, float* __restrict__ ws) {
    constexpr int NV = T * T + T;
    __shared__ float red[AGG_TPB / 64][NV];
    float w[T * T], bb[T];
    agg_load_w<T>(W, b, w, bb);
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    const size_t stride = (size_t)gridDim.x * AGG_TPB;
    for (size_t u = (size_t)blockIdx.x * AGG_TPB + threadIdx.x; u < n4; u += stride) {
        f32x4 x[T], pk[T], dx[T];
#pragma unroll
        for (int t = 0; t < T; ++t) x[t] = reinterpret_cast<const f32x4*>(h.p[t])[u];
        if (KEPT) {
#pragma unroll
            for (int s = 0; s < T; ++s) pk[s] = reinterpret_cast<const f32x4*>(aux)[(size_t)s * n4 + u];
        }
        const f32x4 g = reinterpret_cast<const f32x4*>(dy)[u];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float xe[T], p[T], dz[T];
            float ye = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) xe[t] = x[t][j];
            if (KEPT) {
#pragma unroll
                for (int s = 0; s < T; ++s) {
                    p[s] = pk[s][j];
                    ye = fmaf(p[s], xe[s], ye);
                }
            } else {
                ye = agg_attn_p<T>(xe, w, bb, p);
            }
            // dy == 0 gives dz = dx = 0 whatever x holds: rows no kernel wrote (past the end of a tile table) carry a zero
            // dy and arbitrary bits in x, and must not reach the sums as 0 * inf
            const bool live = g[j] != 0.f;
#pragma unroll
            for (int s = 0; s < T; ++s) {
                dz[s] = live ? p[s] * (xe[s] - ye) * g[j] : 0.f;
                acc[T * T + s] += dz[s];
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (!live) xe[t] = 0.f;
                float v = live ? p[t] * g[j] : 0.f;
#pragma unroll
                for (int s = 0; s < T; ++s) {
                    v = fmaf(w[s * T + t], dz[s], v);
                    acc[s * T + t] = fmaf(dz[s], xe[t], acc[s * T + t]);
                }
                dx[t][j] = v;
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) reinterpret_cast<f32x4*>(dh.p[t])[u] = dx[t];
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float v = acc[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wv][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int i = threadIdx.x;
        ws[(size_t)blockIdx.x * NV + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    }
}

// out[i] (=|+=) the nb workgroup partials of value i, in a fixed order: thread t adds partials t, t + 256, ... in double,
// then the butterfly and the four wave sums in wave order.  One workgroup per value; i < T*T is dW, the rest db.
__global__ __launch_bounds__(AGG_TPB) void k_agg_reduce(const float* __restrict__ ws, int nb, int nv, int tt, float* __restrict__ dW,
                                                        float* __restrict__ db, int accumulate) {
    __shared__ double red[AGG_TPB / 64];
    const int i = blockIdx.x;
    double s = 0.0;
    for (int k = threadIdx.x; k < nb; k += AGG_TPB) s += (double)ws[(size_t)k * nv + i];
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = (float)(((red[0] + red[1]) + red[2]) + red[3]);
        float* dst = i < tt ? dW + i : db + (i - tt);
        if (i < tt || db) *dst = accumulate ? *dst + v : v;
    }
}

static inline bool agg_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" size_t bmp_layer_agg_ws_floats(int n_rows, int d, int T) {
    if (n_rows <= 0 || d <= 0 || T <= 0) return 0;
    return (size_t)agg_blocks((size_t)n_rows * d / 4) * (size_t)(T * T + T);
}

template <int MODE>
static int agg_fwd_launch(const AggIn& in, int T, size_t n4, const float* W, const float* b, float* y, void* aux, hipStream_t st) {
    const dim3 grid(agg_blocks(n4)), blk(AGG_TPB);
#define AGG_FWD_CASE(TT)                                                                              \
    case TT: hipLaunchKernelGGL((k_agg_fwd<TT, MODE>), grid, blk, 0, st, in, n4, W, b, y, aux); break;
    switch (T) {
        AGG_FWD_CASE(1) AGG_FWD_CASE(2) AGG_FWD_CASE(3) AGG_FWD_CASE(4)
        AGG_FWD_CASE(5) AGG_FWD_CASE(6) AGG_FWD_CASE(7) AGG_FWD_CASE(8)
        default: return -1000 - __LINE__;
    }
#undef AGG_FWD_CASE
    BMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int bmp_layer_agg_fwd(const float* const* h, int T, int n_rows, int d, int mode, const float* W, const float* b,
                                 float* y, void* aux, hipStream_t st) {
    BMP_REQUIRE(h && T >= 1 && T <= AGG_MAXT && n_rows > 0 && d > 0 && d % 4 == 0 && y && agg_aligned(y) && agg_aligned(aux));
    BMP_REQUIRE(mode == BMP_AGG_MAX || (mode == BMP_AGG_ATTN && W));
    AggIn in = {};
    for (int t = 0; t < T; ++t) {
        BMP_REQUIRE(h[t] && agg_aligned(h[t]));
        in.p[t] = h[t];
    }
    const size_t n4 = (size_t)n_rows * d / 4;
    return mode == BMP_AGG_MAX ? agg_fwd_launch<BMP_AGG_MAX>(in, T, n4, W, b, y, aux, st)
                               : agg_fwd_launch<BMP_AGG_ATTN>(in, T, n4, W, b, y, aux, st);
}

extern "C" int bmp_layer_agg_bwd(const float* dy, const float* const* h, int T, int n_rows, int d, int mode, const float* W,
                                 const float* b, const void* aux, float* const* dh, float* dW, float* db, int accumulate_w,
                                 float* ws, size_t ws_floats, hipStream_t st) {
    BMP_REQUIRE(dy && agg_aligned(dy) && dh && T >= 1 && T <= AGG_MAXT && n_rows > 0 && d > 0 && d % 4 == 0 && agg_aligned(aux));
    BMP_REQUIRE(mode == BMP_AGG_MAX || mode == BMP_AGG_ATTN);
    AggOut out = {};
    for (int t = 0; t < T; ++t) {
        BMP_REQUIRE(dh[t] && agg_aligned(dh[t]));
        out.p[t] = dh[t];
    }
    const size_t n4 = (size_t)n_rows * d / 4;
    const int nb = agg_blocks(n4);
    const dim3 grid(nb), blk(AGG_TPB);
    if (mode == BMP_AGG_MAX) {
        BMP_REQUIRE(aux);
        const unsigned* m = reinterpret_cast<const unsigned*>(aux);
#define AGG_MAX_CASE(TT) \
    case TT: hipLaunchKernelGGL((k_agg_bwd_max<TT>), grid, blk, 0, st, dy, n4, m, out); break;
        switch (T) {
            AGG_MAX_CASE(1) AGG_MAX_CASE(2) AGG_MAX_CASE(3) AGG_MAX_CASE(4)
            AGG_MAX_CASE(5) AGG_MAX_CASE(6) AGG_MAX_CASE(7) AGG_MAX_CASE(8)
            default: return -1000 - __LINE__;
        }
#undef AGG_MAX_CASE
        BMP_LAUNCH_CHECK();
        return 0;
    }
    const int nv = T * T + T;
    BMP_REQUIRE(h && W && dW && ws && ws_floats >= (size_t)nb * nv);
    AggIn in = {};
    for (int t = 0; t < T; ++t) {
        BMP_REQUIRE(h[t] && agg_aligned(h[t]));
        in.p[t] = h[t];
    }
    const float* p = reinterpret_cast<const float*>(aux);
#define AGG_ATTN_CASE(TT)                                                                                                  \
    case TT:                                                                                                               \
        if (p) hipLaunchKernelGGL((k_agg_bwd_attn<TT, true>), grid, blk, 0, st, dy, in, n4, W, b, p, out, ws);             \
        else hipLaunchKernelGGL((k_agg_bwd_attn<TT, false>), grid, blk, 0, st, dy, in, n4, W, b, p, out, ws);              \
        break;
    switch (T) {
        AGG_ATTN_CASE(1) AGG_ATTN_CASE(2) AGG_ATTN_CASE(3) AGG_ATTN_CASE(4)
        AGG_ATTN_CASE(5) AGG_ATTN_CASE(6) AGG_ATTN_CASE(7) AGG_ATTN_CASE(8)
        default: return -1000 - __LINE__;
    }
#undef AGG_ATTN_CASE
    BMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_agg_reduce, dim3(nv), blk, 0, st, (const float*)ws, nb, nv, T * T, dW, db, accumulate_w);
    BMP_LAUNCH_CHECK();
    return 0;
}
