// The jumping-knowledge GGNN encoders -- models/ggnn_dev_jknet.py:99-142, 215-226, 297-344 and models/ggnn_dev_jk_gru.py:74-120 of
// the reference: a propagation step whose node update is a relu-linear with no gate, and the parameter-free 'mean' / 'attn'
// layer aggregators.
//
// The step.  The message is the GGNN's (bmp_ggnn_step_*), with the self loop of jk_gru where asked for:
//   m = sum_e (agg_e . W_e + wdeg_e b_e) [+ h . WsT + bs],  agg_e = the neighbour sum over the bonds of type e;
//   out = relu([h, m] . AU + bU),  AU [2d x Nu], Nu = NG d: NG = 1 the whole update of jknet, NG = 2 the 2d-wide layer in front of
//   jk_gru's GRU (which stays the GRU operator: a 2d-wide x tile beside h and m does not fit the LDS of a CU at d = 128).
// One kernel per direction, one workgroup of 512 threads (8 waves) per 128-row tile, d in {64, 128}, exact-f32 MFMA 32x32x2, the
// machinery of bmp_wtile.h, two [128][d + 4] tiles in LDS, A and B, as bmp_gate.hip:
//   forward   h -> A;  per bond type: agg_e = typed gather(A) -> B, acc_m += B . W_e;  self loop: acc_m += A . WsT;
//             m = acc_m + the biases -> B (and global);  acc_u = A . AU[:d] + B . AU[d:] for the NG column blocks at once;
//             a barrier;  relu(acc_u + bU) through A / B in turn to global, row-major with 16-byte stores.
//   backward  per block g: dpre_g = dout_g * [out_g > 0] -> A or B in turn (and into gda), acc_dh | acc_dm += dpre_g . U_g;
//             dm = acc_dm -> the tile X the last product did not read (and into gda with the self loop, acc_dh += X . Ws);
//             per bond type: G_e = typed transposed-CSR gather(X) -> the other tile (and into gda), acc_dh += it . W_e^T;
//             dh = acc_dh.      gda [N x ((4 + loop) d + Nu)] = [G_0 .. G_3 | dm (self loop only) | dpre]
// The two bodies live in bmp_wtile_jk.h: this file instantiates them on whole tiles, bmp_jk_table.hip over a tile table.
// The weight gradients are the caller's two calls of bmp_linear_wgrad on gda: X = h over all of gda's columns, X = m over its
// last Nu.  Every term of the backward carries a factor dout: a zero dout row leaves with zero dh and gda rows.
//
// The aggregators.  With H_t the T step outputs [N x d] and w = row_w (the pad row counts with its multiplicity):
//   attn   E_t = sum_rows w <H_t, H_T> + sum_rows w <H_t, H_1> over the rows of ONE batch side (a contiguous range of tiles),
//          c = softmax_t(E),  y = sum_t c_t H_t;         mean   c_t = 1 / T.
// Memory-bound, three launches per direction: per-tile partial inner products (one workgroup per tile; a butterfly over the
// wave, the four wave sums in wave order), a fold per side over its tiles in a fixed order with the softmax, and the
// elementwise combine.  No floating-point atomics: two runs add the same numbers in the same order.
//   backward  dc_t = sum_rows <dy, H_t> (unweighted: the pad row's dy carries its multiplicity);  dE_t = c_t (dc_t - sum_s c_s dc_s);
//             dH_t = c_t dy + w (dE_t (H_T + H_1) + ([t = T] + [t = 1]) sum_s dE_s H_s)
#include "bmp_wtile_jk.h"

#define JK_FWD_ARGS const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,                  \
                    const float* __restrict__ val, const float* __restrict__ WTp, const float* __restrict__ bE,              \
                    const float* __restrict__ WsTp, const float* __restrict__ bs, const float* __restrict__ AUp,             \
                    const float* __restrict__ bU, float* __restrict__ m, float* __restrict__ out
#define JK_BWD_ARGS const float* __restrict__ dout, const float* __restrict__ out, const int* __restrict__ ptrT,            \
                    const int* __restrict__ colT, const float* __restrict__ valT, const float* __restrict__ Wnp,             \
                    const float* __restrict__ Wsp, const float* __restrict__ Unp, float* __restrict__ dh, float* __restrict__ gda
template <int D>
__global__ __launch_bounds__(512) void k_jk_step1_tile_fwd(JK_FWD_ARGS) {
    jk_step_fwd<D, 1>(h, ptr, col, val, WTp, bE, WsTp, bs, AUp, bU, m, out);
}
template <int D>
__global__ __launch_bounds__(512) void k_jk_step2_tile_fwd(JK_FWD_ARGS) {
    jk_step_fwd<D, 2>(h, ptr, col, val, WTp, bE, WsTp, bs, AUp, bU, m, out);
}
template <int D>
__global__ __launch_bounds__(512) void k_jk_step1_tile_bwd(JK_BWD_ARGS) {
    jk_step_bwd<D, 1>(dout, out, ptrT, colT, valT, Wnp, Wsp, Unp, dh, gda);
}
template <int D>
__global__ __launch_bounds__(512) void k_jk_step2_tile_bwd(JK_BWD_ARGS) {
    jk_step_bwd<D, 2>(dout, out, ptrT, colT, valT, Wnp, Wsp, Unp, dh, gda);
}

extern "C" int bmp_jk_step_supported(int d) { return d == 64 || d == 128; }

// ng 1 / 2: Nu = ng d.  WTp [4d x d], bE [4 x d]: the message weight as bmp_ggnn_step_fwd takes it; WsTp [d x d] K-major, K4-packed,
// and bs [d]: the self loop, both null for none; AUp [2d x Nu]: K-major, rows [h-part; m-part], K4-packed; bU [Nu].  Saves
// m [N x d] (null for forward-only evaluation) and writes out [N x Nu] (what the backward reads back).  N = 128 n_tiles.
extern "C" int bmp_jk_step_tile_fwd(int ng, const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col,
                                    const float* csr_val, const float* WTp, const float* bE, const float* WsTp, const float* bs,
                                    const float* AUp, const float* bU, float* m, float* out, hipStream_t st) {
    if (int rc = jk_fwd_check(bmp_jk_step_supported(d), ng, h, n_tiles, csr_ptr, WTp, bE, WsTp, bs, AUp, bU, m, out)) return rc;
    if (ng == 1)
        WT_LAUNCH(k_jk_step1_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, WsTp, bs, AUp, bU, m, out);
    else
        WT_LAUNCH(k_jk_step2_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, WsTp, bs, AUp, bU, m, out);
    return 0;
}
// Wnat_p [d x 4d]: WT^T as bmp_ggnn_step_bwd takes it; Ws_p [d x d] = (WsT)^T, K4-packed, null for no self loop; Unat_p [Nu x 2d]:
// AU^T, K4-packed.  Writes dh [N x d] and gda [N x ((4 + loop) d + Nu)] = [G_0 .. G_3 | dm (self loop only) | dpre].
extern "C" int bmp_jk_step_tile_bwd(int ng, const float* dout, const float* out, int n_tiles, int d, const int* csrT_ptr,
                                    const int* csrT_col, const float* csrT_val, const float* Wnat_p, const float* Ws_p,
                                    const float* Unat_p, float* dh, float* gda, hipStream_t st) {
    if (int rc = jk_bwd_check(bmp_jk_step_supported(d), ng, dout, out, n_tiles, csrT_ptr, Wnat_p, Ws_p, Unat_p, dh, gda)) return rc;
    if (ng == 1)
        WT_LAUNCH(k_jk_step1_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, Unat_p, dh, gda);
    else
        WT_LAUNCH(k_jk_step2_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, Unat_p, dh, gda);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// 'mean' / 'attn'
// ---------------------------------------------------------------------------------------------------------
#define JK_MAX_SIDES 4

// the T step tensors and the sides' tile boundaries BY VALUE in the kernel arguments (as bmp_agg.hip's AggIn)
struct JkSides { int n; int t[JK_MAX_SIDES + 1]; };           // side s = tiles [t[s], t[s + 1])

__device__ __forceinline__ int jk_side_of(const JkSides& sd, int tile) {
    int s = 0;
#pragma unroll
    for (int k = 1; k < JK_MAX_SIDES; ++k) s += (k < sd.n && tile >= sd.t[k]) ? 1 : 0;
    return s;
}

// One workgroup per tile.  Forward (BWD false): part[tile][t][0 | 1] = sum over the tile's rows of w <H_t, H_T> | w <H_t, H_1>;
// backward: part[tile][t] = sum over the tile's rows of <dy, H_t>.
template <int T, bool BWD>
__global__ __launch_bounds__(JK_TPB) void k_jk_dot(JkIn h, const float* __restrict__ dy, const float* __restrict__ row_w, int d,
                                                   float* __restrict__ part) {
    constexpr int NV = BWD ? T : 2 * T;
    __shared__ float red[JK_TPB / 64][NV];
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    const int d4 = d >> 2;
    const size_t u0 = (size_t)blockIdx.x * WT_R * d4;
    for (int i = threadIdx.x; i < WT_R * d4; i += JK_TPB) {
        const size_t u = u0 + i;
        f32x4 x[T];
#pragma unroll
        for (int t = 0; t < T; ++t) x[t] = reinterpret_cast<const f32x4*>(h.p[t])[u];
        if (BWD) {
            const f32x4 g = reinterpret_cast<const f32x4*>(dy)[u];
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] += (g[0] * x[t][0] + g[1] * x[t][1]) + (g[2] * x[t][2] + g[3] * x[t][3]);
        } else {
            const float w = row_w[(size_t)blockIdx.x * WT_R + i / d4];
            const f32x4 a = x[T - 1] * w, b = x[0] * w;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                acc[2 * t] += (a[0] * x[t][0] + a[1] * x[t][1]) + (a[2] * x[t][2] + a[3] * x[t][3]);
                acc[2 * t + 1] += (b[0] * x[t][0] + b[1] * x[t][1]) + (b[2] * x[t][2] + b[3] * x[t][3]);
            }
        }
    }
    const int lane = threadIdx.x & 63, wvi = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float v = acc[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wvi][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int i = threadIdx.x;
        part[(size_t)blockIdx.x * NV + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    }
}

// One wave per side: the side's tiles folded in a fixed order (lane l adds tiles l, l + 64, ... in double, then the butterfly).
// Forward: E_t, coef[side][t] = softmax_t(E).  Backward: dc_t, then dE[side][t] = c_t (dc_t - sum_s c_s dc_s).
__global__ __launch_bounds__(64) void k_jk_fold(const float* __restrict__ part, JkSides sd, int T, int bwd, float* __restrict__ coef,
                                                float* __restrict__ dE) {
    const int s = blockIdx.x, lane = threadIdx.x, nv = bwd ? T : 2 * T;
    double e[JK_MAXT];
#pragma unroll
    for (int t = 0; t < JK_MAXT; ++t) {
        double v = 0.0;
        if (t < T)
            for (int k = sd.t[s] + lane; k < sd.t[s + 1]; k += 64)
                v += bwd ? (double)part[(size_t)k * nv + t] : (double)part[(size_t)k * nv + 2 * t] + (double)part[(size_t)k * nv + 2 * t + 1];
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        e[t] = v;
    }
    if (lane != 0) return;
    if (!bwd) {
        double mx = -INFINITY, sum = 0.0;
#pragma unroll
        for (int t = 0; t < JK_MAXT; ++t) if (t < T) mx = e[t] > mx ? e[t] : mx;
#pragma unroll
        for (int t = 0; t < JK_MAXT; ++t) if (t < T) { e[t] = exp(e[t] - mx); sum += e[t]; }
#pragma unroll
        for (int t = 0; t < JK_MAXT; ++t) if (t < T) coef[s * T + t] = (float)(e[t] / sum);
    } else {
        double dot = 0.0;
#pragma unroll
        for (int t = 0; t < JK_MAXT; ++t) if (t < T) dot += (double)coef[s * T + t] * e[t];
#pragma unroll
        for (int t = 0; t < JK_MAXT; ++t) if (t < T) dE[s * T + t] = (float)((double)coef[s * T + t] * (e[t] - dot));
    }
}

__global__ __launch_bounds__(64) void k_jk_fill(float* __restrict__ coef, int n, float v) {
    if ((int)threadIdx.x < n) coef[threadIdx.x] = v;
}

// y = sum_t coef[side(row)][t] H_t, the grid strides over the float4 units
template <int T>
__global__ __launch_bounds__(JK_TPB) void k_jk_comb(JkIn h, size_t n4, int d, JkSides sd, const float* __restrict__ coef,
                                                    float* __restrict__ y) {
    const size_t stride = (size_t)gridDim.x * JK_TPB, per_tile = (size_t)WT_R * (d >> 2);
    for (size_t u = (size_t)blockIdx.x * JK_TPB + threadIdx.x; u < n4; u += stride) {
        const float* c = coef + jk_side_of(sd, (int)(u / per_tile)) * T;
        reinterpret_cast<f32x4*>(y)[u] = jk_comb_unit<T>(h, u, c);
    }
}

// dH_t = c_t dy (+ ATTN: w (dE_t (H_T + H_1) + ([t = T] + [t = 1]) sum_s dE_s H_s))
template <int T, bool ATTN>
__global__ __launch_bounds__(JK_TPB) void k_jk_agg_bwd(const float* __restrict__ dy, JkIn h, size_t n4, int d, JkSides sd,
                                                       const float* __restrict__ row_w, const float* __restrict__ coef,
                                                       const float* __restrict__ dE, JkOut dh) {
    const size_t stride = (size_t)gridDim.x * JK_TPB, per_tile = (size_t)WT_R * (d >> 2);
    const int d4 = d >> 2;
    for (size_t u = (size_t)blockIdx.x * JK_TPB + threadIdx.x; u < n4; u += stride) {
        const int s = jk_side_of(sd, (int)(u / per_tile));
        const float* c = coef + s * T;
        const f32x4 g = reinterpret_cast<const f32x4*>(dy)[u];
        if (ATTN) {
            const float* de = dE + s * T;
            const float w = row_w[u / d4];
            f32x4 x[T];
#pragma unroll
            for (int t = 0; t < T; ++t) x[t] = reinterpret_cast<const f32x4*>(h.p[t])[u];
            f32x4 sx = x[0] * de[0];
#pragma unroll
            for (int t = 1; t < T; ++t) sx += x[t] * de[t];
            const f32x4 q = x[T - 1] + x[0];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                f32x4 v = q * de[t];
                if (t == T - 1) v += sx;
                if (t == 0) v += sx;
                reinterpret_cast<f32x4*>(dh.p[t])[u] = g * c[t] + v * w;
            }
        } else {
            jk_scale_unit<T>(dh, u, g, c);
        }
    }
}
static int jk_sides(const int* side_tiles, int n_sides, int n_tiles, JkSides* sd) {
    BMP_REQUIRE(side_tiles && n_sides >= 1 && n_sides <= JK_MAX_SIDES && side_tiles[0] == 0 && side_tiles[n_sides] == n_tiles);
    sd->n = n_sides;
    for (int s = 0; s <= JK_MAX_SIDES; ++s) sd->t[s] = side_tiles[s < n_sides ? s : n_sides];
    for (int s = 0; s < n_sides; ++s) BMP_REQUIRE(sd->t[s] <= sd->t[s + 1]);
    return 0;
}

// floats of the workspace of either direction: the per-tile partials, then (backward) dE [n_sides x T]
extern "C" size_t bmp_jk_agg_ws_floats(int n_tiles, int T) {
    if (n_tiles <= 0 || T <= 0) return 0;
    return (size_t)n_tiles * 2 * T + (size_t)JK_MAX_SIDES * JK_MAXT;
}

// mode 0 mean / 1 attn.  h: T host pointers to the step outputs [128 n_tiles x d]; side_tiles: n_sides + 1 host ints, the tile
// boundaries of the batch sides (read before the call returns).  Writes coef [n_sides x T] (kept for the backward) and y.
extern "C" int bmp_jk_agg_fwd(const float* const* h, int T, int n_tiles, int d, int mode, const float* row_w, const int* side_tiles,
                              int n_sides, float* ws, size_t ws_floats, float* coef, float* y, hipStream_t st) {
    BMP_REQUIRE(h && T >= 1 && T <= JK_MAXT && n_tiles > 0 && d > 0 && d % 4 == 0 && (mode == 0 || mode == 1) && coef && y && jk_aligned(y));
    JkSides sd;
    if (int rc = jk_sides(side_tiles, n_sides, n_tiles, &sd)) return rc;
    JkIn in = {};
    for (int t = 0; t < T; ++t) {
        BMP_REQUIRE(h[t] && jk_aligned(h[t]));
        in.p[t] = h[t];
    }
    if (mode == 1) {
        BMP_REQUIRE(row_w && ws && ws_floats >= bmp_jk_agg_ws_floats(n_tiles, T));
#define JK_CASE(TT) case TT: hipLaunchKernelGGL((k_jk_dot<TT, false>), dim3(n_tiles), dim3(JK_TPB), 0, st, in, (const float*)nullptr, row_w, d, ws); break;
        JK_T_SWITCH(T, JK_CASE)
#undef JK_CASE
        BMP_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jk_fold, dim3(n_sides), dim3(64), 0, st, (const float*)ws, sd, T, 0, coef, (float*)nullptr);
    } else {
        hipLaunchKernelGGL(k_jk_fill, dim3(1), dim3(64), 0, st, coef, n_sides * T, 1.0f / (float)T);
    }
    BMP_LAUNCH_CHECK();
    const size_t n4 = (size_t)n_tiles * WT_R * (d / 4);
#define JK_CASE(TT) case TT: hipLaunchKernelGGL((k_jk_comb<TT>), dim3(jk_blocks(n4)), dim3(JK_TPB), 0, st, in, n4, d, sd, (const float*)coef, y); break;
    JK_T_SWITCH(T, JK_CASE)
#undef JK_CASE
    BMP_LAUNCH_CHECK();
    return 0;
}

// Writes dh[t] [128 n_tiles x d] for every t, zeros included.  coef: the forward's.
extern "C" int bmp_jk_agg_bwd(const float* dy, const float* const* h, int T, int n_tiles, int d, int mode, const float* row_w,
                              const int* side_tiles, int n_sides, const float* coef, float* ws, size_t ws_floats, float* const* dh,
                              hipStream_t st) {
    BMP_REQUIRE(dy && jk_aligned(dy) && h && dh && T >= 1 && T <= JK_MAXT && n_tiles > 0 && d > 0 && d % 4 == 0 && (mode == 0 || mode == 1) && coef);
    JkSides sd;
    if (int rc = jk_sides(side_tiles, n_sides, n_tiles, &sd)) return rc;
    JkIn in = {};
    JkOut out = {};
    for (int t = 0; t < T; ++t) {
        BMP_REQUIRE(h[t] && jk_aligned(h[t]) && dh[t] && jk_aligned(dh[t]));
        in.p[t] = h[t];
        out.p[t] = dh[t];
    }
    const size_t n4 = (size_t)n_tiles * WT_R * (d / 4);
    const dim3 grid(jk_blocks(n4)), blk(JK_TPB);
    if (mode == 0) {
#define JK_CASE(TT) case TT: hipLaunchKernelGGL((k_jk_agg_bwd<TT, false>), grid, blk, 0, st, dy, in, n4, d, sd, row_w, coef, (const float*)nullptr, out); break;
        JK_T_SWITCH(T, JK_CASE)
#undef JK_CASE
        BMP_LAUNCH_CHECK();
        return 0;
    }
    BMP_REQUIRE(row_w && ws && ws_floats >= bmp_jk_agg_ws_floats(n_tiles, T));
    float* dE = ws + (size_t)n_tiles * 2 * T;
#define JK_CASE(TT) case TT: hipLaunchKernelGGL((k_jk_dot<TT, true>), dim3(n_tiles), dim3(JK_TPB), 0, st, in, dy, row_w, d, ws); break;
    JK_T_SWITCH(T, JK_CASE)
#undef JK_CASE
    BMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jk_fold, dim3(n_sides), dim3(64), 0, st, (const float*)ws, sd, T, 1, (float*)coef, dE);
    BMP_LAUNCH_CHECK();
#define JK_CASE(TT) case TT: hipLaunchKernelGGL((k_jk_agg_bwd<TT, true>), grid, blk, 0, st, dy, in, n4, d, sd, row_w, coef, (const float*)dE, out); break;
    JK_T_SWITCH(T, JK_CASE)
#undef JK_CASE
    BMP_LAUNCH_CHECK();
    return 0;
}
