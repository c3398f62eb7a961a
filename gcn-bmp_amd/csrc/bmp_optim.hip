// Chainer's optimizer hooks in front of Adam (train_binary.py:538-543: GradientClipping, WeightDecay, Lasso, added in that
// order when their rates are set), as two launches over the flat buffers:
//   * bmp_grad_sumsq_partials: a fixed grid of P = bmp_sumsq_parts(n) blocks, each writes the sum of squares of its slice of
//     the gradient as clipping sees it (g * grad_scale, plus the decay / Lasso terms of hooks added before the clip);
//   * bmp_adam_step_hooked: every block reduces the same partials in the same order (so every block holds the same clip
//     scale, bit for bit), then each element takes grad_scale, the hooks in their order and bmp_adam_step's update.
// Two launches instead of one with a grid-wide hand-off: no atomics, no spin on blocks that may not be resident.
// bmp_adam_step (bmp_host.hip) stays the launch of a step without hooks.
#include "bmp_common.h"

// hook_order: up to three 2-bit codes, the first hook in the low bits, 0 ends the list
enum { BMP_HOOK_END = 0, BMP_HOOK_CLIP = 1, BMP_HOOK_DECAY = 2, BMP_HOOK_LASSO = 3 };
#define BMP_SUMSQ_PARTS_MAX 256
#define BMP_SUMSQ_CHUNK 2048          // elements per block of the partials grid below the cap

// P depends on n alone: the partials of one gradient always come from the same grid, whatever the stream or occupancy
__host__ __device__ static inline int bmp_sumsq_parts(int n) {
    const int p = (n + BMP_SUMSQ_CHUNK - 1) / BMP_SUMSQ_CHUNK;
    return p < 1 ? 1 : (p > BMP_SUMSQ_PARTS_MAX ? BMP_SUMSQ_PARTS_MAX : p);
}

static bool bmp_hook_order_ok(int order) {
    if (order <= 0 || order >= 64) return false;
    int seen = 0, k = 0;
    for (; k < 3 && ((order >> (2 * k)) & 3); ++k) {
        const int c = (order >> (2 * k)) & 3;
        if (seen & (1 << c)) return false;
        seen |= 1 << c;
    }
    return (order >> (2 * k)) == 0;       // nothing after the terminating 0
}

__device__ __forceinline__ float bmp_sign(float x) { return (float)(x > 0.f) - (float)(x < 0.f); }

// the gradient element as the hooks leave it, up to (not including) the first code equal to `stop`
__device__ __forceinline__ float bmp_hooks_apply(float x, float p, int order, int stop, float scale, float l2, float l1) {
    for (int k = 0; k < 3; ++k) {
        const int c = (order >> (2 * k)) & 3;
        if (c == BMP_HOOK_END || c == stop) break;
        if (c == BMP_HOOK_CLIP) x *= scale;
        else if (c == BMP_HOOK_DECAY) x += l2 * p;
        else x += l1 * bmp_sign(p);
    }
    return x;
}

// fixed-order sum over the block's 256 threads: butterfly within each wave64, then the four wave sums in wave order
__device__ __forceinline__ double bmp_block_sum256(double s, double* lds) {
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__device__ __forceinline__ f32x4 bmp_load4(const float* q, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(q);
    f32x4 r;
    r.x = q[0]; r.y = q[1]; r.z = q[2]; r.w = q[3];
    return r;
}

// The gradient's 16-byte-aligned body goes as float4 units, P equal runs of units, one per block; the <= 3 elements before
// it (a view that starts mid-vector) fall to block 0, the <= 3 after it to block P-1.  p (read only when a decay / Lasso
// hook precedes the clip) is loaded as float4 where its alignment matches g's, element by element otherwise.
__global__ __launch_bounds__(256) void k_grad_sumsq_partials(float* __restrict__ partials, const float* __restrict__ g,
                                                             const float* __restrict__ p, int n, float gscale, float l2_host,
                                                             float l1_host, const float* __restrict__ hook_dev, int order,
                                                             int head) {
    __shared__ double lds[4];
    const float l2 = hook_dev ? hook_dev[1] : l2_host;
    const float l1 = hook_dev ? hook_dev[2] : l1_host;
    const bool pre = (order & 3) != BMP_HOOK_CLIP;    // a decay / Lasso term enters the norm
    const int P = gridDim.x, b = blockIdx.x, t = threadIdx.x;
    const int nv = (n - head) >> 2;
    const int tail = n - head - 4 * nv;
    const int per = (nv + P - 1) / P;
    const int u0 = min(nv, b * per), u1 = min(nv, u0 + per);
    const float* gb = g + head;
    const float* pb = pre ? p + head : nullptr;
    const bool pvec = pre && ((reinterpret_cast<uintptr_t>(pb) & 15) == 0);
    double s = 0.0;
    for (int u = u0 + t; u < u1; u += 256) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(gb + 4 * (size_t)u);
        f32x4 pv = {0.f, 0.f, 0.f, 0.f};
        if (pre) pv = bmp_load4(pb + 4 * (size_t)u, pvec);
        for (int j = 0; j < 4; ++j) {
            const float x = bmp_hooks_apply(gv[j] * gscale, pv[j], order, BMP_HOOK_CLIP, 1.f, l2, l1);
            s += (double)x * (double)x;
        }
    }
    for (int k = 0; k < 2; ++k) {                     // with P = 1 one thread may take a head and a tail element
        const int e = k == 0 ? (b == 0 && t < head ? t : -1) : (b == P - 1 && t < tail ? head + 4 * nv + t : -1);
        if (e < 0) continue;
        const float x = bmp_hooks_apply(g[e] * gscale, pre ? p[e] : 0.f, order, BMP_HOOK_CLIP, 1.f, l2, l1);
        s += (double)x * (double)x;
    }
    s = bmp_block_sum256(s, lds);
    if (t == 0) partials[b] = (float)s;
}

// chainer Adam (k_adam) on the hooked gradient.  With a clip in `order`, the block first sums partials[0..P) -- one per
// thread, then bmp_block_sum256: the same order in every block -- and scale = min(1, threshold / sqrt(sum)) in fp32 (a zero
// norm gives threshold / 0 = inf -> 1).  Block 0 writes the norm to norm_out when given.
__global__ __launch_bounds__(256) void k_adam_hooked(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                     float* __restrict__ v, int n, float alpha_host,
                                                     const float* __restrict__ alpha_dev, float b1, float b2, float eps,
                                                     float wd, float gscale, float thr_host, float l2_host, float l1_host,
                                                     const float* __restrict__ hook_dev, int order,
                                                     const float* __restrict__ partials, int P, float* __restrict__ norm_out) {
    __shared__ double lds[4];
    const float alpha_t = alpha_dev ? alpha_dev[0] : alpha_host;
    const float thr = hook_dev ? hook_dev[0] : thr_host;
    const float l2 = hook_dev ? hook_dev[1] : l2_host;
    const float l1 = hook_dev ? hook_dev[2] : l1_host;
    float scale = 1.f;
    if (partials) {
        const double s = bmp_block_sum256(threadIdx.x < P ? (double)partials[threadIdx.x] : 0.0, lds);
        const float norm = (float)sqrt(s);
        scale = fminf(1.f, thr / norm);
        if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        float pi = p[i];
        const float gi = bmp_hooks_apply(g[i] * gscale, pi, order, -1, scale, l2, l1);
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        if (wd != 0.f) pi *= (1.f - wd);
        p[i] = pi - alpha_t * mi / (sqrtf(vi) + eps);
    }
}

static int bmp_order_has(int order, int code) {
    for (int k = 0; k < 3; ++k)
        if (((order >> (2 * k)) & 3) == code) return 1;
    return 0;
}

extern "C" int bmp_grad_sumsq_partials(float* partials, const float* g, const float* p, int n, float grad_scale,
                                       float l2_rate, float l1_rate, const float* hook_dev, int hook_order, hipStream_t st) {
    BMP_REQUIRE(n >= 1 && partials && g && bmp_hook_order_ok(hook_order) && bmp_order_has(hook_order, BMP_HOOK_CLIP));
    BMP_REQUIRE((reinterpret_cast<uintptr_t>(g) & 3) == 0 && (!p || (reinterpret_cast<uintptr_t>(p) & 3) == 0));
    BMP_REQUIRE(p || (hook_order & 3) == BMP_HOOK_CLIP);
    int head = (int)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2);     // elements before g's first 16-byte boundary
    if (head > n) head = n;
    hipLaunchKernelGGL(k_grad_sumsq_partials, dim3(bmp_sumsq_parts(n)), dim3(256), 0, st, partials, g, p, n, grad_scale,
                       l2_rate, l1_rate, hook_dev, hook_order, head);
    BMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int bmp_adam_step_hooked(float* p, const float* g, float* m, float* v, int n, float alpha_t, const float* alpha_t_dev,
                                    float beta1, float beta2, float eps, float weight_decay_rate, float grad_scale,
                                    float clip_threshold, float l2_rate, float l1_rate, const float* hook_dev, int hook_order,
                                    const float* partials, float* norm_out, hipStream_t st) {
    BMP_REQUIRE(n >= 0 && p && g && m && v && bmp_hook_order_ok(hook_order));
    const int clip = bmp_order_has(hook_order, BMP_HOOK_CLIP);
    BMP_REQUIRE(clip ? partials != nullptr : (partials == nullptr && norm_out == nullptr));
    if (n == 0) return 0;
    int blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_adam_hooked, dim3(blocks), dim3(256), 0, st, p, g, m, v, n, alpha_t, alpha_t_dev, beta1, beta2, eps,
                       weight_decay_rate, grad_scale, clip_threshold, l2_rate, l1_rate, hook_dev, hook_order, partials,
                       bmp_sumsq_parts(n), norm_out);
    BMP_LAUNCH_CHECK();
    return 0;
}
