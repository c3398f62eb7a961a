// Neural-fingerprint (NFP) encoder on the packed layout -- models/models/nfp.py of the reference:
//   layer   (NFPUpdate.__call__, :36-62):   fv = adj . h (one adjacency: every bond counts once, self loop on the real atoms);
//            out_i = sigmoid(fv_i . W_{deg_i} + B), B = the sum of the seven GraphLinear biases; a position whose degree is
//            none of 1..7 (class 0: padding, hubs of degree > 7) gets sigmoid(B).
//   readout (NFPReadout.__call__, :83-91):  g[mol] += sum over the molecule's positions of softmax_channels(h . W_o + b_o).
// The degree is the COLUMN sum of the adjacency (:157), the layer gathers over ROWS (:45): the class comes from the
// transposed CSR + self_w, the gather walks the forward CSR.  Bond types are ignored (csr_col >> 2 is the source row).
//
// This file holds the per-batch derivations (self_w, deg_class, rows by degree class), the row-wise form for every width
// (d_in, d_out, o multiples of 4; 8 rows per workgroup, weights read through L2, exact f32 FMA chains in a fixed order) and,
// in its second half, the fused per-tile MFMA kernels for d in {64, 128}, which are what those widths run.
// The weight gradient of the widths the listed MFMA launch takes (64 <= d <= 128) runs as seven listed problems of
// bmp_launch_wgrad_fused over the class row lists; the other widths take k_nfp_wgrad below.
#include <string.h>
#include "bmp_wtile.h"

#define NFP_NCLS 7          // degree classes 1..7 (max_degree 6 + 1, nfp.py:26,111); class 0 = none of them
#define NFP_RB 8            // rows per workgroup of the row-wise kernels (N is a multiple of 128)

static inline size_t nfp_max(size_t a, size_t b) { return a > b ? a : b; }

// ---------------------------------------------------------------------------------------------
// per-row data of a batch packed from the store: self_w (1 on real atoms, 0 on pad and dead rows) and the degree class
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nfp_rows(const int* __restrict__ ptrT, const float* __restrict__ valT,
                                                  const int* __restrict__ row_mol, const int* __restrict__ mol_row0,
                                                  const int* __restrict__ mol_nrows, int N, float* __restrict__ self_w,
                                                  int* __restrict__ deg_class) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int m = row_mol[r];
    const float sw = (m >= 0 && r != mol_row0[m] + mol_nrows[m] - 1) ? 1.f : 0.f;
    float deg = sw;                                   // self loop first, then the column's entries in CSR order
    for (int e = ptrT[r]; e < ptrT[r + 1]; ++e) deg += valT[e];
    int k = 0;
#pragma unroll
    for (int c = 1; c <= NFP_NCLS; ++c) k = (deg == (float)c) ? c : k;
    self_w[r] = sw;
    deg_class[r] = k;
}

extern "C" int bmp_nfp_rows(const int* csrT_ptr, const float* csrT_val, const int* row_mol, const int* mol_row0,
                            const int* mol_nrows, int N, float* self_w, int* deg_class, hipStream_t st) {
    BMP_REQUIRE(csrT_ptr && row_mol && mol_row0 && mol_nrows && N > 0 && self_w && deg_class);
    hipLaunchKernelGGL(k_nfp_rows, dim3((N + 255) / 256), dim3(256), 0, st, csrT_ptr, csrT_val, row_mol, mol_row0, mol_nrows, N,
                       self_w, deg_class);
    BMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// rows by degree class: idx[(k - 1) * N + p] = the p-th row (ascending) of class k, cnt[k - 1] = their number.  Two passes
// as bmp_type_rows: the row-list builder of bmp_graph.hip with the class array as the source of a row's membership.
// ---------------------------------------------------------------------------------------------
extern "C" size_t bmp_nfp_deg_rows_ws_ints(int N) { return (size_t)((N + 255) / 256) * 8; }
extern "C" int bmp_nfp_deg_rows(const int* deg_class, int N, int* idx, int* cnt, int* ws, hipStream_t st) {
    BMP_REQUIRE(deg_class && N > 0 && idx && cnt && ws);
    return bmp_launch_row_lists(RowListSrc{nullptr, nullptr, nullptr, deg_class}, NFP_NCLS, N, idx, cnt, ws, st);
}

// ---------------------------------------------------------------------------------------------
// layer forward: 8 rows per workgroup.  Phase 1: fv rows into LDS (and to global for the backward), one thread per
// (row, channel).  Phase 2: one thread per output column, the 8 rows' products in registers; neighbouring rows of one
// class share the weight load.  WT [7][d_in][d_out] (K-major per class), B [d_out].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_nfp_layer_fwd(const float* __restrict__ h, int di, int dO, const int* __restrict__ ptr,
                                                       const int* __restrict__ col, const float* __restrict__ val,
                                                       const float* __restrict__ self_w, const int* __restrict__ cls,
                                                       const float* __restrict__ WT, const float* __restrict__ B,
                                                       float* __restrict__ fv, float* __restrict__ out) {
    extern __shared__ float sm[];                  // [NFP_RB][di]
    __shared__ int scls[NFP_RB];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int row0 = blockIdx.x * NFP_RB;
    if (tid < NFP_RB) scls[tid] = cls[row0 + tid];
    for (int i = tid; i < NFP_RB * di; i += nt) {
        const int r = i / di, k = i - r * di, row = row0 + r;
        float acc = self_w[row] * h[(size_t)row * di + k];
        for (int e = ptr[row]; e < ptr[row + 1]; ++e) acc = fmaf(val[e], h[(size_t)(col[e] >> 2) * di + k], acc);
        sm[i] = acc;
        fv[(size_t)row * di + k] = acc;
    }
    __syncthreads();
    for (int c = tid; c < dO; c += nt) {
        float acc[NFP_RB];
#pragma unroll
        for (int r = 0; r < NFP_RB; ++r) acc[r] = 0.f;
        for (int k = 0; k < di; ++k) {
            int pc = 0;
            float w = 0.f;
#pragma unroll
            for (int r = 0; r < NFP_RB; ++r) {
                const int cr = scls[r];
                if (cr != pc) { w = cr ? WT[((size_t)(cr - 1) * di + k) * dO + c] : 0.f; pc = cr; }
                acc[r] = fmaf(sm[r * di + k], w, acc[r]);
            }
        }
        const float b = B[c];
#pragma unroll
        for (int r = 0; r < NFP_RB; ++r) out[(size_t)(row0 + r) * dO + c] = bmp_sigmoid(acc[r] + b);
    }
}

extern "C" int bmp_nfp_layer_fwd(const float* h, int n_tiles, int d_in, int d_out, const int* csr_ptr, const int* csr_col,
                                 const float* csr_val, const float* self_w, const int* deg_class, const float* WT, const float* B,
                                 float* fv, float* out, hipStream_t st) {
    BMP_REQUIRE(h && n_tiles > 0 && d_in > 0 && d_out > 0 && (d_in & 3) == 0 && (d_out & 3) == 0 && d_in <= 1024);
    BMP_REQUIRE(csr_ptr && self_w && deg_class && WT && B && fv && out);
    const int N = n_tiles * BMP_R;
    hipLaunchKernelGGL(k_nfp_layer_fwd, dim3(N / NFP_RB), dim3(d_out > 64 ? 128 : 64), (size_t)NFP_RB * d_in * sizeof(float), st, h,
                       d_in, d_out, csr_ptr, csr_col, csr_val, self_w, deg_class, WT, B, fv, out);
    BMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// layer backward.  k_nfp_bwd_dfv: dpre = dout * out * (1 - out) (0 on rows of weight 0: dead rows and pad rows that stand
// for no position carry no gradient), dfv = dpre . W_{deg}^T (class 0: 0).  Wnat [7][d_out][d_in] (the reference layout).
// k_nfp_bwd_gather: dh = self_w * dfv + transposed-CSR gather of dfv.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_nfp_bwd_dfv(const float* __restrict__ dout, const float* __restrict__ out, int di, int dO,
                                                     const int* __restrict__ cls, const float* __restrict__ row_w,
                                                     const float* __restrict__ Wnat, float* __restrict__ dpre,
                                                     float* __restrict__ dfv) {
    extern __shared__ float sm[];                  // [NFP_RB][dO]
    __shared__ int scls[NFP_RB];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int row0 = blockIdx.x * NFP_RB;
    if (tid < NFP_RB) scls[tid] = cls[row0 + tid];
    for (int i = tid; i < NFP_RB * dO; i += nt) {
        const int r = i / dO, c = i - r * dO, row = row0 + r;
        const float o = out[(size_t)row * dO + c];
        const float g = row_w[row] != 0.f ? dout[(size_t)row * dO + c] * o * (1.f - o) : 0.f;
        sm[i] = g;
        dpre[(size_t)row * dO + c] = g;
    }
    __syncthreads();
    for (int k = tid; k < di; k += nt) {
        float acc[NFP_RB];
#pragma unroll
        for (int r = 0; r < NFP_RB; ++r) acc[r] = 0.f;
        for (int c = 0; c < dO; ++c) {
            int pc = 0;
            float w = 0.f;
#pragma unroll
            for (int r = 0; r < NFP_RB; ++r) {
                const int cr = scls[r];
                if (cr != pc) { w = cr ? Wnat[((size_t)(cr - 1) * dO + c) * di + k] : 0.f; pc = cr; }
                acc[r] = fmaf(sm[r * dO + c], w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < NFP_RB; ++r) dfv[(size_t)(row0 + r) * di + k] = acc[r];
    }
}
__global__ __launch_bounds__(256) void k_nfp_bwd_gather(const float* __restrict__ dfv, int N, int di, const int* __restrict__ ptrT,
                                                        const int* __restrict__ colT, const float* __restrict__ valT,
                                                        const float* __restrict__ self_w, float* __restrict__ dh) {
    const size_t total = (size_t)N * di;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int row = (int)(i / di), k = (int)(i - (size_t)row * di);
        float acc = self_w[row] * dfv[i];
        for (int e = ptrT[row]; e < ptrT[row + 1]; ++e) acc = fmaf(valT[e], dfv[(size_t)(colT[e] >> 2) * di + k], acc);
        dh[i] = acc;
    }
}

// dfv [N x d_in]: caller-provided scratch.  Writes dpre [N x d_out] (the weight gradient's operand) and dh [N x d_in].
extern "C" int bmp_nfp_layer_bwd(const float* dout, const float* out, int n_tiles, int d_in, int d_out, const int* csrT_ptr,
                                 const int* csrT_col, const float* csrT_val, const float* self_w, const int* deg_class,
                                 const float* row_w, const float* Wnat, float* dpre, float* dfv, float* dh, hipStream_t st) {
    BMP_REQUIRE(dout && out && n_tiles > 0 && d_in > 0 && d_out > 0 && (d_in & 3) == 0 && (d_out & 3) == 0 && d_out <= 1024);
    BMP_REQUIRE(csrT_ptr && self_w && deg_class && row_w && Wnat && dpre && dfv && dh);
    const int N = n_tiles * BMP_R;
    hipLaunchKernelGGL(k_nfp_bwd_dfv, dim3(N / NFP_RB), dim3(d_in > 64 ? 128 : 64), (size_t)NFP_RB * d_out * sizeof(float), st, dout,
                       out, d_in, d_out, deg_class, row_w, Wnat, dpre, dfv);
    BMP_LAUNCH_CHECK();
    size_t blocks = ((size_t)N * d_in + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_nfp_bwd_gather, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)dfv, N, d_in, csrT_ptr, csrT_col,
                       csrT_val, self_w, dh);
    BMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// weight gradient, row-wise form: slab[s][p][i][c] = sum over part s of problem p's rows of X[row, i] * dY[row, c];
// problem p walks the row list ridx + p * N (cnt[p] rows) or, without lists, all N rows.  One workgroup = one 64 x 64
// output tile (4 x 4 per thread), 8 rows staged in LDS per step; a fixed-order sum over the parts follows.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nfp_wgrad(const float* __restrict__ X, int K, const float* __restrict__ dY, int Nn, int N,
                                                   const int* __restrict__ ridx, const int* __restrict__ rcnt, int S,
                                                   float* __restrict__ slab) {
    __shared__ float xs[8][64], ys[8][64];
    const int tid = threadIdx.x;
    const int tk = (K + 63) / 64;
    const int i0 = (blockIdx.x % tk) * 64, c0 = (blockIdx.x / tk) * 64;
    const int p = blockIdx.y, s = blockIdx.z;
    const int cnt = ridx ? rcnt[p] : N;
    const int per = (cnt + S - 1) / S;
    const int lo = s * per, hi = (lo + per) < cnt ? (lo + per) : cnt;
    const int ti = (tid >> 4) * 4, tc = (tid & 15) * 4;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int base = lo; base < hi; base += 8) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + 256 * q, j = e >> 6, cc = e & 63;
            float xv = 0.f, yv = 0.f;
            if (base + j < hi) {
                const int row = ridx ? ridx[(size_t)p * N + base + j] : base + j;
                if (i0 + cc < K) xv = X[(size_t)row * K + i0 + cc];
                if (c0 + cc < Nn) yv = dY[(size_t)row * Nn + c0 + cc];
            }
            xs[j][cc] = xv;
            ys[j][cc] = yv;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float xa[4], yb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { xa[a] = xs[j][ti + a]; yb[a] = ys[j][tc + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(xa[a], yb[b], acc[a][b]);
        }
        __syncthreads();
    }
    float* o = slab + ((size_t)s * gridDim.y + p) * K * Nn;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (i0 + ti + a < K && c0 + tc + b < Nn) o[(size_t)(i0 + ti + a) * Nn + c0 + tc + b] = acc[a][b];
}
__global__ __launch_bounds__(256) void k_nfp_wgrad_reduce(const float* __restrict__ slab, int S, size_t total, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += slab[(size_t)s * total + i];
        out[i] = v;
    }
}
static int nfp_wgrad_parts(int N) {
    int S = N / 512;
    return S < 1 ? 1 : (S > 32 ? 32 : S);
}
// P problems [K x Nn] each (out [P][K][Nn]); slab: nfp_wgrad_parts(N) * P * K * Nn floats
static int nfp_launch_wgrad(const float* X, int K, const float* dY, int Nn, int N, int P, const int* ridx, const int* rcnt, float* out,
                            float* slab, hipStream_t st) {
    const int S = nfp_wgrad_parts(N);
    const int tiles = ((K + 63) / 64) * ((Nn + 63) / 64);
    hipLaunchKernelGGL(k_nfp_wgrad, dim3(tiles, P, S), dim3(256), 0, st, X, K, dY, Nn, N, ridx, rcnt, S, slab);
    BMP_LAUNCH_CHECK();
    const size_t total = (size_t)P * K * Nn;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_nfp_wgrad_reduce, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)slab, S, total, out);
    BMP_LAUNCH_CHECK();
    return 0;
}

// expected share of a batch's rows per degree class (drug molecules live in classes 2-4; with the self loop a terminal
// atom has class 2): only the balance of the listed launch depends on it
static const float kNfpClassFrac[NFP_NCLS] = {0.02f, 0.25f, 0.40f, 0.25f, 0.05f, 0.02f, 0.02f};
static bool nfp_wgrad_listed_ok(int N, int d_in, int d_out) {
    return d_in >= 64 && d_in <= 128 && d_out >= 64 && (d_in & 3) == 0 && (d_out & 3) == 0 && (N & 31) == 0 &&
           bmp_wgrad_fused_lists_ok(N);
}
static int nfp_listed_problems(WGArgs* g, const float* fv, const float* dpre, int N, int d_in, int d_out, const int* deg_rows,
                               const int* deg_cnt, float* dWT) {
    for (int k = 0; k < NFP_NCLS; ++k) {
        g[k] = WGArgs{fv, nullptr, d_in, 0, dpre, d_out, d_in, d_out, N, dWT ? dWT + (size_t)k * d_in * d_out : nullptr, d_out, 0};
        g[k].ridx = deg_rows + (size_t)k * N; g[k].rcnt = deg_cnt + k; g[k].rfrac = kNfpClassFrac[k];
    }
    return NFP_NCLS;
}

extern "C" size_t bmp_nfp_layer_wgrad_ws_floats(int N, int d_in, int d_out) {
    size_t a = (size_t)nfp_wgrad_parts(N) * NFP_NCLS * d_in * d_out;
    if (nfp_wgrad_listed_ok(N, d_in, d_out)) {
        WGArgs g[BMP_WG_MAXP];
        const int n = nfp_listed_problems(g, nullptr, nullptr, N, d_in, d_out, (const int*)16, (const int*)16, nullptr);
        a = nfp_max(a, bmp_wgrad_fused_ws_floats(g, n));
    }
    return a + bmp_colsum_ws_floats(N, d_out);
}
// dWT [7][d_in][d_out]: dW_k = sum over the rows of class k of fv_row^T dpre_row (deg_rows [7 x N] / deg_cnt [7] of
// bmp_nfp_deg_rows); dB [d_out] = column sums of dpre over all rows (every b_k receives it: B is their sum).
// listed != 0: the MFMA launch over the row lists where the shape allows; 0: the row-wise kernel.  Both are bitwise
// reproducible run to run.
extern "C" int bmp_nfp_layer_wgrad(const float* fv, const float* dpre, int N, int d_in, int d_out, const int* deg_rows,
                                   const int* deg_cnt, float* dWT, float* dB, int listed, float* ws, size_t ws_floats,
                                   hipStream_t st) {
    BMP_REQUIRE(fv && dpre && N > 0 && (N & 7) == 0 && d_in > 0 && d_out > 0 && deg_rows && deg_cnt && dWT && dB && ws);
    BMP_REQUIRE(ws_floats >= bmp_nfp_layer_wgrad_ws_floats(N, d_in, d_out));
    float* cs_ws = ws + (ws_floats - bmp_colsum_ws_floats(N, d_out));
    int rc;
    if (listed && nfp_wgrad_listed_ok(N, d_in, d_out) && ((uintptr_t)fv & 15) == 0 && ((uintptr_t)dpre & 15) == 0) {
        WGArgs g[BMP_WG_MAXP];
        const int n = nfp_listed_problems(g, fv, dpre, N, d_in, d_out, deg_rows, deg_cnt, dWT);
        if ((rc = bmp_launch_wgrad_fused(g, n, ws, st, BMP_KID_WGRAD_STEP))) return rc;
    } else {
        if ((rc = nfp_launch_wgrad(fv, d_in, dpre, d_out, N, NFP_NCLS, deg_rows, deg_cnt, dWT, ws, st))) return rc;
    }
    return bmp_launch_colsum(dpre, d_out, N, d_out, dB, 0, cs_ws, st);
}

// ---------------------------------------------------------------------------------------------
// softmax readout.  k_nfp_readout_rows: s[row, :] = softmax over the o channels of h[row, :] . WT + b (8 rows per
// workgroup; one wave per row for the softmax).  k_nfp_readout_sum: g[mol, :] (=|+=) sum over the molecule's rows, in row
// order, of row_w * s[row, :].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_nfp_readout_rows(const float* __restrict__ h, int d, int o, const float* __restrict__ WT,
                                                          const float* __restrict__ b, float* __restrict__ sout) {
    extern __shared__ float sm[];                  // hs [NFP_RB][d] | zs [NFP_RB][o]
    float* hs = sm;
    float* zs = sm + NFP_RB * d;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6, nw = nt >> 6;
    const int row0 = blockIdx.x * NFP_RB;
    for (int i = tid; i < NFP_RB * d; i += nt) hs[i] = h[(size_t)row0 * d + i];
    __syncthreads();
    for (int c = tid; c < o; c += nt) {
        float acc[NFP_RB];
        const float bc = b[c];
#pragma unroll
        for (int r = 0; r < NFP_RB; ++r) acc[r] = bc;
        for (int k = 0; k < d; ++k) {
            const float wv = WT[(size_t)k * o + c];
#pragma unroll
            for (int r = 0; r < NFP_RB; ++r) acc[r] = fmaf(hs[r * d + k], wv, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < NFP_RB; ++r) zs[r * o + c] = acc[r];
    }
    __syncthreads();
    for (int r = w; r < NFP_RB; r += nw) {
        float mx = -3.0e38f;
        for (int c = lane; c < o; c += 64) mx = fmaxf(mx, zs[r * o + c]);
        mx = bmp_wave_max(mx);
        float sum = 0.f;
        for (int c = lane; c < o; c += 64) { const float e = bmp_exp(zs[r * o + c] - mx); zs[r * o + c] = e; sum += e; }
        sum = bmp_wave_sum(sum);
        const float inv = 1.0f / sum;
        for (int c = lane; c < o; c += 64) sout[(size_t)(row0 + r) * o + c] = zs[r * o + c] * inv;
    }
}
__global__ __launch_bounds__(128) void k_nfp_readout_sum(const float* __restrict__ s, int o, const float* __restrict__ row_w,
                                                         const int* __restrict__ mol_row0, const int* __restrict__ mol_nrows,
                                                         int accumulate, float* __restrict__ g) {
    const int m = blockIdx.x;
    const int r0 = mol_row0[m], n = mol_nrows[m];
    for (int c = threadIdx.x; c < o; c += blockDim.x) {
        float acc = 0.f;
        for (int r = r0; r < r0 + n; ++r) acc = fmaf(row_w[r], s[(size_t)r * o + c], acc);
        float* q = g + (size_t)m * o + c;
        *q = accumulate ? (*q + acc) : acc;
    }
}

extern "C" int bmp_nfp_readout_fwd(const float* h, int n_tiles, int d, int o, const float* WT, const float* b, const float* row_w,
                                   const int* mol_row0, const int* mol_nrows, int n_mols, float* s, float* g, int accumulate,
                                   hipStream_t st) {
    BMP_REQUIRE(h && n_tiles > 0 && d > 0 && o > 0 && (d & 3) == 0 && (o & 3) == 0 && d + o <= 1536);
    BMP_REQUIRE(WT && b && row_w && mol_row0 && mol_nrows && n_mols > 0 && s && g);
    const int N = n_tiles * BMP_R;
    hipLaunchKernelGGL(k_nfp_readout_rows, dim3(N / NFP_RB), dim3(128), (size_t)NFP_RB * (d + o) * sizeof(float), st, h, d, o, WT, b, s);
    BMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_nfp_readout_sum, dim3(n_mols), dim3(o > 64 ? 128 : 64), 0, st, (const float*)s, o, row_w, mol_row0, mol_nrows,
                       accumulate, g);
    BMP_LAUNCH_CHECK();
    return 0;
}

// backward: dz[row, c] = row_w * s[row, c] * (dg[mol, c] - sum_c' dg[mol, c'] s[row, c'])  (the softmax Jacobian; rows of no
// molecule: 0), dh = dz . Wnat (Wnat [o x d], the reference layout), dWT [d x o] = h^T dz, db [o] = column sums of dz.
__global__ __launch_bounds__(128) void k_nfp_readout_bwd(const float* __restrict__ dg, const float* __restrict__ s, int d, int o,
                                                         const float* __restrict__ Wnat, const float* __restrict__ row_w,
                                                         const int* __restrict__ row_mol, float* __restrict__ dz,
                                                         float* __restrict__ dh) {
    extern __shared__ float sm[];                  // dzs [NFP_RB][o]
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6, nw = nt >> 6;
    const int row0 = blockIdx.x * NFP_RB;
    for (int r = w; r < NFP_RB; r += nw) {
        const int row = row0 + r;
        const int m = row_mol[row];
        const float rw = m >= 0 ? row_w[row] : 0.f;
        float dot = 0.f;
        if (rw != 0.f)
            for (int c = lane; c < o; c += 64) dot = fmaf(dg[(size_t)m * o + c], s[(size_t)row * o + c], dot);
        dot = bmp_wave_sum(dot);
        for (int c = lane; c < o; c += 64) {
            const float v = rw != 0.f ? rw * s[(size_t)row * o + c] * (dg[(size_t)m * o + c] - dot) : 0.f;
            sm[r * o + c] = v;
            dz[(size_t)row * o + c] = v;
        }
    }
    __syncthreads();
    for (int k = tid; k < d; k += nt) {
        float acc[NFP_RB];
#pragma unroll
        for (int r = 0; r < NFP_RB; ++r) acc[r] = 0.f;
        for (int c = 0; c < o; ++c) {
            const float wv = Wnat[(size_t)c * d + k];
#pragma unroll
            for (int r = 0; r < NFP_RB; ++r) acc[r] = fmaf(sm[r * o + c], wv, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < NFP_RB; ++r) dh[(size_t)(row0 + r) * d + k] = acc[r];
    }
}

extern "C" size_t bmp_nfp_readout_bwd_ws_floats(int N, int d, int o) {
    return (size_t)N * o + nfp_max((size_t)nfp_wgrad_parts(N) * d * o, bmp_wgrad_ws_floats(N, d, o)) + bmp_colsum_ws_floats(N, o);
}
extern "C" int bmp_nfp_readout_bwd(const float* dg, const float* h, const float* s, int n_tiles, int d, int o, const float* Wnat,
                                   const float* row_w, const int* row_mol, float* dh, float* dWT, float* db, float* ws,
                                   size_t ws_floats, hipStream_t st) {
    BMP_REQUIRE(dg && h && s && n_tiles > 0 && d > 0 && o > 0 && (d & 3) == 0 && (o & 3) == 0 && o <= 1024);
    BMP_REQUIRE(Wnat && row_w && row_mol && dh && dWT && db && ws);
    const int N = n_tiles * BMP_R;
    BMP_REQUIRE(ws_floats >= bmp_nfp_readout_bwd_ws_floats(N, d, o));
    float* dz = ws;
    float* slab = dz + (size_t)N * o;
    float* cs_ws = ws + (bmp_nfp_readout_bwd_ws_floats(N, d, o) - bmp_colsum_ws_floats(N, o));
    hipLaunchKernelGGL(k_nfp_readout_bwd, dim3(N / NFP_RB), dim3(128), (size_t)NFP_RB * o * sizeof(float), st, dg, s, d, o, Wnat, row_w,
                       row_mol, dz, dh);
    BMP_LAUNCH_CHECK();
    int rc;
    if ((rc = nfp_launch_wgrad(h, d, dz, o, N, 1, nullptr, nullptr, dWT, slab, st))) return rc;
    return bmp_launch_colsum(dz, o, N, o, db, 0, cs_ws, st);
}

// =============================================================================================
// Fused per-tile forms for d in {64, 128} (exact-f32 MFMA 32x32x2).  One workgroup of 512 threads (8 waves) per 128-row
// tile; wave w owns the 32-row block w >> 1 of the operand tile and the column half w & 1.
//
// Degree-class walk: the tile's rows are ranked by (class 1..7, then class 0; row) -- a fixed order, computed from the
// classes alone -- and the operand rows (fv forward, dpre backward) are laid into LDS at their ranks.  A 32-row block of
// the ranked tile then holds a contiguous run of classes; for every class present in the block the wave runs the MFMAs of
// that class's matrix over the block with the other rows zeroed in the A operand.  Every row belongs to one class, so its
// accumulators receive its product once plus exact zeros; blocks of class-0 rows (pad rows, dead rows at the tile's end,
// hubs) run no MFMA at all.  Work = (block, class) pairs present: at most blocks + classes - 1 block passes per tile.
// Weights are K4-packed per class ([K/4][N][4], as for bmp_ggnn_step_*): a lane's four k values are one 16-byte load.
// The tile load, the MFMA loop, the wave product, the gather and the launch are the shared ones of bmp_wtile.h.
// =============================================================================================
#define NFP_LDZ 132         // row stride of the readout's z / dz tile (o <= 128)

struct NfpOrder { int scl[WT_R]; int skey[WT_R]; unsigned char inv[WT_R]; unsigned char perm[WT_R]; };
// rank of every tile row in the order (class 1..7, class 0; row); ends with a workgroup barrier
__device__ __forceinline__ void nfp_rank_rows(NfpOrder& o, const int* __restrict__ cls, int row0) {
    const int tid = threadIdx.x;
    if (tid < WT_R) o.scl[tid] = cls[row0 + tid];
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

template <int D>
__global__ __launch_bounds__(512) void k_nfp_tile_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                                      const float* __restrict__ val, const float* __restrict__ self_w,
                                                      const int* __restrict__ cls, const float* __restrict__ WTp,
                                                      const float* __restrict__ B, float* __restrict__ fv, float* __restrict__ out) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16;
    extern __shared__ float sm[];
    float* ht = sm;                        // h tile, tile-row order
    float* ft = sm + WT_R * LD;            // fv tile, ranked order
    __shared__ NfpOrder o;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int row0 = blockIdx.x * WT_R;
    wt_load_tile<D>(ht, h, row0, tid);
    nfp_rank_rows(o, cls, row0);           // (its barriers also publish the h tile)
    {
        const int row = tid >> 2, q = tid & 3;
        f32x4 acc[F];
        wt_tile_gather<D, true>(acc, ht, row, q, row0, ptr, col, val, self_w[row0 + row]);
        float* d = ft + o.inv[row] * LD + q * (D / 4);
        float* gq = fv + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) { *(f32x4*)(d + 4 * f) = acc[f]; *(f32x4*)(gq + 4 * f) = acc[f]; }
    }
    __syncthreads();
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

template <int D>
__global__ __launch_bounds__(512) void k_nfp_tile_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                                      const int* __restrict__ ptrT, const int* __restrict__ colT,
                                                      const float* __restrict__ valT, const float* __restrict__ self_w,
                                                      const int* __restrict__ cls, const float* __restrict__ row_w,
                                                      const float* __restrict__ Wnp, float* __restrict__ dpre, float* __restrict__ dh) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16;
    extern __shared__ float sm[];
    float* dt = sm;                        // dpre tile, ranked order
    float* gt = sm + WT_R * LD;            // dfv tile, tile-row order
    __shared__ NfpOrder o;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int row0 = blockIdx.x * WT_R;
    nfp_rank_rows(o, cls, row0);
    for (int i = tid; i < WT_R * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        const size_t g = (size_t)(row0 + r) * D + 4 * q4;
        const f32x4 ov = *(const f32x4*)(out + g), gv = *(const f32x4*)(dout + g);
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (row_w[row0 + r] != 0.f) v = gv * ov * ((f32x4){1.f, 1.f, 1.f, 1.f} - ov);
        *(f32x4*)(dpre + g) = v;
        *(f32x4*)(dt + o.inv[r] * LD + 4 * q4) = v;
    }
    __syncthreads();
    f32x16 acc[NB];
    nfp_class_walk<D>(acc, dt, o, Wnp, wv);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int c = wt_col(wv, NB, nb);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) gt[o.perm[wt_row(wv, reg)] * LD + c] = acc[nb][reg];
    }
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
        f32x4 a[F];
        wt_tile_gather<D, true>(a, gt, row, q, row0, ptrT, colT, valT, self_w[row0 + row]);
        float* gq = dh + (size_t)(row0 + row) * D + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) *(f32x4*)(gq + 4 * f) = a[f];
    }
}

extern "C" int bmp_nfp_layer_supported(int d) { return d == 64 || d == 128; }

// The fused layer: d_in == d_out == d with bmp_nfp_layer_supported(d).  WTp [7][d x d]: W_k^T (K-major) K4-packed per class.
extern "C" int bmp_nfp_layer_tile_fwd(const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col, const float* csr_val,
                                      const float* self_w, const int* deg_class, const float* WTp, const float* B, float* fv,
                                      float* out, hipStream_t st) {
    BMP_REQUIRE(h && n_tiles > 0 && bmp_nfp_layer_supported(d) && csr_ptr && self_w && deg_class && WTp && B && fv && out);
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)WTp | (uintptr_t)fv) & 15) == 0);
    WT_LAUNCH(k_nfp_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, self_w, deg_class, WTp, B, fv, out);
    return 0;
}
// Wnp [7][d x d]: W_k in the reference layout [out x in] (the K-major operand of dfv = dpre . W_k), K4-packed per class.
extern "C" int bmp_nfp_layer_tile_bwd(const float* dout, const float* out, int n_tiles, int d, const int* csrT_ptr, const int* csrT_col,
                                      const float* csrT_val, const float* self_w, const int* deg_class, const float* row_w,
                                      const float* Wnp, float* dpre, float* dh, hipStream_t st) {
    BMP_REQUIRE(dout && out && n_tiles > 0 && bmp_nfp_layer_supported(d) && csrT_ptr && self_w && deg_class && row_w && Wnp && dpre && dh);
    BMP_REQUIRE((((uintptr_t)dout | (uintptr_t)out | (uintptr_t)Wnp | (uintptr_t)dpre | (uintptr_t)dh) & 15) == 0);
    WT_LAUNCH(k_nfp_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, csrT_ptr, csrT_col, csrT_val, self_w, deg_class, row_w, Wnp, dpre, dh);
    return 0;
}

// ---- the readout per tile: z = h . W_o + b_o on MFMA (column blocks of 32, o a multiple of 8 up to 128), softmax per row
// (4 threads per row), the tile's molecules summed in row order by one thread per channel --------------------------------
template <int D>
__global__ __launch_bounds__(512) void k_nfp_readout_tile_fwd(const float* __restrict__ h, int o, const float* __restrict__ WoTp,
                                                              const float* __restrict__ bo, const float* __restrict__ row_w,
                                                              const int* __restrict__ row_mol, float* __restrict__ sout,
                                                              float* __restrict__ g, int accumulate) {
    constexpr int LD = D + 4;
    extern __shared__ float sm[];
    float* ht = sm;
    float* zt = sm + WT_R * LD;            // [128][NFP_LDZ]
    __shared__ int rmol[WT_R];
    __shared__ float rw[WT_R];
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int lane = wv.lane;
    const int row0 = blockIdx.x * WT_R;
    wt_load_tile<D>(ht, h, row0, tid);
    if (tid < WT_R) { rmol[tid] = row_mol[row0 + tid]; rw[tid] = row_w[row0 + tid]; }
    __syncthreads();
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
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
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
template <int D>
__global__ __launch_bounds__(512) void k_nfp_readout_tile_bwd(const float* __restrict__ dg, const float* __restrict__ s, int o,
                                                              const float* __restrict__ Wnp, const float* __restrict__ row_w,
                                                              const int* __restrict__ row_mol, float* __restrict__ dz,
                                                              float* __restrict__ dh) {
    constexpr int NB = D / 64;
    extern __shared__ float sm[];
    float* zt = sm;                        // dz tile [128][NFP_LDZ]
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int row0 = blockIdx.x * WT_R;
    {
        const int row = tid >> 2, q = tid & 3, gr = row0 + row;
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
    __syncthreads();
    f32x16 acc[NB];
    wt_wave_mma<D>(acc, zt, NFP_LDZ, Wnp, o, wv);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int c = wt_col(wv, NB, nb);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) dh[(size_t)(row0 + wt_row(wv, reg)) * D + c] = acc[nb][reg];
    }
}

extern "C" int bmp_nfp_readout_tile_supported(int d, int o) { return (d == 64 || d == 128) && o >= 8 && o <= 128 && (o & 7) == 0; }
// WoTp: W_o^T [d x o] K4-packed; row_mol [N].  Every molecule lies in one tile, whose workgroup takes its sum in row order.
extern "C" int bmp_nfp_readout_tile_fwd(const float* h, int n_tiles, int d, int o, const float* WoTp, const float* b, const float* row_w,
                                        const int* row_mol, float* s, float* g, int accumulate, hipStream_t st) {
    BMP_REQUIRE(h && n_tiles > 0 && bmp_nfp_readout_tile_supported(d, o) && WoTp && b && row_w && row_mol && s && g);
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)WoTp) & 15) == 0);
    const size_t lds = (size_t)WT_R * (d + 4 + NFP_LDZ) * sizeof(float);
    WT_LAUNCH(k_nfp_readout_tile_fwd, d, n_tiles, lds, st, h, o, WoTp, b, row_w, row_mol, s, g, accumulate);
    return 0;
}
// Wnp: W_o [o x d] (reference layout = the K-major operand of dh = dz . W_o) K4-packed.  ws as bmp_nfp_readout_bwd.
extern "C" int bmp_nfp_readout_tile_bwd(const float* dg, const float* h, const float* s, int n_tiles, int d, int o, const float* Wnp,
                                        const float* row_w, const int* row_mol, float* dh, float* dWT, float* db, float* ws,
                                        size_t ws_floats, hipStream_t st) {
    BMP_REQUIRE(dg && h && s && n_tiles > 0 && bmp_nfp_readout_tile_supported(d, o) && Wnp && row_w && row_mol && dh && dWT && db && ws);
    BMP_REQUIRE(((uintptr_t)Wnp & 15) == 0);
    const int N = n_tiles * BMP_R;
    BMP_REQUIRE(ws_floats >= bmp_nfp_readout_bwd_ws_floats(N, d, o));
    float* dz = ws;
    float* slab = dz + (size_t)N * o;
    float* cs_ws = ws + (bmp_nfp_readout_bwd_ws_floats(N, d, o) - bmp_colsum_ws_floats(N, o));
    const size_t lds = (size_t)WT_R * NFP_LDZ * sizeof(float);
    WT_LAUNCH(k_nfp_readout_tile_bwd, d, n_tiles, lds, st, dg, s, o, Wnp, row_w, row_mol, dz, dh);
    int rc;
    if (o >= 64 && ((uintptr_t)h & 15) == 0) {          // dW_o [d x o] and db on the LDS-staged MFMA weight-gradient GEMM
        WGArgs gw{h, nullptr, d, 0, dz, o, d, o, N, dWT, o, 0};
        gw.cs = db;
        return bmp_launch_wgrad(gw, slab, st);
    }
    if ((rc = nfp_launch_wgrad(h, d, dz, o, N, 1, nullptr, nullptr, dWT, slab, st))) return rc;
    return bmp_launch_colsum(dz, o, N, o, db, 0, cs_ws, st);
}
