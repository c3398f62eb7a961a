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
#include "bmp_wtile_nfp.h"

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

// The same on the ENCODER layout (bmp/enclayout.py), whose conventions differ: mol_nrows counts real atoms only and row_mol is
// u >= 0 on a real atom, <= -2 on a tile's pad row and -1 on a dead row.  self_w = 1 exactly where row_mol >= 0; live [N] = 1
// where row_mol != -1 (real atoms and pad rows: the rows that carry gradient, the layer backward's weight there).
__global__ __launch_bounds__(256) void k_nfp_rows_enc(const int* __restrict__ ptrT, const float* __restrict__ valT,
                                                      const int* __restrict__ row_mol, int N, float* __restrict__ self_w,
                                                      int* __restrict__ deg_class, float* __restrict__ live) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int m = row_mol[r];
    const float sw = m >= 0 ? 1.f : 0.f;
    float deg = sw;                                   // self loop first, then the column's entries in CSR order
    for (int e = ptrT[r]; e < ptrT[r + 1]; ++e) deg += valT[e];
    int k = 0;
#pragma unroll
    for (int c = 1; c <= NFP_NCLS; ++c) k = (deg == (float)c) ? c : k;
    self_w[r] = sw;
    deg_class[r] = k;
    live[r] = m != -1 ? 1.f : 0.f;
}

extern "C" int bmp_nfp_rows_enc(const int* csrT_ptr, const float* csrT_val, const int* row_mol, int N, float* self_w, int* deg_class,
                                float* live, hipStream_t st) {
    BMP_REQUIRE(csrT_ptr && row_mol && N > 0 && self_w && deg_class && live);
    hipLaunchKernelGGL(k_nfp_rows_enc, dim3((N + 255) / 256), dim3(256), 0, st, csrT_ptr, csrT_val, row_mol, N, self_w, deg_class, live);
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

// ---------------------------------------------------------------------------------------------
// The readout of a batch in the encoder layout, per INSTANCE from the sums over the encoder rows (beside bmp_encrows_expand /
// bmp_encrows_reduce of bmp_enc.hip).  A padded position leaves layer l as sigmoid(B_l) whatever the molecule, so
//   g_inst[i] = g_real[uid[i]] + padcount[i] * P,   P [o] = sum_l softmax(sigmoid(B_l) . Wo_l^T + bo_l)  (the caller's),
// padcount[i] = row_w of the instance's pad row (inst_row0[i] + inst_nrows[i] - 1).  The backward sums, per encoded molecule
// and in the fixed order of uptr / uinst, the gradients of its instances: no atomics, bitwise reproducible.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nfp_inst_expand(const float* __restrict__ g_real, const float* __restrict__ P, int o,
                                                         const int* __restrict__ uid, const float* __restrict__ row_w,
                                                         const int* __restrict__ inst_row0, const int* __restrict__ inst_nrows, int I,
                                                         float* __restrict__ g_inst) {
    const int total = I * o;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int i = idx / o, c = idx - i * o;
        const float pc = row_w[inst_row0[i] + inst_nrows[i] - 1];
        g_inst[idx] = g_real[(size_t)uid[i] * o + c] + pc * P[c];
    }
}
__global__ __launch_bounds__(256) void k_nfp_inst_reduce(const float* __restrict__ dg_inst, int o, const int* __restrict__ uptr,
                                                         const int* __restrict__ uinst, int U, float* __restrict__ dg_real) {
    const int total = U * o;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int u = idx / o, c = idx - u * o;
        float acc = 0.f;
        for (int k = uptr[u]; k < uptr[u + 1]; ++k) acc += dg_inst[(size_t)uinst[k] * o + c];
        dg_real[idx] = acc;
    }
}
static inline int nfp_inst_blocks(int total) {
    const int b = (total + 255) / 256;
    return b > 4096 ? 4096 : b;
}
extern "C" int bmp_nfp_inst_expand(const float* g_real, const float* P, int o, const int* uid, const float* row_w, const int* inst_row0,
                                   const int* inst_nrows, int n_inst, float* g_inst, hipStream_t st) {
    BMP_REQUIRE(g_real && P && o > 0 && uid && row_w && inst_row0 && inst_nrows && n_inst > 0 && g_inst);
    BMP_REQUIRE((long long)n_inst * o < (1ll << 31));
    hipLaunchKernelGGL(k_nfp_inst_expand, dim3(nfp_inst_blocks(n_inst * o)), dim3(256), 0, st, g_real, P, o, uid, row_w, inst_row0,
                       inst_nrows, n_inst, g_inst);
    BMP_LAUNCH_CHECK();
    return 0;
}
extern "C" int bmp_nfp_inst_reduce(const float* dg_inst, int o, const int* uptr, const int* uinst, int n_enc, float* dg_real,
                                   hipStream_t st) {
    BMP_REQUIRE(dg_inst && o > 0 && uptr && uinst && n_enc > 0 && dg_real);
    BMP_REQUIRE((long long)n_enc * o < (1ll << 31));
    hipLaunchKernelGGL(k_nfp_inst_reduce, dim3(nfp_inst_blocks(n_enc * o)), dim3(256), 0, st, dg_inst, o, uptr, uinst, n_enc, dg_real);
    BMP_LAUNCH_CHECK();
    return 0;
}

// =============================================================================================
// Fused per-tile forms for d in {64, 128} (exact-f32 MFMA 32x32x2).  One workgroup of 512 threads (8 waves) per 128-row
// tile; wave w owns the 32-row block w >> 1 of the operand tile and the column half w & 1.  The bodies -- the degree-class
// walk, the layer both ways, the readout both ways -- are bmp_wtile_nfp.h's, which the tile-table kernels of
// bmp_nfp_table.hip instantiate too; the tile load, the MFMA loop, the wave product, the gather and the launch are the shared
// ones of bmp_wtile.h.
// =============================================================================================
template <int D>
__global__ __launch_bounds__(512) void k_nfp_tile_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                                      const float* __restrict__ val, const float* __restrict__ self_w,
                                                      const int* __restrict__ cls, const float* __restrict__ WTp,
                                                      const float* __restrict__ B, float* __restrict__ fv, float* __restrict__ out) {
    nfp_layer_fwd<D>(h, ptr, col, val, self_w, cls, WTp, B, fv, out);
}

template <int D>
__global__ __launch_bounds__(512) void k_nfp_tile_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                                      const int* __restrict__ ptrT, const int* __restrict__ colT,
                                                      const float* __restrict__ valT, const float* __restrict__ self_w,
                                                      const int* __restrict__ cls, const float* __restrict__ row_w,
                                                      const float* __restrict__ Wnp, float* __restrict__ dpre, float* __restrict__ dh) {
    nfp_layer_bwd<D>(dout, out, ptrT, colT, valT, self_w, cls, row_w, Wnp, dpre, dh);
}

extern "C" int bmp_nfp_layer_supported(int d) { return d == 64 || d == 128; }

// The fused layer: d_in == d_out == d with bmp_nfp_layer_supported(d).  WTp [7][d x d]: W_k^T (K-major) K4-packed per class.
extern "C" int bmp_nfp_layer_tile_fwd(const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col, const float* csr_val,
                                      const float* self_w, const int* deg_class, const float* WTp, const float* B, float* fv,
                                      float* out, hipStream_t st) {
    if (int rc = nfp_layer_fwd_check(bmp_nfp_layer_supported(d), fv != nullptr, h, n_tiles, csr_ptr, self_w, deg_class, WTp, B, fv, out))
        return rc;
    WT_LAUNCH(k_nfp_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, self_w, deg_class, WTp, B, fv, out);
    return 0;
}
// Wnp [7][d x d]: W_k in the reference layout [out x in] (the K-major operand of dfv = dpre . W_k), K4-packed per class.
extern "C" int bmp_nfp_layer_tile_bwd(const float* dout, const float* out, int n_tiles, int d, const int* csrT_ptr, const int* csrT_col,
                                      const float* csrT_val, const float* self_w, const int* deg_class, const float* row_w,
                                      const float* Wnp, float* dpre, float* dh, hipStream_t st) {
    if (int rc = nfp_layer_bwd_check(bmp_nfp_layer_supported(d), dout, out, n_tiles, csrT_ptr, self_w, deg_class, row_w, Wnp, dpre, dh))
        return rc;
    WT_LAUNCH(k_nfp_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, csrT_ptr, csrT_col, csrT_val, self_w, deg_class, row_w, Wnp, dpre, dh);
    return 0;
}

template <int D>
__global__ __launch_bounds__(512) void k_nfp_readout_tile_fwd(const float* __restrict__ h, int o, const float* __restrict__ WoTp,
                                                              const float* __restrict__ bo, const float* __restrict__ row_w,
                                                              const int* __restrict__ row_mol, float* __restrict__ sout,
                                                              float* __restrict__ g, int accumulate) {
    nfp_readout_fwd<D>(h, o, WoTp, bo, row_w, row_mol, sout, g, accumulate);
}
template <int D>
__global__ __launch_bounds__(512) void k_nfp_readout_tile_bwd(const float* __restrict__ dg, const float* __restrict__ s, int o,
                                                              const float* __restrict__ Wnp, const float* __restrict__ row_w,
                                                              const int* __restrict__ row_mol, float* __restrict__ dz,
                                                              float* __restrict__ dh) {
    nfp_readout_bwd<D>(dg, s, o, Wnp, row_w, row_mol, dz, dh);
}

int nfp_readout_wgrad(const float* h, int N, int d, int o, float* dWT, float* db, float* ws, hipStream_t st) {
    float* dz = ws;
    float* slab = dz + (size_t)N * o;
    float* cs_ws = ws + (bmp_nfp_readout_bwd_ws_floats(N, d, o) - bmp_colsum_ws_floats(N, o));
    if (o >= 64 && ((uintptr_t)h & 15) == 0) {          // dW_o [d x o] and db on the LDS-staged MFMA weight-gradient GEMM
        WGArgs gw{h, nullptr, d, 0, dz, o, d, o, N, dWT, o, 0};
        gw.cs = db;
        return bmp_launch_wgrad(gw, slab, st);
    }
    if (int rc = nfp_launch_wgrad(h, d, dz, o, N, 1, nullptr, nullptr, dWT, slab, st)) return rc;
    return bmp_launch_colsum(dz, o, N, o, db, 0, cs_ws, st);
}

extern "C" int bmp_nfp_readout_tile_supported(int d, int o) { return (d == 64 || d == 128) && o >= 8 && o <= 128 && (o & 7) == 0; }
// WoTp: W_o^T [d x o] K4-packed; row_mol [N].  Every molecule lies in one tile, whose workgroup takes its sum in row order.
extern "C" int bmp_nfp_readout_tile_fwd(const float* h, int n_tiles, int d, int o, const float* WoTp, const float* b, const float* row_w,
                                        const int* row_mol, float* s, float* g, int accumulate, hipStream_t st) {
    if (int rc = nfp_readout_fwd_check(bmp_nfp_readout_tile_supported(d, o), h, n_tiles, WoTp, b, row_w, row_mol, s, g)) return rc;
    const size_t lds = (size_t)WT_R * (d + 4 + NFP_LDZ) * sizeof(float);
    WT_LAUNCH(k_nfp_readout_tile_fwd, d, n_tiles, lds, st, h, o, WoTp, b, row_w, row_mol, s, g, accumulate);
    return 0;
}
// Wnp: W_o [o x d] (reference layout = the K-major operand of dh = dz . W_o) K4-packed.  ws as bmp_nfp_readout_bwd.
extern "C" int bmp_nfp_readout_tile_bwd(const float* dg, const float* h, const float* s, int n_tiles, int d, int o, const float* Wnp,
                                        const float* row_w, const int* row_mol, float* dh, float* dWT, float* db, float* ws,
                                        size_t ws_floats, hipStream_t st) {
    if (int rc = nfp_readout_bwd_check(bmp_nfp_readout_tile_supported(d, o), dg, h, s, n_tiles, Wnp, row_w, row_mol, dh, dWT, db, ws))
        return rc;
    const int N = n_tiles * BMP_R;
    BMP_REQUIRE(ws_floats >= bmp_nfp_readout_bwd_ws_floats(N, d, o));
    const size_t lds = (size_t)WT_R * NFP_LDZ * sizeof(float);
    WT_LAUNCH(k_nfp_readout_tile_bwd, d, n_tiles, lds, st, dg, s, o, Wnp, row_w, row_mol, ws, dh);
    return nfp_readout_wgrad(h, N, d, o, dWT, db, ws, st);
}
