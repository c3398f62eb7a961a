// GGNN propagation step with a fuse gate or a simple convex gate in the GRU's place -- models/ggnn_dev_fuse.py:70-131 and
// models/ggnn_dev_gate.py:73-119 of the reference.  The message is the GGNN's (bmp_ggnn_step_*):
//   m = sum_e (agg_e . W_e + wdeg_e b_e),  agg_e = the neighbour sum over the bonds of type e, wdeg_e their summed values;
// the update reads x = [h, m] through linears that are independent of each other:
//   fuse (kind 0):  z = tanh(x W1^T + b1), r = sigmoid(x W2^T + b2), f = sigmoid(x W3^T + b3);  out = keep * (r * h) + f * z
//                   (keep: the dropout mask on r * h, 0 or 1 / (1 - p); null: none)
//   gate (kind 1):  a = sigmoid(x Wg^T + bg);  out = (1 - a) * h + a * m
//
// One kernel per direction, one workgroup of 512 threads (8 waves) per 128-row tile, d in {64, 128}, exact-f32 MFMA 32x32x2, the
// machinery of bmp_wtile.h.  Two [128][d + 4] tiles in LDS, A and B (wave w owns the 32-row block w >> 1 and the column half w & 1):
//   forward   h -> A;  per bond type: agg_e = typed gather(A) -> B, acc_m += B . W_e;  m = acc_m + the bias -> B (and global);
//             acc_u = A . AU[:d] + B . AU[d:] for all Nu / d gates at once;  a barrier (the products read whole rows of A and
//             B);  the activations and out in the accumulators, each lane reading and overwriting its own elements of A and B;
//             then through A / B in turn to global, row-major with 16-byte accesses.
//   backward  per gate g: dpre_g -> A or B in turn (and into gda), acc_dh += dpre_g . U_g[:, :d], acc_dm += dpre_g . U_g[:, d:];
//             dm = acc_dm (+ dout * a, gate) -> B;  per bond type: G_e = typed transposed-CSR gather(B) -> A (and into gda),
//             acc_dh += A . W_e^T;  dh = acc_dh + the direct term (keep * dout * r, fuse; dout * (1 - a), gate).
// h and m never leave the CU between the gather and the update.  The weight gradients are the caller's two calls of
// bmp_linear_wgrad on gda: X = h over all of gda's columns, X = m over its last Nu.
// Weights are K4-packed ([K/4][N][4], as for bmp_ggnn_step_*): a lane's four k values are one 16-byte load.
// The typed message phase reads like the GRU step body's (bmp_wtile_gru.h) and stays inline here: it has no fifth operand to
// switch on, and as a function shared with that body it would be the per-phase split that spills there.
#include "bmp_wtile.h"

enum { GATE_FUSE = 0, GATE_SIMPLE = 1 };

template <int D, int KIND>
__device__ __forceinline__ void gate_step_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                              const float* __restrict__ val, const float* __restrict__ WTp,
                                              const float* __restrict__ bE, const float* __restrict__ AUp,
                                              const float* __restrict__ bU, const float* __restrict__ keep, float* __restrict__ m,
                                              float* __restrict__ act, float* __restrict__ hout) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16, NG = KIND == GATE_FUSE ? 3 : 1, NU = NG * D;
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
        wt_acc_to_tile<D>(tb, am, wv);
    }
    __syncthreads();
    {   // + sum_e wdeg_e b_e, by the thread that took the row's weighted degrees
        float* d = tb + row * LD + q * (D / 4);
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const int c = q * (D / 4) + 4 * f;
            f32x4 v = *(const f32x4*)(d + 4 * f);
#pragma unroll
            for (int e = 0; e < 4; ++e) v += *(const f32x4*)(bE + e * D + c) * wd[e];
            *(f32x4*)(d + 4 * f) = v;
            if (m) *(f32x4*)(m + (size_t)(row0 + row) * D + c) = v;
        }
    }
    __syncthreads();
    f32x16 au[NG][NB];
#pragma unroll
    for (int g = 0; g < NG; ++g) zero_acc(au[g]);
    const float* Bu = AUp + ((size_t)(wv.lane >> 5) * NU + bcol) * 4;
    wt_block_mma_g<NG, NB>(au, ta + aoff, Bu, NU, D, D);
    wt_block_mma_g<NG, NB>(au, tb + aoff, Bu + (size_t)D * NU, NU, D, D);
    // A wave's products read all d columns of its rows of A and B, the column half of its sibling wave included: nobody
    // writes into A or B before every wave has left the products.  Behind the barrier each (row, column) is read and
    // written by the one lane that holds its accumulator element: in place.
    __syncthreads();
    if constexpr (KIND == GATE_FUSE) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = wt_col(wv, NB, nb);
            const float bz = bU[c], br = bU[D + c], bf = bU[2 * D + c];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i = wt_row(wv, reg) * LD + c;
                const float z = bmp_tanh(au[0][nb][reg] + bz), r = bmp_sigmoid(au[1][nb][reg] + br), f = bmp_sigmoid(au[2][nb][reg] + bf);
                au[0][nb][reg] = z; au[1][nb][reg] = r; au[2][nb][reg] = f;
                ta[i] = r * ta[i];
                tb[i] = f * z;
            }
        }
        __syncthreads();
        for (int i = tid; i < WT_R * (D / 4); i += 512) {
            const int r = i / (D / 4), q4 = i % (D / 4);
            const size_t g = (size_t)(row0 + r) * D + 4 * q4;
            f32x4 rh = *(const f32x4*)(ta + r * LD + 4 * q4);
            if (keep) rh = rh * *(const f32x4*)(keep + g);
            *(f32x4*)(hout + g) = rh + *(const f32x4*)(tb + r * LD + 4 * q4);
        }
        if (act == nullptr) return;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float* t = (g & 1) ? tb : ta;                     // z -> A, r -> B, f -> A: one barrier between a store and the next fill
            if (g != 1) __syncthreads();
            wt_acc_to_tile<D>(t, au[g], wv);
            if (g != 0) {
                __syncthreads();
                if (g == 1) wt_store_tile<D>(ta, act, NU, 0, row0, tid);
                wt_store_tile<D>(t, act, NU, g * D, row0, tid);
            }
        }
    } else {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int c = wt_col(wv, NB, nb);
            const float bg = bU[c];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i = wt_row(wv, reg) * LD + c;
                const float a = bmp_sigmoid(au[0][nb][reg] + bg);
                ta[i] = (1.f - a) * ta[i] + a * tb[i];
                tb[i] = a;
            }
        }
        __syncthreads();
        wt_store_tile<D>(ta, hout, D, 0, row0, tid);
        if (act) wt_store_tile<D>(tb, act, NU, 0, row0, tid);
    }
}

template <int D, int KIND>
__device__ __forceinline__ void gate_step_bwd(const float* __restrict__ dhout, const float* __restrict__ h, const float* __restrict__ m,
                                              const float* __restrict__ act, const float* __restrict__ keep,
                                              const int* __restrict__ ptrT, const int* __restrict__ colT,
                                              const float* __restrict__ valT, const float* __restrict__ Wnp,
                                              const float* __restrict__ Unp, float* __restrict__ dh, float* __restrict__ gda) {
    constexpr int LD = D + 4, NB = D / 64, F = D / 16, NG = KIND == GATE_FUSE ? 3 : 1, NU = NG * D, LDG = 4 * D + NU;
    extern __shared__ float sm[];
    float* ta = sm;
    float* tb = sm + WT_R * LD;
    const int tid = threadIdx.x;
    const WtWave wv = wt_wave(tid);
    const int row0 = blockIdx.x * WT_R;
    const int aoff = (wv.b * 32 + (wv.lane & 31)) * LD + 4 * (wv.lane >> 5);
    const size_t bcol = wv.ch * NB * 32 + (wv.lane & 31);
    const f32x4 one4 = (f32x4){1.f, 1.f, 1.f, 1.f};
    f32x16 ad[2][NB];                                         // [0]: dh, [1]: dm
    zero_acc(ad[0]);
    zero_acc(ad[1]);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        float* t = (g & 1) ? tb : ta;                         // in turn: the fill of gate g + 1 needs no barrier of its own
        for (int i = tid; i < WT_R * (D / 4); i += 512) {
            const int r = i / (D / 4), q4 = i % (D / 4);
            const size_t x = (size_t)(row0 + r) * D + 4 * q4;
            const float* ar = act + (size_t)(row0 + r) * NU + 4 * q4;
            const f32x4 dv = *(const f32x4*)(dhout + x);
            f32x4 dp;
            if constexpr (KIND == GATE_FUSE) {
                const f32x4 zv = *(const f32x4*)ar, fv = *(const f32x4*)(ar + 2 * D);
                if (g == 0) dp = dv * fv * (one4 - zv * zv);
                else if (g == 2) dp = dv * zv * fv * (one4 - fv);
                else {
                    const f32x4 rv = *(const f32x4*)(ar + D);
                    dp = dv * *(const f32x4*)(h + x) * rv * (one4 - rv);
                    if (keep) dp = dp * *(const f32x4*)(keep + x);
                }
            } else {
                const f32x4 av = *(const f32x4*)ar;
                dp = dv * (*(const f32x4*)(m + x) - *(const f32x4*)(h + x)) * av * (one4 - av);
                *(f32x4*)(tb + r * LD + 4 * q4) = dv * av;                            // dm's direct term
            }
            *(f32x4*)(t + r * LD + 4 * q4) = dp;
            *(f32x4*)(gda + (size_t)(row0 + r) * LDG + 4 * D + g * D + 4 * q4) = dp;
        }
        __syncthreads();
        wt_block_mma_g<2, NB>(ad, t + aoff, Unp + (size_t)g * D * 2 * D + ((size_t)(wv.lane >> 5) * 2 * D + bcol) * 4, 2 * D, D, D);
    }
    // dm -> B.  fuse: B was last read by gate 1's product, which every wave left before the barrier of gate 2;
    // gate: no product read B, it holds the direct term, each element its lane's own.
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int c = wt_col(wv, NB, nb);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float* p = tb + wt_row(wv, reg) * LD + c;
            *p = KIND == GATE_FUSE ? ad[1][nb][reg] : *p + ad[1][nb][reg];
        }
    }
    __syncthreads();
    {
        const int row = tid >> 2, q = tid & 3;
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
    wt_acc_to_tile<D>(ta, ad[0], wv);                         // (behind the loop's last barrier)
    __syncthreads();
    for (int i = tid; i < WT_R * (D / 4); i += 512) {
        const int r = i / (D / 4), q4 = i % (D / 4);
        const size_t x = (size_t)(row0 + r) * D + 4 * q4;
        const float* ar = act + (size_t)(row0 + r) * NU + 4 * q4;
        f32x4 dv = *(const f32x4*)(dhout + x);
        if constexpr (KIND == GATE_FUSE) {
            dv = dv * *(const f32x4*)(ar + D);
            if (keep) dv = dv * *(const f32x4*)(keep + x);
        } else {
            dv = dv * (one4 - *(const f32x4*)ar);
        }
        *(f32x4*)(dh + x) = *(const f32x4*)(ta + r * LD + 4 * q4) + dv;
    }
}

#define GATE_FWD_ARGS const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,                \
                      const float* __restrict__ val, const float* __restrict__ WTp, const float* __restrict__ bE,            \
                      const float* __restrict__ AUp, const float* __restrict__ bU, const float* __restrict__ keep,           \
                      float* __restrict__ m, float* __restrict__ act, float* __restrict__ hout
#define GATE_BWD_ARGS const float* __restrict__ dhout, const float* __restrict__ h, const float* __restrict__ m,            \
                      const float* __restrict__ act, const float* __restrict__ keep, const int* __restrict__ ptrT,           \
                      const int* __restrict__ colT, const float* __restrict__ valT, const float* __restrict__ Wnp,           \
                      const float* __restrict__ Unp, float* __restrict__ dh, float* __restrict__ gda
template <int D>
__global__ __launch_bounds__(512) void k_fuse_step_tile_fwd(GATE_FWD_ARGS) {
    gate_step_fwd<D, GATE_FUSE>(h, ptr, col, val, WTp, bE, AUp, bU, keep, m, act, hout);
}
template <int D>
__global__ __launch_bounds__(512) void k_gate_step_tile_fwd(GATE_FWD_ARGS) {
    gate_step_fwd<D, GATE_SIMPLE>(h, ptr, col, val, WTp, bE, AUp, bU, keep, m, act, hout);
}
template <int D>
__global__ __launch_bounds__(512) void k_fuse_step_tile_bwd(GATE_BWD_ARGS) {
    gate_step_bwd<D, GATE_FUSE>(dhout, h, m, act, keep, ptrT, colT, valT, Wnp, Unp, dh, gda);
}
template <int D>
__global__ __launch_bounds__(512) void k_gate_step_tile_bwd(GATE_BWD_ARGS) {
    gate_step_bwd<D, GATE_SIMPLE>(dhout, h, m, act, keep, ptrT, colT, valT, Wnp, Unp, dh, gda);
}

extern "C" int bmp_ggnn_gate_step_supported(int d) { return d == 64 || d == 128; }

// kind 0 fuse / 1 gate.  WTp [4d x d]: the message weight as bmp_ggnn_step_fwd takes it; bE [4 x d]; AUp [2d x Nu]: K-major, rows
// [h-part; m-part], columns [z | r | f] (Nu = 3d, fuse) or the gate's (Nu = d), K4-packed; bU [Nu]; keep [N x d] or null (read for
// fuse only).  Saves m [N x d] and act [N x Nu] (post-activation), both null for forward-only evaluation.  N = 128 n_tiles.
extern "C" int bmp_ggnn_gate_step_tile_fwd(int kind, const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col,
                                           const float* csr_val, const float* WTp, const float* bE, const float* AUp, const float* bU,
                                           const float* keep, float* m, float* act, float* hout, hipStream_t st) {
    BMP_REQUIRE((kind == GATE_FUSE || kind == GATE_SIMPLE) && h && n_tiles > 0 && bmp_ggnn_gate_step_supported(d));
    BMP_REQUIRE(csr_ptr && WTp && bE && AUp && bU && hout && (m == nullptr) == (act == nullptr));
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)WTp | (uintptr_t)bE | (uintptr_t)AUp | (uintptr_t)keep | (uintptr_t)m | (uintptr_t)act |
                  (uintptr_t)hout) & 15) == 0);
    if (kind == GATE_FUSE)
        WT_LAUNCH(k_fuse_step_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, AUp, bU, keep, m, act, hout);
    else
        WT_LAUNCH(k_gate_step_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, AUp, bU, keep, m, act, hout);
    return 0;
}
// Wnat_p [d x 4d]: WT^T (row c, column e d + k) as bmp_ggnn_step_bwd takes it; Unat_p [Nu x 2d]: AU^T, K4-packed.  Writes dh [N x d]
// and gda [N x (4d + Nu)] = [G_0 .. G_3 | dpre]: the transposed-CSR gathers of dm per bond type, then the gradient at the update's
// pre-activations.
extern "C" int bmp_ggnn_gate_step_tile_bwd(int kind, const float* dhout, const float* h, const float* m, const float* act,
                                           const float* keep, int n_tiles, int d, const int* csrT_ptr, const int* csrT_col,
                                           const float* csrT_val, const float* Wnat_p, const float* Unat_p, float* dh, float* gda,
                                           hipStream_t st) {
    BMP_REQUIRE((kind == GATE_FUSE || kind == GATE_SIMPLE) && dhout && h && m && act && n_tiles > 0 && bmp_ggnn_gate_step_supported(d));
    BMP_REQUIRE(csrT_ptr && Wnat_p && Unat_p && dh && gda);
    BMP_REQUIRE((((uintptr_t)dhout | (uintptr_t)h | (uintptr_t)m | (uintptr_t)act | (uintptr_t)keep | (uintptr_t)Wnat_p |
                  (uintptr_t)Unat_p | (uintptr_t)dh | (uintptr_t)gda) & 15) == 0);
    if (kind == GATE_FUSE)
        WT_LAUNCH(k_fuse_step_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, m, act, keep, csrT_ptr, csrT_col, csrT_val, Wnat_p, Unat_p, dh, gda);
    else
        WT_LAUNCH(k_gate_step_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, m, act, keep, csrT_ptr, csrT_col, csrT_val, Wnat_p, Unat_p, dh, gda);
    return 0;
}
