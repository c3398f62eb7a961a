// GGNN propagation step with a per-atom self loop in the message -- models/ggnn_dev_self_loop.py:67-110 (= models/ggnn_dev_edge.py)
// of the reference: the GRU step of bmp_ggnn_step_* with a fifth message operand,
//   m = sum_e (agg_e . W_e + wdeg_e b_e) + h . W_s^T + b_s,   agg_e = the neighbour sum over the bonds of type e,
//   out = GRU([h, m]) with the state folded into the h-part (`first`: no r gate, no U term).
//
// One kernel per direction, one workgroup of 512 threads (8 waves) per 128-row tile, d in {64, 128}.  The kernels' body is
// wg_step_fwd / wg_step_bwd<D, FIRST, WG_SELF_LOOP> of bmp_wtile_gru.h, which the edge-network kernels (bmp_edge.hip) share; this
// file holds the kernels and the C entries.  `first` is a TEMPLATE parameter of the body and an argument of the C entries, which
// pick the instance: 2 directions x 2 call forms x 2 widths = 8 kernels.  Weights are K4-packed ([K/4][N][4], as for
// bmp_ggnn_step_*); the weight gradients are the caller's calls of bmp_linear_wgrad on gda (include/bmp.h).
#include "bmp_wtile_gru.h"

#define LOOP_FWD_ARGS const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col, const float* __restrict__ val,            \
                      const float* __restrict__ WTp, const float* __restrict__ bE, const float* __restrict__ WsTp, const float* __restrict__ bs,       \
                      const float* __restrict__ ATp, const float* __restrict__ UcTp, const float* __restrict__ b, float* __restrict__ m,               \
                      float* __restrict__ rz, float* __restrict__ c, float* __restrict__ hout
#define LOOP_BWD_ARGS const float* __restrict__ dhout, const float* __restrict__ h, const float* __restrict__ rz, const float* __restrict__ c,         \
                      const int* __restrict__ ptrT, const int* __restrict__ colT, const float* __restrict__ valT, const float* __restrict__ Wnp,       \
                      const float* __restrict__ Wsp, const float* __restrict__ Anp, const float* __restrict__ Ucp, float* __restrict__ dh,             \
                      float* __restrict__ gda, float* __restrict__ rh

template <int D> __global__ __launch_bounds__(512) void k_loop_step_first_tile_fwd(LOOP_FWD_ARGS) {
    wg_step_fwd<D, true, WG_SELF_LOOP>(h, ptr, col, val, EdgeSeg{}, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout);
}
template <int D> __global__ __launch_bounds__(512) void k_loop_step_later_tile_fwd(LOOP_FWD_ARGS) {
    wg_step_fwd<D, false, WG_SELF_LOOP>(h, ptr, col, val, EdgeSeg{}, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout);
}
template <int D> __global__ __launch_bounds__(512) void k_loop_step_first_tile_bwd(LOOP_BWD_ARGS) {
    wg_step_bwd<D, true, WG_SELF_LOOP>(dhout, h, rz, c, ptrT, colT, valT, EdgeSeg{}, Wnp, Wsp, Anp, Ucp, dh, gda, rh);
}
template <int D> __global__ __launch_bounds__(512) void k_loop_step_later_tile_bwd(LOOP_BWD_ARGS) {
    wg_step_bwd<D, false, WG_SELF_LOOP>(dhout, h, rz, c, ptrT, colT, valT, EdgeSeg{}, Wnp, Wsp, Anp, Ucp, dh, gda, rh);
}

extern "C" int bmp_ggnn_loop_step_supported(int d) { return d == 64 || d == 128; }

// WTp [4d x d], bE [4 x d], ATp [2d x 3d], UcTp [d x d], b [3d]: as bmp_ggnn_step_fwd takes them; WsTp [d x d]: W_s^T (K-major),
// K4-packed; bs [d].  Saves m [N x d], rz [N x 2d] and c [N x d], all three null for forward-only evaluation.  N = 128 n_tiles.
extern "C" int bmp_ggnn_loop_step_tile_fwd(const float* h, int n_tiles, int d, int first, const int* csr_ptr, const int* csr_col,
                                           const float* csr_val, const float* WTp, const float* bE, const float* WsTp, const float* bs,
                                           const float* ATp, const float* UcTp, const float* b, float* m, float* rz, float* c,
                                           float* hout, hipStream_t st) {
    BMP_REQUIRE(bE && bs && (((uintptr_t)bE | (uintptr_t)bs) & 15) == 0);
    if (int rc = wg_fwd_check(bmp_ggnn_loop_step_supported(d), h, n_tiles, first, csr_ptr, WTp, WsTp, ATp, UcTp, b, m, rz, c, hout)) return rc;
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
    if (int rc = wg_bwd_check(bmp_ggnn_loop_step_supported(d), dhout, h, rz, c, n_tiles, first, csrT_ptr, Wnat_p, Ws_p, A_p, Uc_p, dh, gda, rh)) return rc;
    if (first)
        WT_LAUNCH(k_loop_step_first_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, A_p, Uc_p, dh, gda, rh);
    else
        WT_LAUNCH(k_loop_step_later_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, A_p, Uc_p, dh, gda, rh);
    return 0;
}
