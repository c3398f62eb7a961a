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
// The tile load, the MFMA loop, the wave product, the gather and the launch are the shared ones of bmp_wtile.h; the two bodies
// are gin_layer_fwd / gin_layer_bwd of bmp_wtile_gin.h, which the tile-table kernels of bmp_gin_table.hip instantiate with VAR.
#include "bmp_wtile_gin.h"

template <int D>
__global__ __launch_bounds__(512) void k_gin_tile_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                                      const float* __restrict__ val, const float* __restrict__ W1p,
                                                      const float* __restrict__ b1, const float* __restrict__ W2p,
                                                      const float* __restrict__ b2, const float* __restrict__ keep,
                                                      float* __restrict__ s, float* __restrict__ t, float* __restrict__ out) {
    gin_layer_fwd<D>(h, ptr, col, val, W1p, b1, W2p, b2, keep, s, t, out);
}

template <int D>
__global__ __launch_bounds__(512) void k_gin_tile_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                                      const float* __restrict__ keep, const float* __restrict__ t,
                                                      const int* __restrict__ ptrT, const int* __restrict__ colT,
                                                      const float* __restrict__ valT, const float* __restrict__ W2np,
                                                      const float* __restrict__ W1np, float* __restrict__ dp2,
                                                      float* __restrict__ dp1, float* __restrict__ dh) {
    gin_layer_bwd<D>(dout, out, keep, t, ptrT, colT, valT, W2np, W1np, dp2, dp1, dh);
}

extern "C" int bmp_gin_layer_supported(int d) { return d == 64 || d == 128; }

// W1p / W2p [d x d]: W1^T / W2^T (K-major) K4-packed.  keep [N x d] or null (no dropout).  Saves s, t [N x d]; N = 128 n_tiles.
extern "C" int bmp_gin_layer_tile_fwd(const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col, const float* csr_val,
                                      const float* W1p, const float* b1, const float* W2p, const float* b2, const float* keep,
                                      float* s, float* t, float* out, hipStream_t st) {
    if (int rc = gin_fwd_check(bmp_gin_layer_supported(d), s && t, h, n_tiles, csr_ptr, W1p, b1, W2p, b2, keep, s, t, out)) return rc;
    WT_LAUNCH(k_gin_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, W1p, b1, W2p, b2, keep, s, t, out);
    return 0;
}
// W2np / W1np [d x d]: W2 / W1 in the reference layout [out x in] (the K-major operands of dt = dp2 . W2, ds = dp1 . W1), K4-packed.
extern "C" int bmp_gin_layer_tile_bwd(const float* dout, const float* out, const float* keep, const float* t, int n_tiles, int d,
                                      const int* csrT_ptr, const int* csrT_col, const float* csrT_val, const float* W2np,
                                      const float* W1np, float* dp2, float* dp1, float* dh, hipStream_t st) {
    if (int rc = gin_bwd_check(bmp_gin_layer_supported(d), dout, out, keep, t, n_tiles, csrT_ptr, W2np, W1np, dp2, dp1, dh)) return rc;
    WT_LAUNCH(k_gin_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, keep, t, csrT_ptr, csrT_col, csrT_val, W2np, W1np, dp2, dp1, dh);
    return 0;
}
