// Fuse-gate / simple-gate GGNN step for NARROW hidden widths (d = 32) on gfx950: the step of bmp_gate.hip (the GGNN message,
// then the fuse gate, kind 0, or the simple convex gate, kind 1, on x = [h, m]; models/ggnn_dev_fuse.py:70-131,
// models/ggnn_dev_gate.py:73-119) with the same operands, outputs and weight layouts, in the wave-local layout of
// bmp_fused_small.hip.
//
// d = 32 is the width of the one recorded run of the fuse-gate encoder (RECORD.txt:404-405: --fp-hidden-dim=32 --conv-layers=8
// --weight-tying=False).  A 128-row tile then holds about 2.6 MFLOP, and the operator chain the kernel replaces (message
// operator, cat, row linear, six to eight elementwise operators forward and twice that backward) is bound by launch latency and
// by the HBM round trips of m, x, pre, z, r, f and r * h.
//
//   workgroup = 256 threads = 4 waves, one 128-row tile; wave w owns the 32-row block w in every phase (gather rows, MFMA A
//   rows, epilogue rows: bmp_stile.h).  LDS = two [128 x 36] f32 tiles + the per-row weighted degrees + the tile's CSR = 48 KB,
//   three workgroups per CU.  Weights are K4-packed and stream from L2 into the MFMA B registers (tile_mma, bmp_tile.h).
//   forward   h -> H, CSR -> LDS; BARRIER; per bond type: typed gather(H) -> A (own rows), acc_m += A . W_e unless the wave's rows
//             hold no bond of the type; m = acc_m + sum_e wdeg_e b_e -> A (and global); acc_u[g] = H . AU[:d, g] + A . AU[d:, g];
//             the activations and out in the accumulators.  One workgroup barrier.
//   backward  dpre_g -> X / Y (own rows, and into gda), [dh | dm] += dpre_g . U_g; dm (+ dout * a, gate) -> X; BARRIER (the
//             transposed gather reads dm of every row of the tile, and the staged CSR); per bond type: G_e = gather^T(X) -> Y
//             (and into gda), dh += Y . W_e^T unless absent; dh += the direct term.  One workgroup barrier.
// A null keep means no dropout; null m and act together select the forward that saves nothing.
// The _table entries take a tile table (encoder layout, bmp/enclayout.py; fixed-shape batch, bmp.packed.StaticPairBatch): tile t =
// rows [mt_row0[t], + 32 * mt_nblk[t]), 1..4 live blocks.  The waves of the dead blocks stage their share of the CSR, meet the
// kernel's barrier and leave; with a fixed tile stride the rows of the dead blocks are cleared in everything the kernel writes,
// because the weight-gradient GEMMs behind the step walk all rows.
#include "bmp_stile.h"
#include "bmp_gate_small.h"

size_t gs_lds_bytes(int D) { return ((size_t)2 * FS_R * (D + 4) + FS_R * 4 + 132 + 2 * FZ_ECAP + 4) * sizeof(float); }

extern "C" int bmp_ggnn_gate_step_small_supported(int d) { return d == 32; }

// The d = 32 form of bmp_ggnn_gate_step_tile_fwd (bmp_gate.hip): the same arguments, layouts and checks.
extern "C" int bmp_ggnn_gate_step_small_fwd(int kind, const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col,
                                            const float* csr_val, const float* WTp, const float* bE, const float* AUp, const float* bU,
                                            const float* keep, float* m, float* act, float* hout, hipStream_t st) {
    return gs_fwd<false>(kind, h, n_tiles, d, csr_ptr, csr_col, csr_val, WTp, bE, AUp, bU, keep, m, act, hout, nullptr, nullptr, 0, st);
}

// The d = 32 form of bmp_ggnn_gate_step_tile_bwd.
extern "C" int bmp_ggnn_gate_step_small_bwd(int kind, const float* dhout, const float* h, const float* m, const float* act,
                                            const float* keep, int n_tiles, int d, const int* csrT_ptr, const int* csrT_col,
                                            const float* csrT_val, const float* Wnat_p, const float* Unat_p, float* dh, float* gda,
                                            hipStream_t st) {
    return gs_bwd<false>(kind, dhout, h, m, act, keep, n_tiles, d, csrT_ptr, csrT_col, csrT_val, Wnat_p, Unat_p, dh, gda, nullptr, nullptr, 0, st);
}
