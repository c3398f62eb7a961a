// Kernels and launchers of the d = 32 fuse-gate / simple-gate GGNN step (see bmp_gate_small.hip for the design): shared by the
// whole-tile entries (bmp_gate_small.hip, VAR = false) and the tile-table entries (bmp_gate_small_table.hip, VAR = true), each file
// instantiating its own six kernels.
#pragma once
#include "bmp_stile.h"

enum { GS_FUSE = 0, GS_GATE = 1 };

struct GateSmallArgs {
    const int* ptr; const int* col; const float* val;      // CSR (fwd) or transposed CSR (bwd)
    const float* h;                 // [N x D]
    const float* keep;              // [N x D] or null
    // forward
    const float* WTp;               // [4D x D]  message weights, K-major, K4-packed
    const float* bE;                // [4 x D]
    const float* AUp;               // [2D x Nu] rows [h ; m], columns [z | r | f] or the gate's, K4-packed
    const float* bU;                // [Nu]
    float* m_out; float* act_out; float* hout;
    // backward
    const float* dhout; const float* m; const float* act;
    const float* Wnp;               // [D x 4D]  (= WT^T), K4-packed
    const float* Unp;               // [Nu x 2D] (= AU^T), K4-packed
    float* dh;                      // [N x D]
    float* gda;                     // [N x (4D + Nu)] = [G_0 .. G_3 | dpre]
    // optional tile table (VAR kernels): StepArgs' mt_row0 / mt_nblk / tile_stride (bmp_tile.h)
    const int* mt_row0; const int* mt_nblk;
    int tile_stride;
};

template <int D, int KIND, bool SAVE, bool VAR>
__global__ __launch_bounds__(FS_NT) void k_gate_step_fwd_s(GateSmallArgs a) {
    static_assert(D == 32, "one 32-column MFMA block per row");
    constexpr int LD = D + 4, NG = KIND == GS_FUSE ? 3 : 1, NU = NG * D;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Hs = lds;                         // [128 x LD]  h tile (whole step)
    float* As = lds + FS_R * LD;             // [128 x LD]  AGG_e -> m   (each wave: its own 32 rows)
    float* wds = As + FS_R * LD;             // [128 x 4]   weighted degree per bond type
    int* rptr = (int*)(wds + FS_R * 4);      // [132]
    int* ecol = rptr + 132;                  // [FZ_ECAP]
    float* evalv = (float*)(ecol + FZ_ECAP); // [FZ_ECAP]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int row0 = VAR ? a.mt_row0[blockIdx.x] : blockIdx.x * FS_R;
    const int nblk = VAR ? a.mt_nblk[blockIdx.x] : 4;
    const int nrows = VAR ? nblk * 32 : FS_R;
    if (VAR && a.tile_stride > nrows) {      // fixed-stride tile table: the blocks without atoms, in every array written
        const int e = row0 + a.tile_stride;
        fz_clear_rows<FS_NT>(a.hout, D, row0 + nrows, e, tid);
        fz_clear_rows<FS_NT>(a.m_out, D, row0 + nrows, e, tid);
        fz_clear_rows<FS_NT>(a.act_out, NU, row0 + nrows, e, tid);
    }
    const int col = l31;
    const int wrow0 = w * 32;
    const int lrow = wrow0 + 4 * hi;         // this lane's row for accumulator register 0
    const int grow = wrow0 + (lane >> 1), gq = lane & 1;      // this lane's row and column half in the gathers
    const int rot = (blockIdx.x * 8) % D;
    const float* Hw = Hs + (wrow0 + l31) * LD + 4 * hi;
    const float* Aw = As + (wrow0 + l31) * LD + 4 * hi;
    float* Hl = Hs + lrow * LD + col;
    float* Al = As + lrow * LD + col;

    for (int idx = tid; idx < nrows * (D / 4); idx += FS_NT) {
        const int r = idx / (D / 4), c4 = idx % (D / 4);
        *(f32x4*)(Hs + r * LD + 4 * c4) = *(const f32x4*)(a.h + (size_t)(row0 + r) * D + 4 * c4);
    }
    const bool csr_lds = stage_csr(a.ptr, a.col, a.val, row0, rptr, ecol, evalv, nrows, FS_NT);
    __syncthreads();                         // the only workgroup barrier: h and the CSR are in place
    if (VAR && w >= nblk) return;            // a short tile: this block has no rows

    int tmask = 0, types = 0;
    // ---- message: m = sum_e AGG_e . W_e + wdeg_e * b_e ----
    f32x16 acc_m[1][1];
    zero_acc(acc_m[0]);
    for (int e = 0; e < 4; ++e) {
        const float* const Bp[1] = {a.WTp + (size_t)(e * D + 4 * hi) * D + 4 * col};
        const int ldw[1] = {D};
        BPre<1> pre;
        tile_b_prefetch<1>(pre, Bp, ldw, D, rot);
        const float wd = FS_GATHER(Hs, As, e);
        if (gq == 0) wds[grow * 4 + e] = wd;
        if (e == 0) types = fs_wave_types(tmask);         // the first pass walks every entry of the wave's rows
        FS_WSYNC();
        if ((types >> e) & 1) tile_mma<1, 1, 1>(acc_m, Aw, LD, Bp, ldw, D, rot, &pre);
        FS_WSYNC();
    }
    int ldwg[NG];
    const float* Bh[NG]; const float* Bm[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        ldwg[g] = NU;
        Bh[g] = a.AUp + (size_t)(4 * hi) * NU + 4 * col + 4 * D * g;
        Bm[g] = a.AUp + (size_t)(D + 4 * hi) * NU + 4 * col + 4 * D * g;
    }
    BPre<NG> pre_h;
    tile_b_prefetch<NG>(pre_h, (const float* const (&)[NG])Bh, (const int (&)[NG])ldwg, D, rot);
    {   // m -> LDS (A operand of the update) and global (saved for the backward)
        const AccBuf mo = acc_buf<D>(a.m_out, row0, lrow, col);
        float be[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) be[e] = a.bE[e * D + col];
        FS_FOR_ACC {
            const int r = lrow + (reg & 3) + 8 * (reg >> 2);
            const f32x4 wd4 = *(const f32x4*)(wds + r * 4);
            const float v = __builtin_fmaf(wd4[3], be[3], __builtin_fmaf(wd4[2], be[2], __builtin_fmaf(wd4[1], be[1],
                                           __builtin_fmaf(wd4[0], be[0], acc_m[0][0][reg]))));
            Al[FS_LOFF(reg)] = v;
            if (SAVE) acc_st<D>(mo, 0, reg, v);
        }
    }
    FS_WSYNC();
    // ---- update: acc_u[g] = [h, m] . AU[:, g] ----
    f32x16 acc_u[NG][1];
#pragma unroll
    for (int g = 0; g < NG; ++g) zero_acc(acc_u[g]);
    {
        BPre<NG> pre_m;
        tile_b_prefetch<NG>(pre_m, (const float* const (&)[NG])Bm, (const int (&)[NG])ldwg, D, rot);
        tile_mma<NG, 1, 1>(acc_u, Hw, LD, (const float* const (&)[NG])Bh, (const int (&)[NG])ldwg, D, rot, &pre_h);
        tile_mma<NG, 1, 1>(acc_u, Aw, LD, (const float* const (&)[NG])Bm, (const int (&)[NG])ldwg, D, rot, &pre_m);
    }
    const AccBuf ho = acc_buf<D>(a.hout, row0, lrow, col);
    const AccBuf ao = acc_buf<NU>(a.act_out, row0, lrow, col);
    if constexpr (KIND == GS_FUSE) {         // out = keep * (r * h) + f * z
        const float bz = a.bU[col], br = a.bU[D + col], bf = a.bU[2 * D + col];
        const bool has_keep = a.keep != nullptr;
        const AccBuf ko = acc_buf<D>(a.keep, row0, lrow, col);
        FS_FOR_ACC {
            const float z = bmp_tanh(acc_u[0][0][reg] + bz);
            const float r = bmp_sigmoid(acc_u[1][0][reg] + br);
            const float f = bmp_sigmoid(acc_u[NG - 1][0][reg] + bf);
            float rh = r * Hl[FS_LOFF(reg)];
            if (has_keep) rh *= acc_ld<D>(ko, 0, reg);
            acc_st<D>(ho, 0, reg, rh + f * z);
            if (SAVE) {
                acc_st<NU>(ao, 0, reg, z, 0);
                acc_st<NU>(ao, 0, reg, r, D);
                acc_st<NU>(ao, 0, reg, f, 2 * D);
            }
        }
    } else {                                 // out = (1 - a) * h + a * m   (m: the lane's own elements of A)
        const float bg = a.bU[col];
        FS_FOR_ACC {
            const float av = bmp_sigmoid(acc_u[0][0][reg] + bg);
            acc_st<D>(ho, 0, reg, (1.f - av) * Hl[FS_LOFF(reg)] + av * Al[FS_LOFF(reg)]);
            if (SAVE) acc_st<NU>(ao, 0, reg, av, 0);
        }
    }
}

// Backward-data of one step for one tile: dh and gda [N x (4D + Nu)] = [G_0..G_3 | dpre], the formulas of gate_step_bwd
// (bmp_gate.hip).
template <int D, int KIND, bool VAR>
__global__ __launch_bounds__(FS_NT) void k_gate_step_bwd_s(GateSmallArgs a) {
    static_assert(D == 32, "one 32-column MFMA block per row");
    constexpr int LD = D + 4, NG = KIND == GS_FUSE ? 3 : 1, NU = NG * D, LDG = 4 * D + NU;
    constexpr int F4 = D / 4;                // float4 per row
    constexpr int NV = D / 8;                // float4 slots per lane of a 32-row block (64 lanes)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Xs = lds;                         // [128 x LD]  dpre_z -> dpre_f -> dm   (fuse);  dpre -> dm   (gate)
    float* Ys = lds + FS_R * LD;             // [128 x LD]  dpre_r (fuse) / dout * a (gate) -> G_e -> dh
    int* rptr = (int*)(Ys + FS_R * LD + FS_R * 4);           // (the forward's [128 x 4] weighted degrees lie in between: one
    int* ecol = rptr + 132;                                  //  LDS layout and one gs_lds_bytes for both directions; unused here)
    float* evalv = (float*)(ecol + FZ_ECAP);

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int row0 = VAR ? a.mt_row0[blockIdx.x] : blockIdx.x * FS_R;
    const int nblk = VAR ? a.mt_nblk[blockIdx.x] : 4;
    const int nrows = VAR ? nblk * 32 : FS_R;
    if (VAR && a.tile_stride > nrows) {      // (fixed-stride tile table: the dead blocks read as zero to the weight-gradient GEMMs
        const int e = row0 + a.tile_stride;  //  and to the step below)
        fz_clear_rows<FS_NT>(a.dh, D, row0 + nrows, e, tid);
        fz_clear_rows<FS_NT>(a.gda, LDG, row0 + nrows, e, tid);
    }
    const int col = l31;
    const int wrow0 = w * 32;
    const int lrow = wrow0 + 4 * hi;
    const int grow = wrow0 + (lane >> 1), gq = lane & 1;
    const int rot = (blockIdx.x * 8) % D;
    const float* Xw = Xs + (wrow0 + l31) * LD + 4 * hi;
    const float* Yw = Ys + (wrow0 + l31) * LD + 4 * hi;
    float* Xl = Xs + lrow * LD + col;
    float* Yl = Ys + lrow * LD + col;
#define RM_ROW(v) (wrow0 + (v) * (64 / F4) + lane / F4)
#define RM_C4(v) (lane % F4)
#define RM_LDS(T, v) (*(f32x4*)((T) + RM_ROW(v) * LD + 4 * RM_C4(v)))
    const bool csr_lds = stage_csr(a.ptr, a.col, a.val, row0, rptr, ecol, evalv, nrows, FS_NT);
    if (VAR && w >= nblk) {                  // a short tile: this block has no rows; it has staged its share of the CSR, meets
        __syncthreads();                     // the kernel's barrier and leaves
        return;
    }
    const AccBuf b_g = fs_rm_buf<D, D>(a.dhout, row0, wrow0, lane), b_h = fs_rm_buf<D, D>(a.h, row0, wrow0, lane);
    const AccBuf b_a = fs_rm_buf<D, NU>(a.act, row0, wrow0, lane);
    const AccBuf b_o = fs_rm_buf<D, LDG>(a.gda, row0, wrow0, lane), b_dh = fs_rm_buf<D, D>(a.dh, row0, wrow0, lane);
    const f32x4 one = (f32x4){1.f, 1.f, 1.f, 1.f};

    const int ld2[2] = {2 * D, 2 * D};
    const float* const U0 = a.Unp + (size_t)(4 * hi) * 2 * D + 4 * col;      // gate g: + g * D * 2D; the dm half: + 4D
    const float* const B0[2] = {U0, U0 + 4 * D};
    BPre<2> pre0;
    tile_b_prefetch<2>(pre0, B0, ld2, D, rot);

    // ---- dpre_g, wave-local; ex: the direct part of dh ----
    f32x4 ex[NV];
    f32x16 acc_x[2][1];                      // [0] = dh, [1] = dm
    zero_acc(acc_x[0]); zero_acc(acc_x[1]);
    if constexpr (KIND == GS_FUSE) {
        const bool has_keep = a.keep != nullptr;
        const AccBuf b_k = fs_rm_buf<D, D>(a.keep, row0, wrow0, lane);
        f32x4 pf[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const f32x4 g4 = fs_rm_ld<D, D>(b_g, v), h4 = fs_rm_ld<D, D>(b_h, v);
            const f32x4 z4 = fs_rm_ld<D, NU>(b_a, v, 0), r4 = fs_rm_ld<D, NU>(b_a, v, D), f4 = fs_rm_ld<D, NU>(b_a, v, 2 * D);
            const f32x4 dz = g4 * f4 * (one - z4 * z4);
            f32x4 dr = g4 * h4 * r4 * (one - r4);
            const f32x4 df = g4 * z4 * f4 * (one - f4);
            f32x4 e4 = g4 * r4;
            if (has_keep) { const f32x4 k4 = fs_rm_ld<D, D>(b_k, v); dr = dr * k4; e4 = e4 * k4; }
            ex[v] = e4;
            pf[v] = df;
            RM_LDS(Xs, v) = dz;
            RM_LDS(Ys, v) = dr;
            fs_rm_st<D, LDG>(b_o, v, dz, 4 * D);
            fs_rm_st<D, LDG>(b_o, v, dr, 5 * D);
            fs_rm_st<D, LDG>(b_o, v, df, 6 * D);
        }
        FS_WSYNC();
        const float* const B1[2] = {U0 + (size_t)D * 2 * D, U0 + (size_t)D * 2 * D + 4 * D};
        const float* const B2[2] = {U0 + (size_t)2 * D * 2 * D, U0 + (size_t)2 * D * 2 * D + 4 * D};
        tile_mma<2, 1, 1>(acc_x, Xw, LD, B0, ld2, D, rot, &pre0);                // [dh | dm] += dpre_z . U_z
        tile_mma<2, 1, 1>(acc_x, Yw, LD, B1, ld2, D, rot);                       //            + dpre_r . U_r
        FS_WSYNC();                          // the wave is done with dpre_z in X
#pragma unroll
        for (int v = 0; v < NV; ++v) RM_LDS(Xs, v) = pf[v];
        FS_WSYNC();
        tile_mma<2, 1, 1>(acc_x, Xw, LD, B2, ld2, D, rot);                       //            + dpre_f . U_f
        FS_WSYNC();
        FS_FOR_ACC { Xl[FS_LOFF(reg)] = acc_x[1][0][reg]; }                      // X <- dm
    } else {
        const AccBuf b_m = fs_rm_buf<D, D>(a.m, row0, wrow0, lane);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const f32x4 g4 = fs_rm_ld<D, D>(b_g, v), h4 = fs_rm_ld<D, D>(b_h, v), m4 = fs_rm_ld<D, D>(b_m, v);
            const f32x4 a4 = fs_rm_ld<D, NU>(b_a, v, 0);
            const f32x4 dp = g4 * (m4 - h4) * a4 * (one - a4);
            ex[v] = g4 * (one - a4);
            RM_LDS(Xs, v) = dp;
            RM_LDS(Ys, v) = g4 * a4;         // dm's direct term
            fs_rm_st<D, LDG>(b_o, v, dp, 4 * D);
        }
        FS_WSYNC();
        tile_mma<2, 1, 1>(acc_x, Xw, LD, B0, ld2, D, rot, &pre0);                // [dh | dm] += dpre . U
        FS_WSYNC();
        FS_FOR_ACC { Xl[FS_LOFF(reg)] = acc_x[1][0][reg] + Yl[FS_LOFF(reg)]; }   // X <- dm
    }
    __syncthreads();                         // the only workgroup barrier: the transposed gather reads dm of every row of the
                                             // tile, through the staged CSR

    // ---- message backward: G_e = gather^T_e(dm) ; dh += G_e . W_e^T ----
    f32x16 acc_h[1][1];
    acc_h[0][0] = acc_x[0][0];
    int tmask = 0, types = 0;
    for (int e = 0; e < 4; ++e) {
        const float* const Bp[1] = {a.Wnp + (size_t)(4 * hi) * 4 * D + 4 * (e * D + col)};
        const int ldw[1] = {4 * D};
        BPre<1> pre;
        tile_b_prefetch<1>(pre, Bp, ldw, D, rot);
        (void)FS_GATHER(Xs, Ys, e);
        {   // G_e -> global for the weight-gradient GEMM (the lane's own half row, 16-byte stores)
            const float* s = Ys + grow * LD + gq * (D / 2);
            float* o = a.gda + (size_t)(row0 + grow) * LDG + e * D + gq * (D / 2);
#pragma unroll
            for (int f = 0; f < D / 8; ++f) *(f32x4*)(o + 4 * f) = *(const f32x4*)(s + 4 * f);
        }
        if (e == 0) types = fs_wave_types(tmask);
        FS_WSYNC();
        if ((types >> e) & 1) tile_mma<1, 1, 1>(acc_h, Yw, LD, Bp, ldw, D, rot, &pre);
        FS_WSYNC();
    }
    // ---- dh = (MFMA part, via Y) + ex ----
    FS_FOR_ACC { Yl[FS_LOFF(reg)] = acc_h[0][0][reg]; }
    FS_WSYNC();
#pragma unroll
    for (int v = 0; v < NV; ++v) fs_rm_st<D, D>(b_dh, v, RM_LDS(Ys, v) + ex[v]);
#undef RM_ROW
#undef RM_C4
#undef RM_LDS
}

size_t gs_lds_bytes(int D);                // bmp_gate_small.hip
extern "C" int bmp_ggnn_gate_step_small_supported(int d);

template <int KIND, bool VAR>
static void gs_launch_fwd(const GateSmallArgs& a, int n_tiles, hipStream_t st) {
    const size_t lds = gs_lds_bytes(32);     // 48 KB: under the 64 KB a launch may ask for without an attribute
    const dim3 grid(n_tiles), block(FS_NT);
    if (a.m_out) hipLaunchKernelGGL((k_gate_step_fwd_s<32, KIND, true, VAR>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((k_gate_step_fwd_s<32, KIND, false, VAR>), grid, block, lds, st, a);
}

// VAR: the launch reads the tile table (mt_row0 / mt_nblk non-null, checked by the caller); otherwise whole 128-row tiles
template <bool VAR>
static int gs_fwd(int kind, const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col, const float* csr_val,
                  const float* WTp, const float* bE, const float* AUp, const float* bU, const float* keep, float* m, float* act,
                  float* hout, const int* mt_row0, const int* mt_nblk, int tile_stride, hipStream_t st) {
    BMP_REQUIRE((kind == GS_FUSE || kind == GS_GATE) && h && n_tiles > 0 && bmp_ggnn_gate_step_small_supported(d));
    BMP_REQUIRE(csr_ptr && csr_col && csr_val && WTp && bE && AUp && bU && hout && (m == nullptr) == (act == nullptr));
    BMP_REQUIRE((((uintptr_t)h | (uintptr_t)WTp | (uintptr_t)bE | (uintptr_t)AUp | (uintptr_t)keep | (uintptr_t)m | (uintptr_t)act |
                  (uintptr_t)hout) & 15) == 0);
    GateSmallArgs a = {};
    a.ptr = csr_ptr; a.col = csr_col; a.val = csr_val;
    a.h = h; a.keep = kind == GS_FUSE ? keep : nullptr;
    a.WTp = WTp; a.bE = bE; a.AUp = AUp; a.bU = bU;
    a.m_out = m; a.act_out = act; a.hout = hout;
    a.mt_row0 = mt_row0; a.mt_nblk = mt_nblk; a.tile_stride = tile_stride;
    if (kind == GS_FUSE) gs_launch_fwd<GS_FUSE, VAR>(a, n_tiles, st);
    else gs_launch_fwd<GS_GATE, VAR>(a, n_tiles, st);
    BMP_LAUNCH_CHECK();
    return 0;
}

template <bool VAR>
static int gs_bwd(int kind, const float* dhout, const float* h, const float* m, const float* act, const float* keep, int n_tiles,
                  int d, const int* csrT_ptr, const int* csrT_col, const float* csrT_val, const float* Wnat_p, const float* Unat_p,
                  float* dh, float* gda, const int* mt_row0, const int* mt_nblk, int tile_stride, hipStream_t st) {
    BMP_REQUIRE((kind == GS_FUSE || kind == GS_GATE) && dhout && h && m && act && n_tiles > 0 && bmp_ggnn_gate_step_small_supported(d));
    BMP_REQUIRE(csrT_ptr && csrT_col && csrT_val && Wnat_p && Unat_p && dh && gda);
    BMP_REQUIRE((((uintptr_t)dhout | (uintptr_t)h | (uintptr_t)m | (uintptr_t)act | (uintptr_t)keep | (uintptr_t)Wnat_p |
                  (uintptr_t)Unat_p | (uintptr_t)dh | (uintptr_t)gda) & 15) == 0);
    GateSmallArgs a = {};
    a.ptr = csrT_ptr; a.col = csrT_col; a.val = csrT_val;
    a.h = h; a.keep = kind == GS_FUSE ? keep : nullptr;
    a.dhout = dhout; a.m = m; a.act = act; a.Wnp = Wnat_p; a.Unp = Unat_p; a.dh = dh; a.gda = gda;
    a.mt_row0 = mt_row0; a.mt_nblk = mt_nblk; a.tile_stride = tile_stride;
    const size_t lds = gs_lds_bytes(32);
    const dim3 grid(n_tiles), block(FS_NT);
    if (kind == GS_FUSE) hipLaunchKernelGGL((k_gate_step_bwd_s<32, GS_FUSE, VAR>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((k_gate_step_bwd_s<32, GS_GATE, VAR>), grid, block, lds, st, a);
    BMP_LAUNCH_CHECK();
    return 0;
}
