// Wave-local tile machinery of the d = 32 step kernels (bmp_fused_small.hip, bmp_gate_small.hip): one workgroup of 256 threads
// (4 waves) per 128-row tile, wave w owns the 32-row block w in every phase; the typed gather of a wave's rows, the wave's
// bond-type mask, the wave-local LDS fence and the row-major 16-byte access to a wave's rows.
#pragma once
#include "bmp_tile.h"

#define FS_R 128
#define FS_NT 256
#define FS_LOFF(reg) ((((reg) & 3) + 8 * ((reg) >> 2)) * LD)
#define FS_FOR_ACC _Pragma("unroll") for (int reg = 0; reg < 16; ++reg)
// wave-local ordering of LDS traffic (write by some lanes, read by others of the SAME wave)
#define FS_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// This wave's 32 rows of a per-bond-type neighbour gather: dst[row, :] = sum over the CSR entries of `row` with type e of
// val * src[col_local, :].  Two lanes per row, D / 2 columns each.  Returns the row's weighted degree for that type.
template <int D>
__device__ __forceinline__ float fs_gather(const float* src, float* dst, int LD, const int* ptr, const int* col, const float* val,
                                           int row0, int row, int q, int e, int* tmask) {
    constexpr int F = D / 8;                  // float4 per lane
    f32x4 acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float wd = 0.f;
    const int e0 = ptr[row], e1 = ptr[row + 1];
    for (int ed = e0; ed < e1; ++ed) {
        const int cv = col[ed];
        *tmask |= 1 << (cv & 3);
        if ((cv & 3) == e) {
            const float v = val[ed];
            const float* s = src + ((cv >> 2) - row0) * LD + q * (D / 2);
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] += *(const f32x4*)(s + 4 * f) * v;
            wd += v;
        }
    }
    float* o = dst + row * LD + q * (D / 2);
#pragma unroll
    for (int f = 0; f < F; ++f) *(f32x4*)(o + 4 * f) = acc[f];
    return wd;
}

// fs_gather through the tile's staged CSR when it fits in LDS (stage_csr), from global memory otherwise: the kernel's names
// (csr_lds, rptr, ecol, evalv, row0, grow, gq, tmask, LD, D and the argument block a with ptr / col / val)
#define FS_GATHER(srcT, dstT, e) (csr_lds ? fs_gather<D>(srcT, dstT, LD, rptr, ecol, evalv, row0, grow, gq, e, &tmask) \
                                          : fs_gather<D>(srcT, dstT, LD, a.ptr + row0, a.col, a.val, row0, grow, gq, e, &tmask))

// bond types present among this wave's rows (bit e), from the lanes' masks after a pass that walked every entry
__device__ __forceinline__ int fs_wave_types(int tmask) {
    int m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) m |= (__ballot((tmask >> e) & 1) != 0ull) ? (1 << e) : 0;
    return m;
}

// Row-major 16-byte access to this wave's 32 rows: slot v of a lane = float4 (row v * (256 / D) + lane / (D / 4), column
// lane % (D / 4)); all slots of an array share one voffset (AccBuf, bmp_tile.h).
template <int D, int LDP>
__device__ __forceinline__ AccBuf fs_rm_buf(const float* base, int tile_row0, int wrow0, int lane) {
    AccBuf b;
    b.rs = __builtin_amdgcn_make_buffer_rsrc((void*)(base + (size_t)tile_row0 * LDP), 0, 0x7FFFFFFF, 0x00020000);
    b.vo = ((wrow0 + lane / (D / 4)) * LDP + 4 * (lane % (D / 4))) * 4;
    return b;
}
template <int D, int LDP>
__device__ __forceinline__ f32x4 fs_rm_ld(const AccBuf& b, int v, int coff = 0) {
    const int so = (v * (256 / D) * LDP + coff) * 4;
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b.rs, b.vo, so, 0));
}
template <int D, int LDP>
__device__ __forceinline__ void fs_rm_st(const AccBuf& b, int v, f32x4 x, int coff = 0) {
    const int so = (v * (256 / D) * LDP + coff) * 4;          // in the voffset: see rm_st (bmp_tile.h) for the store hazard
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, x), b.rs, b.vo + so, 0, 0);
}
