// Evaluation scores kept on the device: bmp_eval_append copies one batch's rows (logits, up to three more float row blocks,
// int32 labels, one loss scalar) behind the rows of the batches before it, at a cursor that lives in DEVICE memory.  Every
// address and width travels by value in the kernel arguments, so a launch captured in a HIP graph replays with the addresses
// it was recorded with and still lands behind the previous replay: the write position is the one thing it reads at run time.
//
// Form chosen: TWO kernels behind the one entry, in stream order -- k_eval_copy (any number of workgroups; each reads the
// cursor, checks the capacity and copies its share) and then k_eval_advance (one thread: the same check, then either the
// overflow word or both cursor words).  The stream runs the second after the first has finished, which is all the ordering
// "every workgroup reads the cursor before anyone advances it" needs.  The alternative, one kernel whose last-arriving
// workgroup advances (the integer ticket of bmp_mlp_sce_fwdbwd), needs a word that is zero before every launch -- which this
// entry's caller would have to own and keep per stream -- plus a device-scope fence in every workgroup; for a copy of a few
// KB to a few MB one more one-thread node in a replayed chain of ~30 is the smaller price (not measured apart), and there is
// no atomic at all.
// Plain vector stores only; the copy never writes a float through an atomic.
#include "bmp_common.h"

#define EVAL_NT 256
#define EVAL_MAX_WG 256
#define EVAL_NBLK 4

struct EvalArgs {
    const float* src[EVAL_NBLK];
    float* dst[EVAL_NBLK];
    int width[EVAL_NBLK];      // 0: block absent
    const int* lab;            // NULL: no labels
    int* lab_dst;
    int lab_width;
    const float* loss;         // NULL: no loss
    float* loss_slots;
    int B;
    const int* cursor;         // [2]: rows appended, batches appended
    int cap_rows, cap_batches;
};

__device__ __forceinline__ bool eval_fits(int rows, int batches, int B, int cap_rows, int cap_batches) {
    // (subtractions: no overflow of rows + B; a cursor outside [0, cap] is refused like a full one)
    return rows >= 0 && batches >= 0 && rows <= cap_rows - B && batches <= cap_batches - 1;
}

__global__ __launch_bounds__(EVAL_NT) void k_eval_copy(EvalArgs a) {
    const int rows = a.cursor[0], batches = a.cursor[1];
    if (!eval_fits(rows, batches, a.B, a.cap_rows, a.cap_batches)) return;        // k_eval_advance reports it
    const size_t tid = (size_t)blockIdx.x * EVAL_NT + threadIdx.x, nth = (size_t)gridDim.x * EVAL_NT;
#pragma unroll
    for (int k = 0; k < EVAL_NBLK; ++k) {
        const int w = a.width[k];
        if (w == 0) continue;
        const float* s = a.src[k];
        float* d = a.dst[k] + (size_t)rows * w;
        const size_t n = (size_t)a.B * w;
        // 16-byte copies when the block is whole float4s and both ends are aligned HERE (the destination offset moves with
        // the cursor: a width of 4 k floats keeps it aligned, any other width does not); dwords otherwise.  Per block.
        const bool vec = (w & 3) == 0 && (((uintptr_t)s | (uintptr_t)d) & 15) == 0;
        if (vec) {
            const f32x4* s4 = reinterpret_cast<const f32x4*>(s);
            f32x4* d4 = reinterpret_cast<f32x4*>(d);
            for (size_t i = tid; i < n / 4; i += nth) d4[i] = s4[i];
        } else {
            for (size_t i = tid; i < n; i += nth) d[i] = s[i];
        }
    }
    if (a.lab) {
        int* d = a.lab_dst + (size_t)rows * a.lab_width;
        const size_t n = (size_t)a.B * a.lab_width;
        for (size_t i = tid; i < n; i += nth) d[i] = a.lab[i];
    }
    if (a.loss && tid == 0) a.loss_slots[batches] = a.loss[0];
}

__global__ void k_eval_advance(int* cursor, int* overflow, int B, int cap_rows, int cap_batches) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int rows = cursor[0], batches = cursor[1];
    if (!eval_fits(rows, batches, B, cap_rows, cap_batches)) {
        *overflow = 1;
        return;
    }
    cursor[0] = rows + B;
    cursor[1] = batches + 1;
}

// src / dst / width: HOST arrays of 4 (device pointers; src[k] NULL or width[k] 0 = block k absent); block k is [B x width[k]]
// and lands at dst[k] + cursor[0] * width[k]; dst[k] holds cap_rows rows.  lab [B x lab_width] int32 -> lab_dst likewise;
// loss[0] -> loss_slots[cursor[1]] (cap_batches slots).  A batch that does not fit (cursor[0] + B > cap_rows or cursor[1] + 1 >
// cap_batches) sets overflow[0] = 1 and writes nothing else; otherwise cursor += {B, 1} after the copy.
extern "C" int bmp_eval_append(const float* const* src, const int* width, const int* lab, int lab_width, const float* loss, int B,
                               float* const* dst, int* lab_dst, float* loss_slots, int* cursor, int cap_rows, int cap_batches,
                               int* overflow, hipStream_t st) {
    BMP_REQUIRE(src && width && dst);
    BMP_REQUIRE(B > 0);
    BMP_REQUIRE(cursor && overflow);
    BMP_REQUIRE(cap_rows > 0 && cap_batches > 0);
    EvalArgs a;
    size_t total = 0;
    for (int k = 0; k < EVAL_NBLK; ++k) {
        BMP_REQUIRE(width[k] >= 0);
        const bool present = src[k] != nullptr && width[k] > 0;
        BMP_REQUIRE(!present || dst[k] != nullptr);
        a.src[k] = present ? src[k] : nullptr;
        a.dst[k] = present ? dst[k] : nullptr;
        a.width[k] = present ? width[k] : 0;
        total += present ? ((size_t)B * width[k] + 3) / 4 : 0;       // in 16-byte units (a dword block: fewer threads, longer loops)
    }
    BMP_REQUIRE(lab == nullptr || (lab_dst != nullptr && lab_width > 0));
    BMP_REQUIRE(loss == nullptr || loss_slots != nullptr);
    a.lab = lab; a.lab_dst = lab_dst; a.lab_width = lab ? lab_width : 0;
    a.loss = loss; a.loss_slots = loss_slots;
    a.B = B; a.cursor = cursor; a.cap_rows = cap_rows; a.cap_batches = cap_batches;
    if (lab) total += ((size_t)B * lab_width + 3) / 4;
    size_t wg = (total + EVAL_NT - 1) / EVAL_NT;
    wg = wg < 1 ? 1 : (wg > EVAL_MAX_WG ? EVAL_MAX_WG : wg);
    hipLaunchKernelGGL(k_eval_copy, dim3((unsigned)wg), dim3(EVAL_NT), 0, st, a);
    BMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_eval_advance, dim3(1), dim3(1), 0, st, cursor, overflow, B, cap_rows, cap_batches);
    BMP_LAUNCH_CHECK();
    return 0;
}
