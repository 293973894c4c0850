/*
 * hydk_asm_common.h — what the two device-side assemblers (assemble.hip, assemble_tiles.hip) ask of a blob and of the
 * HIP runtime in the same words.  The slot-record check also runs on the host (hydk_tiles.h under HYD_TEST_HOOKS); the
 * rest is for the two .hip files only.  Include hydrium_amd.h first (HydAmdBlobHeader, HydAmdBlobSlot).
 */
#ifndef HYD_ASM_COMMON_H_
#define HYD_ASM_COMMON_H_

#include "hydk_assemble.h"
#include "hydk_pieces.h"

/* a slot record an assembler can follow?  `preset`: what the plan expects, `lf_capacity`: bytes of the packed LF streams */
HYDK_HD uint32_t hydk_slot_check(const HydAmdBlobSlot *rec, uint32_t preset, uint64_t lf_capacity) {
    const uint64_t lf_end = (uint64_t)rec->lf.offset + (((uint64_t)rec->lf.bit_count + 7) >> 3);
    if (rec->preset != preset || rec->table_error || rec->lf.error || lf_end > lf_capacity || (rec->lf.offset & 3u) || rec->lf.alphabet < 1 ||
        rec->lf.alphabet > HYDK_LF_RUN_BASE + 128u)
        return HYDK_ASM_E_SLOT;
    return 0;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <stdio.h>

#define ST_OK 0
#define ST_NOMEM (-13)
#define ST_API_ERROR (-14)
#define ST_INTERNAL_ERROR (-15)

/* ends one launch of k_pieces_copy keeps in LDS (16 KB): assemble_tiles.hip's list is the longer one */
#define HYDK_COPY_MAX_PIECES 2040

namespace hydk {
/* assemble.hip: bytes [range[1], range[1] + range[2]) of `out` (4-byte aligned) from the sorted pieces P, unless the error
 * word range[0] is set or the range is empty; `range` and, when given, the piece count `np_dev` are read on the device */
hipError_t launch_pieces_copy(const HydkPiece *P, uint32_t np, const uint32_t *np_dev, const uint64_t *range, void *out, hipStream_t stream);
} // namespace hydk

constexpr uint32_t kBlobMagic = 0x42445948u;
/* a blob whose two byte strings stay where the context keeps them (hydamd_export_frame_owned, hydamd_export_batch_owned):
 * header.lf_coded carries this mark and header.reserved[1..4] the device addresses of the packed LF streams and HF sections */
constexpr uint32_t kLfCodedView = 0x101u;

static __device__ __forceinline__ const uint8_t *blob_lf_bytes(const uint8_t *blob) {
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    if (h->lf_coded == kLfCodedView)
        return (const uint8_t *)(((uint64_t)h->reserved[2] << 32) | h->reserved[1]);
    return blob + sizeof(HydAmdBlobHeader) + (uint64_t)h->num_slots * sizeof(HydAmdBlobSlot);
}
static __device__ __forceinline__ const uint8_t *blob_hf_bytes(const uint8_t *blob) {
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    if (h->lf_coded == kLfCodedView)
        return (const uint8_t *)(((uint64_t)h->reserved[4] << 32) | h->reserved[3]);
    return blob + (h->total_bytes - h->hf_bytes);
}
/* whose header, and is the blob complete?  (0, or HYDK_ASM_E_* bits; where its byte strings lie is each assembler's to check) */
static __device__ __forceinline__ uint32_t blob_ident(const HydAmdBlobHeader *h, uint32_t want_slots) {
    if (h->magic != kBlobMagic || h->version != 1 || h->num_slots != want_slots)
        return HYDK_ASM_E_BLOB;
    return ((h->status & HYDAMD_BLOB_RETRY) ? HYDK_ASM_E_RETRY : 0u) | ((h->status & 1u) ? HYDK_ASM_E_NAN : 0u);
}

/* a batch view of `slots` slot records (hydamd_export_batch_owned), for the assemblers that follow views only */
static __device__ __forceinline__ uint32_t blob_view_check(const uint8_t *blob, uint32_t slots) {
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    if (h->lf_coded != kLfCodedView || !(h->reserved[1] | h->reserved[2]) || !(h->reserved[3] | h->reserved[4]) || (h->reserved[1] & 3u))
        return HYDK_ASM_E_BLOB;
    return blob_ident(h, slots);
}

/* block-wide exclusive prefix sum over 256 threads; returns the thread's offset, *total the sum */
static __device__ __forceinline__ uint64_t scan256(uint64_t v, uint64_t *s_wave /* [4] */, uint64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d);
        if (lane >= d)
            inc += t;
    }
    __syncthreads(); /* s_wave may still be read from an earlier call */
    if (lane == 63)
        s_wave[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int w = 0; w < 4; w++) {
        before += w < wave ? s_wave[w] : 0;
        all += s_wave[w];
    }
    *total = all;
    return before + inc - v;
}

/* `a`: an assembler object with a `char error[256]`, or null */
template <class A> static int hydk_fail(A *a, int code, const char *what, hipError_t e = hipSuccess) {
    if (a) {
        if (e != hipSuccess)
            snprintf(a->error, sizeof(a->error), "%s: %s", what, hipGetErrorString(e));
        else
            snprintf(a->error, sizeof(a->error), "%s", what);
    }
    return code;
}
#define HYDK_TRY(a, call)                                                                                 \
    do {                                                                                                  \
        hipError_t e__ = (call);                                                                          \
        if (e__ != hipSuccess)                                                                            \
            return hydk_fail(a, e__ == hipErrorOutOfMemory ? ST_NOMEM : ST_INTERNAL_ERROR, #call, e__);   \
    } while (0)
#endif /* __HIPCC__ */

#endif /* HYD_ASM_COMMON_H_ */
