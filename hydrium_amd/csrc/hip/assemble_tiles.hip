/*
 * assemble_tiles.hip — the frames of a launch group of tiles, assembled side by side on the GPU.
 *
 * Tile mode codes every tile as a frame of its own (reference libhydrium.c:147-203, encoder.c:339-398,968-1005); a tile
 * is one LF group, so hydamd_begin_batch(ctx, 1, F) codes F of them in one launch group.  What follows the entropy
 * stage used to be a host round trip per tile.  Here one launch sequence in the context's stream takes the batch's
 * results as a view (hydamd_export_batch_owned: slot records, packed LF streams, packed HF sections, all in place) and
 * writes F complete frames back to back into one output buffer, behind whatever earlier launch groups of the same
 * image wrote:
 *
 *   k_tiles_prepare  one wavefront per frame: the data-dependent fields (hydk_tiles.h: LF prefix codes, HFGlobal's
 *                    histograms, the TOC) into per-frame scratch, and the frame's size
 *   k_tiles_layout   one workgroup: prefix sums over the frames' sizes and over their extents in the packed strings;
 *                    the group starts at the running offset kept in device memory, which it advances — only when the
 *                    group is complete (no buffer of the context outgrown, no NaN) and fits the output
 *   k_tiles_copy     every output word composed from the pieces that touch it and stored once; the words the group
 *                    shares with its neighbours (first and last) are written byte by byte.  Nothing is zeroed
 *                    beforehand, nothing is ORed into memory.
 *
 * Frames of one group take the same path as all others: their single section is four bit strings at bit positions
 * that depend on the pixels (hydk_tiles.h).  The host contributes the plan (csrc/host/tiled.c), once per image shape.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "../../../include/hydrium_amd.h"
#include "hydk_tiles.h"

#define ST_OK 0
#define ST_NOMEM (-13)
#define ST_API_ERROR (-14)
#define ST_INTERNAL_ERROR (-15)

namespace {

constexpr uint32_t kBlobMagic = 0x42445948u;
constexpr uint32_t kLfCodedView = 0x101u;
constexpr int kCopyBlocks = 1024;
constexpr int kMaxPieces = HYDK_TILE_MAX_FRAMES * HYDK_TILE_PIECES;

struct TileScratch { /* device pointers */
    uint32_t *head;         /* [frames][HYDK_TILE_HEAD_WORDS] */
    uint32_t *mid;          /* [frames][HYDK_TILE_MID_WORDS] */
    uint32_t *toc;          /* [frames][HYDK_TILE_TOC_WORDS] */
    HydkTileSizes *sizes;   /* [frames] */
    HydkTilePiece *pieces;  /* [frames][HYDK_TILE_PIECES] */
    uint64_t *cursor;       /* [1] bytes of the file written by the launch groups so far */
    uint64_t *result;       /* [4] error word, first byte of this group, bytes behind it, bytes the output must hold */
};

__device__ __forceinline__ uint32_t view_check(const uint8_t *blob, uint32_t frames) {
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    if (h->magic != kBlobMagic || h->version != 1 || h->num_slots != frames || h->lf_coded != kLfCodedView ||
        !(h->reserved[1] | h->reserved[2]) || !(h->reserved[3] | h->reserved[4]) || (h->reserved[1] & 3u))
        return HYDK_ASM_E_BLOB;
    uint32_t e = 0;
    if (h->status & HYDAMD_BLOB_RETRY)
        e |= HYDK_ASM_E_RETRY;
    if (h->status & 1u)
        e |= HYDK_ASM_E_NAN;
    return e;
}
__device__ __forceinline__ const uint8_t *view_lf(const uint8_t *blob) {
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    return (const uint8_t *)(((uint64_t)h->reserved[2] << 32) | h->reserved[1]);
}
__device__ __forceinline__ const uint8_t *view_hf(const uint8_t *blob) {
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    return (const uint8_t *)(((uint64_t)h->reserved[4] << 32) | h->reserved[3]);
}

/* block-wide exclusive prefix sum over 256 threads; returns the thread's offset, *total the sum */
__device__ __forceinline__ uint64_t scan256(uint64_t v, uint64_t *s_wave /* [4] */, uint64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d);
        if (lane >= d)
            inc += t;
    }
    __syncthreads();
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

/* ---- a batch's results, frame by frame: grid 1, block 256 ---- */
__global__ __launch_bounds__(256) void k_batch_extents(const uint8_t *__restrict__ blob, uint32_t frames, HydkTileExtent *__restrict__ ext) {
    __shared__ uint64_t s_wave[4];
    const uint32_t t = threadIdx.x;
    const HydAmdBlobSlot *rec = (const HydAmdBlobSlot *)(blob + sizeof(HydAmdBlobHeader)) + t;
    uint64_t hf = 0, lf_off = 0, lf_bytes = 0;
    if (t < frames) {
        for (int g = 0; g < HYDAMD_GROUPS_PER_LFG; g++)
            hf += ((uint64_t)rec->group_bits[g] + 7) >> 3;
        lf_off = rec->lf.offset;
        lf_bytes = ((uint64_t)rec->lf.bit_count + 7) >> 3;
    }
    uint64_t total = 0;
    const uint64_t off = scan256(hf, s_wave, &total);
    if (t < frames) {
        const HydkTileExtent e = {lf_off, lf_bytes, off, hf};
        ext[t] = e;
    }
}

/* ---- k_tiles_prepare: grid = frames, block = 64 (one wavefront) ---- */
__global__ __launch_bounds__(64) void k_tiles_prepare(const uint8_t *__restrict__ planb, uint32_t first_frame, const uint8_t *__restrict__ blob,
                                                      uint32_t frames, TileScratch S) {
    __shared__ uint32_t s_head[HYDK_TILE_HEAD_WORDS];
    __shared__ uint32_t s_mid[HYDK_TILE_MID_WORDS];
    __shared__ uint32_t s_toc[HYDK_TILE_TOC_WORDS];
    __shared__ uint8_t s_len[HYDK_LF_CODES];
    __shared__ HydkTileScratch s_scratch;
    __shared__ HydkTileSizes s_sizes;
    const int t = threadIdx.x;
    const uint32_t f = blockIdx.x;
    if (view_check(blob, frames)) { /* the layout kernel reports it */
        if (t == 0) {
            HydkTileSizes z = {};
            S.sizes[f] = z;
        }
        return;
    }
    const HydkTilePlan *plan = (const HydkTilePlan *)planb;
    const HydkTileFrame fr = ((const HydkTileFrame *)(planb + plan->frames_off))[first_frame + f];
    const HydkTileShape *sh = &plan->shapes[fr.shape];
    const HydAmdBlobSlot *rec = (const HydAmdBlobSlot *)(blob + sizeof(HydAmdBlobHeader)) + f;
    for (int i = t; i < HYDK_TILE_HEAD_WORDS; i += 64)
        s_head[i] = 0;
    for (int i = t; i < HYDK_TILE_MID_WORDS; i += 64)
        s_mid[i] = 0;
    for (int i = t; i < HYDK_TILE_TOC_WORDS; i += 64)
        s_toc[i] = 0;
    for (int i = t; i < HYDK_LF_CODES; i += 64)
        s_len[i] = rec->lf.lengths[i];
    __syncthreads();
    hydk_tile_prepare(planb, &fr, sh, rec, s_len, ((const HydAmdBlobHeader *)blob)->lf_bytes, s_head, s_mid, s_toc, &s_scratch, &s_sizes);
    __syncthreads();
    const HydkTileSizes z = s_sizes;
    uint32_t *head = S.head + (size_t)f * HYDK_TILE_HEAD_WORDS, *mid = S.mid + (size_t)f * HYDK_TILE_MID_WORDS,
             *toc = S.toc + (size_t)f * HYDK_TILE_TOC_WORDS;
    for (uint32_t i = t; i < (z.head_bits + 31u) >> 5; i += 64)
        head[i] = s_head[i];
    for (uint32_t i = t; i < (z.mid_bits + 31u) >> 5; i += 64)
        mid[i] = s_mid[i];
    for (uint32_t i = t; i < (z.toc_bits + 31u) >> 5; i += 64)
        toc[i] = s_toc[i];
    if (t == 0)
        S.sizes[f] = z;
}

/* ---- k_tiles_layout: grid 1, block 256 ---- */
__global__ __launch_bounds__(256) void k_tiles_layout(const uint8_t *__restrict__ planb, uint32_t first_frame, const uint8_t *__restrict__ blob,
                                                      uint32_t frames, const HydkTileExtent *__restrict__ ext, TileScratch S, int first_group,
                                                      uint64_t out_cap, uint64_t *h_result /* pinned [4] */) {
    __shared__ uint64_t s_wave[4];
    const uint32_t t = threadIdx.x;
    const uint64_t start = first_group ? 0 : *S.cursor;
    uint32_t e = view_check(blob, frames);
    const HydkTilePlan *plan = (const HydkTilePlan *)planb;
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    HydkTileSizes z = {};
    if (!e && t < frames) {
        z = S.sizes[t];
        e = z.err;
        if (!e && (ext[t].hf_bytes != z.hf_bytes || ext[t].hf_off + z.hf_bytes > h->hf_bytes))
            e = HYDK_ASM_E_SIZE;
    }
    /* every thread needs the union of the error words */
    __shared__ uint32_t s_err;
    if (t == 0)
        s_err = 0;
    __syncthreads();
    if (e)
        atomicOr(&s_err, e);
    __syncthreads();
    const uint32_t err = s_err;
    uint64_t total = 0;
    const uint64_t at = scan256(err ? 0 : z.frame_bytes, s_wave, &total);
    uint32_t fin = err;
    if (!fin && start + total > out_cap)
        fin = HYDK_ASM_E_SPACE;
    if (!fin && t < frames) {
        const HydkTileFrame fr = ((const HydkTileFrame *)(planb + plan->frames_off))[first_frame + t];
        const HydAmdBlobSlot *rec = (const HydAmdBlobSlot *)(blob + sizeof(HydAmdBlobHeader)) + t;
        hydk_tile_pieces(planb, &fr, &plan->shapes[fr.shape], &z, rec, S.head + (size_t)t * HYDK_TILE_HEAD_WORDS,
                         S.mid + (size_t)t * HYDK_TILE_MID_WORDS, S.toc + (size_t)t * HYDK_TILE_TOC_WORDS, view_lf(blob) + ext[t].lf_off,
                         view_hf(blob) + ext[t].hf_off, start + at, S.pieces + (size_t)t * HYDK_TILE_PIECES);
    }
    if (t == 0) {
        S.result[0] = fin;
        S.result[1] = start;
        S.result[2] = fin ? 0 : total;
        S.result[3] = start + total;
        if (!fin)
            *S.cursor = start + total;
        for (int i = 0; i < 4; i++)
            h_result[i] = S.result[i];
    }
}

/* ---- k_tiles_copy ---- */
__global__ __launch_bounds__(256) void k_tiles_copy(TileScratch S, uint32_t frames, uint8_t *__restrict__ out) {
    __shared__ uint64_t s_end[kMaxPieces];
    if (S.result[0] || !S.result[2])
        return;
    const uint64_t b_lo = S.result[1], b_hi = b_lo + S.result[2]; /* bytes [b_lo, b_hi) are this group's */
    const uint32_t np = frames * HYDK_TILE_PIECES;
    for (uint32_t i = threadIdx.x; i < np; i += 256)
        s_end[i] = S.pieces[i].dst_bit + S.pieces[i].nbits;
    __syncthreads();
    uint32_t *out32 = (uint32_t *)out;
    const uint64_t w_lo = b_lo >> 2, w_hi = (b_hi + 3) >> 2;
    for (uint64_t W = w_lo + (uint64_t)blockIdx.x * 256u + threadIdx.x; W < w_hi; W += (uint64_t)gridDim.x * 256u) {
        const uint32_t v = hydk_tile_word(S.pieces, s_end, np, W);
        const uint64_t b0 = W * 4u;
        if (b0 >= b_lo && b0 + 4 <= b_hi) {
            out32[W] = v;
            continue;
        }
        for (uint32_t j = 0; j < 4; j++) /* a word shared with the launch group in front, or the file's last */
            if (b0 + j >= b_lo && b0 + j < b_hi)
                out[b0 + j] = (uint8_t)(v >> (8u * j));
    }
}

} // namespace

namespace hydk {
hipError_t launch_batch_extents(const void *blob, int frames, void *extents, hipStream_t stream) {
    hipLaunchKernelGGL(k_batch_extents, dim3(1), dim3(256), 0, stream, (const uint8_t *)blob, (uint32_t)frames, (HydkTileExtent *)extents);
    return hipGetLastError();
}
} // namespace hydk

struct HydkTileAsm {
    int device = 0;
    char error[256] = "";
    uint8_t *plan = nullptr;
    uint32_t plan_frames = 0;
    TileScratch S = {};
    uint64_t *h_result = nullptr; /* pinned [4] */
    uint8_t *out = nullptr;       /* the file: owned, grown on demand (hydk_tiles_reserve) */
    uint64_t out_cap = 0;
};

namespace {
int tfail(HydkTileAsm *a, int code, const char *what, hipError_t e = hipSuccess) {
    if (a) {
        if (e != hipSuccess)
            snprintf(a->error, sizeof(a->error), "%s: %s", what, hipGetErrorString(e));
        else
            snprintf(a->error, sizeof(a->error), "%s", what);
    }
    return code;
}
#define TILE_TRY(a, call)                                                                             \
    do {                                                                                              \
        hipError_t e__ = (call);                                                                      \
        if (e__ != hipSuccess)                                                                        \
            return tfail(a, e__ == hipErrorOutOfMemory ? ST_NOMEM : ST_INTERNAL_ERROR, #call, e__);   \
    } while (0)
} // namespace

extern "C" {

const char *hydk_tiles_error(HydkTileAsm *a) { return a ? a->error : "null tile assembler"; }

void hydk_tiles_destroy(HydkTileAsm *a) {
    if (!a)
        return;
    (void)hipSetDevice(a->device);
    void *dev[] = {a->out, a->plan, a->S.head, a->S.mid, a->S.toc, a->S.sizes, a->S.pieces, a->S.cursor, a->S.result};
    for (void *p : dev)
        if (p)
            (void)hipFree(p);
    if (a->h_result)
        (void)hipHostFree(a->h_result);
    delete a;
}

/* scratch for launch groups of up to `max_frames` frames; the plan (hydk_tiles.h) is copied to the device */
int hydk_tiles_create(int device, int max_frames, const void *plan, size_t plan_bytes, HydkTileAsm **out) {
    if (!out)
        return ST_API_ERROR;
    *out = nullptr;
    const HydkTilePlan *hp = (const HydkTilePlan *)plan;
    if (max_frames < 1 || max_frames > HYDK_TILE_MAX_FRAMES || !plan || plan_bytes < sizeof(HydkTilePlan) || hp->magic != HYDK_TILE_MAGIC ||
        hp->total_bytes != plan_bytes || hp->nshapes > HYDK_TILE_MAX_SHAPES)
        return ST_API_ERROR;
    HydkTileAsm *a = new (std::nothrow) HydkTileAsm();
    if (!a)
        return ST_NOMEM;
    a->device = device;
    a->plan_frames = hp->num_frames;
    const size_t n = (size_t)max_frames;
    auto alloc = [&]() -> int {
        TILE_TRY(a, hipSetDevice(device));
        TILE_TRY(a, hipMalloc(&a->plan, plan_bytes + 16)); /* + 16: the copy kernel reads whole words */
        TILE_TRY(a, hipMemcpy(a->plan, plan, plan_bytes, hipMemcpyHostToDevice));
        TILE_TRY(a, hipMalloc(&a->S.head, n * HYDK_TILE_HEAD_WORDS * sizeof(uint32_t)));
        TILE_TRY(a, hipMalloc(&a->S.mid, n * HYDK_TILE_MID_WORDS * sizeof(uint32_t)));
        TILE_TRY(a, hipMalloc(&a->S.toc, n * HYDK_TILE_TOC_WORDS * sizeof(uint32_t)));
        TILE_TRY(a, hipMalloc(&a->S.sizes, n * sizeof(HydkTileSizes)));
        TILE_TRY(a, hipMalloc(&a->S.pieces, n * HYDK_TILE_PIECES * sizeof(HydkTilePiece)));
        TILE_TRY(a, hipMalloc(&a->S.cursor, sizeof(uint64_t)));
        TILE_TRY(a, hipMalloc(&a->S.result, 4 * sizeof(uint64_t)));
        TILE_TRY(a, hipMemset(a->S.cursor, 0, sizeof(uint64_t)));
        TILE_TRY(a, hipStreamSynchronize(nullptr)); /* the memset runs in the NULL stream, which the context's stream does not wait for */
        TILE_TRY(a, hipHostMalloc((void **)&a->h_result, 4 * sizeof(uint64_t), hipHostMallocDefault));
        memset(a->h_result, 0, 4 * sizeof(uint64_t));
        return ST_OK;
    };
    const int st = alloc();
    if (st != ST_OK) {
        hydk_tiles_destroy(a);
        return st;
    }
    *out = a;
    return ST_OK;
}

/* enqueue the assembly of frames [first_frame, first_frame + frames) of the plan on `stream`, behind whatever fills the
 * view `blob` (hydamd_export_batch_owned) and its extents; first_group: the file starts here (running offset 0) */
int hydk_tiles_run(HydkTileAsm *a, uint32_t first_frame, uint32_t frames, const void *blob, const void *extents, int first_group, void *stream) {
    void *out = a ? a->out : nullptr;
    const uint64_t out_cap = a ? a->out_cap : 0;
    if (!a || !blob || !extents || !out || frames < 1 || frames > HYDK_TILE_MAX_FRAMES || (uint64_t)first_frame + frames > a->plan_frames)
        return tfail(a, ST_API_ERROR, "bad launch group");
    if (((uintptr_t)out & 3u) || ((uintptr_t)blob & 15u))
        return tfail(a, ST_API_ERROR, "output buffer must be 4-byte aligned, the view 16-byte aligned");
    TILE_TRY(a, hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tiles_prepare, dim3(frames), dim3(64), 0, st, (const uint8_t *)a->plan, first_frame, (const uint8_t *)blob, frames, a->S);
    hipLaunchKernelGGL(k_tiles_layout, dim3(1), dim3(256), 0, st, (const uint8_t *)a->plan, first_frame, (const uint8_t *)blob, frames,
                       (const HydkTileExtent *)extents, a->S, first_group, out_cap, a->h_result);
    hipLaunchKernelGGL(k_tiles_copy, dim3(kCopyBlocks), dim3(256), 0, st, a->S, frames, (uint8_t *)out);
    TILE_TRY(a, hipGetLastError());
    return ST_OK;
}

/* the output buffer holds at least `bytes`; its first `keep` bytes survive a move.  Waits for `stream` when it has to move. */
int hydk_tiles_reserve(HydkTileAsm *a, uint64_t bytes, uint64_t keep, void *stream) {
    if (!a)
        return ST_API_ERROR;
    if (bytes <= a->out_cap)
        return ST_OK;
    TILE_TRY(a, hipSetDevice(a->device));
    TILE_TRY(a, hipStreamSynchronize((hipStream_t)stream));
    uint8_t *bigger = nullptr;
    TILE_TRY(a, hipMalloc(&bigger, bytes + 16));
    if (a->out && keep) {
        const hipError_t e = hipMemcpy(bigger, a->out, keep < a->out_cap ? keep : a->out_cap, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            (void)hipFree(bigger);
            return tfail(a, ST_INTERNAL_ERROR, "moving the output buffer", e);
        }
    }
    if (a->out)
        (void)hipFree(a->out);
    a->out = bigger;
    a->out_cap = bytes;
    return ST_OK;
}

const uint8_t *hydk_tiles_out(HydkTileAsm *a) { return a ? a->out : nullptr; }
uint64_t hydk_tiles_out_capacity(HydkTileAsm *a) { return a ? a->out_cap : 0; }

int hydk_tiles_wait(HydkTileAsm *a, void *stream) {
    if (!a)
        return ST_API_ERROR;
    TILE_TRY(a, hipSetDevice(a->device));
    TILE_TRY(a, hipStreamSynchronize((hipStream_t)stream));
    return ST_OK;
}

int hydk_tiles_read(HydkTileAsm *a, uint8_t *dst, size_t n) {
    if (!a || !dst || !a->out || n > a->out_cap)
        return tfail(a, ST_API_ERROR, "nothing to read");
    TILE_TRY(a, hipSetDevice(a->device));
    TILE_TRY(a, hipMemcpy(dst, a->out, n, hipMemcpyDeviceToHost));
    return ST_OK;
}

/* free device memory right now (what an object holds = the difference around its creation) */
uint64_t hydk_tiles_device_free(int device) {
    size_t fr = 0, total = 0;
    if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&fr, &total) != hipSuccess)
        return 0;
    return fr;
}

/* after the stream has been synchronised: the device's error word (HYDK_ASM_E_*), the bytes of the file behind this
 * group, and the bytes the output buffer must hold for it */
int hydk_tiles_result(HydkTileAsm *a, uint32_t *err, uint64_t *file_bytes, uint64_t *needed) {
    if (!a)
        return ST_API_ERROR;
    if (err)
        *err = (uint32_t)a->h_result[0];
    if (file_bytes)
        *file_bytes = a->h_result[0] ? a->h_result[1] : a->h_result[1] + a->h_result[2];
    if (needed)
        *needed = a->h_result[3];
    return ST_OK;
}

} /* extern "C" */
