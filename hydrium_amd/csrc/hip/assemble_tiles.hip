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
 *   k_pieces_copy    (assemble.hip, shared with the frame assembler) every output word composed from the pieces
 *                    that touch it (hydk_pieces.h) and stored once; the words the group shares with its neighbours
 *                    (first and last) are written byte by byte.  Nothing is zeroed beforehand, nothing is ORed into
 *                    memory.
 *
 * Frames of one group take the same path as all others: their single section is four bit strings at bit positions
 * that depend on the pixels (hydk_tiles.h).  The host contributes the plan (csrc/host/tiled.c), once per image shape.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <new>

#include "../../../include/hydrium_amd.h"
#include "hydk_tile_asm.h"
#include "hydk_tiles.h"

namespace {

static_assert(HYDK_TILE_MAX_FRAMES * HYDK_TILE_PIECES <= HYDK_COPY_MAX_PIECES, "k_pieces_copy keeps every end in LDS");

struct TileScratch { /* device pointers */
    uint32_t *head;         /* [frames][HYDK_TILE_HEAD_WORDS] */
    uint32_t *mid;          /* [frames][HYDK_TILE_MID_WORDS] */
    uint32_t *toc;          /* [frames][HYDK_TILE_TOC_WORDS] */
    HydkTileSizes *sizes;   /* [frames] */
    HydkPiece *pieces;  /* [frames][HYDK_TILE_PIECES] */
    uint64_t *cursor;       /* [1] bytes of the file written by the launch groups so far */
    uint64_t *result;       /* [4] error word, first byte of this group, bytes behind it (what k_pieces_copy reads), bytes the output must hold */
};

/* ---- a batch's results, slot by slot (a tile frame is one slot; `frames` = slots of the view): grid 1, block 256 ---- */
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
    const uint32_t f = blockIdx.x;
    if (blob_view_check(blob, frames)) { /* the layout kernel reports it */
        if (threadIdx.x == 0) {
            HydkTileSizes z = {};
            S.sizes[f] = z;
        }
        return;
    }
    const HydkTilePlan *plan = (const HydkTilePlan *)planb;
    const HydkTileFrame fr = ((const HydkTileFrame *)(planb + plan->frames_off))[first_frame + f];
    const HydAmdBlobSlot *rec = (const HydAmdBlobSlot *)(blob + sizeof(HydAmdBlobHeader)) + f;
    const HydkTileSizes z = hydk_tile_prepare_wave(planb, &fr, &plan->shapes[fr.shape], rec, ((const HydAmdBlobHeader *)blob)->lf_bytes,
                                                   S.head + (size_t)f * HYDK_TILE_HEAD_WORDS, S.mid + (size_t)f * HYDK_TILE_MID_WORDS,
                                                   S.toc + (size_t)f * HYDK_TILE_TOC_WORDS);
    if (threadIdx.x == 0)
        S.sizes[f] = z;
}

/* ---- k_tiles_layout: grid 1, block 256 ---- */
__global__ __launch_bounds__(256) void k_tiles_layout(const uint8_t *__restrict__ planb, uint32_t first_frame, const uint8_t *__restrict__ blob,
                                                      uint32_t frames, const HydkTileExtent *__restrict__ ext, TileScratch S, int first_group,
                                                      uint64_t out_cap, uint64_t *h_result /* pinned [4] */) {
    __shared__ uint64_t s_wave[4];
    const uint32_t t = threadIdx.x;
    const uint64_t start = first_group ? 0 : *S.cursor;
    uint32_t e = blob_view_check(blob, frames);
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
                         S.mid + (size_t)t * HYDK_TILE_MID_WORDS, S.toc + (size_t)t * HYDK_TILE_TOC_WORDS, blob_lf_bytes(blob) + ext[t].lf_off,
                         blob_hf_bytes(blob) + ext[t].hf_off, start + at, S.pieces + (size_t)t * HYDK_TILE_PIECES);
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
        HYDK_TRY(a, hipSetDevice(device));
        HYDK_TRY(a, hipMalloc(&a->plan, plan_bytes + 16)); /* + 16: the copy kernel reads whole words */
        HYDK_TRY(a, hipMemcpy(a->plan, plan, plan_bytes, hipMemcpyHostToDevice));
        HYDK_TRY(a, hipMalloc(&a->S.head, n * HYDK_TILE_HEAD_WORDS * sizeof(uint32_t)));
        HYDK_TRY(a, hipMalloc(&a->S.mid, n * HYDK_TILE_MID_WORDS * sizeof(uint32_t)));
        HYDK_TRY(a, hipMalloc(&a->S.toc, n * HYDK_TILE_TOC_WORDS * sizeof(uint32_t)));
        HYDK_TRY(a, hipMalloc(&a->S.sizes, n * sizeof(HydkTileSizes)));
        HYDK_TRY(a, hipMalloc(&a->S.pieces, n * HYDK_TILE_PIECES * sizeof(HydkPiece)));
        HYDK_TRY(a, hipMalloc(&a->S.cursor, sizeof(uint64_t)));
        HYDK_TRY(a, hipMalloc(&a->S.result, 4 * sizeof(uint64_t)));
        HYDK_TRY(a, hipMemset(a->S.cursor, 0, sizeof(uint64_t)));
        HYDK_TRY(a, hipStreamSynchronize(nullptr)); /* the memset runs in the NULL stream, which the context's stream does not wait for */
        HYDK_TRY(a, hipHostMalloc((void **)&a->h_result, 4 * sizeof(uint64_t), hipHostMallocDefault));
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
        return hydk_fail(a, ST_API_ERROR, "bad launch group");
    if (((uintptr_t)out & 3u) || ((uintptr_t)blob & 15u))
        return hydk_fail(a, ST_API_ERROR, "output buffer must be 4-byte aligned, the view 16-byte aligned");
    HYDK_TRY(a, hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tiles_prepare, dim3(frames), dim3(64), 0, st, (const uint8_t *)a->plan, first_frame, (const uint8_t *)blob, frames, a->S);
    HYDK_TRY(a, hipGetLastError());
    hipLaunchKernelGGL(k_tiles_layout, dim3(1), dim3(256), 0, st, (const uint8_t *)a->plan, first_frame, (const uint8_t *)blob, frames,
                       (const HydkTileExtent *)extents, a->S, first_group, out_cap, a->h_result);
    HYDK_TRY(a, hipGetLastError());
    HYDK_TRY(a, hydk::launch_pieces_copy(a->S.pieces, frames * HYDK_TILE_PIECES, nullptr, a->S.result, out, st));
    return ST_OK;
}

/* the output buffer holds at least `bytes`; its first `keep` bytes survive a move.  Waits for `stream` when it has to move. */
int hydk_tiles_reserve(HydkTileAsm *a, uint64_t bytes, uint64_t keep, void *stream) {
    if (!a)
        return ST_API_ERROR;
    if (bytes <= a->out_cap)
        return ST_OK;
    HYDK_TRY(a, hipSetDevice(a->device));
    HYDK_TRY(a, hipStreamSynchronize((hipStream_t)stream));
    uint8_t *bigger = nullptr;
    HYDK_TRY(a, hipMalloc(&bigger, bytes + 16));
    if (a->out && keep) {
        const hipError_t e = hipMemcpy(bigger, a->out, keep < a->out_cap ? keep : a->out_cap, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            (void)hipFree(bigger);
            return hydk_fail(a, ST_INTERNAL_ERROR, "moving the output buffer", e);
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
    HYDK_TRY(a, hipSetDevice(a->device));
    HYDK_TRY(a, hipStreamSynchronize((hipStream_t)stream));
    return ST_OK;
}

int hydk_tiles_read(HydkTileAsm *a, uint8_t *dst, size_t n) {
    if (!a || !dst || !a->out || n > a->out_cap)
        return hydk_fail(a, ST_API_ERROR, "nothing to read");
    HYDK_TRY(a, hipSetDevice(a->device));
    HYDK_TRY(a, hipMemcpy(dst, a->out, n, hipMemcpyDeviceToHost));
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
