/*
 * assemble.hip — a frame put together where its sections are: on the GPU.
 *
 * What it replaces (file:line relative to /root/reference/src/libhydrium/): the closing part of
 * hyd_encode_xyb_buffer — LF group sections around their coefficient streams (encoder.c:539-629 with the
 * stream header of entropy.c:835-927), HFGlobal's histograms (encoder.c:959-967, entropy.c:303-369), the TOC
 * (encoder.c:992-1005) and the concatenation of all sections behind the frame header (encoder.c:968-1005).
 * The host used to do this from results read back piece by piece: 5.6 ms per 16384 x 16384 frame against
 * 1.9 ms of kernels.  Here the input is the shard blobs as hydamd_export_frame leaves them in device
 * memory (one per GPU that coded LF groups of the frame, gathered by RCCL or exported locally), the
 * output the finished codestream in one buffer, and the host contributes a PLAN (hydk_assemble.h): the
 * bytes that do not depend on the pixels.
 *
 *   k_asm_prepare   one launch of (LF groups + 1) workgroups (the writers are hydk_asm_writers.h's, shared with
 *                   assemble_batch.hip, which builds the frames of a batch side by side):
 *       asm_slot      one per LF group: checks its blob and slot record, writes the bits in front of the LF
 *                     coefficient symbols (constant fields from the plan + alphabet sizes and prefix codes, written
 *                     by a wavefront, hydk_sections.h) and the TOC sizes of its sections
 *       asm_hfglobal  the one behind them: the ANS histograms of every cluster, each written by a thread at the
 *                     bit offset a prefix sum gives it
 *       asm_layout    whichever workgroup finishes last: TOC entries (same scheme), where every section goes, the
 *                     frame's size
 *   k_pieces_copy   the frame as a sorted list of PIECES, each one bit string at a bit position (hydk_pieces.h:
 *                   a section is one piece, an LF group three — head, coefficient stream, geometry tail — and the
 *                   padding that ends it the gap before the next); every output word is composed from the pieces that
 *                   touch it and stored once, the first and last word of the range byte by byte, so nothing is
 *                   zeroed beforehand and nothing is ORed.  The tile assembler writes its launch groups with the same
 *                   kernel (hydk::launch_pieces_copy).
 *
 * Frames of a single group are one bit-contiguous section (encoder.c:837-850,968-981 guards): THIS assembler leaves
 * them to the host (hydamd_frame_from_blobs).  Tile-mode frames, single-group ones included, are built on the device by
 * assemble_tiles.hip, many at a time; the frames of a batch of one-frame images by assemble_batch.hip.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <new>

#include "../../../include/hydrium_amd.h"
#include "hydk_asm_common.h"
#include "hydk_common.h"
#include "hydk_asm_writers.h"

namespace {

constexpr int kHfgWords = 40 * 1024;    /* HFGlobal: <= 256 histograms of <= 73 words + the cluster map */
constexpr int kTocWords = 18 * 1024;    /* <= 16579 entries of <= 32 bits */
constexpr int kMaxPieces = 4 + 3 * HYDAMD_MAX_LF_GROUPS + HYDK_ASM_MAX_BLOBS; /* prefix, TOC, LFGlobal, HFGlobal; three per LF group; a blob's HF bytes */
constexpr int kCopyBlocks = 1024;
static_assert(kMaxPieces <= HYDK_COPY_MAX_PIECES, "k_pieces_copy keeps every end in LDS");

/* ---- k_asm_prepare: grid = LF groups + 1, block = 256: the frame's parts (hydk_asm_writers.h, asm_frame) ---- */
__global__ __launch_bounds__(256) void k_asm_prepare(const uint8_t *__restrict__ planb, BlobArgs blobs, Scratch S, uint64_t out_cap,
                                                     uint64_t *h_result) {
    __builtin_amdgcn_s_setprio(3); /* late work of a frame whose stream holds nothing else */
    const AsmFrame whole = {};
    asm_frame(planb, blobs, S, whole, blockIdx.x, gridDim.x, out_cap, h_result);
}

/* ---- k_pieces_copy: any grid, block = 256.  Word W of the range belongs to thread W mod (grid x 256) ---- */
__global__ __launch_bounds__(256) void k_pieces_copy(const HydkPiece *__restrict__ P, uint32_t np, const uint32_t *__restrict__ np_dev,
                                                     const uint64_t *__restrict__ range, uint8_t *__restrict__ out) {
    __shared__ uint64_t s_end[HYDK_COPY_MAX_PIECES];
    if (range[0] || !range[2])
        return;
    const uint64_t b_lo = range[1], b_hi = b_lo + range[2]; /* bytes [b_lo, b_hi) are this launch's */
    if (np_dev)
        np = *np_dev;
    np = min(np, (uint32_t)HYDK_COPY_MAX_PIECES);
    for (uint32_t i = threadIdx.x; i < np; i += 256)
        s_end[i] = P[i].dst_bit + P[i].nbits;
    __syncthreads();
    const uint64_t w_lo = b_lo >> 2, w_hi = (b_hi + 3) >> 2;
    for (uint64_t W = w_lo + (uint64_t)blockIdx.x * 256u + threadIdx.x; W < w_hi; W += (uint64_t)gridDim.x * 256u)
        hydk_store_word(out, W, hydk_pieces_word(P, s_end, np, W), b_lo, b_hi);
}

} // namespace

namespace hydk {
hipError_t launch_pieces_copy(const HydkPiece *P, uint32_t np, const uint32_t *np_dev, const uint64_t *range, void *out, hipStream_t stream) {
    hipLaunchKernelGGL(k_pieces_copy, dim3(kCopyBlocks), dim3(256), 0, stream, P, np, np_dev, range, (uint8_t *)out);
    return hipGetLastError();
}
} // namespace hydk

extern "C" void hydamd_host_copy(void *dst, const void *src, size_t n); /* device_api.hip */

struct HydkAsm {
    int device = 0;
    char error[256] = "";
    uint8_t *plan = nullptr; /* device copy */
    size_t plan_cap = 0;
    HydkAsmPlan hplan;       /* host copy of the header */
    bool have_plan = false;
    Scratch S = {};
    uint64_t *h_result = nullptr; /* pinned */
    uint8_t *own_out = nullptr;   /* output buffer for callers that bring none (hydk_asm_run with out == NULL) */
    size_t own_cap = 0;
    uint8_t *last_out = nullptr;  /* where the last run wrote */
    hipStream_t last_stream = nullptr; /* ... and the stream it ran in (the caller's: it must outlive hydk_asm_read of that run) */
    hipEvent_t done = nullptr;    /* the assembler's own: recorded behind every run; what a plan change and a run in another stream wait for */
    uint64_t last_cap = 0;        /* ... and how large that buffer is */
    bool ran = false;             /* `done` was recorded behind a complete run */
    bool unsettled = false;       /* a run's launches began and its event was never recorded (a launch failed in between): `done` says nothing about them */
    uint8_t *bounce = nullptr;    /* pinned: hydk_asm_read lands frames here (DMA engines), then copies to the caller's memory */
    size_t bounce_cap = 0;
};

extern "C" {

const char *hydk_asm_error(HydkAsm *a) { return a ? a->error : "null assembler"; }

void hydk_asm_destroy(HydkAsm *a) {
    if (!a)
        return;
    (void)hipSetDevice(a->device);
    void *dev[] = {a->own_out, a->plan, a->S.head, a->S.head_bits, a->S.sizes, a->S.slot_hf, a->S.hfg, a->S.toc, a->S.pieces, a->S.npieces,
                   a->S.err, a->S.done, a->S.result};
    for (void *p : dev)
        if (p)
            (void)hipFree(p);
    if (a->h_result)
        (void)hipHostFree(a->h_result);
    if (a->bounce)
        (void)hipHostFree(a->bounce);
    if (a->done)
        (void)hipEventDestroy(a->done);
    delete a;
}

static int asm_alloc(HydkAsm *a) {
    const size_t slots = HYDAMD_MAX_LF_GROUPS;
    const size_t toc_max = 2 + slots + slots * HYDK_GROUPS_PER_LFG;
    HYDK_TRY(a, hipSetDevice(a->device));
    HYDK_TRY(a, hipMalloc(&a->S.head, slots * kHeadWords * sizeof(uint32_t)));
    HYDK_TRY(a, hipMalloc(&a->S.head_bits, slots * sizeof(uint32_t)));
    HYDK_TRY(a, hipMalloc(&a->S.sizes, toc_max * sizeof(uint64_t)));
    HYDK_TRY(a, hipMalloc(&a->S.slot_hf, slots * sizeof(uint64_t)));
    HYDK_TRY(a, hipMalloc(&a->S.hfg, (size_t)kHfgWords * sizeof(uint32_t)));
    HYDK_TRY(a, hipMalloc(&a->S.toc, (size_t)kTocWords * sizeof(uint32_t)));
    HYDK_TRY(a, hipMalloc(&a->S.pieces, (size_t)kMaxPieces * sizeof(HydkPiece)));
    HYDK_TRY(a, hipMalloc(&a->S.npieces, sizeof(uint32_t)));
    HYDK_TRY(a, hipMalloc(&a->S.err, sizeof(uint32_t)));
    HYDK_TRY(a, hipMalloc(&a->S.done, sizeof(uint32_t)));
    HYDK_TRY(a, hipMemset(a->S.err, 0, sizeof(uint32_t)));
    HYDK_TRY(a, hipMemset(a->S.done, 0, sizeof(uint32_t)));
    /* hipMemset of device memory returns before it has run, in the NULL stream, which non-blocking streams do not wait
     * for: without this wait the first frame's kernels can pass the memsets (seen as a "malformed blob" once the
     * caller's stream and the null stream sat on different hardware queues) */
    HYDK_TRY(a, hipStreamSynchronize(nullptr));
    HYDK_TRY(a, hipMalloc(&a->S.result, 4 * sizeof(uint64_t)));
    a->S.hfg_words = kHfgWords;
    a->S.toc_words = kTocWords;
    HYDK_TRY(a, hipHostMalloc((void **)&a->h_result, 2 * sizeof(uint64_t), hipHostMallocDefault));
    a->h_result[0] = a->h_result[1] = 0;
    HYDK_TRY(a, hipEventCreateWithFlags(&a->done, hipEventDisableTiming));
    return ST_OK;
}

int hydk_asm_create(int device, HydkAsm **out) {
    int n = 0;
    if (!out)
        return ST_API_ERROR;
    *out = nullptr;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return ST_INTERNAL_ERROR;
    HydkAsm *a = new (std::nothrow) HydkAsm();
    if (!a)
        return ST_NOMEM;
    a->device = device;
    const int st = asm_alloc(a);
    if (st != ST_OK) {
        hydk_asm_destroy(a);
        return st;
    }
    *out = a;
    return ST_OK;
}

int hydk_asm_set_plan(HydkAsm *a, const void *plan, size_t bytes) {
    if (!a || !plan || bytes < sizeof(HydkAsmPlan))
        return hydk_fail(a, ST_API_ERROR, "bad plan");
    const HydkAsmPlan *hp = (const HydkAsmPlan *)plan;
    if (hp->magic != HYDK_ASM_PLAN_MAGIC || hp->total_bytes != bytes || hp->num_slots < 1 || hp->num_slots > HYDAMD_MAX_LF_GROUPS ||
        hp->num_blobs < 1 || hp->num_blobs > HYDK_ASM_MAX_BLOBS || hp->num_presets * hp->clusters_per_preset > 256 ||
        hp->toc_n != 2 + hp->num_slots + hp->frame_groups || hp->ntails > HYDK_ASM_MAX_TAILS)
        return hydk_fail(a, ST_API_ERROR, "inconsistent plan");
    HYDK_TRY(a, hipSetDevice(a->device));
    /* an earlier frame may still be reading the old plan: wait for IT only (a device-wide wait would stall every other
     * encoder thread's frames in a batch of differently shaped images) — by the assembler's own event, not by the caller's
     * stream handle, which may be gone by now; runs in different streams are chained behind each other (hydk_asm_run), so
     * the last run's event covers them all */
    if (a->unsettled) { /* kernels of a run that failed half-way may still be reading the old plan and scratch arrays */
        HYDK_TRY(a, hipDeviceSynchronize());
        a->unsettled = false;
    }
    if (a->ran)
        HYDK_TRY(a, hipEventSynchronize(a->done));
    if (bytes > a->plan_cap) {
        if (a->plan)
            (void)hipFree(a->plan);
        a->plan = nullptr;
        a->plan_cap = 0;
        HYDK_TRY(a, hipMalloc(&a->plan, bytes + 16)); /* + 16: the copy kernel reads whole words */
        a->plan_cap = bytes;
    }
    HYDK_TRY(a, hipMemcpy(a->plan, plan, bytes, hipMemcpyHostToDevice));
    a->hplan = *hp;
    a->have_plan = true;
    return ST_OK;
}

int hydk_asm_run(HydkAsm *a, const void *const *blobs, const uint64_t *blob_caps, void *stream, void *out, uint64_t out_cap) {
    if (!a || !a->have_plan || !blobs || !blob_caps)
        return hydk_fail(a, ST_API_ERROR, "assembler not ready");
    HYDK_TRY(a, hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    if (!out) { /* the assembler's own device buffer: `out_cap` bytes if the caller names a size, else what the blobs could hold
                 * (no frame is larger than its self-contained blobs plus its headers; views need a size from the caller) */
        size_t need = (size_t)out_cap;
        if (!need) {
            need = (size_t)1 << 20;
            for (uint32_t b = 0; b < a->hplan.num_blobs; b++)
                need += (size_t)blob_caps[b];
        }
        if (need > a->own_cap) {
            HYDK_TRY(a, hipStreamSynchronize(st));
            if (a->own_out)
                (void)hipFree(a->own_out);
            a->own_out = nullptr;
            a->own_cap = 0;
            HYDK_TRY(a, hipMalloc(&a->own_out, need));
            a->own_cap = need;
        }
        out = a->own_out;
        out_cap = a->own_cap;
    }
    /* k_pieces_copy moves whole 32-bit words of the output and 16-byte-aligned records of the blobs */
    if ((uintptr_t)out & 3u)
        return hydk_fail(a, ST_API_ERROR, "output buffer must be 4-byte aligned");
    if (a->unsettled) { /* the last run failed half-way: nothing says when its kernels are done with the scratch arrays */
        HYDK_TRY(a, hipDeviceSynchronize());
        a->unsettled = false;
    }
    if (a->ran && st != a->last_stream) /* the runs share the assembler's scratch arrays: one behind the other */
        HYDK_TRY(a, hipStreamWaitEvent(st, a->done, 0));
    a->last_out = (uint8_t *)out;
    a->last_cap = out_cap;
    a->last_stream = st;
    a->unsettled = true; /* until this run's event is recorded (`ran` used to be set here, before the launches) */
    BlobArgs args;
    memset(&args, 0, sizeof(args));
    for (uint32_t b = 0; b < a->hplan.num_blobs; b++) {
        if (!blobs[b])
            return hydk_fail(a, ST_API_ERROR, "null blob");
        if ((uintptr_t)blobs[b] & 15u)
            return hydk_fail(a, ST_API_ERROR, "blobs must be 16-byte aligned");
        args.p[b] = (const uint8_t *)blobs[b];
        args.cap[b] = blob_caps[b];
    }
    hipLaunchKernelGGL(k_asm_prepare, dim3(a->hplan.num_slots + 1), dim3(256), 0, st, (const uint8_t *)a->plan, args, a->S, out_cap,
                       a->h_result);
    HYDK_TRY(a, hydk::launch_pieces_copy(a->S.pieces, 0, a->S.npieces, a->S.result, out, st));
    HYDK_TRY(a, hipEventRecord(a->done, st));
    a->ran = true;
    a->unsettled = false;
    return ST_OK;
}

int hydk_asm_result(HydkAsm *a, uint64_t *size, uint32_t *err) {
    if (!a)
        return ST_API_ERROR;
    if (size)
        *size = a->h_result[0];
    if (err)
        *err = (uint32_t)a->h_result[1];
    return ST_OK;
}

/* after the stream has been synchronised: the frame's bytes, copied out of device memory.  `dst` is ordinary (pageable)
 * memory as a rule: a plain hipMemcpy into it is staged by the runtime through shader copies in 3 MB pieces (an 8K frame's
 * 12 MB: 0.6 ms, and a length that is not a multiple of four takes the same path whatever the destination).  So: one DMA
 * of the length rounded up to 256 bytes into a pinned buffer of the assembler's (56 GB/s), then the staging threads' memcpy */
int hydk_asm_read(HydkAsm *a, uint8_t *dst, size_t capacity) {
    if (!a || !dst || !a->last_out)
        return hydk_fail(a, ST_API_ERROR, "nothing to read");
    if (a->h_result[1] || !a->h_result[0] || a->h_result[0] > capacity)
        return hydk_fail(a, ST_API_ERROR, "no finished frame of that size");
    HYDK_TRY(a, hipSetDevice(a->device));
    const size_t n = (size_t)a->h_result[0];
    const size_t padded = (n + 255) & ~(size_t)255;
    if (n < ((size_t)1 << 20) || padded > a->last_cap) { /* small, or no room to round up: the runtime's own path */
        HYDK_TRY(a, hipMemcpy(dst, a->last_out, n, hipMemcpyDeviceToHost));
        return ST_OK;
    }
    if (padded > a->bounce_cap) {
        if (a->bounce)
            (void)hipHostFree(a->bounce);
        a->bounce = nullptr;
        a->bounce_cap = 0;
        const size_t want = padded + (padded >> 2);
        HYDK_TRY(a, hipHostMalloc((void **)&a->bounce, want, hipHostMallocDefault));
        a->bounce_cap = want;
    }
    HYDK_TRY(a, hipMemcpyAsync(a->bounce, a->last_out, padded, hipMemcpyDeviceToHost, a->last_stream));
    HYDK_TRY(a, hipStreamSynchronize(a->last_stream));
    hydamd_host_copy(dst, a->bounce, n);
    return ST_OK;
}

int hydk_asm_debug(HydkAsm *a, uint32_t slot, uint32_t *head_bits, uint32_t *head_words, size_t head_cap, uint32_t *hfg_bits,
                   uint32_t *hfg_words, size_t hfg_cap) {
    if (!a || slot >= HYDAMD_MAX_LF_GROUPS)
        return ST_API_ERROR;
    HYDK_TRY(a, hipSetDevice(a->device));
    HYDK_TRY(a, hipDeviceSynchronize());
    if (head_bits)
        HYDK_TRY(a, hipMemcpy(head_bits, a->S.head_bits + slot, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (head_words)
        HYDK_TRY(a, hipMemcpy(head_words, a->S.head + (size_t)slot * kHeadWords,
                             (head_cap < (size_t)kHeadWords ? head_cap : (size_t)kHeadWords) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (hfg_bits) {
        uint64_t sz = 0;
        HYDK_TRY(a, hipMemcpy(&sz, a->S.sizes + 1 + a->hplan.num_slots, sizeof(uint64_t), hipMemcpyDeviceToHost));
        *hfg_bits = (uint32_t)(sz * 8u);
    }
    if (hfg_words)
        HYDK_TRY(a, hipMemcpy(hfg_words, a->S.hfg, (hfg_cap < (size_t)kHfgWords ? hfg_cap : (size_t)kHfgWords) * sizeof(uint32_t),
                             hipMemcpyDeviceToHost));
    return ST_OK;
}

#ifdef HYD_TEST_HOOKS
/* k_pieces_copy itself on a crafted list (tests/test_gpu_builder_content.py; the probe flavour only): the arguments of
 * tiled.c's hydt_compose_pieces, which runs the same composer on the host, plus what a kernel launch has to be told —
 * how long `src` and `out` are, and the error word of the range.  Piece i is nbits[i] bits from byte src_off[i] of `src`,
 * at bit dst_bit[i]; the range is bytes [lo, lo + bytes) of `out`.  `src` is uploaded into one allocation with 16 bytes
 * of slack on either side, `out` (filled by the caller) as it is; one launch through hydk::launch_pieces_copy, and the
 * WHOLE buffer comes back: a store outside the range shows.  Lists that would read or write outside the two buffers
 * are refused here, before anything is launched. */
__attribute__((visibility("default"))) int hydt_pieces_copy_device(const uint64_t *dst_bit, const uint64_t *nbits, const uint64_t *src_off,
                                                                   uint32_t np, const uint8_t *src, uint64_t src_bytes, uint64_t lo,
                                                                   uint64_t bytes, uint32_t err_word, uint8_t *out, uint64_t out_bytes) {
    constexpr size_t kSlack = 16;
    if (!src || !out || (np && (!dst_bit || !nbits || !src_off)) || np > HYDK_COPY_MAX_PIECES || (out_bytes & 3u) ||
        lo > out_bytes || bytes > out_bytes - lo || ((lo + bytes + 3) & ~(uint64_t)3) > out_bytes)
        return ST_API_ERROR;
    for (uint32_t i = 0; i < np; i++)
        if (src_off[i] > src_bytes || ((nbits[i] + 7) >> 3) > src_bytes - src_off[i])
            return ST_API_ERROR;
    uint8_t *d_src = nullptr, *d_out = nullptr;
    HydkPiece *d_P = nullptr;
    uint64_t *d_range = nullptr;
    HydkPiece *P = new (std::nothrow) HydkPiece[np ? np : 1];
    if (!P)
        return ST_NOMEM;
    auto run = [&]() -> int {
        HYDK_TRY((HydkAsm *)nullptr, hipMalloc(&d_src, (size_t)src_bytes + 2 * kSlack));
        HYDK_TRY((HydkAsm *)nullptr, hipMalloc(&d_out, (size_t)out_bytes + 4));
        HYDK_TRY((HydkAsm *)nullptr, hipMalloc(&d_P, (np ? np : 1) * sizeof(HydkPiece)));
        HYDK_TRY((HydkAsm *)nullptr, hipMalloc(&d_range, 4 * sizeof(uint64_t)));
        for (uint32_t i = 0; i < np; i++)
            P[i] = hydk_piece(dst_bit[i], d_src + kSlack + src_off[i], nbits[i]);
        const uint64_t range[4] = {err_word, lo, bytes, 0};
        HYDK_TRY((HydkAsm *)nullptr, hipMemset(d_src, 0x3C, (size_t)src_bytes + 2 * kSlack));
        HYDK_TRY((HydkAsm *)nullptr, hipMemcpy(d_src + kSlack, src, (size_t)src_bytes, hipMemcpyHostToDevice));
        HYDK_TRY((HydkAsm *)nullptr, hipMemcpy(d_out, out, (size_t)out_bytes, hipMemcpyHostToDevice));
        if (np)
            HYDK_TRY((HydkAsm *)nullptr, hipMemcpy(d_P, P, np * sizeof(HydkPiece), hipMemcpyHostToDevice));
        HYDK_TRY((HydkAsm *)nullptr, hipMemcpy(d_range, range, sizeof(range), hipMemcpyHostToDevice));
        HYDK_TRY((HydkAsm *)nullptr, hipDeviceSynchronize()); /* the memset ran in the NULL stream */
        HYDK_TRY((HydkAsm *)nullptr, hydk::launch_pieces_copy(d_P, np, nullptr, d_range, d_out, nullptr));
        HYDK_TRY((HydkAsm *)nullptr, hipDeviceSynchronize());
        HYDK_TRY((HydkAsm *)nullptr, hipMemcpy(out, d_out, (size_t)out_bytes, hipMemcpyDeviceToHost));
        return ST_OK;
    };
    const int st = run();
    void *dev[] = {d_src, d_out, d_P, d_range};
    for (void *p : dev)
        if (p)
            (void)hipFree(p);
    delete[] P;
    return st;
}
#endif /* HYD_TEST_HOOKS */

} /* extern "C" */
