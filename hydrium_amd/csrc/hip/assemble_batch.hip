/*
 * assemble_batch.hip — the frames of a BATCH of independent one-frame images, assembled side by side on the GPU into
 * finished files.
 *
 * hydamd_encode_image_batch codes F pictures of one shape (n LF groups each) as one launch group and leaves their
 * sections and coded LF streams in the context's buffers.  Here one launch sequence in the context's stream takes
 * those results as a view (hydamd_export_batch_owned: one header, the F x n slot records, frame k's at k n .. k n + n - 1,
 * the packed LF streams and HF sections in place, per-slot extents) and writes F complete files — file header, frame
 * header with is_last, TOC, LFGlobal, LF groups, HFGlobal, HF sections: what the reference writes for each picture
 * alone — back to back at byte granularity into one buffer, with the table of their offsets beside it:
 *
 *   k_batch_prepare      grid F x (n + 1), block 256: workgroup (f, s) is part s of frame f of hydk_asm_writers.h's
 *                        asm_frame — the same writers as k_asm_prepare's, on frame f's slot records and frame f's
 *                        scratch; the frame's last finisher lays it out, its pieces counted from the frame's first byte
 *   k_batch_prepare_one  (shapes of ONE LF group, a single bit-contiguous section included) grid F, block 64: the
 *                        tile assembler's per-frame preparation and pieces (hydk_tiles.h) with a plan whose one frame
 *                        carries the file header and is_last
 *   k_batch_prepare_mixed  (one-LF-group frames EACH OF ITS OWN SIZE, csrc/host/mixed.c) the same wavefront body with
 *                        frame f's own record of a mixed plan — its own file header and frame header — and the shape
 *                        that record names, after checking on the device that the plan covers the batch
 *   k_batch_prepare_frames  (frames of DIFFERENT LF-group counts side by side, a frames plan of mixed.c) grid = sum of
 *                        (n_k + 1) over the frames of several LF groups, block 256: a workgroup looks its (frame, part) up in
 *                        the plan's table and runs asm_frame with THAT frame's plan, slots and share of the scratch; the
 *                        batch's frames of one LF group take the wavefront path beside it (k_batch_prepare_frames_one,
 *                        grid F), on their first slot and their share
 *   k_batch_place        one workgroup: the union of the frames' error words, a prefix sum over their sizes = the
 *                        offsets table, every piece moved to its frame's start, the range k_pieces_copy reads; with
 *                        per-image outcomes (hydk_batch_set_image_errors) a frame ANY of whose slots carries the bad-sample
 *                        flag (HydAmdBlobSlot.reserved[0]) — whichever of the five kernels above prepared it — counts 0
 *                        bytes, has its pieces emptied in place and its status word set, and fails nothing
 *   k_pieces_copy        (assemble.hip) every output word composed from the pieces that touch it and stored once; the
 *                        padding that ends a section, and a file, is the gap no piece covers
 *
 * Every frame of a batch has the same pixel-independent bytes: ONE plan (csrc/host/batch.c builds it with the frame
 * planner, or the tile planner for n = 1) serves all of them; a mixed batch brings a plan of its own, one record per
 * frame and one per distinct shape (and, where frames hold several LF groups, a frame plan per distinct size of those),
 * uploaded in the stream ahead of the assembly.  No host synchronisation between the entropy stage and
 * the finished files.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <new>

#include "../../../include/hydrium_amd.h"
#include "hydk_batch_asm.h"
#include "hydk_tiles.h"
#include "hydk_common.h"
#include "hydk_asm_writers.h"

namespace {

constexpr int kMaxSlots = HYDAMD_MAX_LF_GROUPS; /* F x n: the slots of one context */
/* pieces of a batch: F x (3 n + 5) with F n <= 255 is at most 3 x 255 + 5 F <= 765 + 5 x 255 = 2040; frames of one
 * LF group take HYDK_TILE_PIECES = 8 = 3 + 5 each, the same bound */
static_assert(3 * kMaxSlots + 5 * kMaxSlots <= HYDK_COPY_MAX_PIECES && HYDK_TILE_PIECES * kMaxSlots <= HYDK_COPY_MAX_PIECES,
              "k_pieces_copy keeps every end in LDS");

struct BatchScratch { /* device pointers; frame f's part of each array is what asm_frame / hydk_tile_prepare gets */
    uint32_t *head;       /* [slots][kHeadWords]            | n = 1: [frames][HYDK_TILE_HEAD_WORDS] */
    uint32_t *head_bits;  /* [slots]                        | n = 1: null, like sizes, slot_hf, npieces, err, done */
    uint64_t *sizes;      /* [frames][toc_n] */
    uint64_t *slot_hf;    /* [slots] */
    uint32_t *hfg;        /* [frames][hfg_words]            | n = 1: [frames][HYDK_TILE_MID_WORDS] */
    uint32_t *toc;        /* [frames][toc_words]            | n = 1: [frames][HYDK_TILE_TOC_WORDS] */
    HydkPiece *pieces;    /* [frames][pieces_per_frame] */
    uint32_t *npieces;    /* [frames] */
    uint32_t *err;        /* [frames] */
    uint32_t *done;       /* [frames] */
    uint64_t *result;     /* [frames][4] error word, 0, bytes of the frame, HFGlobal's bit count */
    uint64_t *offsets;    /* [frames + 1] the table the caller gets */
    uint32_t *status;     /* [frames] beside it: 0 a file, HYDAMD_IMAGE_BAD_SAMPLE no bytes (per-image outcomes only) */
    uint64_t *range;      /* [4] error word, 0, bytes of all files (what k_pieces_copy reads), bytes the output must hold */
    uint32_t n, toc_n, hfg_words, toc_words, pieces_per_frame;
    /* a frames plan (hydk_tiles.h, HydkFramesPlan): the five above are zero — every frame's record names its slots and its
     * offsets into hfg, toc, sizes and pieces; head is [slots][HYDK_FRAMES_HEAD_STRIDE] — and these are what the arrays hold */
    uint32_t hfg_cap, toc_cap, sizes_cap, pieces_cap;
};

__device__ __forceinline__ Scratch frame_scratch(const BatchScratch &B, uint32_t f) {
    Scratch S;
    S.head = B.head + (size_t)f * B.n * kHeadWords;
    S.head_bits = B.head_bits + (size_t)f * B.n;
    S.sizes = B.sizes + (size_t)f * B.toc_n;
    S.slot_hf = B.slot_hf + (size_t)f * B.n;
    S.hfg = B.hfg + (size_t)f * B.hfg_words;
    S.toc = B.toc + (size_t)f * B.toc_words;
    S.pieces = B.pieces + (size_t)f * B.pieces_per_frame;
    S.npieces = B.npieces + f;
    S.err = B.err + f;
    S.done = B.done + f;
    S.result = B.result + (size_t)f * 4;
    S.hfg_words = B.hfg_words;
    S.toc_words = B.toc_words;
    return S;
}

/* ---- k_batch_prepare: grid = frames x (n + 1), block = 256 ---- */
__global__ __launch_bounds__(256) void k_batch_prepare(const uint8_t *__restrict__ planb, const uint8_t *__restrict__ blob, uint64_t blob_cap,
                                                       const HydkTileExtent *__restrict__ ext, uint32_t frames, BatchScratch B) {
    __builtin_amdgcn_s_setprio(3); /* late work of a batch whose stream holds nothing else */
    const uint32_t n = B.n, f = blockIdx.x / (n + 1), part = blockIdx.x % (n + 1);
    BlobArgs blobs;
    blobs.p[0] = blob;
    blobs.cap[0] = blob_cap;
    /* the frame's HF sections: its slots' extents, one behind the other in the packed string (k_batch_extents; the
     * layout holds their sum against the section sizes the slot records give, k_batch_place the grand total against the
     * header; until the header has been checked — asm_slot, asm_hfglobal — nothing is read through these) */
    const HydkTileExtent first = ext[(size_t)f * n], last = ext[(size_t)f * n + n - 1];
    AsmFrame F;
    F.slot_base = f * n;
    F.view_slots = frames * n;
    F.hf = blob_hf_bytes(blob) + first.hf_off;
    F.hf_bytes = last.hf_off + last.hf_bytes - first.hf_off;
    asm_frame(planb, blobs, frame_scratch(B, f), F, part, n + 1, ~0ull, nullptr);
}

/* where a frame of one LF group sits: its slot of the view and its share of the scratch arrays */
struct OneFrame {
    uint32_t slot;
    uint32_t *head, *mid, *toc; /* HYDK_TILE_HEAD_WORDS, HYDK_TILE_MID_WORDS, HYDK_TILE_TOC_WORDS words */
    HydkPiece *pieces;          /* HYDK_TILE_PIECES */
};

/* in a view whose every frame holds one LF group, frame f has slot f and the f-th part of every array */
static __device__ __forceinline__ OneFrame one_frame_uniform(const BatchScratch &B, uint32_t f) {
    return {f, B.head + (size_t)f * HYDK_TILE_HEAD_WORDS, B.hfg + (size_t)f * HYDK_TILE_MID_WORDS, B.toc + (size_t)f * HYDK_TILE_TOC_WORDS,
            B.pieces + (size_t)f * HYDK_TILE_PIECES};
}

/* one wavefront, frame f of a view, a frame of ONE LF group: the tile assembler's preparation and pieces with the frame
 * record `fr` and the shape `sh` of the plan `planb` (the view has been checked) */
static __device__ __forceinline__ void prepare_one(const uint8_t *__restrict__ planb, const HydkTileFrame &fr, const HydkTileShape *sh,
                                                   const uint8_t *__restrict__ blob, const HydkTileExtent *__restrict__ ext, uint32_t f,
                                                   const OneFrame &at, const BatchScratch &B) {
    uint64_t *result = B.result + (size_t)f * 4;
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    const HydAmdBlobSlot *rec = (const HydAmdBlobSlot *)(blob + sizeof(HydAmdBlobHeader)) + at.slot;
    uint32_t *head = at.head, *mid = at.mid, *toc = at.toc;
    const HydkTileSizes z = hydk_tile_prepare_wave(planb, &fr, sh, rec, h->lf_bytes, head, mid, toc);
    if (threadIdx.x == 0) {
        const HydkTileExtent x = ext[at.slot];
        uint32_t e = z.err;
        if (!e && (x.hf_bytes != z.hf_bytes || x.hf_off + z.hf_bytes > h->hf_bytes))
            e = HYDK_ASM_E_SIZE;
        if (!e)
            hydk_tile_pieces(planb, &fr, sh, &z, rec, head, mid, toc, blob_lf_bytes(blob) + x.lf_off, blob_hf_bytes(blob) + x.hf_off, 0,
                             at.pieces);
        result[0] = e;
        result[1] = 0;
        result[2] = e ? 0 : z.frame_bytes;
        result[3] = 0;
    }
}

static __device__ __forceinline__ void prepare_failed(const BatchScratch &B, uint32_t f, uint32_t bad) {
    if (threadIdx.x == 0) {
        uint64_t *result = B.result + (size_t)f * 4;
        result[0] = bad;
        result[1] = result[2] = result[3] = 0;
    }
}

/* ---- k_batch_prepare_one: grid = frames, block = 64 (one wavefront); every frame is frame 0 of the tile plan ---- */
__global__ __launch_bounds__(64) void k_batch_prepare_one(const uint8_t *__restrict__ planb, const uint8_t *__restrict__ blob,
                                                          const HydkTileExtent *__restrict__ ext, uint32_t frames, BatchScratch B) {
    const uint32_t f = blockIdx.x;
    const uint32_t bad = blob_view_check(blob, frames);
    if (bad)
        return prepare_failed(B, f, bad);
    const HydkTilePlan *plan = (const HydkTilePlan *)planb;
    const HydkTileFrame fr = ((const HydkTileFrame *)(planb + plan->frames_off))[0];
    prepare_one(planb, fr, &plan->shapes[fr.shape], blob, ext, f, one_frame_uniform(B, f), B);
}

/* ---- k_batch_prepare_mixed: grid = frames, block = 64; frame f is frame f of a MIXED plan (hydk_tiles.h), with its own
 * prefix and the shape it names.  The plan arrives per batch, so what the indices below rest on is checked here: a plan
 * of another kind or of fewer frames than the batch is a malformed input (BLOB), a shape the plan does not hold an
 * inconsistent record (SLOT); nothing behind the plan's header is read before the first, nothing of a shape before the second ---- */
__global__ __launch_bounds__(64) void k_batch_prepare_mixed(const uint8_t *__restrict__ planb, const uint8_t *__restrict__ blob,
                                                            const HydkTileExtent *__restrict__ ext, uint32_t frames, BatchScratch B) {
    const uint32_t f = blockIdx.x;
    const HydkMixedPlan *plan = (const HydkMixedPlan *)planb;
    uint32_t bad = blob_view_check(blob, frames);
    if (!bad && (plan->magic != HYDK_MIXED_MAGIC || plan->num_frames < frames))
        bad = HYDK_ASM_E_BLOB;
    if (bad)
        return prepare_failed(B, f, bad);
    const HydkTileFrame fr = ((const HydkTileFrame *)(planb + plan->frames_off))[f];
    if (fr.shape >= plan->nshapes)
        return prepare_failed(B, f, HYDK_ASM_E_SLOT);
    prepare_one(planb, fr, (const HydkTileShape *)(planb + plan->shapes_off) + fr.shape, blob, ext, f, one_frame_uniform(B, f), B);
}

/* ---- frames of different LF-group counts side by side (a FRAMES plan, hydk_tiles.h).  The plan arrives per batch, so both
 * kernels check on the device what their indices rest on, before they follow any of them: the view, and that the plan is
 * of this kind and covers the batch — its frames, its slots, its tables inside its bytes (BLOB; nothing behind the plan's
 * header is read before); then the frame's record — its slots inside the view, its own plan inside the plan's bytes, of one
 * blob and as many LF groups (SLOT), its share of the scratch inside the arrays (SCRATCH) ---- */
static __device__ __forceinline__ uint32_t frames_plan_check(const uint8_t *__restrict__ planb, const uint8_t *__restrict__ blob, uint32_t frames,
                                                             uint32_t slots) {
    const HydkFramesPlan *plan = (const HydkFramesPlan *)planb;
    const uint32_t bad = blob_view_check(blob, slots);
    if (bad)
        return bad;
    if (plan->magic != HYDK_FRAMES_MAGIC || plan->num_frames != frames || plan->num_slots != slots ||
        (uint64_t)plan->frames_off + (uint64_t)frames * sizeof(HydkBatchFrame) > plan->total_bytes ||
        (uint64_t)plan->shapes_off + (uint64_t)plan->nshapes * sizeof(HydkTileShape) > plan->total_bytes ||
        (uint64_t)plan->parts_off + (uint64_t)plan->nparts * sizeof(uint32_t) > plan->total_bytes)
        return HYDK_ASM_E_BLOB;
    return 0;
}

static __device__ __forceinline__ uint32_t frames_record_check(const uint8_t *__restrict__ planb, const HydkBatchFrame &fr, const BatchScratch &B) {
    const HydkFramesPlan *plan = (const HydkFramesPlan *)planb;
    const uint64_t n = fr.lf_groups;
    if (n < 1 || (uint64_t)fr.first_slot + n > plan->num_slots)
        return HYDK_ASM_E_SLOT;
    uint64_t sizes = 0;
    if (fr.plan_off) {
        if ((fr.plan_off & 15u) || (uint64_t)fr.plan_off + sizeof(HydkAsmPlan) > plan->total_bytes)
            return HYDK_ASM_E_SLOT;
        const HydkAsmPlan *ap = (const HydkAsmPlan *)(planb + fr.plan_off);
        if (ap->magic != HYDK_ASM_PLAN_MAGIC || (uint64_t)fr.plan_off + ap->total_bytes > plan->total_bytes || ap->num_blobs != 1 ||
            ap->num_slots != n || ap->blob_slots[0] != n || ap->num_presets * ap->clusters_per_preset > 256 || ap->ntails > HYDK_ASM_MAX_TAILS)
            return HYDK_ASM_E_SLOT;
        sizes = ap->toc_n;
    } else if (n != 1 || fr.one.shape >= plan->nshapes || fr.hfg_words < HYDK_TILE_MID_WORDS || fr.toc_words < HYDK_TILE_TOC_WORDS) {
        return HYDK_ASM_E_SLOT;
    }
    if ((uint64_t)fr.hfg_off + fr.hfg_words > B.hfg_cap || (uint64_t)fr.toc_off + fr.toc_words > B.toc_cap ||
        (uint64_t)fr.sizes_off + sizes > B.sizes_cap || (uint64_t)fr.piece_base + 3u * n + 5u > B.pieces_cap)
        return HYDK_ASM_E_SCRATCH;
    return 0;
}

/* ---- k_batch_prepare_frames: grid = the plan's parts (n_k + 1 per frame of several LF groups), block = 256 ---- */
__global__ __launch_bounds__(256) void k_batch_prepare_frames(const uint8_t *__restrict__ planb, const uint8_t *__restrict__ blob, uint64_t blob_cap,
                                                              const HydkTileExtent *__restrict__ ext, uint32_t frames, uint32_t slots,
                                                              BatchScratch B) {
    __builtin_amdgcn_s_setprio(3);
    const HydkFramesPlan *plan = (const HydkFramesPlan *)planb;
    const uint32_t bad = frames_plan_check(planb, blob, frames, slots);
    if (bad) { /* no table to look a frame up in: the word goes to every frame (the other launch may have none) */
        if (blockIdx.x == 0)
            for (uint32_t f = threadIdx.x; f < frames; f += 256) {
                uint64_t *result = B.result + (size_t)f * 4;
                result[0] = bad;
                result[1] = result[2] = result[3] = 0;
            }
        return;
    }
    if (blockIdx.x >= plan->nparts)
        return;
    const uint32_t fp = ((const uint32_t *)(planb + plan->parts_off))[blockIdx.x], f = fp >> 8, part = fp & 255u;
    if (f >= frames)
        return;
    const HydkBatchFrame fr = ((const HydkBatchFrame *)(planb + plan->frames_off))[f];
    const uint32_t e = fr.plan_off ? frames_record_check(planb, fr, B) : HYDK_ASM_E_SLOT;
    if (e) { /* every part of the frame sees the same record: none of them counts itself done */
        if (part == 0)
            prepare_failed(B, f, e);
        return;
    }
    if (part > fr.lf_groups)
        return;
    BlobArgs blobs;
    blobs.p[0] = blob;
    blobs.cap[0] = blob_cap;
    Scratch S;
    S.head = B.head + (size_t)fr.first_slot * HYDK_FRAMES_HEAD_STRIDE; /* the frame's slots follow at kHeadWords inside it */
    S.head_bits = B.head_bits + fr.first_slot;
    S.sizes = B.sizes + fr.sizes_off;
    S.slot_hf = B.slot_hf + fr.first_slot;
    S.hfg = B.hfg + fr.hfg_off;
    S.toc = B.toc + fr.toc_off;
    S.pieces = B.pieces + fr.piece_base;
    S.npieces = B.npieces + f;
    S.err = B.err + f;
    S.done = B.done + f;
    S.result = B.result + (size_t)f * 4;
    S.hfg_words = fr.hfg_words;
    S.toc_words = fr.toc_words;
    /* the frame's HF sections: its slots' extents, as k_batch_prepare's */
    const HydkTileExtent first = ext[fr.first_slot], last = ext[fr.first_slot + fr.lf_groups - 1];
    AsmFrame F;
    F.slot_base = fr.first_slot;
    F.view_slots = slots;
    F.hf = blob_hf_bytes(blob) + first.hf_off;
    F.hf_bytes = last.hf_off + last.hf_bytes - first.hf_off;
    asm_frame(planb + fr.plan_off, blobs, S, F, part, fr.lf_groups + 1, ~0ull, nullptr);
}

/* ---- k_batch_prepare_frames_one: grid = frames, block = 64; the frames of ONE LF group of the same plan (the others':
 * nothing to do here), as k_batch_prepare_mixed's but for the frame's slot and its share of the arrays ---- */
__global__ __launch_bounds__(64) void k_batch_prepare_frames_one(const uint8_t *__restrict__ planb, const uint8_t *__restrict__ blob,
                                                                 const HydkTileExtent *__restrict__ ext, uint32_t frames, uint32_t slots,
                                                                 BatchScratch B) {
    const uint32_t f = blockIdx.x;
    const HydkFramesPlan *plan = (const HydkFramesPlan *)planb;
    const uint32_t bad = frames_plan_check(planb, blob, frames, slots);
    if (bad)
        return prepare_failed(B, f, bad);
    const HydkBatchFrame fr = ((const HydkBatchFrame *)(planb + plan->frames_off))[f];
    if (fr.plan_off)
        return;
    const uint32_t e = frames_record_check(planb, fr, B);
    if (e)
        return prepare_failed(B, f, e);
    const OneFrame at = {fr.first_slot, B.head + (size_t)fr.first_slot * HYDK_FRAMES_HEAD_STRIDE, B.hfg + fr.hfg_off, B.toc + fr.toc_off,
                         B.pieces + fr.piece_base};
    prepare_one(planb, fr.one, (const HydkTileShape *)(planb + plan->shapes_off) + fr.one.shape, blob, ext, f, at, B);
}

/* ---- k_batch_place: grid 1, block 256 ---- */
__global__ __launch_bounds__(256) void k_batch_place(const uint8_t *__restrict__ blob, const HydkTileExtent *__restrict__ ext, uint32_t frames,
                                                     uint32_t slots /* of the view */, const uint8_t *__restrict__ frames_plan /* or null */,
                                                     BatchScratch B, uint64_t out_cap, uint32_t per_image,
                                                     uint64_t *h_result /* pinned [4 + frames + 1] */, uint64_t *h_status /* pinned [frames] */) {
    __shared__ uint64_t s_wave[4];
    __shared__ uint64_t s_at[256];
    __shared__ uint8_t s_skip[256];
    __shared__ uint32_t s_err;
    const uint32_t t = threadIdx.x;
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    uint32_t e = 0, skip = 0;
    uint64_t size = 0;
    if (t < frames) {
        e = (uint32_t)B.result[(size_t)t * 4];
        size = B.result[(size_t)t * 4 + 2];
        /* per-image outcomes: the frame's slots are looked at only where its preparation found nothing wrong — the view is
         * this batch's and, with a frames plan, the frame's record names slots inside it (frames_record_check) */
        if (per_image && !e) {
            uint32_t first = t * B.n, n = B.n;
            if (frames_plan) {
                const HydkFramesPlan *plan = (const HydkFramesPlan *)frames_plan;
                const HydkBatchFrame fr = ((const HydkBatchFrame *)(frames_plan + plan->frames_off))[t];
                first = fr.first_slot;
                n = fr.lf_groups;
            }
            const HydAmdBlobSlot *rec = (const HydAmdBlobSlot *)(blob + sizeof(HydAmdBlobHeader)) + first;
            if ((uint64_t)first + n <= slots)
                skip = hydk_frame_flagged(rec, n);
            if (skip)
                size = 0; /* no bytes: offsets[t + 1] == offsets[t] */
        }
    }
    s_skip[t] = (uint8_t)skip;
    if (t == 0) {
        s_err = 0;
        /* the frames' HF extents together are the packed string, no more and no less */
        uint32_t he = blob_ident(h, slots);
        if (per_image)
            he &= ~(uint32_t)HYDK_ASM_E_NAN; /* (a context in per-slot mode never sets the bit: the outcome is the frame's) */
        if (!he && ext[slots - 1].hf_off + ext[slots - 1].hf_bytes != h->hf_bytes)
            he = HYDK_ASM_E_SIZE;
        e |= he;
    }
    __syncthreads();
    if (e)
        atomicOr(&s_err, e);
    __syncthreads();
    const uint32_t err = s_err;
    uint64_t total = 0;
    const uint64_t at = scan256(err ? 0 : size, s_wave, &total);
    s_at[t] = at;
    const uint32_t fin = err ? err : total > out_cap ? HYDK_ASM_E_SPACE : 0u;
    if (t < frames) {
        B.offsets[t] = at;
        h_result[4 + t] = at;
        B.status[t] = skip ? HYDAMD_IMAGE_BAD_SAMPLE : 0u;
        h_status[t] = skip ? HYDAMD_IMAGE_BAD_SAMPLE : 0u;
    }
    __syncthreads();
    /* A skipped frame keeps its places in the piece list — the list k_pieces_copy searches stays as long, contiguous and in
     * output order — but every one of them becomes an EMPTY piece at the frame's offset, which is also the next frame's
     * (hydk_place_piece): ends stay monotone, no bit of the output is covered, and the files on both sides meet inside one
     * output word. */
    if (!fin && frames_plan) {
        /* frames of different LF-group counts: frame f's 3 n + 5 pieces start where its record says — the sum over the
         * frames before it, so that the list stays contiguous and in output order (no error: the plan has been checked) */
        if (t < frames) {
            const HydkFramesPlan *plan = (const HydkFramesPlan *)frames_plan;
            const HydkBatchFrame fr = ((const HydkBatchFrame *)(frames_plan + plan->frames_off))[t];
            for (uint32_t i = 0; i < 3u * fr.lf_groups + 5u; i++)
                hydk_place_piece(&B.pieces[fr.piece_base + i], at, skip);
        }
    } else if (!fin) {
        const uint32_t np = frames * B.pieces_per_frame;
        for (uint32_t i = t; i < np; i += 256) {
            const uint32_t f = i / B.pieces_per_frame;
            hydk_place_piece(&B.pieces[i], s_at[f], s_skip[f]);
        }
    }
    if (t == 0) {
        B.offsets[frames] = total;
        h_result[4 + frames] = total;
        B.range[0] = fin;
        B.range[1] = 0;
        B.range[2] = fin ? 0 : total;
        B.range[3] = total;
        for (int i = 0; i < 4; i++)
            h_result[i] = B.range[i];
    }
}

} // namespace

struct HydkBatchAsm {
    int device = 0;
    char error[256] = "";
    uint8_t *arena = nullptr;     /* the plan, then every array of B: one allocation */
    uint8_t *plan = nullptr;
    int max_frames = 0;
    bool one = false;             /* frames of one LF group: the plan is a tile plan (hydk_tiles.h) */
    bool mixed = false;           /* ... each of its own size: a mixed plan per batch (hydk_batch_set_plan), in a region of its own */
    size_t plan_cap = 0;          /* mixed: bytes of that region and of the pinned buffer the plan travels through */
    uint8_t *h_plan = nullptr;
    uint32_t plan_frames = 0;     /* mixed: frames of the plan on the device */
    bool several = false;         /* mixed, frames of 1..28 LF groups: the plan is a frames plan, and these are its: */
    int max_slots = 0;
    uint32_t plan_slots = 0, plan_parts = 0, plan_pieces = 0;
    BatchScratch B = {};
    uint64_t fixed = 0;           /* bytes of a frame beyond its packed LF streams and HF sections, at most; stays 0 for a
                                   * mixed assembler, whose frames differ: mixed.c sums the same terms per batch, from its plan */
    uint64_t *h_result = nullptr; /* pinned [4 + max_frames + 1 + max_frames]: the range quadruple, the offsets table ([frames + 1]
                                   * of the batch), and from 4 + max_frames + 1 on the frames' status words */
    bool per_image = false;       /* hydk_batch_set_image_errors */
    uint8_t *out = nullptr;       /* the files: owned, grown on demand (hydk_batch_reserve) */
    uint64_t out_cap = 0;
};

extern "C" {

const char *hydk_batch_error(HydkBatchAsm *a) { return a ? a->error : "null batch assembler"; }

void hydk_batch_destroy(HydkBatchAsm *a) {
    if (!a)
        return;
    (void)hipSetDevice(a->device);
    if (a->out)
        (void)hipFree(a->out);
    if (a->mixed && a->plan)
        (void)hipFree(a->plan);
    if (a->h_plan)
        (void)hipHostFree(a->h_plan);
    if (a->arena)
        (void)hipFree(a->arena);
    if (a->h_result)
        (void)hipHostFree(a->h_result);
    delete a;
}

/* scratch for batches of up to `max_frames` frames of the plan's shape; the plan — a HydkAsmPlan of one blob, or a
 * HydkTilePlan of one frame for shapes of one LF group — is copied to the device.  No plan: frames of one LF group, each
 * of its own size, whose (mixed) plan comes with every batch (hydk_batch_set_plan) */
int hydk_batch_create(int device, int max_frames, const void *plan, size_t plan_bytes, HydkBatchAsm **out) {
    if (!out)
        return ST_API_ERROR;
    *out = nullptr;
    if (max_frames < 1 || (plan && plan_bytes < 8))
        return ST_API_ERROR;
    const uint32_t magic = plan ? *(const uint32_t *)plan : 0u;
    const HydkAsmPlan *ap = (const HydkAsmPlan *)plan;
    const HydkTilePlan *tp = (const HydkTilePlan *)plan;
    HydkBatchAsm *a = new (std::nothrow) HydkBatchAsm();
    if (!a)
        return ST_NOMEM;
    a->device = device;
    a->max_frames = max_frames;
    BatchScratch &B = a->B;
    size_t head_words = 0;
    if (!plan && max_frames <= HYDK_TILE_MAX_FRAMES) {
        a->one = a->mixed = true;
        plan_bytes = 0;
    } else if (magic == HYDK_TILE_MAGIC && plan_bytes >= sizeof(HydkTilePlan) && tp->total_bytes == plan_bytes && tp->num_frames == 1 &&
        max_frames <= HYDK_TILE_MAX_FRAMES) {
        a->one = true;
        const HydkTileFrame *fr = (const HydkTileFrame *)((const uint8_t *)plan + tp->frames_off);
        a->fixed = (uint64_t)fr->prefix_bytes + tp->shapes[fr->shape].lfglobal_bytes +
                   4u * (HYDK_TILE_HEAD_WORDS + HYDK_TILE_MID_WORDS + HYDK_TILE_TOC_WORDS) + (tp->shapes[fr->shape].tail_bits >> 3) + 16u;
    } else if (magic == HYDK_ASM_PLAN_MAGIC && plan_bytes >= sizeof(HydkAsmPlan) && ap->total_bytes == plan_bytes && ap->num_blobs == 1 &&
               ap->num_slots >= 1 && (uint64_t)ap->num_slots * (uint64_t)max_frames <= (uint64_t)kMaxSlots &&
               ap->num_presets * ap->clusters_per_preset <= 256 && ap->toc_n == 2 + ap->num_slots + ap->frame_groups &&
               ap->ntails <= HYDK_ASM_MAX_TAILS) {
        const uint32_t C = ap->num_presets * ap->clusters_per_preset;
        B.n = ap->num_slots;
        B.pieces_per_frame = 3 * ap->num_slots + 5;
        /* HFGlobal: the fixed fields, two bits, a configuration of <= 9 bits and a histogram of <= 73 words per cluster */
        B.hfg_words = (ap->hfpre_bits + 2u + C * 9u + 31u) / 32u + C * 73u + 2u;
        B.toc_words = ap->toc_n + 2u; /* entries of <= 32 bits */
        B.toc_n = ap->toc_n;
        head_words = (size_t)B.n * kHeadWords;
        uint32_t tail = 0;
        for (uint32_t i = 0; i < ap->ntails; i++)
            tail = ap->tail_bits[i] > tail ? ap->tail_bits[i] : tail;
        a->fixed = (uint64_t)ap->prefix_bytes + ap->lfglobal_bytes + 4ull * (B.hfg_words + B.toc_words) +
                   (uint64_t)B.n * (4u * kHeadWords + (tail >> 3) + 2u) + 16u;
    } else {
        delete a;
        return ST_API_ERROR;
    }
    if (a->one) {
        B.n = 1;
        B.pieces_per_frame = HYDK_TILE_PIECES;
        B.hfg_words = HYDK_TILE_MID_WORDS;
        B.toc_words = HYDK_TILE_TOC_WORDS;
        B.toc_n = 1;
        head_words = HYDK_TILE_HEAD_WORDS;
    }
    const size_t F = (size_t)max_frames;
    /* one arena: the plan (+ 16: the copy kernel reads whole words), then the arrays, each 16-byte aligned.  The
     * one-LF-group path keeps its sizes in registers and needs no counters: those arrays stay null */
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t off = at;
        at += (bytes + 15) & ~(size_t)15;
        return off;
    };
    const size_t o_plan = take(plan ? plan_bytes + 16 : 0), o_head = take(F * head_words * 4), o_hfg = take(F * B.hfg_words * 4),
                 o_toc = take(F * B.toc_words * 4), o_pieces = take(F * B.pieces_per_frame * sizeof(HydkPiece)),
                 o_result = take(F * 4 * 8), o_offsets = take((F + 1) * 8), o_range = take(4 * 8), o_status = take(F * 4);
    const bool one = a->one;
    const size_t o_head_bits = one ? 0 : take(F * B.n * 4), o_sizes = one ? 0 : take(F * B.toc_n * 8), o_slot_hf = one ? 0 : take(F * B.n * 8),
                 o_npieces = one ? 0 : take(F * 4), o_counters = one ? 0 : take(2 * F * 4);
    auto alloc = [&]() -> int {
        HYDK_TRY(a, hipSetDevice(device));
        HYDK_TRY(a, hipMalloc(&a->arena, at));
        uint8_t *m = a->arena;
        a->plan = plan ? m + o_plan : nullptr;
        B.head = (uint32_t *)(m + o_head);
        B.hfg = (uint32_t *)(m + o_hfg);
        B.toc = (uint32_t *)(m + o_toc);
        B.pieces = (HydkPiece *)(m + o_pieces);
        B.result = (uint64_t *)(m + o_result);
        B.offsets = (uint64_t *)(m + o_offsets);
        B.range = (uint64_t *)(m + o_range);
        B.status = (uint32_t *)(m + o_status);
        if (!one) {
            B.head_bits = (uint32_t *)(m + o_head_bits);
            B.sizes = (uint64_t *)(m + o_sizes);
            B.slot_hf = (uint64_t *)(m + o_slot_hf);
            B.npieces = (uint32_t *)(m + o_npieces);
            B.err = (uint32_t *)(m + o_counters); /* err and done: zero between batches */
            B.done = B.err + F;
            HYDK_TRY(a, hipMemset(B.err, 0, 2 * F * sizeof(uint32_t)));
        }
        if (plan)
            HYDK_TRY(a, hipMemcpy(a->plan, plan, plan_bytes, hipMemcpyHostToDevice));
        HYDK_TRY(a, hipStreamSynchronize(nullptr)); /* the memset runs in the NULL stream, which the context's stream does not wait for */
        HYDK_TRY(a, hipHostMalloc((void **)&a->h_result, (4 + F + 1 + F) * sizeof(uint64_t), hipHostMallocDefault));
        memset(a->h_result, 0, (4 + F + 1 + F) * sizeof(uint64_t));
        return ST_OK;
    };
    const int st = alloc();
    if (st != ST_OK) {
        hydk_batch_destroy(a);
        return st;
    }
    *out = a;
    return ST_OK;
}

/* scratch for batches of up to `max_frames` images of 1..28 LF groups each, `max_slots` LF groups in all, each image of
 * its own size: the arrays hold what hydk_tiles.h's HYDK_FRAMES_*_CAP say, whatever the sizes; the (frames) plan comes
 * with every batch (hydk_batch_set_plan) */
int hydk_batch_create_frames(int device, int max_frames, int max_slots, HydkBatchAsm **out) {
    if (!out)
        return ST_API_ERROR;
    *out = nullptr;
    if (max_frames < 1 || max_frames > HYDK_TILE_MAX_FRAMES || max_slots < max_frames || max_slots > kMaxSlots)
        return ST_API_ERROR;
    HydkBatchAsm *a = new (std::nothrow) HydkBatchAsm();
    if (!a)
        return ST_NOMEM;
    a->device = device;
    a->max_frames = max_frames;
    a->max_slots = max_slots;
    a->mixed = a->several = true;
    BatchScratch &B = a->B;
    const size_t F = (size_t)max_frames, N = (size_t)max_slots;
    B.hfg_cap = (uint32_t)HYDK_FRAMES_HFG_CAP(F, N);
    B.toc_cap = (uint32_t)HYDK_FRAMES_TOC_CAP(F, N);
    B.sizes_cap = (uint32_t)HYDK_FRAMES_SIZES_CAP(F, N);
    B.pieces_cap = (uint32_t)HYDK_FRAMES_PIECES_CAP(F, N);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t off = at;
        at += (bytes + 15) & ~(size_t)15;
        return off;
    };
    const size_t o_head = take(N * HYDK_FRAMES_HEAD_STRIDE * 4), o_hfg = take((size_t)B.hfg_cap * 4), o_toc = take((size_t)B.toc_cap * 4),
                 o_pieces = take((size_t)B.pieces_cap * sizeof(HydkPiece)), o_result = take(F * 4 * 8), o_offsets = take((F + 1) * 8),
                 o_range = take(4 * 8), o_status = take(F * 4), o_head_bits = take(N * 4), o_sizes = take((size_t)B.sizes_cap * 8), o_slot_hf = take(N * 8),
                 o_npieces = take(F * 4), o_counters = take(2 * F * 4);
    auto alloc = [&]() -> int {
        HYDK_TRY(a, hipSetDevice(device));
        HYDK_TRY(a, hipMalloc(&a->arena, at));
        uint8_t *m = a->arena;
        B.head = (uint32_t *)(m + o_head);
        B.hfg = (uint32_t *)(m + o_hfg);
        B.toc = (uint32_t *)(m + o_toc);
        B.pieces = (HydkPiece *)(m + o_pieces);
        B.result = (uint64_t *)(m + o_result);
        B.offsets = (uint64_t *)(m + o_offsets);
        B.range = (uint64_t *)(m + o_range);
        B.status = (uint32_t *)(m + o_status);
        B.head_bits = (uint32_t *)(m + o_head_bits);
        B.sizes = (uint64_t *)(m + o_sizes);
        B.slot_hf = (uint64_t *)(m + o_slot_hf);
        B.npieces = (uint32_t *)(m + o_npieces);
        B.err = (uint32_t *)(m + o_counters); /* err and done: zero between batches */
        B.done = B.err + F;
        HYDK_TRY(a, hipMemset(B.err, 0, 2 * F * sizeof(uint32_t)));
        HYDK_TRY(a, hipStreamSynchronize(nullptr));
        HYDK_TRY(a, hipHostMalloc((void **)&a->h_result, (4 + F + 1 + F) * sizeof(uint64_t), hipHostMallocDefault));
        memset(a->h_result, 0, (4 + F + 1 + F) * sizeof(uint64_t));
        return ST_OK;
    };
    const int st = alloc();
    if (st != ST_OK) {
        hydk_batch_destroy(a);
        return st;
    }
    *out = a;
    return ST_OK;
}

/* bytes a frame can add to its packed LF streams and HF sections: what the plan fixes and the scratch can hold */
uint64_t hydk_batch_fixed_bytes(HydkBatchAsm *a) { return a ? a->fixed : 0; }

/* a mixed assembler's plan for the batches that follow: `bytes` of a HydkMixedPlan, through the pinned buffer and one
 * asynchronous copy on `stream`, ahead of the assembly that reads it.  The caller has waited for the previous batch
 * (one batch in flight per object), so neither buffer is being read; both grow on demand, and wait for `stream` when they do */
/* a frames plan as the kernels will follow it: every table inside its bytes, every frame's slots, share of the scratch
 * and plan where the object can hold them, the workgroup table the frames of several LF groups part by part, in order */
static bool frames_plan_ok(const HydkBatchAsm *a, const uint8_t *plan, size_t bytes) {
    const HydkFramesPlan *fp = (const HydkFramesPlan *)plan;
    if (bytes < sizeof(HydkFramesPlan) || fp->magic != HYDK_FRAMES_MAGIC || fp->total_bytes != bytes || fp->num_frames < 1 ||
        fp->num_frames > (uint32_t)a->max_frames || fp->num_slots > (uint32_t)a->max_slots || fp->nshapes > fp->num_frames ||
        ((fp->shapes_off | fp->frames_off | fp->parts_off) & 3u) ||
        (uint64_t)fp->shapes_off + (uint64_t)fp->nshapes * sizeof(HydkTileShape) > bytes ||
        (uint64_t)fp->frames_off + (uint64_t)fp->num_frames * sizeof(HydkBatchFrame) > bytes ||
        (uint64_t)fp->parts_off + (uint64_t)fp->nparts * sizeof(uint32_t) > bytes)
        return false;
    const HydkBatchFrame *fr = (const HydkBatchFrame *)(plan + fp->frames_off);
    const uint32_t *parts = (const uint32_t *)(plan + fp->parts_off);
    const BatchScratch &B = a->B;
    uint32_t slot = 0, piece = 0, part = 0;
    for (uint32_t f = 0; f < fp->num_frames; f++) {
        const uint32_t n = fr[f].lf_groups;
        uint64_t sizes = 0;
        if (n < 1 || n > HYDK_FRAMES_MAX_LF_GROUPS || fr[f].first_slot != slot || fr[f].piece_base != piece)
            return false;
        if (fr[f].plan_off) {
            const HydkAsmPlan *ap = (const HydkAsmPlan *)(plan + fr[f].plan_off);
            if ((fr[f].plan_off & 15u) || (uint64_t)fr[f].plan_off + sizeof(HydkAsmPlan) > bytes || ap->magic != HYDK_ASM_PLAN_MAGIC ||
                (uint64_t)fr[f].plan_off + ap->total_bytes > bytes || ap->num_blobs != 1 || ap->num_slots != n || ap->blob_slots[0] != n ||
                ap->toc_n != 2 + n + ap->frame_groups || ap->ntails > HYDK_ASM_MAX_TAILS)
                return false;
            sizes = ap->toc_n;
            for (uint32_t i = 0; i <= n; i++, part++)
                if (part >= fp->nparts || parts[part] != (f << 8 | i))
                    return false;
        } else if (n != 1 || fr[f].one.shape >= fp->nshapes || fr[f].hfg_words < HYDK_TILE_MID_WORDS || fr[f].toc_words < HYDK_TILE_TOC_WORDS) {
            return false;
        }
        if ((uint64_t)fr[f].hfg_off + fr[f].hfg_words > B.hfg_cap || (uint64_t)fr[f].toc_off + fr[f].toc_words > B.toc_cap ||
            (uint64_t)fr[f].sizes_off + sizes > B.sizes_cap)
            return false;
        slot += n;
        piece += 3 * n + 5;
    }
    return slot == fp->num_slots && piece == fp->npieces && part == fp->nparts && piece <= B.pieces_cap && piece <= HYDK_COPY_MAX_PIECES;
}

int hydk_batch_set_plan(HydkBatchAsm *a, const void *plan, size_t bytes, void *stream) {
    const HydkMixedPlan *mp = (const HydkMixedPlan *)plan;
    if (a && a->several) {
        if (!plan || !frames_plan_ok(a, (const uint8_t *)plan, bytes))
            return hydk_fail(a, ST_API_ERROR, "bad frames plan");
    } else
    if (!a || !a->mixed || !plan || bytes < sizeof(HydkMixedPlan) || mp->magic != HYDK_MIXED_MAGIC || mp->total_bytes != bytes ||
        mp->num_frames < 1 || mp->num_frames > (uint32_t)a->max_frames || mp->nshapes < 1 || mp->nshapes > mp->num_frames ||
        (uint64_t)mp->shapes_off + (uint64_t)mp->nshapes * sizeof(HydkTileShape) > bytes ||
        (uint64_t)mp->frames_off + (uint64_t)mp->num_frames * sizeof(HydkTileFrame) > bytes)
        return hydk_fail(a, ST_API_ERROR, "bad mixed plan");
    HYDK_TRY(a, hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    a->plan_frames = 0;
    if (bytes > a->plan_cap) {
        HYDK_TRY(a, hipStreamSynchronize(st));
        if (a->plan)
            (void)hipFree(a->plan);
        if (a->h_plan)
            (void)hipHostFree(a->h_plan);
        a->plan = a->h_plan = nullptr;
        a->plan_cap = 0;
        const size_t cap = bytes + (bytes >> 1) + 4096; /* room for the next, larger list of sizes */
        HYDK_TRY(a, hipMalloc(&a->plan, cap + 16));     /* + 16: the copy kernel reads whole words */
        HYDK_TRY(a, hipHostMalloc((void **)&a->h_plan, cap, hipHostMallocDefault));
        a->plan_cap = cap;
    }
    memcpy(a->h_plan, plan, bytes);
    HYDK_TRY(a, hipMemcpyAsync(a->plan, a->h_plan, bytes, hipMemcpyHostToDevice, st));
    a->plan_frames = mp->num_frames; /* (both plan headers begin alike) */
    if (a->several) {
        const HydkFramesPlan *fp = (const HydkFramesPlan *)plan;
        a->plan_slots = fp->num_slots;
        a->plan_parts = fp->nparts;
        a->plan_pieces = fp->npieces;
    }
    return ST_OK;
}

/* enqueue the assembly of `frames` frames on `stream`, behind whatever fills the view `blob` (`blob_cap` readable bytes)
 * and its extents (hydamd_export_batch_owned over frames x n slots): three launches */
int hydk_batch_run(HydkBatchAsm *a, uint32_t frames, const void *blob, uint64_t blob_cap, const void *extents, void *stream) {
    if (!a || !blob || !extents || !a->out || frames < 1 || frames > (uint32_t)a->max_frames)
        return hydk_fail(a, ST_API_ERROR, "bad batch");
    if (((uintptr_t)a->out & 3u) || ((uintptr_t)blob & 15u))
        return hydk_fail(a, ST_API_ERROR, "output buffer must be 4-byte aligned, the view 16-byte aligned");
    HYDK_TRY(a, hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    const HydkTileExtent *ext = (const HydkTileExtent *)extents;
    if (a->mixed && frames > a->plan_frames)
        return hydk_fail(a, ST_API_ERROR, "the batch has more frames than its plan");
    uint32_t slots = frames * a->B.n, npieces = frames * a->B.pieces_per_frame;
    if (a->several) {
        if (frames != a->plan_frames)
            return hydk_fail(a, ST_API_ERROR, "the batch is not its plan's");
        slots = a->plan_slots;
        npieces = a->plan_pieces;
        if (a->plan_parts)
            hipLaunchKernelGGL(k_batch_prepare_frames, dim3(a->plan_parts), dim3(256), 0, st, (const uint8_t *)a->plan, (const uint8_t *)blob,
                               blob_cap, ext, frames, slots, a->B);
        HYDK_TRY(a, hipGetLastError());
        if (a->plan_parts < slots + frames) /* (the parts are n + 1 per frame of several LF groups: some frame has one) */
            hipLaunchKernelGGL(k_batch_prepare_frames_one, dim3(frames), dim3(64), 0, st, (const uint8_t *)a->plan, (const uint8_t *)blob, ext,
                               frames, slots, a->B);
    } else if (a->mixed)
        hipLaunchKernelGGL(k_batch_prepare_mixed, dim3(frames), dim3(64), 0, st, (const uint8_t *)a->plan, (const uint8_t *)blob, ext, frames, a->B);
    else if (a->one)
        hipLaunchKernelGGL(k_batch_prepare_one, dim3(frames), dim3(64), 0, st, (const uint8_t *)a->plan, (const uint8_t *)blob, ext, frames, a->B);
    else
        hipLaunchKernelGGL(k_batch_prepare, dim3(frames * (a->B.n + 1)), dim3(256), 0, st, (const uint8_t *)a->plan, (const uint8_t *)blob,
                           blob_cap, ext, frames, a->B);
    HYDK_TRY(a, hipGetLastError());
    hipLaunchKernelGGL(k_batch_place, dim3(1), dim3(256), 0, st, (const uint8_t *)blob, ext, frames, slots,
                       a->several ? (const uint8_t *)a->plan : (const uint8_t *)nullptr, a->B, a->out_cap, a->per_image ? 1u : 0u,
                       a->h_result, a->h_result + 4 + a->max_frames + 1);
    HYDK_TRY(a, hipGetLastError());
    HYDK_TRY(a, hydk::launch_pieces_copy(a->B.pieces, npieces, nullptr, a->B.range, a->out, st));
    return ST_OK;
}

/* the output buffer holds at least `bytes`.  Waits for `stream` when it has to be replaced. */
int hydk_batch_reserve(HydkBatchAsm *a, uint64_t bytes, void *stream) {
    if (!a)
        return ST_API_ERROR;
    if (bytes <= a->out_cap)
        return ST_OK;
    HYDK_TRY(a, hipSetDevice(a->device));
    HYDK_TRY(a, hipStreamSynchronize((hipStream_t)stream));
    if (a->out)
        (void)hipFree(a->out);
    a->out = nullptr;
    a->out_cap = 0;
    HYDK_TRY(a, hipMalloc(&a->out, bytes + 16));
    a->out_cap = bytes;
    return ST_OK;
}

/* per-image outcomes for the runs that follow: a frame with a flagged slot (the view's context in per-slot mode,
 * hydamd_set_bad_sample_per_slot) yields no bytes and a status word instead of failing the batch */
void hydk_batch_set_image_errors(HydkBatchAsm *a, int per_image) {
    if (a)
        a->per_image = per_image != 0;
}

/* the frames' status words: after the stream has been synchronised the host copy ([frames] of 64 bits, valid until the
 * next run), and the device copy ([frames] of 32 bits) */
const uint64_t *hydk_batch_status(HydkBatchAsm *a) { return a ? a->h_result + 4 + a->max_frames + 1 : nullptr; }
const uint32_t *hydk_batch_status_dev(HydkBatchAsm *a) { return a ? a->B.status : nullptr; }

const uint8_t *hydk_batch_out(HydkBatchAsm *a) { return a ? a->out : nullptr; }
const uint64_t *hydk_batch_offsets_dev(HydkBatchAsm *a) { return a ? a->B.offsets : nullptr; }

int hydk_batch_wait(HydkBatchAsm *a, void *stream) {
    if (!a)
        return ST_API_ERROR;
    HYDK_TRY(a, hipSetDevice(a->device));
    HYDK_TRY(a, hipStreamSynchronize((hipStream_t)stream));
    return ST_OK;
}

/* after the stream has been synchronised: the device's error word (HYDK_ASM_E_*), the bytes of all files, and the
 * host copy of the offsets table ([frames + 1], valid until the next run) */
int hydk_batch_result(HydkBatchAsm *a, uint32_t *err, uint64_t *total, const uint64_t **offsets) {
    if (!a)
        return ST_API_ERROR;
    if (err)
        *err = (uint32_t)a->h_result[0];
    if (total)
        *total = a->h_result[3];
    if (offsets)
        *offsets = a->h_result + 4;
    return ST_OK;
}

int hydk_batch_read(HydkBatchAsm *a, uint64_t from, uint8_t *dst, size_t n) {
    if (!a || !dst || !a->out || from + n > a->out_cap)
        return hydk_fail(a, ST_API_ERROR, "nothing to read");
    if (!n)
        return ST_OK;
    HYDK_TRY(a, hipSetDevice(a->device));
    HYDK_TRY(a, hipMemcpy(dst, a->out + from, n, hipMemcpyDeviceToHost));
    return ST_OK;
}

} /* extern "C" */
