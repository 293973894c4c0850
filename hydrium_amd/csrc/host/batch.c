/*
 * batch.c — a BATCH of one-frame images whose pixels already sit in HBM, every one a finished file, from C
 * (include/hydrium_amd.h, hydamd_batch_*).
 *
 * hydamd_encode_image_batch codes F independent pictures of one shape as one launch group — the fastest regime the
 * library has — and stops at sections and coded LF streams in the context's buffers.  Here one launch sequence behind
 * the batch's entropy stage (csrc/hip/assemble_batch.hip) turns them into F complete files, each what the reference
 * writes for that picture alone (libhydrium.c:172-203, encoder.c:968-1005), back to back in one device buffer with a
 * table of their offsets.
 *
 * This file's own: the PLAN — every byte that does not depend on the pixels, the same for every frame of a batch — built
 * once per object with the planners the other device-side assemblers use (assembler.c's for shapes of several LF groups,
 * tiled.c's shape planner for shapes of one); the argument checks; and the launch group, hydamd_encode_image_batch over
 * max_frames x n slots.  Everything behind the launch group — reservation, assembly, the wait and its rerun, results and
 * read-back, per-image outcomes — is the driver's, which the mixed-size batches share (batchrun.c).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "batchrun.h"
#include "bitio.h"
#include "frame.h"
#include "hydrium_amd.h"
#include "libhydrium/libhydrium.h"
#include "planbuf.h"
#include "../hyd_sample_fmt.h"

#include "../hip/hydk_tiles.h"

#ifndef HYDRIUM_EXPORT
#define HYDRIUM_EXPORT __attribute__((visibility("default")))
#endif

/* k_pieces_copy takes at most 2040 pieces (HYDK_COPY_MAX_PIECES): a batch has F (3 n + 5) of them, and with F n <= 255
 * that is at most 3 x 255 + 5 x 255 = 2040 (frames of one LF group: 8 F) */
#define BATCH_MAX_SLOTS HYDAMD_MAX_LF_GROUPS

/* ---------------------------------------------------------------------------------------------
 * the plan
 * ------------------------------------------------------------------------------------------- */
/* the prefix of a one-frame image of ONE LF group: its file header and the one-frame frame header with is_last, byte
 * aligned, appended to the plan buffer as frame record `fr` names it.  `bits` is the caller's to reuse.  Also what the
 * mixed-size batch object plans every one of its frames with (mixed.c). */
int hydk_plan_one_frame_prefix(Buf *buf, HydBits *bits, const HYDImageMetadata *md, const uint8_t *icc, size_t icc_size, HydkTileFrame *fr,
                               const char **err) {
    HydFrameLfg l;
    memset(&l, 0, sizeof(l));
    l.width = md->width;
    l.height = md->height;
    HydFrameShape shape;
    memset(&shape, 0, sizeof(shape));
    shape.one_frame = 1;
    shape.image_width = shape.frame_width = md->width;
    shape.image_height = shape.frame_height = md->height;
    shape.tile_count_x = shape.tile_count_y = 8;
    shape.lfg_count = 1;
    shape.lfg = &l;
    shape.is_last = 1;
    hb_reset(bits);
    int ret = hyd_internal_file_header(md, icc, icc_size, bits, err);
    if (!ret)
        ret = hyd_write_frame_header(bits, &shape, err);
    if (ret && !*err)
        *err = "frame header could not be written";
    if (ret)
        return ret;
    hb_align(bits);
    uint32_t nbits = 0;
    fr->prefix_off = (uint32_t)buf_add_bits(buf, bits, &nbits);
    fr->prefix_bytes = nbits >> 3;
    return HYD_OK;
}

/* shapes of one LF group: a tile plan (hydk_tiles.h) whose one frame is the whole image — file header, the one-frame
 * frame header, is_last */
static int plan_one_lf_group(const HYDImageMetadata *md, const uint8_t *icc, size_t icc_size, uint8_t **plan_out, size_t *plan_len,
                             const char **err) {
    int ret = HYD_OK;
    Buf buf = {0};
    HydBits bits, part;
    hb_init(&bits);
    hb_init(&part);
    HydkTilePlan plan;
    memset(&plan, 0, sizeof(plan));
    plan.magic = HYDK_TILE_MAGIC;
    plan.num_frames = 1;
    plan.nshapes = 1;
    buf_reserve(&buf, sizeof(plan));
    ret = hydk_tile_plan_shape(&buf, &bits, &part, md->width, md->height, &plan.shapes[0], err);
    const size_t frames_off = ret ? 0 : buf_reserve(&buf, sizeof(HydkTileFrame));
    plan.frames_off = (uint32_t)frames_off;
    if (!ret && !buf.failed) {
        HydkTileFrame fr;
        memset(&fr, 0, sizeof(fr));
        ret = hydk_plan_one_frame_prefix(&buf, &bits, md, icc, icc_size, &fr, err);
        if (!ret && !buf.failed)
            memcpy(buf.p + frames_off, &fr, sizeof(fr));
    }
    if (!ret && (buf.failed || bits.failed || part.failed)) {
        *err = "out of memory";
        ret = HYD_NOMEM;
    }
    if (!ret) {
        buf.len = (buf.len + 15) & ~(size_t)15;
        plan.total_bytes = (uint32_t)buf.len;
        memcpy(buf.p, &plan, sizeof(plan));
        *plan_out = buf.p;
        *plan_len = buf.len;
        buf.p = NULL;
    }
    free(buf.p);
    hb_free(&bits);
    hb_free(&part);
    return ret;
}

/* ---------------------------------------------------------------------------------------------
 * the object
 * ------------------------------------------------------------------------------------------- */
struct HydAmdBatch {
    int device, max_frames;
    size_t W, H, n; /* n: LF groups of a frame */
    HydBatchRun run;
};

static char g_create_error[256];

#define RUN(b) ((b) ? &(b)->run : NULL)

HYDRIUM_EXPORT const char *hydamd_batch_error(HydAmdBatch *b) { return b ? b->run.err : g_create_error; }

HYDRIUM_EXPORT void hydamd_batch_destroy(HydAmdBatch *b) {
    if (!b)
        return;
    hyd_batchrun_close(&b->run);
    free(b);
}

HYDRIUM_EXPORT HydAmdBatch *hydamd_batch_create(int device, const HYDImageMetadata *md, int max_frames, const uint8_t *icc, size_t icc_size,
                                                int *status) {
    int st = HYD_API_ERROR;
    HydAmdBatch *b = NULL;
    uint8_t *plan = NULL;
    uint32_t *ids = NULL;
    size_t plan_len = 0, n = 0;
    const char *err = NULL;
    g_create_error[0] = 0;
    if (!md) {
        err = "null metadata";
        goto out;
    }
    if (md->tile_size_shift_x >= 0 || md->tile_size_shift_y >= 0) {
        err = "a batch holds one-frame images: both tile_size_shift_x and tile_size_shift_y must be -1";
        goto out;
    }
    if (!md->width || !md->height || md->width > (1u << 30) || md->height > (1u << 30)) {
        err = "width or height out of bounds";
        goto out;
    }
    n = (((size_t)md->width + 2047) >> 11) * (((size_t)md->height + 2047) >> 11);
    if (n > HYDAMD_MAX_LF_GROUPS || n == 128) {
        err = "unsupported number of LF groups per frame (1..255 except 128)";
        goto out;
    }
    if (max_frames < 1) {
        err = "max_frames must be at least 1";
        goto out;
    }
    if ((size_t)max_frames * n > BATCH_MAX_SLOTS) {
        err = "max_frames times the LF groups of a frame must not exceed 255 (the slots of one context)";
        goto out;
    }
    if (hydamd_device_count() < 1 || device < 0 || device >= hydamd_device_count()) {
        st = HYD_INTERNAL_ERROR;
        err = "no usable HIP device";
        goto out;
    }
    if ((st = hydk_plan_check_metadata(md, g_create_error, sizeof(g_create_error))) != 0)
        goto out;
    if (n == 1) {
        st = plan_one_lf_group(md, icc, icc_size, &plan, &plan_len, &err);
    } else { /* one blob (the batch view), its LF groups in raster order */
        const uint32_t slots = (uint32_t)n;
        ids = malloc(n * sizeof(*ids));
        for (size_t i = 0; ids && i < n; i++)
            ids[i] = (uint32_t)i;
        st = ids ? hydk_plan_frame(md, 1, 1, 1, &slots, ids, icc, icc_size, &plan, &plan_len, &err) : HYD_NOMEM;
    }
    if (st)
        goto out;
    b = calloc(1, sizeof(*b));
    if (!b) {
        st = HYD_NOMEM;
        goto out;
    }
    b->device = device;
    b->max_frames = max_frames;
    b->W = md->width;
    b->H = md->height;
    b->n = n;
    st = hyd_batchrun_open(&b->run, device, (int)((size_t)max_frames * n), md->linear_light != 0, "hydamd_batch_result", g_create_error,
                           sizeof(g_create_error));
    if (!st)
        st = hyd_batchrun_adopt(&b->run, hydk_batch_create(device, max_frames, plan, plan_len, &b->run.as), g_create_error,
                                sizeof(g_create_error));
    if (st) {
        free(b);
        b = NULL;
        goto out;
    }
    /* what the plan and the assembler's scratch add to every frame: fixed once the assembler of this one shape exists */
    b->run.fixed = (uint64_t)max_frames * hydk_batch_fixed_bytes(b->run.as);
out:
    if (err && !g_create_error[0])
        snprintf(g_create_error, sizeof(g_create_error), "%s", err);
    free(plan);
    free(ids);
    if (status)
        *status = st;
    return b;
}

HYDRIUM_EXPORT int hydamd_encode_batch(HydAmdBatch *b, int frames, const void *const *src, ptrdiff_t row_stride, ptrdiff_t pixel_stride,
                                       int sample_fmt) {
    if (!b)
        return HYD_API_ERROR;
    HydBatchRun *r = &b->run;
    if (frames < 1 || frames > b->max_frames)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "frames must be between 1 and max_frames", NULL);
    if (!src)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "null pixel pointer", NULL);
    for (int i = 0; i < 3 * frames; i++)
        if (!src[i])
            return hyd_batchrun_fail(r, HYD_API_ERROR, "null pixel pointer", NULL);
    const char *refusal = NULL; /* every frame to its layout, then the pitch */
    for (int f = 0; f < frames && !refusal; f++)
        refusal = hyd_fmt_refusal(sample_fmt, src + 3 * f, pixel_stride, 0);
    if (refusal || (refusal = hyd_fmt_refusal(sample_fmt, NULL, pixel_stride, b->W)) != NULL)
        return hyd_batchrun_fail(r, HYD_API_ERROR, refusal, NULL);
    int st = hyd_batchrun_busy(r);
    if (st)
        return st;
    r->err[0] = 0;
    r->have_result = 0;
    r->frames = frames;
    r->slots = (int)((size_t)frames * b->n);
    if ((st = hyd_batchrun_reserve(r)) != 0) /* nothing of this batch is in the stream yet */
        return st;
    r->in_flight = 1;
    st = hydamd_encode_image_batch(r->ctx, frames, src, row_stride, pixel_stride, sample_fmt, b->W, b->H);
    if (st)
        st = hyd_batchrun_fail(r, st, "batch", hydamd_error(r->ctx));
    else
        st = hyd_batchrun_assemble(r);
    if (st)
        hyd_batchrun_drain(r);
    return st;
}

HYDRIUM_EXPORT int hydamd_batch_result(HydAmdBatch *b, size_t *total_bytes) { return hyd_batchrun_result(RUN(b), total_bytes); }

HYDRIUM_EXPORT int hydamd_batch_offsets(HydAmdBatch *b, uint64_t *offsets) { return hyd_batchrun_offsets(RUN(b), offsets); }

HYDRIUM_EXPORT int hydamd_batch_read(HydAmdBatch *b, int frame, uint8_t *dst, size_t capacity) {
    return hyd_batchrun_read(RUN(b), frame, dst, capacity);
}

HYDRIUM_EXPORT const uint8_t *hydamd_batch_device(HydAmdBatch *b) { return hyd_batchrun_device(RUN(b)); }

HYDRIUM_EXPORT const uint64_t *hydamd_batch_offsets_device(HydAmdBatch *b) { return hyd_batchrun_offsets_device(RUN(b)); }

HYDRIUM_EXPORT int hydamd_batch_set_image_errors(HydAmdBatch *b, int per_image) { return hyd_batchrun_set_image_errors(RUN(b), per_image); }

HYDRIUM_EXPORT int hydamd_batch_image_status(HydAmdBatch *b, uint32_t *status) { return hyd_batchrun_image_status(RUN(b), status); }

HYDRIUM_EXPORT const uint32_t *hydamd_batch_image_status_device(HydAmdBatch *b) { return hyd_batchrun_image_status_device(RUN(b)); }

HYDRIUM_EXPORT unsigned hydamd_batch_overflow_reruns(HydAmdBatch *b) { return b ? b->run.reruns : 0; }

/* ---------------------------------------------------------------------------------------------
 * CPU-only test hook: the plan of a batch of one-LF-group frames (plan_one_lf_group above, the product's own) and the
 * batched layout (hydk_tiles.h compiled for the host, tiled.c's hydt_layout_from_streams) on results handed in as
 * hydt_tiles_from_streams takes them, one frame per picture, every one laid out by the plan's ONE frame record — what
 * k_batch_prepare_one, k_batch_place and k_pieces_copy do, held to frame.c by tests/test_batch_layout.py.  (Shapes of
 * several LF groups go through hydk_asm_writers.h, which has no host build: those are held on the GPU only.)
 * ------------------------------------------------------------------------------------------- */
#ifdef HYD_TEST_HOOKS
__attribute__((visibility("default"))) int hydt_batch_from_streams(const HYDImageMetadata *md, size_t nframes, const HydAmdLfStream *lf,
                                                                   const uint32_t *freq, const uint32_t *alphabet, const uint32_t *group_bits,
                                                                   const uint32_t *max_alphabet, const uint8_t *payload, size_t payload_len,
                                                                   uint64_t *frame_offsets /* [nframes + 1] or NULL */, uint8_t **out,
                                                                   size_t *out_len, const char **err) {
    static const char *none = NULL;
    const char **e = err ? err : &none;
    uint8_t *plan = NULL;
    size_t plan_len = 0;
    *e = NULL;
    if (!md || nframes < 1 || nframes > HYDK_TILE_MAX_FRAMES || md->width > 2048 || md->height > 2048) {
        *e = "between 1 and 255 frames of one LF group";
        return HYD_API_ERROR;
    }
    int ret = plan_one_lf_group(md, NULL, 0, &plan, &plan_len, e);
    if (ret)
        return ret;
    const HydkTilePlan *hp = (const HydkTilePlan *)plan;
    HydkTileFrame *frames = malloc(nframes * sizeof(*frames));
    if (!frames) {
        free(plan);
        return HYD_NOMEM;
    }
    for (size_t f = 0; f < nframes; f++) /* k_batch_prepare_one: every frame is frame 0 of the tile plan */
        frames[f] = ((const HydkTileFrame *)(plan + hp->frames_off))[0];
    ret = hydt_layout_from_streams(plan, frames, hp->shapes, nframes, lf, freq, alphabet, group_bits, max_alphabet, payload, payload_len,
                                   frame_offsets, out, out_len, e);
    free(frames);
    free(plan);
    return ret;
}
#endif /* HYD_TEST_HOOKS */
