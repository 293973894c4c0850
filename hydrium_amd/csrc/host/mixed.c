/*
 * mixed.c — a batch of one-frame images EACH OF ITS OWN SIZE whose pixels already sit in HBM, every one a finished file,
 * from C (include/hydrium_amd.h, hydamd_mixed_*).
 *
 * A context takes LF groups of different sizes in one launch group (tiled.c codes a tile-mode image's ragged tiles that
 * way), and hydk_tiles.h lays frames of different shapes side by side.  Here both serve a queue of pictures of many
 * sizes — thumbnails, crops, the output of a decoder — each at most 2048 x 2048 pixels, ONE LF group: the launch group is
 * tiled.c's (hydamd_begin_batch(ctx, 1, frames), one hydamd_encode_lf_group per image with its own pointers, strides and
 * size), the assembly and the protocol are batch.c's (csrc/hip/assemble_batch.hip: every frame a complete file — what the
 * reference writes for that picture alone with both tile_size_shift -1 — back to back in one device buffer, the table of
 * their offsets beside it; the host waits once per batch, hydamd_sync reruns a batch that outgrew the context's buffers
 * and the assembly is repeated behind it; after a failure the stream is drained before the call returns).
 *
 * What is this file's own is the PLAN: no two batches need the same one.  It holds a shape record per DISTINCT size of
 * the batch (tiled.c's shape planner) and a frame record per image whose prefix is that image's file header and one-frame
 * frame header (batch.c's prefix planner) — built per batch on the host, uploaded in the stream ahead of the assembly,
 * and neither rebuilt nor uploaded when a batch's list of sizes equals the previous batch's.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bitio.h"
#include "frame.h"
#include "hydrium_amd.h"
#include "libhydrium/libhydrium.h"
#include "planbuf.h"

#include "../hip/hydk_tiles.h"

#ifndef HYDRIUM_EXPORT
#define HYDRIUM_EXPORT __attribute__((visibility("default")))
#endif

#define MIXED_DEFAULT_FRAMES 32
#define MIXED_MAX_SIDE 2048u /* one LF group */

typedef struct HydkBatchAsm HydkBatchAsm; /* assemble_batch.hip */
int hydk_batch_create(int device, int max_frames, const void *plan, size_t plan_bytes, HydkBatchAsm **out);
void hydk_batch_destroy(HydkBatchAsm *a);
const char *hydk_batch_error(HydkBatchAsm *a);
int hydk_batch_set_plan(HydkBatchAsm *a, const void *plan, size_t bytes, void *stream);
int hydk_batch_run(HydkBatchAsm *a, uint32_t frames, const void *blob, uint64_t blob_cap, const void *extents, void *stream);
int hydk_batch_reserve(HydkBatchAsm *a, uint64_t bytes, void *stream);
const uint8_t *hydk_batch_out(HydkBatchAsm *a);
const uint64_t *hydk_batch_offsets_dev(HydkBatchAsm *a);
int hydk_batch_wait(HydkBatchAsm *a, void *stream);
int hydk_batch_result(HydkBatchAsm *a, uint32_t *err, uint64_t *total, const uint64_t **offsets);
int hydk_batch_read(HydkBatchAsm *a, uint64_t from, uint8_t *dst, size_t n);

/* ---------------------------------------------------------------------------------------------
 * the plan
 * ------------------------------------------------------------------------------------------- */
typedef struct MixedSize {
    uint32_t w, h;
} MixedSize;

/* The mixed plan (hydk_tiles.h, HydkMixedPlan) of `n` images of sizes sz[0 .. n): a shape record per distinct size, a
 * frame record per image.  *fixed: the bytes these frames can add to their packed LF streams and HF sections — what the
 * plan contributes and what the assembler's scratch can hold, as hydk_batch_fixed_bytes states it for one shape. */
static int build_plan(int n, const MixedSize *sz, int linear_light, uint8_t **plan_out, size_t *plan_len, uint64_t *fixed, const char **err) {
    int ret = HYD_OK;
    Buf buf = {0};
    HydBits bits, part;
    hb_init(&bits);
    hb_init(&part);
    HydkMixedPlan plan;
    HydkTileShape *shapes = calloc((size_t)n, sizeof(*shapes));
    HydkTileFrame *frames = calloc((size_t)n, sizeof(*frames));
    MixedSize *distinct = calloc((size_t)n, sizeof(*distinct));
    memset(&plan, 0, sizeof(plan));
    plan.magic = HYDK_MIXED_MAGIC;
    plan.num_frames = (uint32_t)n;
    if (!shapes || !frames || !distinct) {
        *err = "out of memory";
        ret = HYD_NOMEM;
    }
    for (int f = 0; f < n && !ret; f++) { /* at most 255 images: the quadratic search is a few thousand comparisons */
        uint32_t s = 0;
        while (s < plan.nshapes && (distinct[s].w != sz[f].w || distinct[s].h != sz[f].h))
            s++;
        if (s == plan.nshapes)
            distinct[plan.nshapes++] = sz[f];
        frames[f].shape = s;
    }
    buf_reserve(&buf, sizeof(plan));
    plan.shapes_off = (uint32_t)buf_reserve(&buf, (size_t)plan.nshapes * sizeof(*shapes));
    plan.frames_off = (uint32_t)buf_reserve(&buf, (size_t)n * sizeof(*frames));
    for (uint32_t s = 0; s < plan.nshapes && !ret; s++)
        ret = hydk_tile_plan_shape(&buf, &bits, &part, distinct[s].w, distinct[s].h, &shapes[s], err);
    *fixed = 0;
    for (int f = 0; f < n && !ret; f++) {
        HYDImageMetadata md;
        memset(&md, 0, sizeof(md));
        md.width = sz[f].w;
        md.height = sz[f].h;
        md.linear_light = linear_light;
        md.tile_size_shift_x = md.tile_size_shift_y = -1;
        ret = hydk_plan_one_frame_prefix(&buf, &bits, &md, NULL, 0, &frames[f], err);
        const HydkTileShape *sh = &shapes[frames[f].shape];
        *fixed += (uint64_t)frames[f].prefix_bytes + sh->lfglobal_bytes + 4u * (HYDK_TILE_HEAD_WORDS + HYDK_TILE_MID_WORDS + HYDK_TILE_TOC_WORDS) +
                  (sh->tail_bits >> 3) + 16u;
    }
    if (!ret && (buf.failed || bits.failed || part.failed)) {
        *err = "out of memory";
        ret = HYD_NOMEM;
    }
    if (!ret) {
        buf.len = (buf.len + 15) & ~(size_t)15;
        plan.total_bytes = (uint32_t)buf.len;
        memcpy(buf.p, &plan, sizeof(plan));
        memcpy(buf.p + plan.shapes_off, shapes, (size_t)plan.nshapes * sizeof(*shapes));
        memcpy(buf.p + plan.frames_off, frames, (size_t)n * sizeof(*frames));
        *plan_out = buf.p;
        *plan_len = buf.len;
        buf.p = NULL;
    }
    free(buf.p);
    free(shapes);
    free(frames);
    free(distinct);
    hb_free(&bits);
    hb_free(&part);
    return ret;
}

/* ---------------------------------------------------------------------------------------------
 * the object
 * ------------------------------------------------------------------------------------------- */
struct HydAmdMixed {
    int device, max_frames, linear_light;
    HydAmdContext *ctx;
    HydkBatchAsm *as;
    int frames; /* of the batch in flight / finished */
    int in_flight, have_result;
    int planned;                             /* images of the plan on the device (0: none), their sizes: */
    MixedSize sizes[HYDK_TILE_MAX_FRAMES];
    uint64_t fixed;                          /* that plan's share of the output reservation */
    size_t total;
    uint64_t offsets[HYDK_TILE_MAX_FRAMES + 1];
    unsigned reruns;
    char err[256];
};

static char g_create_error[256];

static int fail(HydAmdMixed *m, int code, const char *what, const char *detail) {
    snprintf(m->err, sizeof(m->err), "%s%s%s", what, detail && *detail ? ": " : "", detail && *detail ? detail : "");
    return code;
}

HYDRIUM_EXPORT const char *hydamd_mixed_error(HydAmdMixed *m) { return m ? m->err : g_create_error; }

HYDRIUM_EXPORT void hydamd_mixed_destroy(HydAmdMixed *m) {
    if (!m)
        return;
    if (m->ctx) {
        (void)hydamd_sync(m->ctx);
        hydk_batch_destroy(m->as);
        hydamd_destroy(m->ctx);
    }
    free(m);
}

HYDRIUM_EXPORT HydAmdMixed *hydamd_mixed_create(int device, int max_frames, int linear_light, int *status) {
    int st = HYD_API_ERROR;
    HydAmdMixed *m = NULL;
    g_create_error[0] = 0;
    if (max_frames < 0 || max_frames > HYDK_TILE_MAX_FRAMES) {
        snprintf(g_create_error, sizeof(g_create_error), "max_frames must be between 0 and 255 (the slots of one context; 0: the default, 32)");
        goto out;
    }
    if (hydamd_device_count() < 1 || device < 0 || device >= hydamd_device_count()) {
        st = HYD_INTERNAL_ERROR;
        snprintf(g_create_error, sizeof(g_create_error), "no usable HIP device");
        goto out;
    }
    m = calloc(1, sizeof(*m));
    if (!m) {
        st = HYD_NOMEM;
        goto out;
    }
    m->device = device;
    m->max_frames = max_frames ? max_frames : MIXED_DEFAULT_FRAMES;
    m->linear_light = linear_light != 0;
    m->ctx = hydamd_create(device, m->max_frames, m->linear_light, 0, &st);
    if (!m->ctx) {
        snprintf(g_create_error, sizeof(g_create_error), "%s", hydamd_error(NULL));
        free(m);
        m = NULL;
        goto out;
    }
    if ((st = hydamd_set_lf_coder(m->ctx, 2)) != 0 || (st = hydamd_set_rans_waves(m->ctx, 5)) != 0) {
        snprintf(g_create_error, sizeof(g_create_error), "%s", hydamd_error(m->ctx));
    } else if ((st = hydk_batch_create(device, m->max_frames, NULL, 0, &m->as)) != 0) {
        snprintf(g_create_error, sizeof(g_create_error), "the batch assembler could not be created (status %d)", st);
    }
    if (st) {
        hydamd_destroy(m->ctx);
        free(m);
        m = NULL;
        goto out;
    }
    st = HYD_OK;
out:
    if (status)
        *status = st;
    return m;
}

/* after a failure once work was enqueued: nothing of this object is left running when the call returns */
static void drain(HydAmdMixed *m) {
    (void)hydamd_sync(m->ctx);
    (void)hydk_batch_wait(m->as, hydamd_get_stream(m->ctx));
    m->in_flight = 0;
}

/* The output holds whatever the context's buffers can — their bound for ALL the object's slots, so that only a context
 * that has enlarged its buffers (a rerun) or a plan of larger prefixes makes it grow — plus what THIS batch's plan and
 * the assembler's scratch add.  Replacing the buffer waits for the stream, so it is reserved BEFORE a batch is enqueued,
 * and looked at again before every assembly. */
static int reserve_output(HydAmdMixed *m) {
    const uint64_t want = (uint64_t)hydamd_blob_bound(m->ctx, m->max_frames) + m->fixed;
    const int st = hydk_batch_reserve(m->as, want, hydamd_get_stream(m->ctx));
    return st ? fail(m, st, "output buffer", hydk_batch_error(m->as)) : HYD_OK;
}

/* the batch's plan on the device: the previous batch's when its list of sizes is the same */
static int plan_batch(HydAmdMixed *m, int frames, const HydAmdImageDesc *images) {
    int same = frames == m->planned;
    for (int f = 0; f < frames && same; f++)
        same = m->sizes[f].w == images[f].width && m->sizes[f].h == images[f].height;
    if (same)
        return HYD_OK;
    uint8_t *plan = NULL;
    size_t plan_len = 0;
    const char *err = NULL;
    m->planned = 0;
    for (int f = 0; f < frames; f++) {
        m->sizes[f].w = (uint32_t)images[f].width;
        m->sizes[f].h = (uint32_t)images[f].height;
    }
    int st = build_plan(frames, m->sizes, m->linear_light, &plan, &plan_len, &m->fixed, &err);
    if (st)
        return fail(m, st, "plan", err);
    st = hydk_batch_set_plan(m->as, plan, plan_len, hydamd_get_stream(m->ctx));
    free(plan);
    if (st)
        return fail(m, st, "plan", hydk_batch_error(m->as));
    m->planned = frames;
    return HYD_OK;
}

/* the batch's results as a view, and its assembly behind them */
static int assemble(HydAmdMixed *m) {
    const void *blob = NULL, *ext = NULL;
    size_t cap = 0;
    void *stream = hydamd_get_stream(m->ctx);
    int st = reserve_output(m);
    if (st)
        return st;
    st = hydamd_export_batch_owned(m->ctx, m->frames, &blob, &cap, &ext);
    if (st)
        return fail(m, st, "batch view", hydamd_error(m->ctx));
    st = hydk_batch_run(m->as, (uint32_t)m->frames, blob, cap, ext, stream);
    return st ? fail(m, st, "batch assembly", hydk_batch_error(m->as)) : HYD_OK;
}

/* the launch group: tiled.c's, every image an LF group of its own size in a slot of its own */
static int enqueue(HydAmdMixed *m, const HydAmdImageDesc *images, int sample_fmt) {
    int st = hydamd_begin_batch(m->ctx, 1, m->frames);
    if (st)
        return fail(m, st, "begin launch group", hydamd_error(m->ctx));
    for (int f = 0; f < m->frames; f++) {
        const HydAmdImageDesc *d = &images[f];
        if ((st = hydamd_encode_lf_group(m->ctx, f, d->src, d->row_stride, d->pixel_stride, sample_fmt, d->width, d->height, 0)) != 0)
            return fail(m, st, "image", hydamd_error(m->ctx));
    }
    if ((st = hydamd_finish_frame(m->ctx, m->frames)) != 0)
        return fail(m, st, "launch group", hydamd_error(m->ctx));
    return assemble(m);
}

HYDRIUM_EXPORT int hydamd_encode_mixed(HydAmdMixed *m, int frames, const HydAmdImageDesc *images, int sample_fmt) {
    if (!m)
        return HYD_API_ERROR;
    if (frames < 1 || frames > m->max_frames)
        return fail(m, HYD_API_ERROR, "frames must be between 1 and max_frames", NULL);
    if (!images)
        return fail(m, HYD_API_ERROR, "null image descriptors", NULL);
    for (int f = 0; f < frames; f++) {
        if (!images[f].src[0] || !images[f].src[1] || !images[f].src[2])
            return fail(m, HYD_API_ERROR, "null pixel pointer", NULL);
        if (!images[f].width || !images[f].height || images[f].width > MIXED_MAX_SIDE || images[f].height > MIXED_MAX_SIDE)
            return fail(m, HYD_API_ERROR, "every image of a mixed batch must be between 1 and 2048 pixels in each direction", NULL);
    }
    if (sample_fmt != HYD_UINT8 && sample_fmt != HYD_UINT16 && sample_fmt != HYD_FLOAT32)
        return fail(m, HYD_API_ERROR, "Invalid Sample Format", NULL);
    if (m->in_flight)
        return fail(m, HYD_API_ERROR, "a batch is in flight: hydamd_mixed_result first", NULL);
    m->err[0] = 0;
    m->have_result = 0;
    m->frames = frames;
    int st = plan_batch(m, frames, images); /* nothing of this batch is in the stream yet but, at most, its plan */
    if (!st && (st = reserve_output(m)) != 0) /* the plan's copy may be in the stream, out of the pinned buffer the next plan is written to */
        (void)hydk_batch_wait(m->as, hydamd_get_stream(m->ctx));
    if (st)
        return st;
    m->in_flight = 1;
    st = enqueue(m, images, sample_fmt);
    if (st)
        drain(m);
    return st;
}

/* the batch in flight: wait, let hydamd_sync rerun it if it outgrew a buffer, and see its frames into their files */
static int settle(HydAmdMixed *m) {
    const unsigned before = hydamd_overflow_reruns(m->ctx);
    int st = hydamd_sync(m->ctx);
    if (st)
        return fail(m, st, "batch", hydamd_error(m->ctx));
    m->reruns += hydamd_overflow_reruns(m->ctx) - before;
    for (int attempt = 0; attempt < 4; attempt++) {
        uint32_t err = 0;
        uint64_t total = 0;
        const uint64_t *offsets = NULL;
        hydk_batch_result(m->as, &err, &total, &offsets);
        if (!err) {
            m->total = (size_t)total;
            memcpy(m->offsets, offsets, ((size_t)m->frames + 1) * sizeof(uint64_t));
            return HYD_OK;
        }
        if (err & HYDK_ASM_E_NAN)
            return fail(m, HYD_API_ERROR, "Invalid NaN Float", NULL);
        if (err & HYDK_ASM_E_SPACE) /* the output was sized from the context's capacities */
            return fail(m, HYD_INTERNAL_ERROR, "the batch's files are larger than the bound of their output buffer", NULL);
        if (err & (HYDK_ASM_E_BLOB | HYDK_ASM_E_SLOT | HYDK_ASM_E_HEAD | HYDK_ASM_E_SIZE | HYDK_ASM_E_SCRATCH))
            return fail(m, HYD_INTERNAL_ERROR, "batch assembly failed on the device", NULL);
        /* RETRY: the assembly saw the first run's incomplete results (hydamd_sync has rerun the batch since): the view
         * and the same launches again, with the plan that is still on the device, into an output sized for the enlarged context */
        if ((st = assemble(m)) != 0)
            return st;
        if ((st = hydk_batch_wait(m->as, hydamd_get_stream(m->ctx))) != 0)
            return fail(m, st, "batch assembly", hydk_batch_error(m->as));
    }
    return fail(m, HYD_INTERNAL_ERROR, "a batch is still incomplete after its rerun", NULL);
}

HYDRIUM_EXPORT int hydamd_mixed_result(HydAmdMixed *m, size_t *total_bytes) {
    if (!m)
        return HYD_API_ERROR;
    if (!m->have_result) {
        if (!m->in_flight)
            return fail(m, HYD_API_ERROR, "no batch in flight", NULL);
        const int st = settle(m);
        if (st) {
            drain(m);
            return st;
        }
        m->in_flight = 0;
        m->have_result = 1;
    }
    if (total_bytes)
        *total_bytes = m->total;
    return HYD_OK;
}

HYDRIUM_EXPORT int hydamd_mixed_offsets(HydAmdMixed *m, uint64_t *offsets) {
    if (!m || !m->have_result)
        return m ? fail(m, HYD_API_ERROR, "no finished batch: hydamd_mixed_result first", NULL) : HYD_API_ERROR;
    if (!offsets)
        return fail(m, HYD_API_ERROR, "null output pointer", NULL);
    memcpy(offsets, m->offsets, ((size_t)m->frames + 1) * sizeof(uint64_t));
    return HYD_OK;
}

HYDRIUM_EXPORT int hydamd_mixed_read(HydAmdMixed *m, int frame, uint8_t *dst, size_t capacity) {
    if (!m || !m->have_result)
        return m ? fail(m, HYD_API_ERROR, "no finished batch: hydamd_mixed_result first", NULL) : HYD_API_ERROR;
    if (!dst)
        return fail(m, HYD_API_ERROR, "null output pointer", NULL);
    if (frame < -1 || frame >= m->frames)
        return fail(m, HYD_API_ERROR, "no such frame in the batch", NULL);
    const uint64_t from = frame < 0 ? 0 : m->offsets[frame], to = frame < 0 ? m->total : m->offsets[frame + 1];
    if (capacity < to - from)
        return fail(m, HYD_API_ERROR, "output buffer too small", NULL);
    const int st = hydk_batch_read(m->as, from, dst, (size_t)(to - from));
    return st ? fail(m, st, "read-back", hydk_batch_error(m->as)) : HYD_OK;
}

HYDRIUM_EXPORT const uint8_t *hydamd_mixed_device(HydAmdMixed *m) { return m && m->have_result ? hydk_batch_out(m->as) : NULL; }

HYDRIUM_EXPORT const uint64_t *hydamd_mixed_offsets_device(HydAmdMixed *m) {
    return m && m->have_result ? hydk_batch_offsets_dev(m->as) : NULL;
}

HYDRIUM_EXPORT unsigned hydamd_mixed_overflow_reruns(HydAmdMixed *m) { return m ? m->reruns : 0; }

/* ---------------------------------------------------------------------------------------------
 * CPU-only test hook: the mixed plan (build_plan above, the product's own) and the batched layout (hydk_tiles.h compiled
 * for the host, tiled.c's hydt_layout_from_streams) on results handed in as hydt_tiles_from_streams takes them, one frame
 * per image — what k_batch_prepare_mixed, k_batch_place and k_pieces_copy do, frame by frame, held to frame.c by
 * tests/test_mixed_sections.py.
 * ------------------------------------------------------------------------------------------- */
#ifdef HYD_TEST_HOOKS
#define HYDT_EXPORT __attribute__((visibility("default")))
HYDT_EXPORT int hydt_mixed_from_streams(size_t n, const uint32_t *widths, const uint32_t *heights, const HydAmdLfStream *lf,
                                        const uint32_t *freq, const uint32_t *alphabet, const uint32_t *group_bits,
                                        const uint32_t *max_alphabet, const uint8_t *payload, size_t payload_len,
                                        uint64_t *frame_offsets /* [n + 1] or NULL */, uint8_t **out, size_t *out_len, const char **err) {
    static const char *none = NULL;
    const char **e = err ? err : &none;
    MixedSize sz[HYDK_TILE_MAX_FRAMES];
    uint8_t *plan = NULL;
    size_t plan_len = 0;
    uint64_t fixed = 0;
    *e = NULL;
    if (n < 1 || n > HYDK_TILE_MAX_FRAMES) {
        *e = "between 1 and 255 images";
        return HYD_API_ERROR;
    }
    for (size_t f = 0; f < n; f++) {
        if (!widths[f] || !heights[f] || widths[f] > MIXED_MAX_SIDE || heights[f] > MIXED_MAX_SIDE) {
            *e = "every image of a mixed batch must be between 1 and 2048 pixels in each direction";
            return HYD_API_ERROR;
        }
        sz[f].w = widths[f];
        sz[f].h = heights[f];
    }
    int ret = build_plan((int)n, sz, 0, &plan, &plan_len, &fixed, e);
    if (ret)
        return ret;
    const HydkMixedPlan *hp = (const HydkMixedPlan *)plan;
    const HydkTileFrame *frames = (const HydkTileFrame *)(plan + hp->frames_off);
    /* (k_batch_prepare_mixed's own checks of the plan — HYDK_ASM_E_BLOB, HYDK_ASM_E_SLOT — have no counterpart here: the
     * planner never writes a plan that trips them, and no test does) */
    ret = hydt_layout_from_streams(plan, frames, (const HydkTileShape *)(plan + hp->shapes_off), n, lf, freq, alphabet, group_bits,
                                       max_alphabet, payload, payload_len, frame_offsets, out, out_len, e);
    free(plan);
    return ret;
}

/* what the planner made of a list of sizes: its shape records (one per DISTINCT size) and the plan's bytes */
HYDT_EXPORT int hydt_mixed_plan_counts(size_t n, const uint32_t *widths, const uint32_t *heights, uint32_t *nshapes, size_t *plan_bytes) {
    MixedSize sz[HYDK_TILE_MAX_FRAMES];
    uint8_t *plan = NULL;
    size_t plan_len = 0;
    uint64_t fixed = 0;
    const char *e = NULL;
    if (n < 1 || n > HYDK_TILE_MAX_FRAMES)
        return HYD_API_ERROR;
    for (size_t f = 0; f < n; f++) {
        sz[f].w = widths[f];
        sz[f].h = heights[f];
    }
    const int ret = build_plan((int)n, sz, 0, &plan, &plan_len, &fixed, &e);
    if (!ret) {
        *nshapes = ((const HydkMixedPlan *)plan)->nshapes;
        *plan_bytes = plan_len;
    }
    free(plan);
    return ret;
}
#endif /* HYD_TEST_HOOKS */
