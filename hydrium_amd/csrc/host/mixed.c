/*
 * mixed.c — a batch of one-frame images EACH OF ITS OWN SIZE whose pixels already sit in HBM, every one a finished file,
 * from C (include/hydrium_amd.h, hydamd_mixed_*).
 *
 * A context takes LF groups of different sizes in one launch group (tiled.c codes a tile-mode image's ragged tiles that
 * way), and hydk_tiles.h lays frames of different shapes side by side.  Here both serve a queue of pictures of many
 * sizes — thumbnails, crops, the output of a decoder — each at most 2048 x 2048 pixels, ONE LF group: the launch group is
 * tiled.c's (hydamd_begin_batch(ctx, 1, frames), one hydamd_encode_lf_group per image with its own pointers, strides and
 * size), the assembly is batch.c's (csrc/hip/assemble_batch.hip: every frame a complete file — what the reference writes
 * for that picture alone with both tile_size_shift -1 — back to back in one device buffer, the table of their offsets
 * beside it), and the protocol behind the launch group — reservation, the wait and its rerun, results, read-back, per-image
 * outcomes — is the driver both batch objects share (batchrun.c).
 *
 * What is this file's own is the PLAN: no two batches need the same one.  It holds a shape record per DISTINCT size of
 * the batch (tiled.c's shape planner) and a frame record per image whose prefix is that image's file header and one-frame
 * frame header (batch.c's prefix planner) — built per batch on the host, uploaded in the stream ahead of the assembly,
 * and neither rebuilt nor uploaded when a batch's list of sizes equals the previous batch's.
 *
 * An object made by hydamd_mixed_create_slots also takes images of SEVERAL LF groups, up to 28 (the nine-cluster scheme:
 * hydamd_begin_batch_frames codes frames of 1, 4 and 9 LF groups as one launch group).  Its plan is of a second kind
 * (hydk_tiles.h, HydkFramesPlan): a frame record names its frame's slots and share of the assembler's scratch and says which
 * kind the frame is — one LF group: as above; several: a complete frame plan of that image (assembler.c's planner, as
 * batch.c uses it), one per distinct size.
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

#define MIXED_DEFAULT_FRAMES 32
#define MIXED_MAX_SIDE 2048u /* one LF group */

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

/* LF groups of an image (0: more than a frame of such a batch may hold, or an empty image) */
static uint32_t lf_groups_of(uint64_t w, uint64_t h) {
    if (!w || !h || w > 2048u * HYDK_FRAMES_MAX_LF_GROUPS || h > 2048u * HYDK_FRAMES_MAX_LF_GROUPS)
        return 0;
    const uint64_t n = ((w + 2047) >> 11) * ((h + 2047) >> 11);
    return n <= HYDK_FRAMES_MAX_LF_GROUPS ? (uint32_t)n : 0u;
}

/* The frames plan (hydk_tiles.h, HydkFramesPlan) of `n` images of sizes sz[0 .. n), each of 1..28 LF groups, for an object
 * of max_frames images and max_slots LF groups: a shape record per distinct size of ONE LF group, a frame plan per
 * distinct size of SEVERAL, a frame record per image with its slots and its share of the scratch arrays (prefix sums in
 * batch order), and the table that deals the workgroups of k_batch_prepare_frames.  *fixed as build_plan's, the frames of
 * several LF groups contributing what hydk_batch_create states for a uniform batch of their shape. */
static int build_frames_plan(int n, const MixedSize *sz, int linear_light, int max_frames, int max_slots, uint8_t **plan_out, size_t *plan_len,
                             uint64_t *fixed, const char **err) {
    int ret = HYD_OK;
    Buf buf = {0};
    HydBits bits, part;
    hb_init(&bits);
    hb_init(&part);
    HydkFramesPlan plan;
    HydkTileShape *shapes = calloc((size_t)n, sizeof(*shapes));
    HydkBatchFrame *frames = calloc((size_t)n, sizeof(*frames));
    MixedSize *distinct = calloc((size_t)n, sizeof(*distinct)); /* sizes of one LF group: the shapes */
    MixedSize *planned = calloc((size_t)n, sizeof(*planned));   /* sizes of several: the frame plans, */
    uint32_t *planned_off = calloc((size_t)n, sizeof(*planned_off)); /* where each lies */
    uint32_t *parts = NULL, ids[HYDK_FRAMES_MAX_LF_GROUPS];
    memset(&plan, 0, sizeof(plan));
    plan.magic = HYDK_FRAMES_MAGIC;
    plan.num_frames = (uint32_t)n;
    *fixed = 0;
    for (uint32_t i = 0; i < HYDK_FRAMES_MAX_LF_GROUPS; i++)
        ids[i] = i; /* raster order */
    if (!shapes || !frames || !distinct || !planned || !planned_off) {
        *err = "out of memory";
        ret = HYD_NOMEM;
    }
    for (int f = 0; f < n && !ret; f++) {
        HydkBatchFrame *fr = &frames[f];
        fr->lf_groups = lf_groups_of(sz[f].w, sz[f].h);
        if (!fr->lf_groups) {
            *err = "an image of a mixed batch holds between 1 and 28 LF groups of 2048 x 2048 pixels";
            ret = HYD_API_ERROR;
            break;
        }
        fr->first_slot = plan.num_slots;
        fr->piece_base = plan.npieces;
        plan.num_slots += fr->lf_groups;
        plan.npieces += 3 * fr->lf_groups + 5;
        if (fr->lf_groups > 1) {
            plan.nparts += fr->lf_groups + 1;
            continue;
        }
        uint32_t s = 0;
        while (s < plan.nshapes && (distinct[s].w != sz[f].w || distinct[s].h != sz[f].h))
            s++;
        if (s == plan.nshapes)
            distinct[plan.nshapes++] = sz[f];
        fr->one.shape = s;
    }
    if (!ret && (n > max_frames || plan.num_slots > (uint32_t)max_slots)) {
        *err = "the batch holds more LF groups than the object has slots";
        ret = HYD_API_ERROR;
    }
    if (!ret) {
        buf_reserve(&buf, sizeof(plan));
        plan.shapes_off = (uint32_t)buf_reserve(&buf, (size_t)plan.nshapes * sizeof(*shapes));
        plan.frames_off = (uint32_t)buf_reserve(&buf, (size_t)n * sizeof(*frames));
        plan.parts_off = (uint32_t)buf_reserve(&buf, (size_t)plan.nparts * sizeof(*parts));
        parts = calloc((size_t)plan.nparts + 1, sizeof(*parts));
        if (!parts) {
            *err = "out of memory";
            ret = HYD_NOMEM;
        }
    }
    for (uint32_t s = 0; s < plan.nshapes && !ret; s++)
        ret = hydk_tile_plan_shape(&buf, &bits, &part, distinct[s].w, distinct[s].h, &shapes[s], err);
    uint32_t hfg = 0, toc = 0, sizes = 0, at_part = 0;
    for (int f = 0; f < n && !ret; f++) {
        HydkBatchFrame *fr = &frames[f];
        HYDImageMetadata md;
        memset(&md, 0, sizeof(md));
        md.width = sz[f].w;
        md.height = sz[f].h;
        md.linear_light = linear_light;
        md.tile_size_shift_x = md.tile_size_shift_y = -1;
        fr->hfg_off = hfg;
        fr->toc_off = toc;
        fr->sizes_off = sizes;
        if (fr->lf_groups == 1) {
            ret = hydk_plan_one_frame_prefix(&buf, &bits, &md, NULL, 0, &fr->one, err);
            const HydkTileShape *sh = &shapes[fr->one.shape];
            fr->hfg_words = HYDK_TILE_MID_WORDS;
            fr->toc_words = HYDK_TILE_TOC_WORDS;
            *fixed += (uint64_t)fr->one.prefix_bytes + sh->lfglobal_bytes +
                      4u * (HYDK_TILE_HEAD_WORDS + HYDK_TILE_MID_WORDS + HYDK_TILE_TOC_WORDS) + (sh->tail_bits >> 3) + 16u;
        } else {
            uint32_t k = 0;
            while (k < plan.nplans && (planned[k].w != sz[f].w || planned[k].h != sz[f].h))
                k++;
            if (k == plan.nplans) { /* one blob (the batch view), the image's LF groups in raster order: batch.c's plan of this shape */
                uint8_t *ap = NULL;
                size_t ap_len = 0;
                ret = hydk_plan_frame(&md, 1, 1, 1, &fr->lf_groups, ids, NULL, 0, &ap, &ap_len, err);
                if (ret)
                    break;
                const size_t off = buf_reserve(&buf, ap_len);
                if (!buf.failed)
                    memcpy(buf.p + off, ap, ap_len);
                free(ap);
                if (buf.failed)
                    break;
                planned[k] = sz[f];
                planned_off[k] = (uint32_t)off;
                plan.nplans++;
            }
            fr->plan_off = planned_off[k];
            HydkAsmPlan ap; /* (a copy: appending moves the buffer) */
            memcpy(&ap, buf.p + fr->plan_off, sizeof(ap));
            const uint32_t C = ap.num_presets * ap.clusters_per_preset;
            /* HFGlobal: the fixed fields, two bits, a configuration of <= 9 bits and a histogram of <= 73 words per cluster */
            fr->hfg_words = (ap.hfpre_bits + 2u + C * 9u + 31u) / 32u + C * 73u + 2u;
            fr->toc_words = ap.toc_n + 2u; /* entries of <= 32 bits */
            sizes += ap.toc_n;
            uint32_t tail = 0;
            for (uint32_t i = 0; i < ap.ntails; i++)
                tail = ap.tail_bits[i] > tail ? ap.tail_bits[i] : tail;
            *fixed += (uint64_t)ap.prefix_bytes + ap.lfglobal_bytes + 4ull * (fr->hfg_words + fr->toc_words) +
                      (uint64_t)fr->lf_groups * (4u * HYDK_FRAMES_HEAD_STRIDE + (tail >> 3) + 2u) + 16u;
            for (uint32_t i = 0; i <= fr->lf_groups; i++)
                parts[at_part++] = (uint32_t)f << 8 | i;
        }
        hfg += fr->hfg_words;
        toc += fr->toc_words;
    }
    if (!ret && (buf.failed || bits.failed || part.failed)) {
        *err = "out of memory";
        ret = HYD_NOMEM;
    }
    if (!ret && (hfg > HYDK_FRAMES_HFG_CAP(max_frames, max_slots) || toc > HYDK_FRAMES_TOC_CAP(max_frames, max_slots) ||
                 sizes > HYDK_FRAMES_SIZES_CAP(max_frames, max_slots) || plan.npieces > HYDK_FRAMES_PIECES_CAP(max_frames, max_slots))) {
        *err = "the batch needs more of the assembler's scratch than the object holds";
        ret = HYD_INTERNAL_ERROR;
    }
    if (!ret) {
        buf.len = (buf.len + 15) & ~(size_t)15;
        plan.total_bytes = (uint32_t)buf.len;
        memcpy(buf.p, &plan, sizeof(plan));
        memcpy(buf.p + plan.shapes_off, shapes, (size_t)plan.nshapes * sizeof(*shapes));
        memcpy(buf.p + plan.frames_off, frames, (size_t)n * sizeof(*frames));
        memcpy(buf.p + plan.parts_off, parts, (size_t)plan.nparts * sizeof(*parts));
        *plan_out = buf.p;
        *plan_len = buf.len;
        buf.p = NULL;
    }
    free(buf.p);
    free(shapes);
    free(frames);
    free(distinct);
    free(planned);
    free(planned_off);
    free(parts);
    hb_free(&bits);
    hb_free(&part);
    return ret;
}

/* ---------------------------------------------------------------------------------------------
 * the object
 * ------------------------------------------------------------------------------------------- */
struct HydAmdMixed {
    int device, max_frames, linear_light;
    int several;    /* images of up to 28 LF groups (hydamd_mixed_create_slots) */
    int planned;    /* images of the plan on the device (0: none), their sizes (run.fixed is that plan's): */
    MixedSize sizes[HYDK_TILE_MAX_FRAMES];
    HydBatchRun run;
};

static char g_create_error[256];

#define RUN(m) ((m) ? &(m)->run : NULL)

HYDRIUM_EXPORT const char *hydamd_mixed_error(HydAmdMixed *m) { return m ? m->run.err : g_create_error; }

HYDRIUM_EXPORT void hydamd_mixed_destroy(HydAmdMixed *m) {
    if (!m)
        return;
    hyd_batchrun_close(&m->run);
    free(m);
}

/* max_lf_groups < 0: images of one LF group, a slot per image (hydamd_mixed_create) */
static HydAmdMixed *create(int device, int max_frames, int max_lf_groups, int linear_light, int *status) {
    int st = HYD_API_ERROR;
    HydAmdMixed *m = NULL;
    g_create_error[0] = 0;
    if (max_frames < 0 || max_frames > HYDK_TILE_MAX_FRAMES) {
        snprintf(g_create_error, sizeof(g_create_error), "max_frames must be between 0 and 255 (the slots of one context; 0: the default, 32)");
        goto out;
    }
    if (max_lf_groups >= 0 && (max_lf_groups < (max_frames ? max_frames : MIXED_DEFAULT_FRAMES) || max_lf_groups > HYDK_TILE_MAX_FRAMES)) {
        snprintf(g_create_error, sizeof(g_create_error), "max_lf_groups must be between max_frames and 255 (the slots of one context)");
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
    m->several = max_lf_groups >= 0;
    const int max_slots = m->several ? max_lf_groups : m->max_frames;
    st = hyd_batchrun_open(&m->run, device, max_slots, m->linear_light, "hydamd_mixed_result", g_create_error, sizeof(g_create_error));
    if (!st)
        st = hyd_batchrun_adopt(&m->run,
                                m->several ? hydk_batch_create_frames(device, m->max_frames, max_slots, &m->run.as)
                                           : hydk_batch_create(device, m->max_frames, NULL, 0, &m->run.as),
                                g_create_error, sizeof(g_create_error));
    if (st) {
        free(m);
        m = NULL;
    }
out:
    if (status)
        *status = st;
    return m;
}

HYDRIUM_EXPORT HydAmdMixed *hydamd_mixed_create(int device, int max_frames, int linear_light, int *status) {
    return create(device, max_frames, -1, linear_light, status);
}

HYDRIUM_EXPORT HydAmdMixed *hydamd_mixed_create_slots(int device, int max_frames, int max_lf_groups, int linear_light, int *status) {
    if (max_lf_groups < 0) { /* (not the other constructor's way in) */
        g_create_error[0] = 0;
        snprintf(g_create_error, sizeof(g_create_error), "max_lf_groups must be between max_frames and 255 (the slots of one context)");
        if (status)
            *status = HYD_API_ERROR;
        return NULL;
    }
    return create(device, max_frames, max_lf_groups, linear_light, status);
}

/* the batch's plan on the device: the previous batch's when its list of sizes is the same */
static int plan_batch(HydAmdMixed *m, int frames, const HydAmdImageDesc *images) {
    HydBatchRun *r = &m->run;
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
    int st = m->several ? build_frames_plan(frames, m->sizes, m->linear_light, m->max_frames, r->max_slots, &plan, &plan_len, &r->fixed, &err)
                        : build_plan(frames, m->sizes, m->linear_light, &plan, &plan_len, &r->fixed, &err);
    if (st)
        return hyd_batchrun_fail(r, st, "plan", err);
    st = hydk_batch_set_plan(r->as, plan, plan_len, hydamd_get_stream(r->ctx));
    free(plan);
    if (st)
        return hyd_batchrun_fail(r, st, "plan", hydk_batch_error(r->as));
    m->planned = frames;
    return HYD_OK;
}

/* the launch group of images of 1..28 LF groups: image after image, an image's LF groups in raster order, each with its
 * own pointers — computed from the image's strides as hydamd_encode_image does — and clipped to the image */
static int enqueue_several(HydBatchRun *r, const HydAmdImageDesc *images, const int *sample_fmts) {
    unsigned counts[HYDK_TILE_MAX_FRAMES];
    for (int f = 0; f < r->frames; f++)
        counts[f] = lf_groups_of(images[f].width, images[f].height);
    int st = hydamd_begin_batch_frames(r->ctx, r->frames, counts);
    if (st)
        return hyd_batchrun_fail(r, st, "begin launch group", hydamd_error(r->ctx));
    int slot = 0;
    for (int f = 0; f < r->frames; f++) {
        const HydAmdImageDesc *d = &images[f];
        const int sample_fmt = sample_fmts[f];
        const size_t lfx = (d->width + 2047) >> 11, lfy = (d->height + 2047) >> 11;
        for (size_t ty = 0; ty < lfy; ty++)
            for (size_t tx = 0; tx < lfx; tx++, slot++) {
                const size_t w = d->width - tx * 2048 < 2048 ? d->width - tx * 2048 : 2048;
                const size_t h = d->height - ty * 2048 < 2048 ? d->height - ty * 2048 : 2048;
                /* (the image is the picture: interpolated chroma crosses its LF groups and clamps at its edges) */
                if ((st = hydamd_encode_lf_group_at(r->ctx, slot, d->src, d->row_stride, d->pixel_stride, sample_fmt, d->width, d->height,
                                                    tx * 2048, ty * 2048, w, h, (unsigned)(ty * lfx + tx))) != 0)
                    return hyd_batchrun_fail(r, st, "image", hydamd_error(r->ctx));
            }
    }
    if ((st = hydamd_finish_frame(r->ctx, r->slots)) != 0)
        return hyd_batchrun_fail(r, st, "launch group", hydamd_error(r->ctx));
    return hyd_batchrun_assemble(r);
}

/* the launch group: tiled.c's, every image an LF group of its own size in a slot of its own */
static int enqueue(HydAmdMixed *m, const HydAmdImageDesc *images, const int *sample_fmts) {
    HydBatchRun *r = &m->run;
    if (m->several)
        return enqueue_several(r, images, sample_fmts);
    int st = hydamd_begin_batch(r->ctx, 1, r->frames);
    if (st)
        return hyd_batchrun_fail(r, st, "begin launch group", hydamd_error(r->ctx));
    for (int f = 0; f < r->frames; f++) {
        const HydAmdImageDesc *d = &images[f];
        if ((st = hydamd_encode_lf_group(r->ctx, f, d->src, d->row_stride, d->pixel_stride, sample_fmts[f], d->width, d->height, 0)) != 0)
            return hyd_batchrun_fail(r, st, "image", hydamd_error(r->ctx));
    }
    if ((st = hydamd_finish_frame(r->ctx, r->frames)) != 0)
        return hyd_batchrun_fail(r, st, "launch group", hydamd_error(r->ctx));
    return hyd_batchrun_assemble(r);
}

/* every image in its own sample format: the layer underneath takes a format per LF group (the transform launch builds a
 * format mask, the entropy stage picks its chain form from whether any slot is float), and neither the plan nor its reuse
 * depends on formats */
HYDRIUM_EXPORT int hydamd_encode_mixed_formats(HydAmdMixed *m, int frames, const HydAmdImageDesc *images, const int *sample_fmts) {
    if (!m)
        return HYD_API_ERROR;
    HydBatchRun *r = &m->run;
    if (frames < 1 || frames > m->max_frames)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "frames must be between 1 and max_frames", NULL);
    if (!images)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "null image descriptors", NULL);
    int slots = 0;
    for (int f = 0; f < frames; f++) {
        if (!images[f].src[0] || !images[f].src[1] || !images[f].src[2])
            return hyd_batchrun_fail(r, HYD_API_ERROR, "null pixel pointer", NULL);
        if (m->several) {
            const uint32_t n = lf_groups_of(images[f].width, images[f].height);
            if (!images[f].width || !images[f].height)
                return hyd_batchrun_fail(r, HYD_API_ERROR, "every image of a mixed batch must be at least 1 pixel in each direction", NULL);
            if (!n)
                return hyd_batchrun_fail(r, HYD_API_ERROR, "an image of a mixed batch holds at most 28 LF groups of 2048 x 2048 pixels", NULL);
            slots += (int)n;
            continue;
        }
        slots++;
        if (!images[f].width || !images[f].height || images[f].width > MIXED_MAX_SIDE || images[f].height > MIXED_MAX_SIDE)
            return hyd_batchrun_fail(r, HYD_API_ERROR, "every image of a mixed batch must be between 1 and 2048 pixels in each direction", NULL);
    }
    if (slots > r->max_slots)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "the batch holds more LF groups than the object has slots", NULL);
    if (!sample_fmts)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "null sample formats", NULL);
    const char *refusal = NULL; /* every image's format, then every image's layout, then every image's pitch */
    for (int f = 0; f < frames && !refusal; f++)
        refusal = hyd_fmt_refusal(sample_fmts[f], NULL, 0, 0);
    for (int f = 0; f < frames && !refusal; f++)
        refusal = hyd_fmt_refusal(sample_fmts[f], images[f].src, images[f].pixel_stride, 0);
    for (int f = 0; f < frames && !refusal; f++)
        refusal = hyd_fmt_refusal(sample_fmts[f], NULL, images[f].pixel_stride, images[f].width);
    if (refusal)
        return hyd_batchrun_fail(r, HYD_API_ERROR, refusal, NULL);
    int st = hyd_batchrun_busy(r);
    if (st)
        return st;
    r->err[0] = 0;
    r->have_result = 0;
    r->frames = frames;
    r->slots = slots;
    st = plan_batch(m, frames, images); /* nothing of this batch is in the stream yet but, at most, its plan */
    if (!st && (st = hyd_batchrun_reserve(r)) != 0) /* the plan's copy may be in the stream, out of the pinned buffer the next plan is written to */
        (void)hydk_batch_wait(r->as, hydamd_get_stream(r->ctx));
    if (st)
        return st;
    r->in_flight = 1;
    st = enqueue(m, images, sample_fmts);
    if (st)
        hyd_batchrun_drain(r);
    return st;
}

HYDRIUM_EXPORT int hydamd_encode_mixed(HydAmdMixed *m, int frames, const HydAmdImageDesc *images, int sample_fmt) {
    int fmts[HYDK_TILE_MAX_FRAMES]; /* one format, repeated (a `frames` out of range is refused before any is read) */
    for (int f = 0; f < HYDK_TILE_MAX_FRAMES; f++)
        fmts[f] = sample_fmt;
    return hydamd_encode_mixed_formats(m, frames, images, fmts);
}

HYDRIUM_EXPORT int hydamd_mixed_result(HydAmdMixed *m, size_t *total_bytes) { return hyd_batchrun_result(RUN(m), total_bytes); }

HYDRIUM_EXPORT int hydamd_mixed_offsets(HydAmdMixed *m, uint64_t *offsets) { return hyd_batchrun_offsets(RUN(m), offsets); }

HYDRIUM_EXPORT int hydamd_mixed_read(HydAmdMixed *m, int frame, uint8_t *dst, size_t capacity) {
    return hyd_batchrun_read(RUN(m), frame, dst, capacity);
}

HYDRIUM_EXPORT const uint8_t *hydamd_mixed_device(HydAmdMixed *m) { return hyd_batchrun_device(RUN(m)); }

HYDRIUM_EXPORT const uint64_t *hydamd_mixed_offsets_device(HydAmdMixed *m) { return hyd_batchrun_offsets_device(RUN(m)); }

HYDRIUM_EXPORT int hydamd_mixed_set_image_errors(HydAmdMixed *m, int per_image) { return hyd_batchrun_set_image_errors(RUN(m), per_image); }

HYDRIUM_EXPORT int hydamd_mixed_image_status(HydAmdMixed *m, uint32_t *status) { return hyd_batchrun_image_status(RUN(m), status); }

HYDRIUM_EXPORT const uint32_t *hydamd_mixed_image_status_device(HydAmdMixed *m) { return hyd_batchrun_image_status_device(RUN(m)); }

HYDRIUM_EXPORT unsigned hydamd_mixed_overflow_reruns(HydAmdMixed *m) { return m ? m->run.reruns : 0; }

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

/* the same batch with an outcome per image: flags[f] != 0 stands for what the context leaves in image f's slot record when
 * the picture held a non-finite sample; status [n], piece_bits [n x HYDK_TILE_PIECES][2] (dst_bit, nbits) as placed */
HYDT_EXPORT int hydt_mixed_from_streams_skip(size_t n, const uint32_t *widths, const uint32_t *heights, const HydAmdLfStream *lf,
                                             const uint32_t *freq, const uint32_t *alphabet, const uint32_t *group_bits,
                                             const uint32_t *max_alphabet, const uint8_t *payload, size_t payload_len,
                                             const uint32_t *flags, uint64_t *frame_offsets, uint32_t *status, uint64_t *piece_bits,
                                             uint8_t **out, size_t *out_len, const char **err) {
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
    ret = hydt_layout_from_streams_skip(plan, (const HydkTileFrame *)(plan + hp->frames_off), (const HydkTileShape *)(plan + hp->shapes_off),
                                        n, lf, freq, alphabet, group_bits, max_alphabet, payload, payload_len, flags, frame_offsets, status,
                                        piece_bits, out, out_len, e);
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

/* what the frames planner (build_frames_plan above, the product's own) made of a list of sizes for an object of max_frames
 * images and max_slots LF groups.  per_frame[f][0 .. 10]: kind (0 one LF group, 1 several), first slot, LF groups, plan
 * offset, piece base, HFGlobal offset and words, TOC offset and words, section-size offset and entries.  counts[0 .. 6]:
 * distinct frame plans, shape records, workgroup-table entries, pieces, slots, bytes of the plan.  parts: the table
 * ([510]).  caps[0 .. 4]: what creation allocates — head, HFGlobal and TOC words, section sizes, pieces.  *plan_out
 * (malloc'ed, optional): the plan's bytes. */
HYDT_EXPORT int hydt_mixed_plan_describe(size_t n, const uint32_t *widths, const uint32_t *heights, int max_frames, int max_slots,
                                         uint32_t *per_frame, uint32_t *counts, uint32_t *parts, uint64_t *fixed, uint64_t *caps,
                                         uint8_t **plan_out, size_t *plan_len, const char **err) {
    static const char *none = NULL;
    const char **e = err ? err : &none;
    MixedSize sz[HYDK_TILE_MAX_FRAMES];
    uint8_t *plan = NULL;
    size_t len = 0;
    uint64_t fx = 0;
    *e = NULL;
    if (n < 1 || n > HYDK_TILE_MAX_FRAMES || !widths || !heights || !per_frame || !counts || !parts || !caps) {
        *e = "between 1 and 255 images";
        return HYD_API_ERROR;
    }
    for (size_t f = 0; f < n; f++) {
        sz[f].w = widths[f];
        sz[f].h = heights[f];
    }
    const int ret = build_frames_plan((int)n, sz, 0, max_frames, max_slots, &plan, &len, &fx, e);
    if (ret)
        return ret;
    const HydkFramesPlan *hp = (const HydkFramesPlan *)plan;
    const HydkBatchFrame *fr = (const HydkBatchFrame *)(plan + hp->frames_off);
    for (size_t f = 0; f < n; f++) {
        uint32_t *o = per_frame + 11 * f;
        o[0] = fr[f].plan_off != 0;
        o[1] = fr[f].first_slot;
        o[2] = fr[f].lf_groups;
        o[3] = fr[f].plan_off;
        o[4] = fr[f].piece_base;
        o[5] = fr[f].hfg_off;
        o[6] = fr[f].hfg_words;
        o[7] = fr[f].toc_off;
        o[8] = fr[f].toc_words;
        o[9] = fr[f].sizes_off;
        o[10] = fr[f].plan_off ? ((const HydkAsmPlan *)(plan + fr[f].plan_off))->toc_n : 0u;
    }
    counts[0] = hp->nplans;
    counts[1] = hp->nshapes;
    counts[2] = hp->nparts;
    counts[3] = hp->npieces;
    counts[4] = hp->num_slots;
    counts[5] = hp->total_bytes;
    memcpy(parts, plan + hp->parts_off, (size_t)hp->nparts * sizeof(uint32_t));
    if (fixed)
        *fixed = fx;
    caps[0] = (uint64_t)max_slots * HYDK_FRAMES_HEAD_STRIDE;
    caps[1] = HYDK_FRAMES_HFG_CAP(max_frames, max_slots);
    caps[2] = HYDK_FRAMES_TOC_CAP(max_frames, max_slots);
    caps[3] = HYDK_FRAMES_SIZES_CAP(max_frames, max_slots);
    caps[4] = HYDK_FRAMES_PIECES_CAP(max_frames, max_slots);
    if (plan_out && plan_len) {
        *plan_out = plan;
        *plan_len = len;
    } else {
        free(plan);
    }
    return HYD_OK;
}

/* the frame plan batch.c builds for a uniform batch of w x h images (several LF groups): one blob, raster order, file
 * header, is_last, no ICC profile — what every frame of several LF groups in a frames plan must carry */
HYDT_EXPORT int hydt_mixed_frame_plan_alone(uint32_t w, uint32_t h, uint8_t **plan_out, size_t *plan_len, const char **err) {
    static const char *none = NULL;
    const char **e = err ? err : &none;
    uint32_t ids[HYDK_FRAMES_MAX_LF_GROUPS];
    const uint32_t n = lf_groups_of(w, h);
    HYDImageMetadata md;
    *e = NULL;
    if (n < 2)
        return HYD_API_ERROR;
    for (uint32_t i = 0; i < n; i++)
        ids[i] = i;
    memset(&md, 0, sizeof(md));
    md.width = w;
    md.height = h;
    md.tile_size_shift_x = md.tile_size_shift_y = -1;
    return hydk_plan_frame(&md, 1, 1, 1, &n, ids, NULL, 0, plan_out, plan_len, e);
}
#endif /* HYD_TEST_HOOKS */
