/*
 * multi.c — ONE frame whose pixels already sit in HBM, on N devices of one process, from C.
 *
 * The reference codes a frame's LF groups one after another on one core: hyd_send_tile per tile
 * (libhydrium.c:172-203), per-LF-group tables with the running alphabet maximum (entropy.c:459-460), the frame
 * closed by encoder.c:928-957.  hyd_send_tile's own multi-device form (encoder.c finish_frame_multi) does that on
 * several GPUs but takes its pixels from HOST memory — 805 MB through one caller thread's staging for a 16384^2
 * frame: upload-bound at any N.  This is the same composition without the uploads: the caller's pixels are device
 * pointers, one per shard; LF groups are dealt in raster runs and every shard runs its transform stage.  From there the
 * frame is closed by the procedure both multi-device APIs share (shards.c: floors by peer read, closing stage per shard,
 * views, cross-device waits, assembly, reruns, verification of the peer reads) — no RCCL, no process group, no host copy
 * before the finished file.  Policy HERE: the deal; the assembling shard (the caller's choice per frame — rotate it: the
 * file's D2H copy then leaves through a different GPU's link every time); a file with its header, LF groups in raster
 * order; an output size that stays grown across frames; device pairs latched by device id; the asynchronous split
 * (hydamd_encode_image_multi enqueues, hydamd_multi_result waits); and a peer-read mismatch fails the frame with the pair
 * named (there is no host copy of the pixels to fall back on: the caller owns that decision).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "shards.h"
#include "../hyd_sample_fmt.h"

#ifndef HYDRIUM_EXPORT
#define HYDRIUM_EXPORT __attribute__((visibility("default")))
#endif

#define MULTI_MAX HYDAMD_MAX_PEERS

struct HydAmdMulti {
    HydShardFrame f; /* n, ctx, slots, the assembling shard of the frame in flight, key = device id, out_cap kept across frames */
    size_t first[MULTI_MAX];
    HYDImageMetadata md;
    size_t lfx, lfy, total;
    uint32_t lf_ids[HYDAMD_MAX_LF_GROUPS];
    int in_flight, have_result;
    size_t size;
    char err[200];
};

/* [reading device][owning device]; ids outside the table are verified every time */
static HydPairLatch g_pair_ok = HYD_PAIR_LATCH_INIT;

static int fail(HydAmdMulti *m, int code, const char *what, HydAmdContext *c) {
    const char *d = c ? hydamd_error(c) : NULL;
    snprintf(m->err, sizeof(m->err), "%s%s%s", what, d && *d ? ": " : "", d && *d ? d : "");
    return code;
}

HYDRIUM_EXPORT const char *hydamd_multi_error(HydAmdMulti *m) { return m ? m->err : "null multi-device frame"; }

HYDRIUM_EXPORT void hydamd_multi_destroy(HydAmdMulti *m) {
    if (!m)
        return;
    for (int d = 0; d < m->f.n; d++)
        if (m->f.ctx[d]) {
            (void)hydamd_sync(m->f.ctx[d]);
            hydamd_destroy(m->f.ctx[d]);
        }
    free(m);
}

HYDRIUM_EXPORT HydAmdMulti *hydamd_multi_create(int n, const int *devices, const HYDImageMetadata *md, int *status) {
    int st = HYD_API_ERROR;
    HydAmdMulti *m = NULL;
    if (n < 1 || n > MULTI_MAX || !devices || !md || !md->width || !md->height)
        goto out;
    const size_t lfx = (md->width + 2047) >> 11, lfy = (md->height + 2047) >> 11, total = lfx * lfy;
    if (total > HYDAMD_MAX_LF_GROUPS || total == 128 || total < (size_t)n) /* (128: the reference never returns, entropy.c:99) */
        goto out;
    if (n > 1 && !hydamd_peers_reachable(devices, n)) {
        st = HYD_INTERNAL_ERROR;
        goto out;
    }
    m = calloc(1, sizeof(*m));
    if (!m) {
        st = HYD_NOMEM;
        goto out;
    }
    HydShardFrame *f = &m->f;
    f->n = n;
    f->write_header = 1;
    f->latch = &g_pair_ok;
    f->md = &m->md;
    f->lf_ids = m->lf_ids;
    m->md = *md;
    m->lfx = lfx;
    m->lfy = lfy;
    m->total = total;
    for (size_t g = 0; g < total; g++)
        m->lf_ids[g] = (uint32_t)g; /* raster order = send order = slot order across the shards */
    for (int d = 0; d < n; d++) {
        f->key[d] = devices[d];
        m->first[d] = (size_t)d * total / (size_t)n;
        f->slots[d] = (uint32_t)((size_t)(d + 1) * total / (size_t)n - m->first[d]);
        f->ctx[d] = hydamd_create(devices[d], (int)f->slots[d], md->linear_light != 0, 0, &st);
        if (!f->ctx[d]) {
            hydamd_multi_destroy(m);
            m = NULL;
            goto out;
        }
        if ((st = hydamd_set_lf_coder(f->ctx[d], 2)) != 0 || (st = hydamd_set_rans_waves(f->ctx[d], 5)) != 0) {
            hydamd_multi_destroy(m);
            m = NULL;
            goto out;
        }
    }
    st = HYD_OK;
out:
    if (status)
        *status = st;
    return m;
}

HYDRIUM_EXPORT HydAmdContext *hydamd_multi_context(HydAmdMulti *m, int shard) {
    return m && shard >= 0 && shard < m->f.n ? m->f.ctx[shard] : NULL;
}

HYDRIUM_EXPORT int hydamd_multi_shard_lf_groups(HydAmdMulti *m, int shard, size_t *first, size_t *count) {
    if (!m || shard < 0 || shard >= m->f.n)
        return HYD_API_ERROR;
    if (first)
        *first = m->first[shard];
    if (count)
        *count = m->f.slots[shard];
    return HYD_OK;
}

/* what the closer's outcome means for this API: m->err and the status code */
static int fail_outcome(HydAmdMulti *m, const HydShardOutcome *o) {
    const HydShardFrame *f = &m->f;
    if (o->kind == SHARDS_DEVICE)
        return fail(m, o->code, o->msg, f->ctx[o->shard]);
    if (o->kind != SHARDS_MISMATCH)
        return fail(m, o->code, o->msg, NULL);
    if (o->is_floor)
        snprintf(m->err, sizeof(m->err), "peer read mismatch: device %d did not see the alphabet maxima devices before it wrote (shard %d)",
                 f->key[o->reader], o->shard);
    else
        snprintf(m->err, sizeof(m->err), "peer read mismatch: device %d did not see what device %d wrote (shard %d)", f->key[o->reader],
                 f->key[o->owner], o->shard);
    return o->code;
}

/* src: 3 pointers per shard, [shard][channel], in shard d's device memory: where pixel (0, 0) OF THE IMAGE would sit for
 * that shard's buffer (only the pixels of the shard's own LF groups — hydamd_multi_shard_lf_groups, raster order — are
 * read; a rank-style slab of rows [y0, y1) passes slab - y0 * row_stride).  Strides in samples, as hyd_send_tile's. */
HYDRIUM_EXPORT int hydamd_encode_image_multi(HydAmdMulti *m, const void *const *src, ptrdiff_t row_stride, ptrdiff_t pixel_stride,
                                             int sample_fmt, int assembling_shard) {
    if (!m)
        return HYD_API_ERROR;
    HydShardFrame *f = &m->f;
    if (!src || assembling_shard < 0 || assembling_shard >= f->n)
        return fail(m, HYD_API_ERROR, "bad arguments", NULL);
    const char *refusal = hyd_fmt_refusal(sample_fmt, NULL, pixel_stride, 0); /* the format alone */
    /* a shard's buffer is only promised to hold its own rows, and the filter would read a neighbouring shard's chroma row */
    /* (a planar 4:2:2 window has no other row, but its columns cross into an LF group that another shard owns) */
    if (!refusal && hyd_fmt_describe(sample_fmt).filter != 0)
        refusal = HYD_FMT_NV12_SHARDED_MSG;
    for (int d = 0; d < f->n && !refusal; d++) /* every shard that has pointers to its layout, then the pitch */
        refusal = hyd_fmt_refusal(sample_fmt, src[3 * d + 1] ? src + 3 * d : NULL, pixel_stride, 0);
    if (refusal || (refusal = hyd_fmt_refusal(sample_fmt, NULL, pixel_stride, m->md.width)) != NULL)
        return fail(m, HYD_API_ERROR, refusal, NULL);
    if (m->in_flight)
        return fail(m, HYD_API_ERROR, "a frame is in flight: hydamd_multi_result first", NULL);
    const size_t W = m->md.width, H = m->md.height;
    int st;
    f->assembling = assembling_shard;
    m->have_result = 0;
    m->err[0] = 0;
    for (int d = 0; d < f->n; d++) {
        HydAmdContext *c = f->ctx[d];
        if (!src[3 * d] || !src[3 * d + 1] || !src[3 * d + 2])
            return fail(m, HYD_API_ERROR, "null pixel pointer", NULL);
        if ((st = hydamd_begin_frame(c, (unsigned)m->total)) != 0)
            return fail(m, st, "begin frame", c);
        for (size_t i = 0; i < f->slots[d]; i++) {
            const size_t g = m->first[d] + i, tx = g % m->lfx, ty = g / m->lfx;
            const size_t w = W - tx * 2048 < 2048 ? W - tx * 2048 : 2048, h = H - ty * 2048 < 2048 ? H - ty * 2048 : 2048;
            if ((st = hydamd_encode_lf_group_at(c, (int)i, src + 3 * d, row_stride, pixel_stride, sample_fmt, W, H, tx * 2048, ty * 2048,
                                                w, h, (unsigned)g)) != 0)
                return fail(m, st, "LF group", c);
        }
        if ((st = hydamd_run_transform(c, (int)f->slots[d])) != 0)
            return fail(m, st, "transform stage", c);
    }
    HydShardOutcome o;
    if (hyd_shards_enqueue(f, &o))
        return fail_outcome(m, &o);
    m->in_flight = 1;
    return HYD_OK;
}

/* waits for the frame; *size = bytes of the finished file in the assembling device's memory */
HYDRIUM_EXPORT int hydamd_multi_result(HydAmdMulti *m, size_t *size) {
    if (!m)
        return HYD_API_ERROR;
    if (!m->have_result) {
        if (!m->in_flight)
            return fail(m, HYD_API_ERROR, "no frame in flight", NULL);
        HydShardOutcome o;
        m->in_flight = 0;
        if (hyd_shards_wait(&m->f, &o))
            return fail_outcome(m, &o);
        m->size = o.size;
        m->have_result = 1;
    }
    if (size)
        *size = m->size;
    return HYD_OK;
}

/* the finished file to host memory (one copy from the assembling device) */
HYDRIUM_EXPORT int hydamd_multi_read(HydAmdMulti *m, uint8_t *dst, size_t capacity) {
    if (!m || !m->have_result)
        return m ? fail(m, HYD_API_ERROR, "no finished frame: hydamd_multi_result first", NULL) : HYD_API_ERROR;
    if (!dst || capacity < m->size)
        return fail(m, HYD_NEED_MORE_OUTPUT, "output buffer too small", NULL);
    const int st = hydamd_assembler_read(hydamd_context_assembler(m->f.ctx[m->f.assembling]), dst, m->size);
    return st ? fail(m, st, "read-back", m->f.ctx[m->f.assembling]) : HYD_OK;
}
