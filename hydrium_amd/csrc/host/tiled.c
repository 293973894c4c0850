/*
 * tiled.c — a TILE-MODE image whose pixels already sit in HBM, from C (include/hydrium_amd.h, hydamd_tiled_*).
 *
 * The reference codes a tile-mode image one tile at a time, every tile a Frame of its own (libhydrium.c:147-203,
 * encoder.c:339-398,968-1005); hyd_send_tile does the same from host pixels and assembles every frame on the host.
 * Here the tiles are device pointers.  A tile is one LF group, so they are coded in LAUNCH GROUPS of independent
 * one-LF-group frames (hydamd_begin_batch(ctx, 1, n)), and the frames of a group are assembled on the device by one
 * launch sequence behind its entropy stage (csrc/hip/assemble_tiles.hip), at a running offset kept in device memory.
 *
 * Policy HERE: the PLAN — every byte that does not depend on the pixels (file header once, a frame header per tile
 * with its origin, size and is_last, LFGlobal, the constant sub-streams per tile shape), built once per object with
 * the host frame code (frame.c) and kept on the device; raster order; ONE context and one stream — the host waits once
 * per launch group (hydamd_sync, which is also where a group that outgrew the context's buffers is rerun), checks what
 * the assembly left, repeats the group's assembly if the group was rerun or the output buffer had to grow, and only then
 * enqueues the next group into the same buffers; after a failure the stream is drained before the call returns.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bitio.h"
#include "frame.h"
#include "hydrium_amd.h"
#include "libhydrium/libhydrium.h"
#include "planbuf.h"
#include "../hyd_sample_fmt.h"

#include "../hip/hydk_tile_asm.h"
#include "../hip/hydk_tiles.h"

#ifndef HYDRIUM_EXPORT
#define HYDRIUM_EXPORT __attribute__((visibility("default")))
#endif

#define TILED_DEFAULT_LAUNCH 32

/* ---------------------------------------------------------------------------------------------
 * the plan
 * ------------------------------------------------------------------------------------------- */
typedef struct TileGeometry {
    size_t W, H, tw, th, ntx, nty, ntiles;
} TileGeometry;

static int tile_geometry(const HYDImageMetadata *md, TileGeometry *g, const char **err) {
    if (!md->width || !md->height) {
        *err = "invalid zero-width or zero-height";
        return HYD_API_ERROR;
    }
    if (md->tile_size_shift_x < 0 || md->tile_size_shift_x > 3 || md->tile_size_shift_y < 0 || md->tile_size_shift_y > 3) {
        *err = "tile mode needs both tile_size_shift_x and tile_size_shift_y between 0 and 3";
        return HYD_API_ERROR;
    }
    g->W = md->width;
    g->H = md->height;
    g->tw = (size_t)256 << md->tile_size_shift_x;
    g->th = (size_t)256 << md->tile_size_shift_y;
    g->ntx = (g->W + g->tw - 1) / g->tw;
    g->nty = (g->H + g->th - 1) / g->th;
    g->ntiles = g->ntx * g->nty;
    if (g->ntiles > ((size_t)1 << 24)) {
        *err = "too many tiles";
        return HYD_API_ERROR;
    }
    return HYD_OK;
}

/* the four tile shapes an image can have: (interior | right edge) x (interior | bottom edge) */
static uint32_t shape_of(const TileGeometry *g, size_t tx, size_t ty) { return (tx == g->ntx - 1 ? 1u : 0u) | (ty == g->nty - 1 ? 2u : 0u); }

/* the constant sub-streams of one frame shape of w x h pixels (one LF group), appended to the plan buffer; `bits` and
 * `part` are the caller's to reuse.  Also what the batch object plans its one-LF-group frames with (batch.c). */
int hydk_tile_plan_shape(Buf *buf, HydBits *bits, HydBits *part, size_t w, size_t h, HydkTileShape *sh, const char **err) {
    const size_t vbw = (w + 7) >> 3, vbh = (h + 7) >> 3;
    sh->ngroups = (uint32_t)(((w + 255) >> 8) * ((h + 255) >> 8));
    /* LFGlobal (encoder.c:510-537): a section of its own, or the opening bits of the only one */
    hb_reset(bits);
    hyd_write_lf_global(bits);
    if (sh->ngroups > 1) {
        uint32_t nbits = 0;
        hb_align(bits);
        sh->lfglobal_off = (uint32_t)buf_add_bits(buf, bits, &nbits);
        sh->lfglobal_bytes = nbits >> 3;
        hb_reset(bits);
    }
    int ret = hyd_write_lf_group_fixed_head(bits, err);
    if (ret)
        return ret;
    sh->pre_off = (uint32_t)buf_add_bits(buf, bits, &sh->pre_bits);
    const HydBits *tail = hyd_internal_lf_tail(vbw, vbh);
    if (!tail) { /* the process-wide cache of tails is full: code this one here */
        hb_reset(part);
        ret = hyd_write_lf_group_tail(part, vbw, vbh, err);
        if (ret)
            return ret;
        tail = part;
    }
    sh->tail_off = (uint32_t)buf_add_bits(buf, tail, &sh->tail_bits);
    hb_reset(bits);
    ret = hyd_write_hf_global_fixed(bits, 1, sh->ngroups, NULL, err);
    if (ret)
        return ret;
    sh->hfpre_off = (uint32_t)buf_add_bits(buf, bits, &sh->hfpre_bits);
    if ((uint64_t)sh->tail_bits + sh->hfpre_bits + 2u + 9u * 8u + 9u * 73u * 32u > (uint64_t)HYDK_TILE_MID_WORDS * 32u) {
        *err = "a tile's constant sub-streams do not fit the assembler's scratch";
        return HYD_INTERNAL_ERROR;
    }
    return HYD_OK;
}

static int build_plan(const HYDImageMetadata *md, const TileGeometry *g, uint8_t **plan_out, size_t *plan_len, const char **err) {
    int ret = HYD_OK;
    Buf buf = {0};
    HydBits bits, part;
    hb_init(&bits);
    hb_init(&part);
    HydkTilePlan plan;
    memset(&plan, 0, sizeof(plan));
    plan.magic = HYDK_TILE_MAGIC;
    plan.num_frames = (uint32_t)g->ntiles;
    plan.nshapes = HYDK_TILE_MAX_SHAPES;
    buf_reserve(&buf, sizeof(plan));
    for (uint32_t s = 0; s < HYDK_TILE_MAX_SHAPES && !ret; s++) {
        const size_t w = (s & 1u) ? g->W - (g->ntx - 1) * g->tw : g->tw < g->W ? g->tw : g->W;
        const size_t h = (s & 2u) ? g->H - (g->nty - 1) * g->th : g->th < g->H ? g->th : g->H;
        ret = hydk_tile_plan_shape(&buf, &bits, &part, w, h, &plan.shapes[s], err);
    }
    /* one frame header per tile: origin, size and is_last differ, and with them the header's length */
    const size_t frames_off = ret ? 0 : buf_reserve(&buf, g->ntiles * sizeof(HydkTileFrame));
    plan.frames_off = (uint32_t)frames_off;
    for (size_t i = 0; i < g->ntiles && !ret && !buf.failed; i++) {
        const size_t tx = i % g->ntx, ty = i / g->ntx;
        HydFrameLfg l;
        memset(&l, 0, sizeof(l));
        l.x = tx;
        l.y = ty;
        l.width = (tx + 1) * g->tw > g->W ? g->W - tx * g->tw : g->tw;
        l.height = (ty + 1) * g->th > g->H ? g->H - ty * g->th : g->th;
        HydFrameShape shape;
        memset(&shape, 0, sizeof(shape));
        shape.image_width = g->W;
        shape.image_height = g->H;
        shape.frame_width = l.width;
        shape.frame_height = l.height;
        shape.tile_count_x = g->tw >> 8;
        shape.tile_count_y = g->th >> 8;
        shape.lfg_count = 1;
        shape.lfg = &l;
        shape.is_last = i + 1 == g->ntiles;
        hb_reset(&bits);
        if (i == 0)
            ret = hyd_internal_file_header(md, NULL, 0, &bits, err);
        if (!ret)
            ret = hyd_write_frame_header(&bits, &shape, err);
        if (ret) {
            if (!*err)
                *err = "frame header could not be written";
            break;
        }
        hb_align(&bits);
        HydkTileFrame fr;
        uint32_t nbits = 0;
        memset(&fr, 0, sizeof(fr));
        fr.prefix_off = (uint32_t)buf_add_bits(&buf, &bits, &nbits);
        fr.prefix_bytes = nbits >> 3;
        fr.shape = shape_of(g, tx, ty);
        if (!buf.failed)
            memcpy(buf.p + frames_off + i * sizeof(fr), &fr, sizeof(fr));
    }
    if (!ret && (buf.failed || bits.failed || part.failed || buf.len > (size_t)0xFFFFFF00u)) {
        *err = buf.len > (size_t)0xFFFFFF00u ? "too many tiles for one plan" : "out of memory";
        ret = buf.len > (size_t)0xFFFFFF00u ? HYD_API_ERROR : HYD_NOMEM;
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
struct HydAmdTiled {
    int device, launch;
    HYDImageMetadata md;
    TileGeometry g;
    HydAmdContext *ctx;
    HydkTileAsm *as;
    const void *src[3];
    ptrdiff_t row_stride, pixel_stride;
    int fmt;
    size_t next, in_group; /* first tile and tile count of the launch group in flight */
    int in_flight, have_result;
    size_t size;
    unsigned reruns;
    uint64_t held; /* device memory taken at creation (context, scratch, plan) */
    char err[256];
};

static char g_create_error[256];

static int fail(HydAmdTiled *t, int code, const char *what, const char *detail) {
    snprintf(t->err, sizeof(t->err), "%s%s%s", what, detail && *detail ? ": " : "", detail && *detail ? detail : "");
    return code;
}

HYDRIUM_EXPORT const char *hydamd_tiled_error(HydAmdTiled *t) { return t ? t->err : g_create_error; }

HYDRIUM_EXPORT void hydamd_tiled_destroy(HydAmdTiled *t) {
    if (!t)
        return;
    if (t->ctx) {
        (void)hydamd_sync(t->ctx);
        hydk_tiles_destroy(t->as);
        hydamd_destroy(t->ctx);
    }
    free(t);
}

HYDRIUM_EXPORT HydAmdTiled *hydamd_tiled_create(int device, const HYDImageMetadata *md, int tiles_per_launch, int *status) {
    int st = HYD_API_ERROR;
    HydAmdTiled *t = NULL;
    uint8_t *plan = NULL;
    size_t plan_len = 0;
    const char *err = NULL;
    TileGeometry g;
    g_create_error[0] = 0;
    if (!md || tiles_per_launch < 0 || tiles_per_launch > HYDK_TILE_MAX_FRAMES) {
        err = !md ? "null metadata" : "tiles_per_launch must be between 0 and 255";
        goto out;
    }
    if ((st = tile_geometry(md, &g, &err)) != 0)
        goto out;
    if (hydamd_device_count() < 1 || device < 0 || device >= hydamd_device_count()) {
        st = HYD_INTERNAL_ERROR;
        err = "no usable HIP device";
        goto out;
    }
    if ((st = hydk_plan_check_metadata(md, g_create_error, sizeof(g_create_error))) != 0)
        goto out;
    if ((st = build_plan(md, &g, &plan, &plan_len, &err)) != 0)
        goto out;
    t = calloc(1, sizeof(*t));
    if (!t) {
        st = HYD_NOMEM;
        goto out;
    }
    t->device = device;
    t->md = *md;
    t->g = g;
    t->launch = tiles_per_launch ? tiles_per_launch : TILED_DEFAULT_LAUNCH;
    if ((size_t)t->launch > g.ntiles)
        t->launch = (int)g.ntiles;
    const uint64_t free_before = hydk_tiles_device_free(device);
    t->ctx = hydamd_create(device, t->launch, md->linear_light != 0, 0, &st);
    if (!t->ctx) {
        snprintf(g_create_error, sizeof(g_create_error), "%s", hydamd_error(NULL));
        free(t);
        t = NULL;
        goto out;
    }
    if ((st = hydamd_set_lf_coder(t->ctx, 2)) != 0 || (st = hydamd_set_rans_waves(t->ctx, 5)) != 0 ||
        (st = hydk_tiles_create(device, t->launch, plan, plan_len, &t->as)) != 0) {
        snprintf(g_create_error, sizeof(g_create_error), "%s", st && !t->as ? "the tile assembler could not be created" : hydamd_error(t->ctx));
        hydamd_destroy(t->ctx);
        free(t);
        t = NULL;
        goto out;
    }
    const uint64_t free_after = hydk_tiles_device_free(device);
    t->held = free_before > free_after ? free_before - free_after : 0;
    st = HYD_OK;
out:
    if (err && !g_create_error[0])
        snprintf(g_create_error, sizeof(g_create_error), "%s", err);
    free(plan);
    if (status)
        *status = st;
    return t;
}

/* after a failure once work was enqueued: nothing of this object is left running when the call returns */
static void drain(HydAmdTiled *t) {
    (void)hydamd_sync(t->ctx);
    (void)hydk_tiles_wait(t->as, hydamd_get_stream(t->ctx));
    t->in_flight = 0;
}

static int assemble_group(HydAmdTiled *t) {
    const void *blob = NULL, *ext = NULL;
    size_t cap = 0;
    int st = hydamd_export_batch_owned(t->ctx, (int)t->in_group, &blob, &cap, &ext);
    if (st)
        return fail(t, st, "batch view", hydamd_error(t->ctx));
    st = hydk_tiles_run(t->as, (uint32_t)t->next, (uint32_t)t->in_group, blob, ext, t->next == 0, hydamd_get_stream(t->ctx));
    return st ? fail(t, st, "tile assembly", hydk_tiles_error(t->as)) : HYD_OK;
}

static int enqueue_group(HydAmdTiled *t) {
    const TileGeometry *g = &t->g;
    const size_t left = g->ntiles - t->next, n = left < (size_t)t->launch ? left : (size_t)t->launch;
    int st = hydamd_begin_batch(t->ctx, 1, (int)n);
    if (st)
        return fail(t, st, "begin launch group", hydamd_error(t->ctx));
    for (size_t i = 0; i < n; i++) {
        const size_t k = t->next + i, tx = k % g->ntx, ty = k / g->ntx;
        const size_t w = (tx + 1) * g->tw > g->W ? g->W - tx * g->tw : g->tw, h = (ty + 1) * g->th > g->H ? g->H - ty * g->th : g->th;
        /* (tiles are frames, but the whole image is the picture: interpolated chroma is continuous across tiles) */
        if ((st = hydamd_encode_lf_group_at(t->ctx, (int)i, t->src, t->row_stride, t->pixel_stride, t->fmt, g->W, g->H, tx * g->tw,
                                            ty * g->th, w, h, 0)) != 0)
            return fail(t, st, "tile", hydamd_error(t->ctx));
    }
    if ((st = hydamd_finish_frame(t->ctx, (int)n)) != 0)
        return fail(t, st, "launch group", hydamd_error(t->ctx));
    t->in_group = n;
    return assemble_group(t);
}

HYDRIUM_EXPORT int hydamd_encode_image_tiled(HydAmdTiled *t, const void *const src[3], ptrdiff_t row_stride, ptrdiff_t pixel_stride,
                                             int sample_fmt) {
    if (!t)
        return HYD_API_ERROR;
    if (!src || !src[0] || !src[1] || !src[2])
        return fail(t, HYD_API_ERROR, "null pixel pointer", NULL);
    const char *refusal = hyd_fmt_refusal(sample_fmt, src, pixel_stride, t->g.W);
    if (refusal)
        return fail(t, HYD_API_ERROR, refusal, NULL);
    if (t->in_flight)
        return fail(t, HYD_API_ERROR, "an image is in flight: hydamd_tiled_result first", NULL);
    t->err[0] = 0;
    t->have_result = 0;
    for (int c = 0; c < 3; c++)
        t->src[c] = src[c];
    t->row_stride = row_stride;
    t->pixel_stride = pixel_stride;
    t->fmt = sample_fmt;
    t->next = 0;
    if (!hydk_tiles_out(t->as)) {
        /* a byte per pixel (what the context's own section buffer starts from) plus the constant parts; grown when it proves too small */
        const uint64_t want = (uint64_t)t->g.W * t->g.H + (uint64_t)t->g.ntiles * 1024u + 65536u;
        const int st = hydk_tiles_reserve(t->as, want, 0, hydamd_get_stream(t->ctx));
        if (st)
            return fail(t, st, "output buffer", hydk_tiles_error(t->as));
    }
    t->in_flight = 1;
    const int st = enqueue_group(t);
    if (st)
        drain(t);
    return st;
}

/* the launch group in flight: wait, let hydamd_sync rerun it if it outgrew a buffer, and see its frames into the file */
static int settle_group(HydAmdTiled *t) {
    const unsigned before = hydamd_overflow_reruns(t->ctx);
    int st = hydamd_sync(t->ctx);
    if (st)
        return fail(t, st, "launch group", hydamd_error(t->ctx));
    t->reruns += hydamd_overflow_reruns(t->ctx) - before;
    for (int attempt = 0; attempt < 4; attempt++) {
        uint32_t err = 0;
        uint64_t bytes = 0, needed = 0;
        hydk_tiles_result(t->as, &err, &bytes, &needed);
        if (!err) {
            t->size = (size_t)bytes;
            return HYD_OK;
        }
        if (err & HYDK_ASM_E_NAN)
            return fail(t, HYD_API_ERROR, "Invalid NaN Float", NULL);
        if (err & (HYDK_ASM_E_BLOB | HYDK_ASM_E_SLOT | HYDK_ASM_E_HEAD | HYDK_ASM_E_SIZE | HYDK_ASM_E_SCRATCH))
            return fail(t, HYD_INTERNAL_ERROR, "tile assembly failed on the device", NULL);
        /* RETRY: the assembly saw the first run's incomplete results (hydamd_sync has rerun the group since).  SPACE: the
         * file outgrew its buffer; the bytes of the groups before this one move with it.  Either way the running offset
         * was not advanced: the same launches again, before the context's buffers are reused */
        if (err & HYDK_ASM_E_SPACE) {
            st = hydk_tiles_reserve(t->as, needed + (needed >> 2) + 65536u, bytes, hydamd_get_stream(t->ctx));
            if (st)
                return fail(t, st, "output buffer", hydk_tiles_error(t->as));
        }
        if ((st = assemble_group(t)) != 0)
            return st;
        if ((st = hydk_tiles_wait(t->as, hydamd_get_stream(t->ctx))) != 0)
            return fail(t, st, "tile assembly", hydk_tiles_error(t->as));
    }
    return fail(t, HYD_INTERNAL_ERROR, "a launch group still does not fit after enlarging its buffers", NULL);
}

HYDRIUM_EXPORT int hydamd_tiled_result(HydAmdTiled *t, size_t *size) {
    if (!t)
        return HYD_API_ERROR;
    if (!t->have_result) {
        if (!t->in_flight)
            return fail(t, HYD_API_ERROR, "no image in flight", NULL);
        for (;;) {
            int st = settle_group(t);
            if (!st) {
                t->next += t->in_group;
                if (t->next >= t->g.ntiles)
                    break;
                st = enqueue_group(t);
            }
            if (st) {
                drain(t);
                return st;
            }
        }
        t->in_flight = 0;
        t->have_result = 1;
    }
    if (size)
        *size = t->size;
    return HYD_OK;
}

HYDRIUM_EXPORT int hydamd_tiled_read(HydAmdTiled *t, uint8_t *dst, size_t capacity) {
    if (!t || !t->have_result)
        return t ? fail(t, HYD_API_ERROR, "no finished image: hydamd_tiled_result first", NULL) : HYD_API_ERROR;
    if (!dst)
        return fail(t, HYD_API_ERROR, "null output pointer", NULL);
    if (capacity < t->size)
        return fail(t, HYD_NEED_MORE_OUTPUT, "output buffer too small", NULL);
    const int st = hydk_tiles_read(t->as, dst, t->size);
    return st ? fail(t, st, "read-back", hydk_tiles_error(t->as)) : HYD_OK;
}

HYDRIUM_EXPORT const uint8_t *hydamd_tiled_device(HydAmdTiled *t) { return t && t->have_result ? hydk_tiles_out(t->as) : NULL; }

HYDRIUM_EXPORT unsigned hydamd_tiled_overflow_reruns(HydAmdTiled *t) { return t ? t->reruns : 0; }

HYDRIUM_EXPORT size_t hydamd_tiled_device_bytes(HydAmdTiled *t) { return t ? (size_t)(t->held + hydk_tiles_out_capacity(t->as)) : 0; }

/* ---------------------------------------------------------------------------------------------
 * CPU-only test hook: the plan and the batched layout (hydk_tiles.h compiled for the host) on results handed
 * in as hydamd_frame_from_streams takes them, one frame per tile of the image in raster order — what the kernels
 * of assemble_tiles.hip do, frame by frame, held to frame.c by tests/test_tiled_sections.py.
 * ------------------------------------------------------------------------------------------- */
#ifdef HYD_TEST_HOOKS
#define HYDT_EXPORT __attribute__((visibility("default")))
/* frame f of `plan` laid out by frames[f] and shapes[frames[f].shape]: hydk_tile_prepare, hydk_tile_pieces and the shared
 * composer, frame by frame (planbuf.h; also what mixed.c's hook runs on its own plan) */
/* ... with an outcome per image, as k_batch_place arrives at it (assemble_batch.hip): flags[f] is what the context's export
 * would leave in frame f's slot record (HydAmdBlobSlot.reserved[0]); every frame is prepared and its pieces counted from
 * its own first byte, then a flagged frame counts 0 bytes and each piece is placed by hydk_place_piece.  status[f] (optional):
 * HYDAMD_IMAGE_BAD_SAMPLE or 0; piece_bits (optional): [nframes x HYDK_TILE_PIECES][2] dst_bit and nbits of the placed list. */
int hydt_layout_from_streams_skip(const uint8_t *plan, const HydkTileFrame *frames, const HydkTileShape *shapes, size_t nframes,
                                  const HydAmdLfStream *lf, const uint32_t *freq, const uint32_t *alphabet, const uint32_t *group_bits,
                                  const uint32_t *max_alphabet, const uint8_t *payload, size_t payload_len, const uint32_t *flags,
                                  uint64_t *frame_offsets, uint32_t *status, uint64_t *piece_bits, uint8_t **out, size_t *out_len,
                                  const char **e) {
    int ret = HYD_OK;
    HydAmdBlobSlot *rec = calloc(nframes, sizeof(*rec));
    uint32_t *head = calloc(nframes * HYDK_TILE_HEAD_WORDS, 4), *mid = calloc(nframes * HYDK_TILE_MID_WORDS, 4),
             *toc = calloc(nframes * HYDK_TILE_TOC_WORDS, 4);
    HydkTileSizes *sizes = calloc(nframes, sizeof(*sizes));
    HydkPiece *pieces = calloc(nframes * HYDK_TILE_PIECES, sizeof(*pieces));
    uint64_t *ends = calloc(nframes * HYDK_TILE_PIECES, sizeof(*ends));
    HydkTileScratch *scratch = calloc(1, sizeof(*scratch));
    size_t lf_len = 0;
    for (size_t f = 0; f < nframes; f++)
        lf_len += ((((size_t)lf[f].bit_count + 7) >> 3) + 3) & ~(size_t)3;
    uint8_t *lf_packed = calloc(lf_len + 16, 1);
    uint8_t *hf = calloc(payload_len + 16, 1);
    uint8_t *file = NULL;
    if (!rec || !head || !mid || !toc || !sizes || !pieces || !ends || !scratch || !lf_packed || !hf) {
        *e = "out of memory";
        ret = HYD_NOMEM;
    }
    if (!ret) {
        memcpy(hf, payload, payload_len);
        size_t lf_at = 0, hf_at = 0;
        uint64_t at = 0;
        for (size_t f = 0; f < nframes && !ret; f++) {
            HydAmdBlobSlot *r = &rec[f];
            r->running_max_alphabet = max_alphabet[f];
            memcpy(r->alphabet, alphabet + f * HYDAMD_MAX_CLUSTERS, sizeof(r->alphabet));
            memcpy(r->group_bits, group_bits + f * HYDAMD_GROUPS_PER_LFG, sizeof(r->group_bits));
            memcpy(r->freq, freq + f * HYDAMD_MAX_CLUSTERS * HYDAMD_ALPHABET, sizeof(r->freq));
            memcpy(r->lf.lengths, lf[f].lengths, HYDAMD_LF_CODES);
            r->lf.alphabet = lf[f].alphabet;
            r->lf.run_pairs = lf[f].run_pairs;
            r->lf.bit_count = (uint32_t)lf[f].bit_count;
            r->lf.offset = (uint32_t)lf_at;
            r->reserved[0] = flags ? flags[f] : 0u;
            const size_t nb = ((size_t)lf[f].bit_count + 7) >> 3;
            if (nb)
                memcpy(lf_packed + lf_at, lf[f].bits, nb);
            const HydkTileShape *sh = &shapes[frames[f].shape];
            hydk_tile_prepare(plan, &frames[f], sh, r, r->lf.lengths, lf_len, head + f * HYDK_TILE_HEAD_WORDS, mid + f * HYDK_TILE_MID_WORDS,
                              toc + f * HYDK_TILE_TOC_WORDS, scratch, &sizes[f]);
            if (sizes[f].err || hf_at + sizes[f].hf_bytes > payload_len) {
                *e = "the batched layout rejected a frame";
                ret = HYD_INTERNAL_ERROR;
                break;
            }
            hydk_tile_pieces(plan, &frames[f], sh, &sizes[f], r, head + f * HYDK_TILE_HEAD_WORDS, mid + f * HYDK_TILE_MID_WORDS,
                             toc + f * HYDK_TILE_TOC_WORDS, lf_packed + lf_at, hf + hf_at, 0, pieces + f * HYDK_TILE_PIECES);
            const uint32_t skip = hydk_frame_flagged(r, 1);
            for (uint32_t i = 0; i < HYDK_TILE_PIECES; i++)
                hydk_place_piece(&pieces[f * HYDK_TILE_PIECES + i], at, skip);
            if (frame_offsets)
                frame_offsets[f] = at;
            if (status)
                status[f] = skip ? HYDAMD_IMAGE_BAD_SAMPLE : 0u;
            at += skip ? 0 : sizes[f].frame_bytes;
            lf_at += (nb + 3) & ~(size_t)3;
            hf_at += sizes[f].hf_bytes;
        }
        if (!ret) {
            if (frame_offsets)
                frame_offsets[nframes] = at;
            const uint32_t np = (uint32_t)(nframes * HYDK_TILE_PIECES);
            for (uint32_t i = 0; i < np; i++) {
                ends[i] = pieces[i].dst_bit + pieces[i].nbits;
                if (piece_bits) {
                    piece_bits[2 * i] = pieces[i].dst_bit;
                    piece_bits[2 * i + 1] = pieces[i].nbits;
                }
            }
            file = malloc((size_t)at + 4);
            if (!file) {
                ret = HYD_NOMEM;
            } else {
                for (uint64_t W = 0; W * 4 < at; W++)
                    hydk_store_word(file, W, hydk_pieces_word(pieces, ends, np, W), 0, at);
                *out = file;
                *out_len = (size_t)at;
            }
        }
    }
    free(rec);
    free(head);
    free(mid);
    free(toc);
    free(sizes);
    free(pieces);
    free(ends);
    free(scratch);
    free(lf_packed);
    free(hf);
    return ret;
}

int hydt_layout_from_streams(const uint8_t *plan, const HydkTileFrame *frames, const HydkTileShape *shapes, size_t nframes,
                             const HydAmdLfStream *lf, const uint32_t *freq, const uint32_t *alphabet, const uint32_t *group_bits,
                             const uint32_t *max_alphabet, const uint8_t *payload, size_t payload_len, uint64_t *frame_offsets,
                             uint8_t **out, size_t *out_len, const char **e) {
    return hydt_layout_from_streams_skip(plan, frames, shapes, nframes, lf, freq, alphabet, group_bits, max_alphabet, payload, payload_len,
                                         NULL, frame_offsets, NULL, NULL, out, out_len, e);
}

HYDT_EXPORT int hydt_tiles_from_streams(const HYDImageMetadata *md, size_t nframes, const HydAmdLfStream *lf, const uint32_t *freq,
                                        const uint32_t *alphabet, const uint32_t *group_bits, const uint32_t *max_alphabet,
                                        const uint8_t *payload, size_t payload_len, uint64_t *frame_offsets /* [nframes + 1] or NULL */,
                                        uint8_t **out, size_t *out_len, const char **err) {
    static const char *none = NULL;
    const char **e = err ? err : &none;
    TileGeometry g;
    uint8_t *plan = NULL;
    size_t plan_len = 0;
    *e = NULL;
    int ret = tile_geometry(md, &g, e);
    if (!ret && nframes != g.ntiles) {
        *e = "one frame per tile of the image";
        ret = HYD_API_ERROR;
    }
    if (!ret)
        ret = build_plan(md, &g, &plan, &plan_len, e);
    if (ret)
        return ret;
    const HydkTilePlan *hp = (const HydkTilePlan *)plan;
    ret = hydt_layout_from_streams(plan, (const HydkTileFrame *)(plan + hp->frames_off), hp->shapes, nframes, lf, freq, alphabet, group_bits,
                                   max_alphabet, payload, payload_len, frame_offsets, out, out_len, e);
    free(plan);
    return ret;
}

/* the shared composer (hydk_pieces.h) on a crafted list: piece i is nbits[i] bits from byte src_off[i] of `src`, at bit
 * dst_bit[i]; bytes [lo, lo + bytes) of `out` (4-byte aligned, whole words) are written the way k_pieces_copy writes them */
HYDT_EXPORT int hydt_compose_pieces(const uint64_t *dst_bit, const uint64_t *nbits, const uint64_t *src_off, uint32_t np, const uint8_t *src,
                                    uint64_t lo, uint64_t bytes, uint8_t *out) {
    HydkPiece *P = calloc(np ? np : 1, sizeof(*P));
    uint64_t *ends = calloc(np ? np : 1, sizeof(*ends));
    if (P && ends) {
        for (uint32_t i = 0; i < np; i++) {
            P[i] = hydk_piece(dst_bit[i], src + src_off[i], nbits[i]);
            ends[i] = dst_bit[i] + nbits[i];
        }
        for (uint64_t W = lo >> 2; W * 4 < lo + bytes; W++)
            hydk_store_word(out, W, hydk_pieces_word(P, ends, np, W), lo, lo + bytes);
    }
    const int ret = P && ends ? HYD_OK : HYD_NOMEM;
    free(P);
    free(ends);
    return ret;
}
#endif /* HYD_TEST_HOOKS */
