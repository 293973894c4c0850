/*
 * hostframe.c — frames written on the host (hostframe.h): the result fillers, the one blob reader, the cached LF group
 * tails, the LF group sections coded on a few threads, and the writer all of them end in.
 */
#define _POSIX_C_SOURCE 200809L /* clock_gettime under -std=c99 */
#include <pthread.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "hostframe.h"

#define FAIL(err, code, msg) (*(err) = (msg), (code))

double hyd_now_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
int hyd_trace_on(void) {
    static int on = -1;
    if (on < 0) {
        const char *e = getenv("HYDAMD_TRACE");
        on = e && *e && *e != '0';
    }
    return on;
}

/* ---- results of a context, of a blob ---- */

/* an LF stream record against the byte string it points into: true when it reaches past its end */
static int lf_outside(const HydAmdLfInfo *lf, uint64_t lf_bytes) {
    return (uint64_t)lf->offset + (((uint64_t)lf->bit_count + 7) >> 3) > lf_bytes;
}

static void take_lf_stream(HydLfgResult *r, const HydAmdLfInfo *lf, const uint8_t *lf_bytes) {
    memcpy(r->lf_lengths, lf->lengths, HYD_LF_CODES);
    r->lf_alphabet = lf->alphabet;
    r->lf_run_pairs = lf->run_pairs;
    r->lf_bit_count = lf->bit_count;
    r->lf_bits = (uint8_t *)(uintptr_t)(lf_bytes + lf->offset); /* borrowed */
}

int hyd_read_lf_results(HydAmdContext *ctx, size_t count, HydLfgResult *res, uint8_t **blob, int *device_failed,
                        const char **err) {
    const size_t lf_len = hydamd_lf_payload_size(ctx);
    HydAmdLfInfo *info = malloc(count * sizeof(HydAmdLfInfo));
    *blob = malloc(lf_len ? lf_len : 1);
    *device_failed = 0;
    if (!info || !*blob) {
        free(info);
        return FAIL(err, HYD_NOMEM, "out of memory");
    }
    int ret = hydamd_read_lf_streams(ctx, 0, (int)count, info);
    if (!ret)
        ret = hydamd_read_lf_payload(ctx, *blob, lf_len);
    for (size_t s = 0; s < count && !ret; s++) {
        if (lf_outside(&info[s], lf_len))
            ret = HYD_INTERNAL_ERROR;
        else
            take_lf_stream(&res[s], &info[s], *blob);
    }
    free(info);
    *device_failed = ret != 0;
    return ret;
}

int hyd_read_table_results(HydAmdContext *ctx, const HydFrameLfg *lfg, size_t count, HydLfgResult *res, unsigned *max_alphabet) {
    const int lf_on_gpu = hydamd_lf_coder(ctx);
    int ret = 0;
    for (size_t s = 0; s < count && !ret; s++) {
        const size_t vbw = (lfg[s].width + 7) >> 3, vbh = (lfg[s].height + 7) >> 3;
        uint32_t log_alpha = 0, running = 0;
        if (!lf_on_gpu) {
            res[s].dc = malloc(3 * vbw * vbh * sizeof(int32_t));
            if (!res[s].dc)
                return HYD_NOMEM;
            ret = hydamd_read_dc(ctx, (int)s, res[s].dc, vbw, vbh);
        }
        if (!ret)
            ret = hydamd_read_tables(ctx, (int)s, res[s].freq, res[s].alphabet, &log_alpha, &running);
        if (!ret)
            ret = hydamd_read_sections(ctx, (int)s, res[s].bits, NULL);
        if (running > *max_alphabet)
            *max_alphabet = running;
    }
    return ret;
}

/* a field of a record that lies at any byte address */
#define BLOB_FIELD(dst, rec, type, member) memcpy(&(dst), (rec) + offsetof(type, member), sizeof(dst))

uint32_t hyd_blob_slot_preset(const HydBlobView *view, uint32_t i) {
    uint32_t preset;
    BLOB_FIELD(preset, view->slots + (size_t)i * sizeof(HydAmdBlobSlot), HydAmdBlobSlot, preset);
    return preset;
}

int hyd_read_blob(const void *blob, size_t size, size_t expected_slots, HydBlobView *view, HydLfgResult *res,
                  unsigned *max_alphabet) {
    memset(view, 0, sizeof(*view));
    if (!blob || size < sizeof(view->header))
        return HYD_BLOB_NOT_USABLE;
    /* a blob is a byte string: a caller may hold it at any address (a slice of a receive buffer), so the header is
     * copied out and the slot records are read field by field, never through a pointer of their own type */
    memcpy(&view->header, blob, sizeof(view->header));
    view->has_header = 1;
    const HydAmdBlobHeader *h = &view->header;
    if (h->magic != 0x42445948u || h->version != 1 || h->total_bytes > size || (h->status & HYDAMD_BLOB_RETRY) ||
        h->lf_coded != 1 || /* 0: LF ints not coded; 0x101: a view, for device assemblers only */
        (expected_slots && h->num_slots != expected_slots))
        return HYD_BLOB_NOT_USABLE;
    const uint64_t lf_off = sizeof(*h) + (uint64_t)h->num_slots * sizeof(HydAmdBlobSlot);
    /* every size is checked against the blob's own length before it enters a sum: a damaged lf_bytes near
     * 2^64 must not wrap hf_off back into range */
    const int sane = lf_off <= h->total_bytes && h->lf_bytes <= h->total_bytes - lf_off && h->hf_bytes <= h->total_bytes;
    const uint64_t hf_off = sane ? (lf_off + h->lf_bytes + 15u) & ~(uint64_t)15u : 0;
    if (!sane || hf_off > h->total_bytes || hf_off + h->hf_bytes != h->total_bytes)
        return HYD_BLOB_MALFORMED;
    view->slots = (const uint8_t *)blob + sizeof(*h);
    view->hf = (const uint8_t *)blob + hf_off;
    view->hf_len = (size_t)h->hf_bytes;
    for (uint32_t i = 0; res && i < h->num_slots; i++) {
        const uint8_t *rec = view->slots + (size_t)i * sizeof(HydAmdBlobSlot);
        uint32_t table_error, running;
        HydAmdLfInfo lf;
        BLOB_FIELD(table_error, rec, HydAmdBlobSlot, table_error);
        BLOB_FIELD(lf, rec, HydAmdBlobSlot, lf);
        if (table_error)
            return HYD_BLOB_TABLE_ERROR;
        if (lf.error)
            return HYD_BLOB_LF_ERROR;
        if (lf_outside(&lf, h->lf_bytes))
            return HYD_BLOB_LF_RANGE;
        BLOB_FIELD(res[i].freq, rec, HydAmdBlobSlot, freq);
        BLOB_FIELD(res[i].alphabet, rec, HydAmdBlobSlot, alphabet);
        BLOB_FIELD(res[i].bits, rec, HydAmdBlobSlot, group_bits);
        take_lf_stream(&res[i], &lf, (const uint8_t *)blob + lf_off);
        BLOB_FIELD(running, rec, HydAmdBlobSlot, running_max_alphabet);
        if (running > *max_alphabet)
            *max_alphabet = running;
    }
    return HYD_BLOB_USABLE;
}

/* ---- frame assembly (shared by the product path and the CPU-only test hook) ---- */

/* The LF groups of a frame are independent prefix-coded sections; in a frame with more than one
 * group each starts on a byte boundary, so they are coded by a few host threads into private
 * buffers and appended in send order. */
typedef struct LfWork {
    const HydFrameShape *shape;
    const HydLfgResult *res;
    HydBits *out;       /* [lfg_count] */
    int *status;        /* [lfg_count] */
    const char **err;   /* [lfg_count] */
    size_t first, stride;
} LfWork;

/* The HF-metadata sub-streams of an LF group depend on its geometry only (frame.c:
 * hyd_write_lf_group_tail), cost ~200k symbol sends for a full LF group and compress to a few
 * hundred bytes: keep them per (vbw, vbh) for the life of the process.  Entries are immutable once
 * published, so readers only need the lock to find them. */
typedef struct TailEntry {
    size_t vbw, vbh;
    HydBits bits;
} TailEntry;
static pthread_mutex_t g_tail_lock = PTHREAD_MUTEX_INITIALIZER;
static TailEntry g_tails[32];
static int g_ntails;

static const HydBits *find_tail_locked(size_t vbw, size_t vbh) {
    for (int i = 0; i < g_ntails; i++)
        if (g_tails[i].vbw == vbw && g_tails[i].vbh == vbh)
            return &g_tails[i].bits;
    return NULL;
}

const HydBits *hyd_internal_lf_tail(size_t vbw, size_t vbh) {
    pthread_mutex_lock(&g_tail_lock);
    const HydBits *hit = find_tail_locked(vbw, vbh);
    pthread_mutex_unlock(&g_tail_lock);
    if (hit)
        return hit;
    HydBits fresh;
    const char *err = NULL;
    hb_init(&fresh);
    if (hyd_write_lf_group_tail(&fresh, vbw, vbh, &err) || fresh.failed) {
        hb_free(&fresh);
        return NULL; /* the caller codes it inline and reports the error there */
    }
    pthread_mutex_lock(&g_tail_lock);
    hit = find_tail_locked(vbw, vbh);
    if (!hit && g_ntails < (int)(sizeof(g_tails) / sizeof(g_tails[0]))) {
        g_tails[g_ntails].vbw = vbw;
        g_tails[g_ntails].vbh = vbh;
        g_tails[g_ntails].bits = fresh;
        hit = &g_tails[g_ntails++].bits;
        fresh.data = NULL;
    }
    pthread_mutex_unlock(&g_tail_lock);
    if (fresh.data)
        hb_free(&fresh);
    return hit;
}

static int write_one_lf_group(HydBits *out, const HydLfgResult *r, size_t vbw, size_t vbh, const char **err) {
    if (r->lf_bits) {
        const HydLfCoded lf = {r->lf_lengths, r->lf_alphabet, r->lf_run_pairs, r->lf_bits, r->lf_bit_count};
        return hyd_write_lf_group_coded(out, vbw, vbh, &lf, hyd_internal_lf_tail(vbw, vbh), err);
    }
    return hyd_write_lf_group(out, r->dc, vbw, vbh, err);
}

static void *lf_worker(void *arg) {
    const LfWork *w = arg;
    for (size_t s = w->first; s < w->shape->lfg_count; s += w->stride) {
        const size_t vbw = (w->shape->lfg[s].width + 7) >> 3, vbh = (w->shape->lfg[s].height + 7) >> 3;
        hb_init(&w->out[s]);
        w->err[s] = NULL;
        w->status[s] = write_one_lf_group(&w->out[s], &w->res[s], vbw, vbh, &w->err[s]);
        hb_align(&w->out[s]);
    }
    return NULL;
}

int hyd_code_lf_groups_parallel(const HydFrameShape *shape, const HydLfgResult *res, HydBits *out, const char **error) {
    const size_t n = shape->lfg_count;
    int *status = calloc(n, sizeof(int));
    const char **err = calloc(n, sizeof(char *));
    if (!status || !err) {
        free(status);
        free(err);
        return FAIL(error, HYD_NOMEM, "out of memory");
    }
    long cores = sysconf(_SC_NPROCESSORS_ONLN);
    size_t threads = cores > 1 ? (size_t)cores : 1;
    if (threads > n)
        threads = n;
    if (threads > 16)
        threads = 16;
    LfWork work[16];
    pthread_t tid[16];
    size_t started = 0;
    for (size_t i = 0; i < threads; i++) {
        work[i] = (LfWork){shape, res, out, status, err, i, threads};
        if (i + 1 < threads && pthread_create(&tid[started], NULL, lf_worker, &work[i]) == 0)
            started++;
        else
            lf_worker(&work[i]); /* the calling thread takes the last share (and any that could not be spawned) */
    }
    for (size_t i = 0; i < started; i++)
        pthread_join(tid[i], NULL);
    int ret = 0;
    for (size_t s = 0; s < n && !ret; s++) {
        if (status[s] || out[s].failed) {
            *error = err[s] ? err[s] : "LF group coding failed";
            ret = status[s] ? status[s] : HYD_NOMEM;
        }
    }
    free(status);
    free(err);
    return ret;
}

int hyd_assemble_frame(HydBits *stream, const char **err, HydAmdContext *dev, int *device_failed, const HydFrameShape *shape,
                       const HydLfgResult *res, unsigned max_alphabet, const uint8_t *payload, size_t payload_len,
                       HydBits *lf_prebuilt, const HydPayloadSegments *segs) {
    uint8_t *fetched = NULL;
    const size_t fg = hyd_frame_groups(shape);
    const int multi = fg > 1;
    const size_t toc_n = hyd_toc_entries(shape);
    const unsigned num_presets = (unsigned)shape->lfg_count;
    int ret = 0;
    HydBits body;
    hb_init(&body);
    *device_failed = 0;
    size_t *sizes = calloc(toc_n, sizeof(size_t));
    uint32_t(*freq)[HYD_FRAME_MAX_CLUSTERS][HYD_FRAME_ALPHABET] = calloc(num_presets, sizeof(*freq));
    uint32_t(*alpha)[HYD_FRAME_MAX_CLUSTERS] = calloc(num_presets, sizeof(*alpha));
    if (!sizes || !freq || !alpha) {
        ret = FAIL(err, HYD_NOMEM, "out of memory");
        goto done;
    }
    size_t k = 0, mark = 0;
    int overflow = 0; /* more sections than the frame geometry has TOC entries: inconsistent LF-group list */
#define PUSH_SIZE(v)                       \
    do {                                   \
        if (k < toc_n)                     \
            sizes[k++] = (v);              \
        else                               \
            overflow = 1;                  \
    } while (0)
#define CLOSE_SECTION()                    \
    do {                                   \
        if (multi) {                       \
            hb_align(&body);               \
            PUSH_SIZE(body.len - mark);    \
            mark = body.len;               \
        }                                  \
    } while (0)

    double t0 = hyd_now_ms();
    hyd_write_lf_global(&body);
    CLOSE_SECTION();
    if (multi && lf_prebuilt) { /* coded while the GPU was still busy with the entropy stage */
        for (size_t s = 0; s < shape->lfg_count; s++) {
            hb_append_bytes(&body, lf_prebuilt[s].data, lf_prebuilt[s].len);
            CLOSE_SECTION();
        }
    } else if (multi && shape->lfg_count > 1) {
        HydBits *lf = calloc(shape->lfg_count, sizeof(HydBits));
        if (!lf) {
            ret = FAIL(err, HYD_NOMEM, "out of memory");
            goto done;
        }
        ret = hyd_code_lf_groups_parallel(shape, res, lf, err);
        for (size_t s = 0; s < shape->lfg_count; s++) {
            if (!ret) {
                hb_append_bytes(&body, lf[s].data, lf[s].len);
                CLOSE_SECTION();
            }
            hb_free(&lf[s]);
        }
        free(lf);
        if (ret)
            goto done;
    } else {
        for (size_t s = 0; s < shape->lfg_count; s++) {
            const size_t vbw = (shape->lfg[s].width + 7) >> 3, vbh = (shape->lfg[s].height + 7) >> 3;
            ret = write_one_lf_group(&body, &res[s], vbw, vbh, err);
            if (ret)
                goto done;
            CLOSE_SECTION();
        }
    }
    TRACE("  LF group sections", t0);
    t0 = hyd_now_ms();
    /* tables are signalled per preset = raster LF-group id, whatever the send order was */
    for (size_t s = 0; s < shape->lfg_count; s++) {
        const size_t p = shape->lfg[s].raster_id;
        memcpy(freq[p], res[s].freq, sizeof(res[s].freq));
        memcpy(alpha[p], res[s].alphabet, sizeof(res[s].alphabet));
    }
    ret = hyd_write_hf_global(&body, num_presets, fg, (const uint32_t(*)[HYD_FRAME_MAX_CLUSTERS][HYD_FRAME_ALPHABET])freq,
                              (const uint32_t(*)[HYD_FRAME_MAX_CLUSTERS])alpha, max_alphabet, err);
    if (ret)
        goto done;
    CLOSE_SECTION();
    TRACE("  HFGlobal", t0);
    t0 = hyd_now_ms();
    if (multi) {
        /* the device payload already is: byte-padded sections, send order, raster inside an LF group;
         * it follows the body, so only its sizes are needed here */
        for (size_t s = 0; s < shape->lfg_count; s++) {
            const size_t ng = ((shape->lfg[s].width + 255) >> 8) * ((shape->lfg[s].height + 255) >> 8);
            for (size_t g = 0; g < ng && g < HYDAMD_GROUPS_PER_LFG; g++)
                PUSH_SIZE((res[s].bits[g] + 7u) >> 3);
        }
    } else {
        /* a single-group frame is one bit-contiguous section (encoder.c:837-850,968-981 guards) */
        if (!payload && payload_len) {
            fetched = malloc(payload_len);
            if (!fetched) {
                ret = FAIL(err, HYD_NOMEM, "out of memory");
                goto done;
            }
            ret = hydamd_read_payload(dev, fetched, payload_len);
            if (ret) {
                *device_failed = 1;
                goto done;
            }
            payload = fetched;
        }
        hb_append_bits(&body, payload, res[0].bits[0]);
    }
    hb_align(&body);
    if (!multi)
        PUSH_SIZE(body.len);
    if (overflow || k != toc_n || body.failed) {
        ret = FAIL(err, body.failed ? HYD_NOMEM : HYD_INTERNAL_ERROR, "frame assembly inconsistency");
        goto done;
    }
    ret = hyd_write_frame_header(stream, shape, err);
    if (!ret)
        ret = hyd_write_toc_sizes(stream, sizes, toc_n);
    if (ret) {
        if (!*err)
            *err = "frame header could not be written";
        goto done;
    }
    hb_append_bytes(stream, body.data, body.len);
    if (multi && payload_len) {
        if (segs) { /* straight from the shards' blobs into the output: the only copy the sections see here */
            uint8_t *dst = hb_extend(stream, payload_len);
            for (size_t i = 0; dst && i < segs->count; i++) {
                memcpy(dst, segs->ptr[i], segs->len[i]);
                dst += segs->len[i];
            }
        } else if (payload) {
            hb_append_bytes(stream, payload, payload_len);
        } else {
            uint8_t *dst = hb_extend(stream, payload_len);
            if (dst && (ret = hydamd_read_payload(dev, dst, payload_len)) != 0)
                *device_failed = 1;
        }
    }
    if (!ret && stream->failed)
        ret = FAIL(err, HYD_NOMEM, "out of memory");
    TRACE("  frame header, TOC, body + HF sections", t0);
done:
    free(fetched);
#undef CLOSE_SECTION
#undef PUSH_SIZE
    free(sizes);
    free(freq);
    free(alpha);
    hb_free(&body);
    return ret;
}

#ifdef HYD_TEST_HOOKS
/* what hyd_read_blob makes of (blob, size): its class, for the CPU-only tests of both its callers' needs */
__attribute__((visibility("default"))) int hydt_blob_class(const void *blob, size_t size, size_t expected_slots) {
    HydBlobView view;
    unsigned max_alphabet = 0;
    int cls = hyd_read_blob(blob, size, expected_slots, &view, NULL, &max_alphabet);
    HydLfgResult *res = cls == HYD_BLOB_USABLE ? calloc(view.header.num_slots + 1, sizeof(HydLfgResult)) : NULL;
    if (res)
        cls = hyd_read_blob(blob, size, expected_slots, &view, res, &max_alphabet);
    free(res);
    return cls;
}
#endif
