/*
 * batchrun.c — the host driver of a batch of device-resident images on its way to finished files (batchrun.h): what
 * hydamd_batch_* (batch.c) and hydamd_mixed_* (mixed.c) do once their launch group is planned and enqueued.
 *
 * Policy HERE: ONE context of max_slots slots and one stream; the output is reserved before a batch is enqueued; the
 * host waits once per batch (hydamd_sync, which is also where a batch that outgrew the context's buffers is rerun),
 * checks what the assembly (csrc/hip/assemble_batch.hip) left and repeats it if the batch was rerun; after a failure the
 * stream is drained before the call returns.
 */
#include "batchrun.h"

#include <stdio.h>
#include <string.h>

#include "libhydrium/libhydrium.h"

int hyd_batchrun_fail(HydBatchRun *r, int code, const char *what, const char *detail) {
    snprintf(r->err, sizeof(r->err), "%s%s%s", what, detail && *detail ? ": " : "", detail && *detail ? detail : "");
    return code;
}

/* the calls that come too early or too late send the caller to the owner's result call */
static int result_first(HydBatchRun *r, const char *what) {
    snprintf(r->err, sizeof(r->err), "%s: %s first", what, r->result_call);
    return HYD_API_ERROR;
}

int hyd_batchrun_open(HydBatchRun *r, int device, int max_slots, int linear_light, const char *result_call, char *create_err, size_t n) {
    int st = HYD_API_ERROR;
    r->max_slots = max_slots;
    r->result_call = result_call;
    r->ctx = hydamd_create(device, max_slots, linear_light, 0, &st);
    if (!r->ctx) {
        snprintf(create_err, n, "%s", hydamd_error(NULL));
        return st;
    }
    if ((st = hydamd_set_lf_coder(r->ctx, 2)) != 0 || (st = hydamd_set_rans_waves(r->ctx, 5)) != 0) {
        snprintf(create_err, n, "%s", hydamd_error(r->ctx));
        hydamd_destroy(r->ctx);
        r->ctx = NULL;
    }
    return st;
}

int hyd_batchrun_adopt(HydBatchRun *r, int st, char *create_err, size_t n) {
    if (st) {
        snprintf(create_err, n, "the batch assembler could not be created (status %d)", st);
        hydamd_destroy(r->ctx);
        r->ctx = NULL;
    }
    return st;
}

void hyd_batchrun_close(HydBatchRun *r) {
    if (!r->ctx)
        return;
    (void)hydamd_sync(r->ctx);
    hydk_batch_destroy(r->as);
    hydamd_destroy(r->ctx);
    r->ctx = NULL;
}

int hyd_batchrun_busy(HydBatchRun *r) { return r->in_flight ? result_first(r, "a batch is in flight") : HYD_OK; }

void hyd_batchrun_drain(HydBatchRun *r) {
    (void)hydamd_sync(r->ctx);
    (void)hydk_batch_wait(r->as, hydamd_get_stream(r->ctx));
    r->in_flight = 0;
}

/* The output holds whatever the context's buffers can: their bound for ALL the object's slots — so that only a context
 * that has enlarged its buffers (a rerun) or a plan of larger prefixes makes it grow — plus what the plan and the
 * assembler's scratch add (r->fixed).  Replacing the buffer waits for the stream, so it is reserved BEFORE a batch is
 * enqueued (an object's first batch allocates, later ones find it there), and looked at again before every assembly. */
int hyd_batchrun_reserve(HydBatchRun *r) {
    const uint64_t want = (uint64_t)hydamd_blob_bound(r->ctx, r->max_slots) + r->fixed;
    const int st = hydk_batch_reserve(r->as, want, hydamd_get_stream(r->ctx));
    return st ? hyd_batchrun_fail(r, st, "output buffer", hydk_batch_error(r->as)) : HYD_OK;
}

int hyd_batchrun_assemble(HydBatchRun *r) {
    const void *blob = NULL, *ext = NULL;
    size_t cap = 0;
    void *stream = hydamd_get_stream(r->ctx);
    int st = hyd_batchrun_reserve(r);
    if (st)
        return st;
    st = hydamd_export_batch_owned(r->ctx, r->slots, &blob, &cap, &ext);
    if (st)
        return hyd_batchrun_fail(r, st, "batch view", hydamd_error(r->ctx));
    st = hydk_batch_run(r->as, (uint32_t)r->frames, blob, cap, ext, stream);
    return st ? hyd_batchrun_fail(r, st, "batch assembly", hydk_batch_error(r->as)) : HYD_OK;
}

/* the batch in flight: wait, let hydamd_sync rerun it if it outgrew a buffer, and see its frames into their files */
static int settle(HydBatchRun *r) {
    const unsigned before = hydamd_overflow_reruns(r->ctx);
    int st = hydamd_sync(r->ctx);
    if (st)
        return hyd_batchrun_fail(r, st, "batch", hydamd_error(r->ctx));
    r->reruns += hydamd_overflow_reruns(r->ctx) - before;
    for (int attempt = 0; attempt < 4; attempt++) {
        uint32_t err = 0;
        uint64_t total = 0;
        const uint64_t *offsets = NULL;
        hydk_batch_result(r->as, &err, &total, &offsets);
        if (!err) {
            r->total = (size_t)total;
            memcpy(r->offsets, offsets, ((size_t)r->frames + 1) * sizeof(uint64_t));
            for (int f = 0; f < r->frames; f++)
                r->status[f] = (uint32_t)hydk_batch_status(r->as)[f];
            return HYD_OK;
        }
        if (err & HYDK_ASM_E_NAN)
            return hyd_batchrun_fail(r, HYD_API_ERROR, "Invalid NaN Float", NULL);
        if (err & HYDK_ASM_E_SPACE) /* the output was sized from the context's capacities */
            return hyd_batchrun_fail(r, HYD_INTERNAL_ERROR, "the batch's files are larger than the bound of their output buffer", NULL);
        if (err & (HYDK_ASM_E_BLOB | HYDK_ASM_E_SLOT | HYDK_ASM_E_HEAD | HYDK_ASM_E_SIZE | HYDK_ASM_E_SCRATCH))
            return hyd_batchrun_fail(r, HYD_INTERNAL_ERROR, "batch assembly failed on the device", NULL);
        /* RETRY: the assembly saw the first run's incomplete results (hydamd_sync has rerun the batch since): the view
         * and the same launches again, with the plan that is still on the device, into an output sized for the enlarged context */
        if ((st = hyd_batchrun_assemble(r)) != 0)
            return st;
        if ((st = hydk_batch_wait(r->as, hydamd_get_stream(r->ctx))) != 0)
            return hyd_batchrun_fail(r, st, "batch assembly", hydk_batch_error(r->as));
    }
    return hyd_batchrun_fail(r, HYD_INTERNAL_ERROR, "a batch is still incomplete after its rerun", NULL);
}

int hyd_batchrun_result(HydBatchRun *r, size_t *total_bytes) {
    if (!r)
        return HYD_API_ERROR;
    if (!r->have_result) {
        if (!r->in_flight)
            return hyd_batchrun_fail(r, HYD_API_ERROR, "no batch in flight", NULL);
        const int st = settle(r);
        if (st) {
            hyd_batchrun_drain(r);
            return st;
        }
        r->in_flight = 0;
        r->have_result = 1;
    }
    if (total_bytes)
        *total_bytes = r->total;
    return HYD_OK;
}

int hyd_batchrun_offsets(HydBatchRun *r, uint64_t *offsets) {
    if (!r || !r->have_result)
        return r ? result_first(r, "no finished batch") : HYD_API_ERROR;
    if (!offsets)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "null output pointer", NULL);
    memcpy(offsets, r->offsets, ((size_t)r->frames + 1) * sizeof(uint64_t));
    return HYD_OK;
}

int hyd_batchrun_read(HydBatchRun *r, int frame, uint8_t *dst, size_t capacity) {
    if (!r || !r->have_result)
        return r ? result_first(r, "no finished batch") : HYD_API_ERROR;
    if (!dst)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "null output pointer", NULL);
    if (frame < -1 || frame >= r->frames)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "no such frame in the batch", NULL);
    const uint64_t from = frame < 0 ? 0 : r->offsets[frame], to = frame < 0 ? r->total : r->offsets[frame + 1];
    if (capacity < to - from)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "output buffer too small", NULL);
    const int st = hydk_batch_read(r->as, from, dst, (size_t)(to - from));
    return st ? hyd_batchrun_fail(r, st, "read-back", hydk_batch_error(r->as)) : HYD_OK;
}

const uint8_t *hyd_batchrun_device(HydBatchRun *r) { return r && r->have_result ? hydk_batch_out(r->as) : NULL; }

const uint64_t *hyd_batchrun_offsets_device(HydBatchRun *r) { return r && r->have_result ? hydk_batch_offsets_dev(r->as) : NULL; }

/* per-image outcomes: the context flags non-finite float samples per slot and codes them as 0.0, the assembly gives a
 * flagged image no bytes and a status word; off, a NaN fails the batch as hydamd_sync and the view's header report it */
int hyd_batchrun_set_image_errors(HydBatchRun *r, int per_image) {
    if (!r)
        return HYD_API_ERROR;
    if (r->in_flight)
        return hyd_batchrun_busy(r);
    const int st = hydamd_set_bad_sample_per_slot(r->ctx, per_image != 0);
    if (st)
        return hyd_batchrun_fail(r, st, "image errors", hydamd_error(r->ctx));
    hydk_batch_set_image_errors(r->as, per_image != 0);
    return HYD_OK;
}

int hyd_batchrun_image_status(HydBatchRun *r, uint32_t *status) {
    if (!r || !r->have_result)
        return r ? result_first(r, "no finished batch") : HYD_API_ERROR;
    if (!status)
        return hyd_batchrun_fail(r, HYD_API_ERROR, "null output pointer", NULL);
    memcpy(status, r->status, (size_t)r->frames * sizeof(uint32_t));
    return HYD_OK;
}

const uint32_t *hyd_batchrun_image_status_device(HydBatchRun *r) { return r && r->have_result ? hydk_batch_status_dev(r->as) : NULL; }
