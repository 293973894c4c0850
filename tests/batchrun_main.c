/*
 * batchrun_main.c — the batch driver (hydrium_amd/csrc/host/batchrun.c) alone, without a device: the context and the
 * assembler are stubs that hand it a scripted sequence of result words, and the program checks what the driver returns,
 * says and remembers for each.  Built with the address and undefined-behaviour sanitizers and run by
 * tests/test_batch_driver_api.py; exit status 0 and "ok" on its output when every check held.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "batchrun.h"
#include "libhydrium/libhydrium.h"

static int g_ctx, g_asm; /* what the opaque pointers point at */
static uint32_t g_script[8];
static int g_at, g_runs, g_waits, g_syncs;
static uint64_t g_h_result[2 + 3 + 2]; /* total, pad, offsets[3], status[2] */

HydAmdContext *hydamd_create(int device, int max_lf_groups, int linear_light, int debug_planes, int *status) {
    *status = device ? HYD_INTERNAL_ERROR : HYD_OK;
    return device ? NULL : (HydAmdContext *)&g_ctx;
}
void hydamd_destroy(HydAmdContext *ctx) {}
const char *hydamd_error(HydAmdContext *ctx) { return ctx ? "context error" : "create error"; }
void *hydamd_get_stream(HydAmdContext *ctx) { return NULL; }
int hydamd_set_rans_waves(HydAmdContext *ctx, int waves) { return waves == 5 ? HYD_OK : HYD_API_ERROR; }
int hydamd_set_lf_coder(HydAmdContext *ctx, int on_device) { return on_device == 2 ? HYD_OK : HYD_API_ERROR; }
int hydamd_sync(HydAmdContext *ctx) { return g_syncs++, HYD_OK; }
int hydamd_set_bad_sample_per_slot(HydAmdContext *ctx, int on) { return HYD_OK; }
unsigned hydamd_overflow_reruns(HydAmdContext *ctx) { return (unsigned)g_syncs; } /* (every wait has rerun the batch) */
size_t hydamd_blob_bound(HydAmdContext *ctx, int num_slots) { return 1000u * (size_t)num_slots; }
int hydamd_export_batch_owned(HydAmdContext *ctx, int num_slots, const void **blob_dev, size_t *capacity, const void **extents_dev) {
    *blob_dev = *extents_dev = &g_ctx;
    *capacity = 64;
    return HYD_OK;
}

void hydk_batch_destroy(HydkBatchAsm *a) {}
const char *hydk_batch_error(HydkBatchAsm *a) { return "assembler error"; }
int hydk_batch_run(HydkBatchAsm *a, uint32_t frames, const void *blob, uint64_t blob_cap, const void *extents, void *stream) {
    return g_runs++, HYD_OK;
}
int hydk_batch_reserve(HydkBatchAsm *a, uint64_t bytes, void *stream) { return bytes == 2000u + 77u ? HYD_OK : HYD_INTERNAL_ERROR; }
const uint8_t *hydk_batch_out(HydkBatchAsm *a) { return (const uint8_t *)&g_asm; }
const uint64_t *hydk_batch_offsets_dev(HydkBatchAsm *a) { return g_h_result + 2; }
int hydk_batch_wait(HydkBatchAsm *a, void *stream) { return g_waits++, HYD_OK; }
int hydk_batch_result(HydkBatchAsm *a, uint32_t *err, uint64_t *total, const uint64_t **offsets) {
    *err = g_script[g_at++];
    *total = g_h_result[0];
    *offsets = g_h_result + 2;
    return HYD_OK;
}
int hydk_batch_read(HydkBatchAsm *a, uint64_t from, uint8_t *dst, size_t n) { return memset(dst, (int)from, n), HYD_OK; }
void hydk_batch_set_image_errors(HydkBatchAsm *a, int per_image) {}
const uint64_t *hydk_batch_status(HydkBatchAsm *a) { return g_h_result + 5; }
const uint32_t *hydk_batch_status_dev(HydkBatchAsm *a) { return NULL; }

#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("line %d: %s (err \"%s\")\n", __LINE__, #x, r.err); \
            return 1;                                                \
        }                                                            \
    } while (0)

/* a batch of two frames in flight, the result words it will meet; returns what the result call says */
static int settle(HydBatchRun *r, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    const uint32_t script[4] = {w0, w1, w2, w3};
    memcpy(g_script, script, sizeof(script));
    g_at = g_runs = g_waits = 0;
    r->frames = r->slots = 2;
    r->have_result = 0;
    r->in_flight = 1;
    r->err[0] = 0;
    size_t total = 0;
    const int st = hyd_batchrun_result(r, &total);
    return st ? st : total == g_h_result[0] ? HYD_OK : 1;
}

int main(void) {
    HydBatchRun r;
    char create_err[256] = "";
    uint8_t out[16];
    uint64_t off[3];
    uint32_t status[2];
    memset(&r, 0, sizeof(r));
    CHECK(hyd_batchrun_open(&r, 1, 2, 0, "hydamd_test_result", create_err, sizeof(create_err)) == HYD_INTERNAL_ERROR && !r.ctx);
    CHECK(!strcmp(create_err, "create error"));
    CHECK(hyd_batchrun_open(&r, 0, 2, 0, "hydamd_test_result", create_err, sizeof(create_err)) == HYD_OK && r.ctx && r.max_slots == 2);
    CHECK(hyd_batchrun_adopt(&r, HYD_NOMEM, create_err, sizeof(create_err)) == HYD_NOMEM && !r.ctx);
    CHECK(!strcmp(create_err, "the batch assembler could not be created (status -13)"));
    CHECK(hyd_batchrun_open(&r, 0, 2, 0, "hydamd_test_result", create_err, sizeof(create_err)) == HYD_OK);
    r.as = (HydkBatchAsm *)&g_asm;
    CHECK(hyd_batchrun_adopt(&r, HYD_OK, create_err, sizeof(create_err)) == HYD_OK && r.ctx);
    r.fixed = 77;
    g_h_result[0] = 9, g_h_result[2] = 0, g_h_result[3] = 4, g_h_result[4] = 9, g_h_result[5] = 0, g_h_result[6] = 1;

    /* nothing in flight, nothing finished */
    CHECK(hyd_batchrun_result(&r, NULL) == HYD_API_ERROR && !strcmp(r.err, "no batch in flight"));
    CHECK(hyd_batchrun_offsets(&r, off) == HYD_API_ERROR && !strcmp(r.err, "no finished batch: hydamd_test_result first"));
    CHECK(hyd_batchrun_read(&r, 0, out, sizeof(out)) == HYD_API_ERROR && !strcmp(r.err, "no finished batch: hydamd_test_result first"));
    CHECK(hyd_batchrun_image_status(&r, status) == HYD_API_ERROR && !strcmp(r.err, "no finished batch: hydamd_test_result first"));
    CHECK(!hyd_batchrun_device(&r) && !hyd_batchrun_offsets_device(&r) && !hyd_batchrun_image_status_device(&r));
    CHECK(hyd_batchrun_busy(&r) == HYD_OK && hyd_batchrun_reserve(&r) == HYD_OK);
    CHECK(hyd_batchrun_result(NULL, NULL) == HYD_API_ERROR && hyd_batchrun_offsets(NULL, off) == HYD_API_ERROR && !hyd_batchrun_device(NULL));

    /* OK at once: no assembly repeated */
    CHECK(settle(&r, 0, 0, 0, 0) == HYD_OK && g_at == 1 && g_runs == 0 && !r.in_flight && r.have_result && r.total == 9);
    CHECK(r.offsets[1] == 4 && r.offsets[2] == 9 && r.status[0] == 0 && r.status[1] == 1 && r.reruns == 1);
    CHECK(hyd_batchrun_result(&r, NULL) == HYD_OK && g_at == 1); /* (asked again: the same answer, no second wait) */
    CHECK(hyd_batchrun_offsets(&r, off) == HYD_OK && off[2] == 9 && hyd_batchrun_image_status(&r, status) == HYD_OK && status[1] == 1);
    CHECK(hyd_batchrun_read(&r, 1, out, 5) == HYD_OK && out[0] == 4 && hyd_batchrun_read(&r, -1, out, 9) == HYD_OK && out[8] == 0);
    CHECK(hyd_batchrun_read(&r, 2, out, sizeof(out)) == HYD_API_ERROR && !strcmp(r.err, "no such frame in the batch"));
    CHECK(hyd_batchrun_read(&r, 1, out, 4) == HYD_API_ERROR && !strcmp(r.err, "output buffer too small"));
    CHECK(hyd_batchrun_read(&r, 0, NULL, 4) == HYD_API_ERROR && !strcmp(r.err, "null output pointer"));
    CHECK(hyd_batchrun_device(&r) && hyd_batchrun_offsets_device(&r));
    /* RETRY, then OK: one more assembly and one wait for it */
    CHECK(settle(&r, HYDK_ASM_E_RETRY, 0, 0, 0) == HYD_OK && g_at == 2 && g_runs == 1 && g_waits == 1 && !r.in_flight && r.have_result);
    /* the refusals: the stream drained, nothing in flight, no result */
    CHECK(settle(&r, HYDK_ASM_E_NAN, 0, 0, 0) == HYD_API_ERROR && !strcmp(r.err, "Invalid NaN Float") && g_runs == 0 && g_waits == 1);
    CHECK(!r.in_flight && !r.have_result);
    CHECK(settle(&r, HYDK_ASM_E_SPACE, 0, 0, 0) == HYD_INTERNAL_ERROR && g_runs == 0 && !r.in_flight && !r.have_result);
    CHECK(!strcmp(r.err, "the batch's files are larger than the bound of their output buffer"));
    CHECK(settle(&r, HYDK_ASM_E_RETRY | HYDK_ASM_E_SLOT, 0, 0, 0) == HYD_INTERNAL_ERROR && !strcmp(r.err, "batch assembly failed on the device"));
    /* four RETRYs: four assemblies, then it gives up */
    CHECK(settle(&r, HYDK_ASM_E_RETRY, HYDK_ASM_E_RETRY, HYDK_ASM_E_RETRY, HYDK_ASM_E_RETRY) == HYD_INTERNAL_ERROR);
    CHECK(g_at == 4 && g_runs == 4 && g_waits == 5 && !r.in_flight && !r.have_result);
    CHECK(!strcmp(r.err, "a batch is still incomplete after its rerun"));
    /* in flight: who comes now is sent to the owner's result call */
    r.in_flight = 1;
    CHECK(hyd_batchrun_busy(&r) == HYD_API_ERROR && !strcmp(r.err, "a batch is in flight: hydamd_test_result first"));
    CHECK(hyd_batchrun_set_image_errors(&r, 1) == HYD_API_ERROR && !strcmp(r.err, "a batch is in flight: hydamd_test_result first"));
    r.in_flight = 0;
    CHECK(hyd_batchrun_set_image_errors(&r, 1) == HYD_OK);
    r.fixed = 78; /* a bound the stub's output cannot hold */
    CHECK(hyd_batchrun_reserve(&r) == HYD_INTERNAL_ERROR && !strcmp(r.err, "output buffer: assembler error"));
    hyd_batchrun_close(&r);
    CHECK(!r.ctx);
    hyd_batchrun_close(&r); /* (closed twice: nothing to do) */
    puts("ok");
    return 0;
}
