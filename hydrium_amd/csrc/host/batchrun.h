/*
 * batchrun.h — the host driver both device-batch objects embed (batch.c: images of one shape; mixed.c: each of its own
 * size): one context and one stream, one batch in flight, its files and their offsets once it has settled.  The owner
 * plans, checks its arguments and enqueues the launch group; everything behind that is here.  Internal: nothing is exported.
 */
#ifndef HYD_BATCHRUN_H_
#define HYD_BATCHRUN_H_

#include <stddef.h>
#include <stdint.h>

#include "hydrium_amd.h"

#include "../hip/hydk_batch_asm.h"
#include "../hip/hydk_tiles.h"

#if HYDAMD_MAX_LF_GROUPS != HYDK_TILE_MAX_FRAMES
#error "a batch has at most as many frames as a context has LF-group slots: one bound sizes the tables below"
#endif

typedef struct HydBatchRun {
    HydAmdContext *ctx;
    HydkBatchAsm *as;        /* the owner's, made between hyd_batchrun_open and hyd_batchrun_adopt */
    int max_slots;           /* LF-group slots of the context */
    int frames, slots;       /* of the batch in flight / finished: the owner sets both before it reserves */
    uint64_t fixed;          /* the plan's share of the output reservation: the owner's to keep current */
    int in_flight, have_result;
    size_t total;
    uint64_t offsets[HYDK_TILE_MAX_FRAMES + 1];
    uint32_t status[HYDK_TILE_MAX_FRAMES]; /* of the finished batch's images */
    unsigned reruns;
    const char *result_call; /* the owner's result call, as the messages that send the caller there name it */
    char err[256];
} HydBatchRun;

/* sets r->err ("what: detail") and returns code */
int hyd_batchrun_fail(HydBatchRun *r, int code, const char *what, const char *detail);
/* a context of max_slots slots that codes as the batches need it (LF coder mode 2, lane-form rANS).  A failure leaves
 * nothing behind and its message in create_err, the owner's create-error buffer. */
int hyd_batchrun_open(HydBatchRun *r, int device, int max_slots, int linear_light, const char *result_call, char *create_err, size_t n);
/* the owner's assembler behind it: `st` is what its constructor, called into r->as, returned.  A failure closes r. */
int hyd_batchrun_adopt(HydBatchRun *r, int st, char *create_err, size_t n);
void hyd_batchrun_close(HydBatchRun *r);
/* "a batch is in flight: <result call> first" when one is */
int hyd_batchrun_busy(HydBatchRun *r);
/* after a failure once work was enqueued: nothing of this object is left running when the call returns */
void hyd_batchrun_drain(HydBatchRun *r);
int hyd_batchrun_reserve(HydBatchRun *r);
/* the batch's results as a view, and its assembly behind them */
int hyd_batchrun_assemble(HydBatchRun *r);
/* what the exported hydamd_batch_* / hydamd_mixed_* calls of the same names forward to (r NULL: as they answer a null object) */
int hyd_batchrun_result(HydBatchRun *r, size_t *total_bytes);
int hyd_batchrun_offsets(HydBatchRun *r, uint64_t *offsets);
int hyd_batchrun_read(HydBatchRun *r, int frame, uint8_t *dst, size_t capacity);
const uint8_t *hyd_batchrun_device(HydBatchRun *r);
const uint64_t *hyd_batchrun_offsets_device(HydBatchRun *r);
int hyd_batchrun_set_image_errors(HydBatchRun *r, int per_image);
int hyd_batchrun_image_status(HydBatchRun *r, uint32_t *status);
const uint32_t *hyd_batchrun_image_status_device(HydBatchRun *r);

#endif /* HYD_BATCHRUN_H_ */
