/*
 * hydk_batch_asm.h — private interface between the host side of the device batches (csrc/host/batchrun.c, batch.c,
 * mixed.c, C99) and the device-side batch assembler (csrc/hip/assemble_batch.hip), which includes it too: a prototype
 * that drifts from its definition does not compile.  Nothing here is exported from the library.
 */
#ifndef HYD_BATCH_ASM_H_
#define HYD_BATCH_ASM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct HydkBatchAsm HydkBatchAsm;

/* all int results are HYDStatusCode-compatible; hydk_batch_error() describes the last failure */
/* frames of the plan's one shape (a HydkAsmPlan of one blob, or a HydkTilePlan of one frame); no plan: frames of one LF
 * group, each of its own size, whose mixed plan comes with every batch */
int hydk_batch_create(int device, int max_frames, const void *plan, size_t plan_bytes, HydkBatchAsm **out);
/* images of 1..28 LF groups each, `max_slots` in all, each of its own size: a frames plan comes with every batch */
int hydk_batch_create_frames(int device, int max_frames, int max_slots, HydkBatchAsm **out);
void hydk_batch_destroy(HydkBatchAsm *a);
const char *hydk_batch_error(HydkBatchAsm *a);
/* bytes a frame of a uniform assembler can add to its packed LF streams and HF sections; fixed at creation */
uint64_t hydk_batch_fixed_bytes(HydkBatchAsm *a);
/* the plan of the batches that follow, copied on `stream` ahead of the assembly that reads it */
int hydk_batch_set_plan(HydkBatchAsm *a, const void *plan, size_t bytes, void *stream);
/* enqueue the assembly of `frames` frames on `stream`, behind whatever fills the view `blob` and its extents */
int hydk_batch_run(HydkBatchAsm *a, uint32_t frames, const void *blob, uint64_t blob_cap, const void *extents, void *stream);
/* the output buffer holds at least `bytes`; waits for `stream` when it has to be replaced */
int hydk_batch_reserve(HydkBatchAsm *a, uint64_t bytes, void *stream);
const uint8_t *hydk_batch_out(HydkBatchAsm *a);
const uint64_t *hydk_batch_offsets_dev(HydkBatchAsm *a);
int hydk_batch_wait(HydkBatchAsm *a, void *stream);
/* after the stream has been synchronised: the device's error word (HYDK_ASM_E_*), the bytes of all files and the host
 * copy of the offsets table ([frames + 1], valid until the next run) */
int hydk_batch_result(HydkBatchAsm *a, uint32_t *err, uint64_t *total, const uint64_t **offsets);
int hydk_batch_read(HydkBatchAsm *a, uint64_t from, uint8_t *dst, size_t n);
/* per-image outcomes for the runs that follow; the frames' status words: host copy ([frames] of 64 bits, valid until
 * the next run) and device copy ([frames] of 32 bits) */
void hydk_batch_set_image_errors(HydkBatchAsm *a, int per_image);
const uint64_t *hydk_batch_status(HydkBatchAsm *a);
const uint32_t *hydk_batch_status_dev(HydkBatchAsm *a);

#ifdef __cplusplus
}
#endif

#endif /* HYD_BATCH_ASM_H_ */
