/*
 * hostframe.h — a frame written on the host from read-back results: what a context (or a blob a context exported) knows
 * about each LF group of the frame, the fillers that bring it into host memory, and the writer that wraps it into
 * LFGlobal, LF groups, HFGlobal, TOC and frame header around the device-coded HF sections.  Knows contexts and bit
 * buffers, not encoders: hyd_send_tile (encoder.c) and the no-GPU hydamd_frame_from_* entry points are its callers.
 */
#ifndef HYD_HOSTFRAME_H_
#define HYD_HOSTFRAME_H_

#include <stdio.h>

#include "frame.h"
#include "hydrium_amd.h"

/* HYDAMD_TRACE=1 prints where the host-pointer API path spends its wall time (stderr) */
double hyd_now_ms(void);
int hyd_trace_on(void);
#define TRACE_MS(label, ms)                                               \
    do {                                                                  \
        if (hyd_trace_on())                                               \
            fprintf(stderr, "[hydrium] %-28s %8.3f ms\n", (label), (ms)); \
    } while (0)
#define TRACE(label, t0) TRACE_MS(label, hyd_now_ms() - (t0))

typedef struct HydLfgResult {
    int32_t *dc; /* [3][vbh][vbw]; NULL when the LF coefficients were coded on the device */
    uint8_t *lf_bits;                    /* device-coded LF-coefficient symbols (borrowed) or NULL */
    uint8_t lf_lengths[HYD_LF_CODES];
    uint32_t lf_alphabet, lf_run_pairs, lf_bit_count;
    uint32_t freq[HYD_FRAME_MAX_CLUSTERS][HYD_FRAME_ALPHABET];
    uint32_t alphabet[HYD_FRAME_MAX_CLUSTERS];
    uint32_t bits[HYDAMD_GROUPS_PER_LFG];
} HydLfgResult;

/* frame groups (256 x 256) of the frame: one means a single bit-contiguous section, more a TOC of byte-padded ones */
static inline size_t hyd_frame_groups(const HydFrameShape *shape) {
    return ((shape->frame_width + 255) >> 8) * ((shape->frame_height + 255) >> 8);
}

/* ---- Two classes of failure: the host's (no memory, an inconsistent frame description) set *err; a device call's — its
 * status, or HYD_INTERNAL_ERROR for a device record that points outside its buffer — set *device_failed and leave the
 * message to the caller, who knows what else a failed device means to it. ---- */
/* the coded LF streams of slots 0 .. count-1 of ctx in two copies; res[s].lf_bits borrow from *blob, which the caller frees */
int hyd_read_lf_results(HydAmdContext *ctx, size_t count, HydLfgResult *res, uint8_t **blob, int *device_failed,
                        const char **err);
/* tables and section sizes of slots 0 .. count-1 (LF groups lfg[0 .. count-1]), slot by slot, and when the LF coder is off
 * the LF ints (res[s].dc, the caller frees); *max_alphabet keeps the running maximum.  Every failure is the device's. */
int hyd_read_table_results(HydAmdContext *ctx, const HydFrameLfg *lfg, size_t count, HydLfgResult *res, unsigned *max_alphabet);

/* The one reader of the blobs hydamd_export_frame / hydamd_stage_frame_blob write.  Every size is checked against the
 * blob's own length before it enters a sum, nothing beyond `size` is read.  res == NULL: header only. */
enum {
    HYD_BLOB_USABLE = 0,
    HYD_BLOB_NOT_USABLE, /* magic, version, lf_coded, total_bytes > size, HYDAMD_BLOB_RETRY, or not `expected_slots` (> 0) slots */
    HYD_BLOB_MALFORMED,  /* its sizes do not add up */
    HYD_BLOB_TABLE_ERROR, HYD_BLOB_LF_ERROR, HYD_BLOB_LF_RANGE /* a slot: the device's two error words, an LF stream outside lf_bytes */
};
typedef struct HydBlobView {
    HydAmdBlobHeader header; /* a copy: the blob is a byte string and may lie at any address */
    int has_header;          /* 0: the blob is shorter than a header */
    const uint8_t *slots;    /* header.num_slots records of sizeof(HydAmdBlobSlot) bytes, at any address: read field by field */
    const uint8_t *hf;       /* the packed HF sections */
    size_t hf_len;
} HydBlobView;
uint32_t hyd_blob_slot_preset(const HydBlobView *view, uint32_t i);
int hyd_read_blob(const void *blob, size_t size, size_t expected_slots, HydBlobView *view, HydLfgResult *res,
                  unsigned *max_alphabet);

typedef struct HydPayloadSegments { /* for the writer: the packed HF sections in pieces (one per shard blob) instead of one string */
    size_t count;
    const uint8_t *const *ptr;
    const size_t *len;
} HydPayloadSegments;

int hyd_code_lf_groups_parallel(const HydFrameShape *shape, const HydLfgResult *res, HydBits *out, const char **err);
/* Appends the frame to `stream`.  payload == NULL: the packed HF sections are still on the device (`dev`) and are copied
 * straight into the stream; a failure of that copy is returned with *device_failed set, every other failure with *err */
int hyd_assemble_frame(HydBits *stream, const char **err, HydAmdContext *dev, int *device_failed, const HydFrameShape *shape,
                       const HydLfgResult *res, unsigned max_alphabet, const uint8_t *payload, size_t payload_len,
                       HydBits *lf_prebuilt, const HydPayloadSegments *segs);

#endif /* HYD_HOSTFRAME_H_ */
