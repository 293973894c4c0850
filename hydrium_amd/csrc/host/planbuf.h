/*
 * planbuf.h — the growing buffer a device-side assembler's PLAN is built in (assembler.c, tiled.c): 16-byte aligned
 * records and bit strings as zero-padded words, addressed by their byte offsets.
 */
#ifndef HYD_PLANBUF_H_
#define HYD_PLANBUF_H_

#include <stddef.h>
#include <stdint.h>

#include "bitio.h"
#include "libhydrium/libhydrium.h"

typedef struct Buf {
    uint8_t *p;
    size_t len, cap;
    int failed;
} Buf;

/* returns the 16-byte aligned offset of n fresh zero bytes */
size_t buf_reserve(Buf *b, size_t n);
/* a bit string (whole bytes + pending bits of a HydBits) as zero-padded words; returns its offset, *bits its length */
size_t buf_add_bits(Buf *b, const HydBits *src, uint32_t *bits);

/* the bytes a plan is made of are written by an encoder object, which also checks the image's bounds: what it says to
 * `md` (its message in msg[n] when it refuses) */
int hydk_plan_check_metadata(const HYDImageMetadata *md, char *msg, size_t n);

/* the planners themselves, for the objects that build plans of their own (batch.c):
 * assembler.c — the plan of one frame (csrc/hip/hydk_assemble.h) from its description as hydamd_assembler_plan takes it;
 * *plan_out is malloc'ed.  The caller has checked the description (every LF group once, at most 255, not 128).
 * tiled.c — the constant sub-streams of one frame shape of one LF group (csrc/hip/hydk_tiles.h), appended to `b`
 * batch.c — the prefix of a one-frame image of one LF group (file header, frame header with is_last), appended to `b` */
int hydk_plan_frame(const HYDImageMetadata *md, int write_header, int is_last, size_t nblobs, const uint32_t *blob_slots,
                    const uint32_t *lf_ids, const uint8_t *icc, size_t icc_size, uint8_t **plan_out, size_t *plan_len, const char **err);
struct HydkTileShape;
struct HydkTileFrame;
int hydk_tile_plan_shape(Buf *b, HydBits *bits, HydBits *part, size_t w, size_t h, struct HydkTileShape *sh, const char **err);
int hydk_plan_one_frame_prefix(Buf *b, HydBits *bits, const HYDImageMetadata *md, const uint8_t *icc, size_t icc_size,
                               struct HydkTileFrame *fr, const char **err);

#ifdef HYD_TEST_HOOKS
/* tiled.c — the batched layout (hydk_tiles.h compiled for the host) over `nframes` frames of a plan, frame f laid out by
 * frames[f] and shapes[frames[f].shape], on stage results as hydt_tiles_from_streams takes them: what both CPU hooks run */
struct HydAmdLfStream;
int hydt_layout_from_streams(const uint8_t *plan, const struct HydkTileFrame *frames, const struct HydkTileShape *shapes, size_t nframes,
                             const struct HydAmdLfStream *lf, const uint32_t *freq, const uint32_t *alphabet, const uint32_t *group_bits,
                             const uint32_t *max_alphabet, const uint8_t *payload, size_t payload_len, uint64_t *frame_offsets,
                             uint8_t **out, size_t *out_len, const char **err);
/* the same with an outcome per image: flags[f] as the slot record would carry it; a flagged frame yields no bytes */
int hydt_layout_from_streams_skip(const uint8_t *plan, const struct HydkTileFrame *frames, const struct HydkTileShape *shapes, size_t nframes,
                                  const struct HydAmdLfStream *lf, const uint32_t *freq, const uint32_t *alphabet, const uint32_t *group_bits,
                                  const uint32_t *max_alphabet, const uint8_t *payload, size_t payload_len, const uint32_t *flags,
                                  uint64_t *frame_offsets, uint32_t *status, uint64_t *piece_bits, uint8_t **out, size_t *out_len,
                                  const char **err);
#endif

#endif /* HYD_PLANBUF_H_ */
