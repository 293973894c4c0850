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

/* the planners themselves, for the objects that build plans of their own (batch.c):
 * assembler.c — the plan of one frame (csrc/hip/hydk_assemble.h) from its description as hydamd_assembler_plan takes it;
 * *plan_out is malloc'ed.  The caller has checked the description (every LF group once, at most 255, not 128).
 * tiled.c — the constant sub-streams of one frame shape of one LF group (csrc/hip/hydk_tiles.h), appended to `b` */
int hydk_plan_frame(const HYDImageMetadata *md, int write_header, int is_last, size_t nblobs, const uint32_t *blob_slots,
                    const uint32_t *lf_ids, const uint8_t *icc, size_t icc_size, uint8_t **plan_out, size_t *plan_len, const char **err);
struct HydkTileShape;
int hydk_tile_plan_shape(Buf *b, HydBits *bits, HydBits *part, size_t w, size_t h, struct HydkTileShape *sh, const char **err);

#endif /* HYD_PLANBUF_H_ */
