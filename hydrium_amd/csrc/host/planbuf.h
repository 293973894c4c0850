/*
 * planbuf.h — the growing buffer a device-side assembler's PLAN is built in (assembler.c, tiled.c): 16-byte aligned
 * records and bit strings as zero-padded words, addressed by their byte offsets.
 */
#ifndef HYD_PLANBUF_H_
#define HYD_PLANBUF_H_

#include <stddef.h>
#include <stdint.h>

#include "bitio.h"

typedef struct Buf {
    uint8_t *p;
    size_t len, cap;
    int failed;
} Buf;

/* returns the 16-byte aligned offset of n fresh zero bytes */
size_t buf_reserve(Buf *b, size_t n);
/* a bit string (whole bytes + pending bits of a HydBits) as zero-padded words; returns its offset, *bits its length */
size_t buf_add_bits(Buf *b, const HydBits *src, uint32_t *bits);

#endif /* HYD_PLANBUF_H_ */
