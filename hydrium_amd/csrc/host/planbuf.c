#include "planbuf.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int hydk_plan_check_metadata(const HYDImageMetadata *md, char *msg, size_t n) {
    HYDEncoder *e = hyd_encoder_new();
    const int st = e ? hyd_set_metadata(e, md) : HYD_NOMEM;
    if (st && e)
        snprintf(msg, n, "%s", hyd_error_message_get(e));
    hyd_encoder_destroy(e);
    return st;
}

size_t buf_reserve(Buf *b, size_t n) {
    const size_t at = (b->len + 15) & ~(size_t)15;
    const size_t need = at + ((n + 15) & ~(size_t)15) + 16;
    if (need > b->cap) {
        size_t ncap = b->cap ? b->cap : 4096;
        while (ncap < need)
            ncap *= 2;
        uint8_t *np = realloc(b->p, ncap);
        if (!np) {
            b->failed = 1;
            return 0;
        }
        memset(np + b->cap, 0, ncap - b->cap);
        b->p = np;
        b->cap = ncap;
    }
    b->len = at + n;
    return at;
}

size_t buf_add_bits(Buf *b, const HydBits *src, uint32_t *bits) {
    const size_t nbytes = src->len + (size_t)((src->nacc + 7) >> 3);
    const size_t at = buf_reserve(b, nbytes ? nbytes : 1);
    if (b->failed)
        return 0;
    memset(b->p + at, 0, (nbytes + 15) & ~(size_t)15);
    if (src->len)
        memcpy(b->p + at, src->data, src->len);
    uint64_t acc = src->acc;
    if (src->nacc < 64)
        acc &= (UINT64_C(1) << src->nacc) - 1;
    for (int i = 0; i * 8 < src->nacc; i++)
        b->p[at + src->len + (size_t)i] = (uint8_t)(acc >> (8 * i));
    *bits = (uint32_t)(src->len * 8 + (size_t)src->nacc);
    return at;
}
