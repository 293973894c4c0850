/*
 * hydk_pieces.h — an output as a sorted list of PIECES, each one bit string at a bit position, and the composition
 * of its 32-bit words.  Both device-side assemblers describe what they write this way (assemble.hip: the sections of
 * one frame at byte-aligned positions; assemble_tiles.hip: the bit strings of many tile frames) and one kernel,
 * k_pieces_copy (assemble.hip), stores it.  Like hydk_sections.h the same source runs on the host: tests/test_pieces.py
 * holds it to a bit-by-bit model, tests/test_tiled_sections.py to frame.c.
 *
 * Pieces are in output order and do not overlap; bits no piece covers (the padding that ends a section) read as zero;
 * empty pieces may stand anywhere in the list.
 */
#ifndef HYD_PIECES_H_
#define HYD_PIECES_H_

#include <stdint.h>

#include "hydk_sections.h"

typedef struct HydkPiece {
    uint64_t dst_bit, nbits;
    const uint32_t *src; /* 4-byte aligned */
    uint32_t src_bit;    /* first bit of the string inside src[0] (a byte string that starts off a word boundary) */
    uint32_t pad;
} HydkPiece;

/* `src`: any byte address */
HYDK_HD HydkPiece hydk_piece(uint64_t dst_bit, const void *src, uint64_t nbits) {
    HydkPiece p;
    const uintptr_t a = (uintptr_t)src;
    p.dst_bit = dst_bit;
    p.nbits = nbits;
    p.src = (const uint32_t *)(a & ~(uintptr_t)3);
    p.src_bit = (uint32_t)(a & 3u) * 8u;
    p.pad = 0;
    return p;
}

/* bits [q, q + 32) of a piece's string as an output word sees them; zero outside the string.  Reads no word of the
 * source that holds none of the string's bits. */
HYDK_HD uint32_t hydk_piece_bits(const HydkPiece *p, int64_t q) {
    if (!p->nbits || q <= -32 || q >= (int64_t)p->nbits)
        return 0;
    const uint64_t lo = q < 0 ? 0 : (uint64_t)q;
    const uint64_t hi = (uint64_t)(q + 32) < p->nbits ? (uint64_t)(q + 32) : p->nbits;
    const uint32_t n = (uint32_t)(hi - lo);
    const uint64_t a = (uint64_t)p->src_bit + lo;
    const uint64_t i = a >> 5;
    const uint32_t sh = (uint32_t)(a & 31u);
    uint32_t v = p->src[i] >> sh;
    if (sh && sh + n > 32u)
        v |= p->src[i + 1] << (32u - sh);
    if (n < 32u)
        v &= (1u << n) - 1u;
    return v << (uint32_t)((int64_t)lo - q);
}

/* output word W (bits [32 W, 32 W + 32) of the output) from a sorted piece list; ends[i] = dst_bit + nbits of piece i */
HYDK_HD uint32_t hydk_pieces_word(const HydkPiece *P, const uint64_t *ends, uint32_t np, uint64_t W) {
    const uint64_t b0 = W * 32u;
    uint32_t lo = 0, hi = np; /* the first piece that ends behind b0 */
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if (ends[m] > b0)
            hi = m;
        else
            lo = m + 1;
    }
    uint32_t v = 0;
    for (uint32_t i = lo; i < np && P[i].dst_bit < b0 + 32u; i++)
        v |= hydk_piece_bits(&P[i], (int64_t)b0 - (int64_t)P[i].dst_bit);
    return v;
}

/* word W of `out` (4-byte aligned) for a writer that owns bytes [b_lo, b_hi): a word inside the range is stored whole,
 * one it shares with a neighbour (the first or the last) byte by byte — nothing is zeroed beforehand, nothing ORed */
HYDK_HD void hydk_store_word(uint8_t *out, uint64_t W, uint32_t v, uint64_t b_lo, uint64_t b_hi) {
    const uint64_t b0 = W * 4u;
    if (b0 >= b_lo && b0 + 4 <= b_hi) {
        ((uint32_t *)out)[W] = v;
        return;
    }
    for (uint32_t j = 0; j < 4; j++)
        if (b0 + j >= b_lo && b0 + j < b_hi)
            out[b0 + j] = (uint8_t)(v >> (8u * j));
}

#endif /* HYD_PIECES_H_ */
