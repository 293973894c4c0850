/*
 * hydk_edges.h — the first and last 32-bit word of a byte-aligned section, written as byte stores of exactly the
 * section's own bytes.  Compiles for host and device (as hydk_half.h does): k_rans_emit's self-placing mode and the
 * stand-alone host test share this text.
 *
 * HF sections lie back to back in the frame's payload at byte offsets, and their writers assemble whole 32-bit words.  A
 * word that holds the end of one section and the start of the next (or, for sections of one to three bytes, up to four of
 * them) has several writers: each stores only the bytes of [lo_byte, hi_byte) that fall into the word, so no writer needs
 * the word cleared first and none touches a neighbour's bytes, in whatever order they run.
 */
#ifndef HYD_SECTION_EDGES_H_
#define HYD_SECTION_EDGES_H_

#include <stdint.h>

#ifdef __HIPCC__
#define HYDK_EDGE_FN __host__ __device__ static inline
#else
#define HYDK_EDGE_FN static inline
#endif

/* which of the four bytes of 32-bit word `word` of the payload lie inside the section [lo_byte, hi_byte): bit b = byte b */
HYDK_EDGE_FN uint32_t hydk_edge_byte_mask(uint64_t word, uint64_t lo_byte, uint64_t hi_byte) {
    const uint64_t w0 = word * 4u, w1 = w0 + 4u;
    const uint64_t a = lo_byte > w0 ? lo_byte : w0, b = hi_byte < w1 ? hi_byte : w1;
    if (a >= b)
        return 0u;
    return (0xFu >> (4u - (uint32_t)(b - a))) << (uint32_t)(a - w0);
}

/* v: the word's content as its section sees it (little endian: byte b is bits 8b .. 8b + 7; foreign bytes are ignored).
 * A word that lies wholly inside the section is one 32-bit store. */
HYDK_EDGE_FN void hydk_store_edge_word(uint8_t *payload, uint64_t word, uint32_t v, uint64_t lo_byte, uint64_t hi_byte) {
    const uint32_t mask = hydk_edge_byte_mask(word, lo_byte, hi_byte);
    if (mask == 0xFu) {
        *(uint32_t *)(payload + word * 4u) = v; /* the payload is at least 4-byte aligned */
        return;
    }
    for (uint32_t b = 0; b < 4u; b++)
        if ((mask >> b) & 1u)
            payload[word * 4u + b] = (uint8_t)(v >> (8u * b));
}

#endif /* HYD_SECTION_EDGES_H_ */
