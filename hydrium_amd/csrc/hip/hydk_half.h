/*
 * hydk_half.h — half-precision samples widened to float32, exactly.  Compiles for host and device (as hydk_sections.h
 * does): the transform kernel's loader, the probe flavour's test entries and the stand-alone host tests share this text.
 *
 * Integer bit manipulation only, so that no denormal mode of either processor has a say: binary16 subnormals come out as
 * the float32 normals they are, signed zero keeps its sign, and an all-ones exponent stays all ones (infinities, and NaNs
 * with their payload moved up) — which is what the float class's non-finite check looks at.
 */
#ifndef HYD_HALF_WIDEN_H_
#define HYD_HALF_WIDEN_H_

#include <stdint.h>

#include "hydk_store.h" /* HYDK_STORE_F32, _F16, _BF16: the storage forms of a float-class LF group */

#ifdef __HIPCC__
#define HYDK_HALF_FN __host__ __device__ static inline
#else
#define HYDK_HALF_FN static inline
#endif

/* bfloat16 is the upper half of a float32 */
HYDK_HALF_FN uint32_t hydk_widen_bf16(uint32_t bits) { return (bits & 0xFFFFu) << 16; }

/* IEEE binary16 (1 + 5 + 10) -> float32 bits */
HYDK_HALF_FN uint32_t hydk_widen_f16(uint32_t bits) {
    const uint32_t sign = (bits & 0x8000u) << 16, exp = (bits >> 10) & 0x1Fu, man = bits & 0x3FFu;
    if (exp == 31u) /* infinity, NaN */
        return sign | 0x7F800000u | (man << 13);
    if (exp != 0u) /* normal: the exponent re-biased from 15 to 127 */
        return sign | ((exp + 112u) << 23) | (man << 13);
    if (man == 0u)
        return sign;
    /* subnormal: man * 2^-24, normalised — the leading one moves up to bit 10 and out of the field */
    const uint32_t shift = (uint32_t)__builtin_clz(man) - 21u;
    return sign | ((113u - shift) << 23) | (((man << shift) & 0x3FFu) << 13);
}

HYDK_HALF_FN uint32_t hydk_widen_half(int storage, uint32_t bits) {
    return storage == HYDK_STORE_BF16 ? hydk_widen_bf16(bits) : hydk_widen_f16(bits);
}

#endif /* HYD_HALF_WIDEN_H_ */
