/*
 * hydk_ufloat.h — a pixel in ONE 32-BIT WORD of three UNSIGNED FLOATS (R11G11B10F, RGB9E5; hyd_sample_fmt.h 8388608, 8388609): where
 * the fields sit, what a field stands for, and one pixel of such a picture.  Compiles for host and device (as hydk_half.h and
 * hydk_rgb10.h do): the transform kernel's loader, the probe flavour's test entries and the stand-alone host tests share this
 * text, and it is the only place the rule lives.
 *
 * A row of a W-pixel picture is W dwords.
 *
 *   R11G11B10F (DXGI R11G11B10_FLOAT, Vulkan B10G11R11_UFLOAT_PACK32, GL R11F_G11F_B10F): R in bits 0 ... 10, G in 11 ... 21, B in
 *   22 ... 31.  A field has no sign, a 5-bit exponent e with bias 15 above M mantissa bits m, M = 6 (R, G) or 5 (B):
 *     e = 1 ... 30   2^(e - 15) * (1 + m / 2^M)
 *     e = 0          m * 2^(-14 - M): subnormals, m = 0 is zero; the smallest is 2^-20 (R, G) or 2^-19 (B)
 *     e = 31         m = 0 is +Inf, anything else NaN
 *
 *   RGB9E5 (DXGI R9G9B9E5_SHAREDEXP, Vulkan E5B9G9R9_UFLOAT_PACK32, GL RGB9_E5): R's mantissa in bits 0 ... 8, G's in 9 ... 17, B's in
 *   18 ... 26, the shared exponent E in 27 ... 31.  A channel is m * 2^(E - 24), no implicit leading one; the smallest is 2^-24, the
 *   largest 511 * 2^7.  Every dword is a finite picture, and nothing couples the channels but E.
 *
 * A sample is widened EXACTLY to float32: every value of both formats is a float32 normal or zero.  Integer bit manipulation
 * only, as hydk_half.h's — the exponent re-biased, a subnormal (and every RGB9E5 mantissa) normalised by a count of leading zeros,
 * an all-ones exponent kept all ones — so that no denormal or rounding mode of either processor has a say.  An R11G11B10F NaN
 * keeps its mantissa bits, moved to the top of the float32 mantissa: it is a NaN, and the float class's non-finite check sees
 * it as it sees a float32 one.  From the widened sample on a pixel is a float32 pixel.
 *
 * Nothing outside the W dwords of a row is read.
 */
#ifndef HYD_UFLOAT_H_
#define HYD_UFLOAT_H_

#include <stdint.h>

#ifdef __HIPCC__
#define HYDK_UFLOAT_FN __host__ __device__ static inline
#else
#define HYDK_UFLOAT_FN static inline
#endif

/* which of the two a dword is: the order of their sample formats and of their storage forms */
#define HYDK_UFLOAT_R11G11B10F 0
#define HYDK_UFLOAT_RGB9E5 1

/* an unsigned float of a 5-bit exponent above M mantissa bits (M = 6: an 11-bit field, 5: a 10-bit one) -> float32 bits */
HYDK_UFLOAT_FN uint32_t hydk_ufloat_widen_field(uint32_t v, int M) {
    const uint32_t exp = (v >> M) & 0x1Fu, man = v & ((1u << M) - 1u);
    if (exp == 31u) /* infinity, NaN */
        return 0x7F800000u | (man << (23 - M));
    if (exp != 0u) /* normal: the exponent re-biased from 15 to 127 */
        return ((exp + 112u) << 23) | (man << (23 - M));
    if (man == 0u)
        return 0u;
    /* subnormal: man * 2^(-14 - M), normalised — the leading one moves up to bit M and out of the field */
    const uint32_t shift = (uint32_t)__builtin_clz(man) - (uint32_t)(31 - M);
    return ((113u - shift) << 23) | (((man << shift) & ((1u << M) - 1u)) << (23 - M));
}

/* an RGB9E5 channel, man * 2^(exp - 24) for man in 0 ... 511 and exp in 0 ... 31 -> float32 bits */
HYDK_UFLOAT_FN uint32_t hydk_rgb9e5_widen(uint32_t man, uint32_t exp) {
    if (man == 0u)
        return 0u;
    /* the leading one at bit p = 31 - clz: 2^(p + exp - 24) * 1.f, the bits under it moved to the top of the mantissa */
    const uint32_t lz = (uint32_t)__builtin_clz(man);
    return ((134u + exp - lz) << 23) | ((man << (lz - 8u)) & 0x7FFFFFu);
}

/* one R11G11B10F pixel: rgb[0 ... 2] the float32 bits of R, G, B */
HYDK_UFLOAT_FN void hydk_r11g11b10f_to_f32(uint32_t dword, uint32_t rgb[3]) {
    rgb[0] = hydk_ufloat_widen_field(dword & 0x7FFu, 6);
    rgb[1] = hydk_ufloat_widen_field((dword >> 11) & 0x7FFu, 6);
    rgb[2] = hydk_ufloat_widen_field(dword >> 22, 5);
}

/* one RGB9E5 pixel */
HYDK_UFLOAT_FN void hydk_rgb9e5_to_f32(uint32_t dword, uint32_t rgb[3]) {
    const uint32_t exp = dword >> 27;
    rgb[0] = hydk_rgb9e5_widen(dword & 0x1FFu, exp);
    rgb[1] = hydk_rgb9e5_widen((dword >> 9) & 0x1FFu, exp);
    rgb[2] = hydk_rgb9e5_widen((dword >> 18) & 0x1FFu, exp);
}

HYDK_UFLOAT_FN void hydk_ufloat_to_f32(int which, uint32_t dword, uint32_t rgb[3]) {
    if (which == HYDK_UFLOAT_RGB9E5)
        hydk_rgb9e5_to_f32(dword, rgb);
    else
        hydk_r11g11b10f_to_f32(dword, rgb);
}

/* One pixel of the picture, the definition whole: surface the PICTURE's first dword, rows `pitch` dwords apart (either sign);
 * which: HYDK_UFLOAT_*. */
HYDK_UFLOAT_FN void hydk_ufloat_pixel(int which, const uint32_t *surface, long long pitch, int32_t x, int32_t y, uint32_t rgb[3]) {
    hydk_ufloat_to_f32(which, surface[(long long)y * pitch + x], rgb);
}

#endif /* HYD_UFLOAT_H_ */
