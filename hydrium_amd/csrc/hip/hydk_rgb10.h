/*
 * hydk_rgb10.h — a pixel in ONE 32-BIT WORD of three 10-bit fields and two spare bits (RGB10A2, BGR10A2, Y410; hyd_sample_fmt.h
 * 131072 ...): where the fields sit, what a field stands for, and one pixel of such a picture.  Compiles for host and device (as
 * hydk_y216.h does): the transform kernel's RGB10 and Y410 loaders and the probe flavour's two test entries share this text, and it
 * is the only place the rule lives.
 *
 * A row of a W-pixel picture is W dwords.  Field k of a dword d is (d >> 10 k) & 1023, k = 0, 1, 2; bits 30 and 31 never matter.
 *
 *   RGB10A2 (order 0): R, G, B = fields 0, 1, 2.    BGR10A2 (order 1): B, G, R = fields 0, 1, 2.
 *   A field v stands for the 16-bit sample nearest to v / 1023:  s = (v * 65535 + 511) / 1023 in integers.  65535 / 1023 =
 *   21845 / 341 with 341 odd, so no v lands on a tie; 0 -> 0, 1023 -> 65535.  hydk_rgb10_widen computes that s with one multiply,
 *   add and shift, (v * 1049585 + 8192) >> 14 — below 2^31, and equal on all 1024 values (tests/test_dword_formats.py holds it to
 *   the division).  Bit replication, v << 6 | v >> 4, is NOT that sample: it is one less at v = 9, for one.  The picture is the
 *   RGB16 picture of those samples.
 *
 *   Y410: U, Y, V = fields 0, 1, 2.  A field v stands for the P010 sample v << 6 (what the LSB-aligned word v of I410 stands for,
 *   hydk_yuvp16.h), and from there hydk_yuv16_to_rgb under hydk_yuv16_matrix(HYDK_YUV16_P010, matrix), unchanged: a Y410 picture is
 *   the I410 picture of its three fields.  There is no constant of its own here.
 *
 * Nothing outside the W dwords of a row is read.
 */
#ifndef HYD_RGB10_H_
#define HYD_RGB10_H_

#include <stdint.h>

#include "hydk_yuv16.h"

/* field k = 0, 1, 2 of a pixel's dword */
HYDK_YUV_FN uint32_t hydk_rgb10_field(uint32_t dword, int k) { return (dword >> (10 * k)) & 1023u; }

/* the 16-bit sample a 10-bit RGB field stands for: (v * 65535 + 511) / 1023 for v in 0 ... 1023 */
HYDK_YUV_FN uint32_t hydk_rgb10_widen(uint32_t v) { return (v * 1049585u + 8192u) >> 14; }

/* one RGB pixel: order 0 — R in the low field (RGB10A2), 1 — B in the low field (BGR10A2); rgb[0 ... 2] in 0 ... 65535 */
HYDK_YUV_FN void hydk_rgb10_to_rgb(int order, uint32_t dword, uint32_t rgb[3]) {
    rgb[0] = hydk_rgb10_widen(hydk_rgb10_field(dword, order ? 2 : 0));
    rgb[1] = hydk_rgb10_widen(hydk_rgb10_field(dword, 1));
    rgb[2] = hydk_rgb10_widen(hydk_rgb10_field(dword, order ? 0 : 2));
}

/* one Y410 pixel under m = hydk_yuv16_matrix(HYDK_YUV16_P010, matrix) */
HYDK_YUV_FN void hydk_y410_to_rgb(const HydkYuvMatrix m, uint32_t dword, uint32_t rgb[3]) {
    hydk_yuv16_to_rgb(m, hydk_rgb10_field(dword, 1) << 6, hydk_rgb10_field(dword, 0) << 6, hydk_rgb10_field(dword, 2) << 6, rgb);
}

/* One pixel of the picture, the definition whole: surface the PICTURE's first dword, rows `pitch` dwords apart (either sign).
 * ycbcr 0: an RGB form, `which` its order; 1: Y410, `which` its matrix HYDK_YUV_*. */
HYDK_YUV_FN void hydk_dword_pixel(int ycbcr, int which, const uint32_t *surface, long long pitch, int32_t x, int32_t y, uint32_t rgb[3]) {
    const uint32_t dword = surface[(long long)y * pitch + x];
    if (ycbcr)
        hydk_y410_to_rgb(hydk_yuv16_matrix(HYDK_YUV16_P010, which), dword, rgb);
    else
        hydk_rgb10_to_rgb(which, dword, rgb);
}

#endif /* HYD_RGB10_H_ */
