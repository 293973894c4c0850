/*
 * hydk_yuv16.h — P010 / P012 / P016: one YCbCr pixel of 16-bit words to 16-bit RGB, and one pixel's interpolated U or V out of
 * a 4:2:0 plane of 16-bit pairs.  Compiles for host and device (as hydk_yuv.h and hydk_chroma.h do): the transform kernel's
 * P016 and P016I loaders and the probe flavour's four test entries share this text, and it is the only place the formula
 * lives.  The taps are hydk_chroma.h's, unchanged.
 *
 *   c = Y - yo, d = U - 32768, e = V - 32768        (the 16-bit words AS STORED: low bits are not masked)
 *   R = clamp((cy * c           + crv * e + 2^19) >> 20, 0, 65535)
 *   G = clamp((cy * c - cgu * d - cgv * e + 2^19) >> 20, 0, 65535)
 *   B = clamp((cy * c + cbu * d           + 2^19) >> 20, 0, 65535)
 *
 * 64-bit two's complement, `>>` arithmetic.  The coefficients are floor(v * 2^20 + 0.5) of cy = sy, crv = 2 (1 - Kr) sc,
 * cbu = 2 (1 - Kb) sc, cgu = 2 (1 - Kb) Kb / Kg sc, cgv = 2 (1 - Kr) Kr / Kg sc with Kr, Kb as in hydk_yuv.h.  Limited range, at
 * every depth (the standards scale the range with the depth, so MSB-aligned words need none): yo = 4096, sy = 65535 / (219 *
 * 256), sc = 65535 / (224 * 256).  Full range: yo = 0, sy = sc = 65535 / ((2^n - 1) * 2^(16 - n)) for n significant bits, which
 * is 1 for n = 16 and makes 10-bit code 1023 white.  Every coefficient is below 2^23 and c, d, e fit 18 signed bits: a
 * product is a signed 24 x 24-bit multiply with a 48-bit result, a sum stays below 2^43, and the shifted sum fits 32 bits.
 * A coefficient is off by at most 2^-21, which comes to 65535 * 2^-21 + 2 * 32768 * 2^-21 = 0.0625; with half a code of
 * rounding the result is within 0.5625 of the clamped real-valued conversion (tests/test_p016_formats.py).
 */
#ifndef HYD_YUV16_TO_RGB_H_
#define HYD_YUV16_TO_RGB_H_

#include <stdint.h>

#include "hydk_chroma.h"
#include "hydk_yuv.h"

/* depths (HydkLfJob.matrix of these storage forms is matrix + 4 * depth; hyd_sample_fmt.h: (sample format - 16) >> 6) */
#define HYDK_YUV16_P010 1
#define HYDK_YUV16_P012 2
#define HYDK_YUV16_P016 3
#define HYDK_YUV16_DEPTHS 3

/* row (depth - 1) * 4 + matrix; HydkYuvMatrix's fields at the scale 2^20 */
HYDK_YUV_FN HydkYuvMatrix hydk_yuv16_matrix(int depth, int matrix) {
    const int32_t table[HYDK_YUV16_DEPTHS * HYDK_YUV_MATRICES][6] = {
        {4096, 1225714, 1887168, 224481, 560979, 2223666}, /* 10 bits: BT.709, limited range */
        {0, 1049585, 1652886, 196613, 491336, 1947610},    /* BT.709, full range */
        {4096, 1225714, 1680093, 412397, 855788, 2123484}, /* BT.601, limited range */
        {0, 1049585, 1471518, 361200, 749547, 1859865},    /* BT.601, full range */
        {4096, 1225714, 1887168, 224481, 560979, 2223666}, /* 12 bits */
        {0, 1048816, 1651676, 196469, 490976, 1946183},
        {4096, 1225714, 1680093, 412397, 855788, 2123484},
        {0, 1048816, 1470440, 360936, 748998, 1858502},
        {4096, 1225714, 1887168, 224481, 560979, 2223666}, /* 16 bits */
        {0, 1048576, 1651297, 196424, 490864, 1945738},
        {4096, 1225714, 1680093, 412397, 855788, 2123484},
        {0, 1048576, 1470104, 360853, 748826, 1858077},
    };
    const int dz = depth < HYDK_YUV16_P010 ? 0 : depth > HYDK_YUV16_P016 ? HYDK_YUV16_DEPTHS - 1 : depth - 1;
    const int32_t *t = table[dz * HYDK_YUV_MATRICES + (matrix & 3)];
    const HydkYuvMatrix m = {t[0], t[1], t[2], t[3], t[4], t[5]};
    return m;
}
/* of HydkLfJob.matrix = matrix + 4 * depth */
HYDK_YUV_FN HydkYuvMatrix hydk_yuv16_job_matrix(uint32_t job_matrix) { return hydk_yuv16_matrix((int)(job_matrix >> 2), (int)(job_matrix & 3u)); }

/* a sum of the formula, shifted and clamped: |sum| < 2^43, so the shifted sum is exact in 32 bits */
HYDK_YUV_FN uint32_t hydk_yuv16_round(int64_t sum) {
    const int32_t v = (int32_t)(sum >> 20);
    return (uint32_t)(v < 0 ? 0 : v > 65535 ? 65535 : v);
}

/* y, u, v in 0 ... 65535 as stored; rgb[0 ... 2] in 0 ... 65535 */
HYDK_YUV_FN void hydk_yuv16_to_rgb(const HydkYuvMatrix m, uint32_t y, uint32_t u, uint32_t v, uint32_t rgb[3]) {
    const int32_t c = (int32_t)y - m.yo, d = (int32_t)u - 32768, e = (int32_t)v - 32768;
    const int64_t luma = (int64_t)m.cy * c + ((int64_t)1 << 19);
    rgb[0] = hydk_yuv16_round(luma + (int64_t)m.crv * e);
    rgb[1] = hydk_yuv16_round(luma - (int64_t)m.cgu * d - (int64_t)m.cgv * e);
    rgb[2] = hydk_yuv16_round(luma + (int64_t)m.cbu * d);
}

/* hydk_chroma_pair on 16-bit samples: near, far are the first WORD of the picture's chroma rows y >> 1 and
 * hydk_chroma_vy(y, ch), rows of cw (U, V) pairs.  The vertical mix is at most 4 * 65535, the horizontal one below 2^21, the
 * result 0 ... 65535. */
HYDK_CHROMA_FN void hydk_chroma16_pair(int filter, const uint16_t *near, const uint16_t *far, int32_t cw, int32_t x, uint32_t uv[2]) {
    const int32_t cx = x >> 1, hx = hydk_chroma_hx(filter, x, cw);
    for (int c = 0; c < 2; c++)
        uv[c] = hydk_chroma_hmix(filter, x & 1, hydk_chroma_vmix(near[2 * cx + c], far[2 * cx + c]),
                                 hydk_chroma_vmix(near[2 * hx + c], far[2 * hx + c]));
}

#endif /* HYD_YUV16_TO_RGB_H_ */
