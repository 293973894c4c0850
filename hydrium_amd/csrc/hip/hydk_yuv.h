/*
 * hydk_yuv.h — one YCbCr pixel to 8-bit RGB, in fixed point.  Compiles for host and device (as hydk_half.h does): the
 * transform kernel's NV12 loader and the probe flavour's two test entries share this text, and it is the only place the
 * formula lives.
 *
 *   c = Y - yo, d = U - 128, e = V - 128
 *   R = clamp((cy * c           + crv * e + 8192) >> 14, 0, 255)
 *   G = clamp((cy * c - cgu * d - cgv * e + 8192) >> 14, 0, 255)
 *   B = clamp((cy * c + cbu * d           + 8192) >> 14, 0, 255)
 *
 * 32-bit integers, `>>` arithmetic.  The coefficients are round(v * 2^14) of sy = 255/219 (limited range) or 1 (full),
 * sc = 255/224 or 1, crv = 2 (1 - Kr) sc, cbu = 2 (1 - Kb) sc, cgu = 2 (1 - Kb) Kb / Kg sc, cgv = 2 (1 - Kr) Kr / Kg sc with
 * Kr, Kb = 0.2126, 0.0722 (BT.709) or 0.299, 0.114 (BT.601) and Kg = 1 - Kr - Kb.  Over all 2^24 (Y, U, V) every accumulator
 * stays below 2^24 in magnitude and every operand fits 24 bits (the device multiplies with the 24-bit multiplier), and the
 * result is within 0.51 of the clamped real-valued conversion: half a code of rounding and less than 0.01 from the
 * coefficients' own rounding (tests/test_yuv_formats.py walks all of them).
 */
#ifndef HYD_YUV_TO_RGB_H_
#define HYD_YUV_TO_RGB_H_

#include <stdint.h>

#include "hydk_store.h" /* HYDK_STORE_NV12 */

#ifdef __HIPCC__
#define HYDK_YUV_FN __host__ __device__ static inline
#else
#define HYDK_YUV_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define HYDK_YUV_MUL(a, b) __mul24((a), (b))
#else
#define HYDK_YUV_MUL(a, b) ((a) * (b))
#endif

/* matrices (HydkLfJob.matrix; hyd_sample_fmt.h: sample format - 16) */
#define HYDK_YUV_BT709 0
#define HYDK_YUV_BT709_FULL 1
#define HYDK_YUV_BT601 2
#define HYDK_YUV_BT601_FULL 3
#define HYDK_YUV_MATRICES 4

typedef struct HydkYuvMatrix {
    int32_t yo, cy, crv, cgu, cgv, cbu;
} HydkYuvMatrix;

HYDK_YUV_FN HydkYuvMatrix hydk_yuv_matrix(int matrix) {
    const int32_t table[HYDK_YUV_MATRICES][6] = {
        {16, 19077, 29372, 3494, 8731, 34610}, /* BT.709, limited range */
        {0, 16384, 25802, 3069, 7670, 30402},  /* BT.709, full range */
        {16, 19077, 26149, 6419, 13320, 33050}, /* BT.601, limited range */
        {0, 16384, 22970, 5638, 11700, 29032},  /* BT.601, full range */
    };
    const int32_t *t = table[matrix & 3];
    const HydkYuvMatrix m = {t[0], t[1], t[2], t[3], t[4], t[5]};
    return m;
}

HYDK_YUV_FN int32_t hydk_yuv_clamp8(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

/* y, u, v in 0 ... 255; rgb[0 ... 2] in 0 ... 255 */
HYDK_YUV_FN void hydk_yuv_to_rgb(const HydkYuvMatrix m, uint32_t y, uint32_t u, uint32_t v, uint32_t rgb[3]) {
    const int32_t c = (int32_t)y - m.yo, d = (int32_t)u - 128, e = (int32_t)v - 128;
    const int32_t luma = HYDK_YUV_MUL(m.cy, c) + 8192;
    rgb[0] = (uint32_t)hydk_yuv_clamp8((luma + HYDK_YUV_MUL(m.crv, e)) >> 14);
    rgb[1] = (uint32_t)hydk_yuv_clamp8((luma - HYDK_YUV_MUL(m.cgu, d) - HYDK_YUV_MUL(m.cgv, e)) >> 14);
    rgb[2] = (uint32_t)hydk_yuv_clamp8((luma + HYDK_YUV_MUL(m.cbu, d)) >> 14);
}

#endif /* HYD_YUV_TO_RGB_H_ */
