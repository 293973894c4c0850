/*
 * hydk_quad.h — a pixel in ONE GROUP OF FOUR SAMPLES, Y, U, V and a fourth that is ignored: packed 4:4:4 YCbCr (AYUV, Y412, Y416;
 * hyd_sample_fmt.h 524288 ...): where the samples sit, and one pixel of such a picture.  Compiles for host and device (as
 * hydk_rgb10.h does): the transform kernel's AYUV and Y416 loaders and the probe flavour's two test entries share this text, and it
 * is the only place the rule lives.  There is no arithmetic of its own here.
 *
 *   AYUV (depth 0): a pixel is one dword, little-endian the bytes V, U, Y, A — V = d & 255, U = (d >> 8) & 255, Y = (d >> 16) & 255.
 *   A storage form of the 8-bit class: hydk_yuv_to_rgb under hydk_yuv_matrix(matrix), unchanged, so an AYUV picture is the I444
 *   picture of its three bytes.  A row of a W-pixel picture is W dwords.
 *
 *   Y412, Y416 (depth HYDK_YUV16_P012, _P016): a pixel is one qword, little-endian the words U, Y, V, A — as two dwords, lo = U |
 *   Y << 16 and hi = V | A << 16.  Storage forms of the 16-bit class, MSB-aligned: the words count AS STORED, low bits are not
 *   masked (the P01x rule, hydk_yuv16.h), under hydk_yuv16_to_rgb and hydk_yuv16_matrix(depth, matrix), unchanged.  A Y416 picture
 *   is the I416 picture of its three words; a Y412 picture whose low four bits are zero is the I412 picture of the words >> 4.
 *   A row of a W-pixel picture is W qwords, 2 W dwords.
 *
 * The fourth sample never matters, and nothing outside the W pixels of a row is read.
 */
#ifndef HYD_QUAD_H_
#define HYD_QUAD_H_

#include <stdint.h>

#include "hydk_yuv.h"
#include "hydk_yuv16.h"

/* one AYUV pixel under m = hydk_yuv_matrix(matrix); rgb[0 ... 2] in 0 ... 255 */
HYDK_YUV_FN void hydk_ayuv_to_rgb(const HydkYuvMatrix m, uint32_t dword, uint32_t rgb[3]) {
    hydk_yuv_to_rgb(m, (dword >> 16) & 255u, (dword >> 8) & 255u, dword & 255u, rgb);
}

/* one Y412 / Y416 pixel under m = hydk_yuv16_matrix(depth, matrix): lo, hi the qword's two dwords; rgb[0 ... 2] in 0 ... 65535 */
HYDK_YUV_FN void hydk_y416_to_rgb(const HydkYuvMatrix m, uint32_t lo, uint32_t hi, uint32_t rgb[3]) {
    hydk_yuv16_to_rgb(m, lo >> 16, lo & 65535u, hi & 65535u, rgb);
}

/* One pixel of the picture, the definition whole: surface the PICTURE's first pixel as dwords, rows `pitch` PIXELS apart (either
 * sign).  depth 0: AYUV, a dword a pixel; HYDK_YUV16_P012 or _P016: Y412 / Y416, two dwords a pixel.  matrix: HYDK_YUV_*. */
HYDK_YUV_FN void hydk_quad_pixel(int depth, int matrix, const uint32_t *surface, long long pitch, int32_t x, int32_t y, uint32_t rgb[3]) {
    const long long at = (long long)y * pitch + x;
    if (depth)
        hydk_y416_to_rgb(hydk_yuv16_matrix(depth, matrix), surface[2 * at], surface[2 * at + 1], rgb);
    else
        hydk_ayuv_to_rgb(hydk_yuv_matrix(matrix), surface[at], rgb);
}

#endif /* HYD_QUAD_H_ */
