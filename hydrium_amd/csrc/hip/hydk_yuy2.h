/*
 * hydk_yuy2.h — packed 4:2:2 YCbCr (YUY2 / YUYV, UYVY, YVYU, VYUY; hyd_sample_fmt.h 8192 ...): where a pixel's three bytes sit, and
 * one pixel of such a picture.  Compiles for host and device (as hydk_chroma.h and hydk_yuvp16.h do): the transform kernel's YUY2
 * and YUY2I loaders and the probe flavour's two test entries share this text, and it is the only place the rule lives.  There is
 * no arithmetic of its own here and no table: the taps are hydk_chroma.h's 4:2:2 ones, the conversion hydk_yuv.h's.
 *
 * A row of a W-pixel picture is cw = ceil(W / 2) GROUPS of 4 bytes, two pixels each.  With yp, up and vp the first Y, U and V byte
 * of the row (three pointers into the same group, in one of the four orders of hyd_fmt_packed_order):
 *
 *   Y[x] = yp[2 x]        U[cx] = up[4 cx]        V[cx] = vp[4 cx]
 *
 * and the picture is the I422 picture of those planes: nearest chroma takes C[x >> 1]; otherwise the horizontal taps of
 * hydk_chroma.h apply to U and to V by themselves (4:2:2: the far row is the near row), clamped at the picture's first and last
 * chroma column; then hydk_yuv_to_rgb under hydk_yuv_matrix(matrix).  For odd W the last group's second Y byte belongs to the row
 * and is no pixel.  Nothing outside the 4 cw bytes of a row is read.
 */
#ifndef HYD_YUY2_H_
#define HYD_YUY2_H_

#include <stdint.h>

#include "hydk_chroma.h"
#include "hydk_yuv.h"

/* where Y sits in its pair of bytes, by byte order (HYD_PACKED_*, HydkLfJob.sub): 0 — YUYV, YVYU; 1 — UYVY, VYUY.  The group of
 * pixel 0 starts that many bytes before src[0] */
HYDK_CHROMA_FN int hydk_yuy2_y_offset(int order) { return (order >> 1) & 1; }
/* whether V comes before U in the group: YVYU, VYUY */
HYDK_CHROMA_FN int hydk_yuy2_v_first(int order) { return order & 1; }

/* U' or V' of pixel x of a row: crow the row's first byte of that component, cw groups.  filter: HYDK_CHROMA_NEAREST, _CENTRE, _LEFT */
HYDK_CHROMA_FN uint32_t hydk_yuy2_chroma(int filter, const uint8_t *crow, int32_t cw, int32_t x) {
    const int32_t cx = x >> 1;
    if (filter == HYDK_CHROMA_NEAREST)
        return crow[4 * cx];
    const int32_t hx = hydk_chroma_hx(filter, x, cw);
    const uint32_t a = crow[4 * cx], b = crow[4 * hx];
    return hydk_chroma_hmix(filter, x & 1, hydk_chroma_vmix(a, a), hydk_chroma_vmix(b, b));
}

/* One pixel of the picture, the definition whole: yp, up, vp the PICTURE's first Y, U and V byte, rows `pitch` bytes apart (either
 * sign), width pixels across; matrix HYDK_YUV_*. */
HYDK_CHROMA_FN void hydk_yuy2_pixel(int filter, int matrix, const uint8_t *yp, const uint8_t *up, const uint8_t *vp, long long pitch,
                                    int32_t width, int32_t x, int32_t y, uint32_t rgb[3]) {
    const int32_t cw = (width + 1) >> 1;
    const long long row = (long long)y * pitch;
    hydk_yuv_to_rgb(hydk_yuv_matrix(matrix), yp[row + 2 * x], hydk_yuy2_chroma(filter, up + row, cw, x), hydk_yuy2_chroma(filter, vp + row, cw, x), rgb);
}

#endif /* HYD_YUY2_H_ */
