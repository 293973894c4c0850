/*
 * hydk_y216.h — packed 4:2:2 YCbCr of 16-bit words (Y210, Y212, Y216 and their three word orders; hyd_sample_fmt.h 32832 ...): where
 * a pixel's three words sit, and one pixel of such a picture.  Compiles for host and device (as hydk_yuy2.h does for bytes): the
 * transform kernel's Y216 and Y216I loaders and the probe flavour's two test entries share this text, and it is the only place the
 * rule lives.  There is no arithmetic of its own here and no table: the taps are hydk_chroma.h's 4:2:2 ones, the conversion
 * hydk_yuv16.h's.
 *
 * A row of a W-pixel picture is cw = ceil(W / 2) GROUPS of four 16-bit words, two pixels each.  With yp, up and vp the first Y, U
 * and V word of the row (three pointers into the same group, in one of the four orders of hyd_fmt_packed_order), in words:
 *
 *   Y[x] = yp[2 x]        U[cx] = up[4 cx]        V[cx] = vp[4 cx]
 *
 * The words are MSB-aligned, as P010's are, and count AS STORED: low bits are not masked (the P01x rule of hydk_yuv16.h).  The
 * picture is the 4:2:2 picture of those samples: nearest chroma takes C[x >> 1]; otherwise the horizontal taps of hydk_chroma.h
 * apply to U and to V by themselves (4:2:2: the far row is the near row), clamped at the picture's first and last chroma column;
 * then hydk_yuv16_to_rgb under hydk_yuv16_matrix(depth, matrix) — the depth changes the full-range matrices and nothing else.  For
 * odd W the last group's second Y word belongs to the row and is no pixel.  Nothing outside the 4 cw words of a row is read.
 */
#ifndef HYD_Y216_H_
#define HYD_Y216_H_

#include <stdint.h>

#include "hydk_chroma.h"
#include "hydk_yuv16.h"
#include "hydk_yuy2.h" /* hydk_yuy2_y_offset, hydk_yuy2_v_first: the four orders are the same four, in words */

/* U' or V' of pixel x of a row: crow the row's first word of that component, cw groups.  filter: HYDK_CHROMA_NEAREST, _CENTRE, _LEFT */
HYDK_CHROMA_FN uint32_t hydk_y216_chroma(int filter, const uint16_t *crow, int32_t cw, int32_t x) {
    const int32_t cx = x >> 1;
    if (filter == HYDK_CHROMA_NEAREST)
        return crow[4 * cx];
    const int32_t hx = hydk_chroma_hx(filter, x, cw);
    const uint32_t a = crow[4 * cx], b = crow[4 * hx];
    return hydk_chroma_hmix(filter, x & 1, hydk_chroma_vmix(a, a), hydk_chroma_vmix(b, b));
}

/* One pixel of the picture, the definition whole: yp, up, vp the PICTURE's first Y, U and V word, rows `pitch` words apart (either
 * sign), width pixels across; depth HYDK_YUV16_P010 ... _P016, matrix HYDK_YUV_*. */
HYDK_CHROMA_FN void hydk_y216_pixel(int filter, int depth, int matrix, const uint16_t *yp, const uint16_t *up, const uint16_t *vp, long long pitch,
                                    int32_t width, int32_t x, int32_t y, uint32_t rgb[3]) {
    const int32_t cw = (width + 1) >> 1;
    const long long row = (long long)y * pitch;
    hydk_yuv16_to_rgb(hydk_yuv16_matrix(depth, matrix), yp[row + 2 * x], hydk_y216_chroma(filter, up + row, cw, x),
                      hydk_y216_chroma(filter, vp + row, cw, x), rgb);
}

#endif /* HYD_Y216_H_ */
