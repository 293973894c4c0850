/*
 * hydk_yuvp16.h — planar YCbCr of 16-bit words (I010, I210, I410, I012 ... I416; hyd_sample_fmt.h 2112 ...): what a stored word
 * stands for, and one pixel of such a picture.  Compiles for host and device (as hydk_yuv16.h and hydk_chroma.h do): the transform
 * kernel's YUVP16 and YUVP16I loaders and the probe flavour's two test entries share this text, and it is the only place the rule
 * lives.  There is no arithmetic of its own here and no table: the taps are hydk_chroma.h's, the conversion hydk_yuv16.h's.
 *
 *   A stored word w of a picture of n = 10, 12 or 16 significant bits, LSB-ALIGNED, is the sample  s = (w << (16 - n)) & 0xFFFF.
 *
 * Bits above the depth are shifted out and not trusted, which makes the definition total; depth 16 takes the word as stored
 * (so an MSB-aligned planar surface of any depth and limited range goes in as I*16).  From there the picture is the P01x
 * picture of the same depth and matrix on the planar family's geometry: nearest chroma takes C[y >> sy][x >> sx]; otherwise
 * the taps of hydk_chroma.h apply to the SHIFTED samples of each plane by itself, 4:2:2 with the far row equal to the near one;
 * then hydk_yuv16_to_rgb under hydk_yuv16_matrix(depth, matrix).
 */
#ifndef HYD_YUVP16_H_
#define HYD_YUVP16_H_

#include <stdint.h>

#include "hydk_yuv16.h"

/* the left shift that MSB-aligns a word of depth index HYDK_YUV16_P010 ... _P016 (1, 2, 3): 6, 4, 0 */
HYDK_CHROMA_FN int hydk_yuvp16_shift(int depth) { return depth == HYDK_YUV16_P010 ? 6 : depth == HYDK_YUV16_P012 ? 4 : 0; }
/* the sample a stored word stands for */
HYDK_CHROMA_FN uint32_t hydk_yuvp16_sample(int shift, uint32_t word) { return (word << shift) & 0xFFFFu; }
/* the same for the two words of a dword at once */
HYDK_CHROMA_FN uint32_t hydk_yuvp16_sample2(int shift, uint32_t words) { return (words << shift) & (((0xFFFFu << shift) & 0xFFFFu) * 0x10001u); }

/* hydk_planar_sample on 16-bit words: U' or V' of pixel (x, y) out of ONE plane, read word by word with the clamps.  plane: the
 * PICTURE's sample (0, 0) of that plane, cw x ch words, rows `pitch` WORDS apart (either sign).  Nothing outside the cw x ch words
 * is read. */
HYDK_CHROMA_FN uint32_t hydk_planar16_sample(int sub, int filter, int shift, const uint16_t *plane, long long pitch, int32_t cw, int32_t ch,
                                             int32_t x, int32_t y) {
    const int sx = hydk_planar_sx(sub), sy = hydk_planar_sy(sub);
    const uint16_t *near = plane + (long long)(y >> sy) * pitch;
    if (filter == HYDK_CHROMA_NEAREST || !sx)
        return hydk_yuvp16_sample(shift, near[x >> sx]);
    /* 4:2:2: the far row is the near row */
    const uint16_t *far = sy ? plane + (long long)hydk_chroma_vy(y, ch) * pitch : near;
    const int32_t cx = x >> 1, hx = hydk_chroma_hx(filter, x, cw);
    return hydk_chroma_hmix(filter, x & 1, hydk_chroma_vmix(hydk_yuvp16_sample(shift, near[cx]), hydk_yuvp16_sample(shift, far[cx])),
                            hydk_chroma_vmix(hydk_yuvp16_sample(shift, near[hx]), hydk_yuvp16_sample(shift, far[hx])));
}

/* One pixel of the picture, the definition whole: yp, up, vp the picture's first Y, U and V word, the Y rows ypitch and the chroma
 * rows cpitch words apart; depth HYDK_YUV16_P010 ... _P016, matrix HYDK_YUV_*. */
HYDK_CHROMA_FN void hydk_planar16_pixel(int sub, int filter, int depth, int matrix, const uint16_t *yp, long long ypitch, const uint16_t *up,
                                        const uint16_t *vp, long long cpitch, int32_t cw, int32_t ch, int32_t x, int32_t y, uint32_t rgb[3]) {
    const int shift = hydk_yuvp16_shift(depth);
    hydk_yuv16_to_rgb(hydk_yuv16_matrix(depth, matrix), hydk_yuvp16_sample(shift, yp[(long long)y * ypitch + x]),
                      hydk_planar16_sample(sub, filter, shift, up, cpitch, cw, ch, x, y),
                      hydk_planar16_sample(sub, filter, shift, vp, cpitch, cw, ch, x, y), rgb);
}

#endif /* HYD_YUVP16_H_ */
