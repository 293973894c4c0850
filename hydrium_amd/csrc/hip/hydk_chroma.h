/*
 * hydk_chroma.h — one pixel's U or V out of a 4:2:0 chroma plane, interpolated, in exact integers.  Compiles for host and
 * device (as hydk_yuv.h does): the transform kernel's NV12I loader and the probe flavour's two test entries share this text,
 * and it is the only place the taps live.
 *
 * The PICTURE is W x H pixels with a chroma plane of cw = ceil(W / 2) by ch = ceil(H / 2) samples.  For pixel (x, y) in
 * picture coordinates, cx = x >> 1, cy = y >> 1, vy = clamp(cy + (y odd ? 1 : -1), 0, ch - 1), and with C one component:
 *
 *   centre-sited (JPEG / JFIF, MPEG-1), hx = clamp(cx + (x odd ? 1 : -1), 0, cw - 1):
 *       C' = (9 C[cy][cx] + 3 C[cy][hx] + 3 C[vy][cx] + C[vy][hx] + 8) >> 4
 *   left-sited (MPEG-2; chroma_sample_loc_type 0 of H.264, HEVC, AV1), x even:
 *       C' = (3 C[cy][cx] + C[vy][cx] + 2) >> 2
 *   left-sited, x odd, hx = min(cx + 1, cw - 1):
 *       C' = (3 (C[cy][cx] + C[cy][hx]) + C[vy][cx] + C[vy][hx] + 4) >> 3
 *
 * All three are the vertical mix v(c) = 3 C[cy][c] + C[vy][c] (at most 1020) followed by a horizontal one —
 * (3 v(cx) + v(hx) + 8) >> 4, (v(cx) + 2) >> 2, (v(cx) + v(hx) + 4) >> 3 — the same integers before the shift, so the same
 * result; the taps sum to the divisor, so a result stays in 0 ... 255.  Clamping is at the edges of the picture: no index
 * outside rows 0 ... ch - 1, columns 0 ... cw - 1 is ever formed.
 *
 * PLANAR chroma (three planes, hyd_sample_fmt.h 512 ...) uses the same taps on each plane by itself.  4:2:0 as above.  4:2:2 has
 * a chroma row for every picture row, ch = H, so only the horizontal taps remain, with cx = x >> 1:
 *
 *   centre-sited, hx = clamp(cx + (x odd ? 1 : -1), 0, cw - 1):   C' = (3 C[y][cx] + C[y][hx] + 2) >> 2
 *   left-sited, x even:                                           C' = C[y][cx]
 *   left-sited, x odd, hx = min(cx + 1, cw - 1):                  C' = (C[y][cx] + C[y][hx] + 1) >> 1
 *
 * These are the 4:2:0 formulas with the far row equal to the near row: v(c) = 4 C[y][c], and (3 * 4a + 4b + 8) >> 4 =
 * (3a + b + 2) >> 2, (4a + 2) >> 2 = a, (4a + 4b + 4) >> 3 = (a + b + 1) >> 1 exactly.  So 4:2:2 is
 * hydk_chroma_hmix(filter, x & 1, hydk_chroma_vmix(a, a), hydk_chroma_vmix(b, b)) and the taps stay in this one place
 * (hydk_planar_sample below, and the transform kernel's planar loader, which takes the near dword for the far one).
 */
#ifndef HYD_CHROMA_UPSAMPLE_H_
#define HYD_CHROMA_UPSAMPLE_H_

#include <stdint.h>

#include "hydk_store.h" /* HYDK_STORE_NV12I, _YUVP, _YUVPI */

#ifdef __HIPCC__
#define HYDK_CHROMA_FN __host__ __device__ static inline
#else
#define HYDK_CHROMA_FN static inline
#endif

/* filters (HydkLfJob.filter; hyd_sample_fmt.h: (sample format - 16) >> 4) */
#define HYDK_CHROMA_NEAREST 0
#define HYDK_CHROMA_CENTRE 1
#define HYDK_CHROMA_LEFT 2
#define HYDK_CHROMA_FILTERS 3

/* the other chroma row and the other chroma column of a pixel, clamped to the picture's plane */
HYDK_CHROMA_FN int32_t hydk_chroma_vy(int32_t y, int32_t ch) {
    const int32_t v = (y >> 1) + ((y & 1) ? 1 : -1);
    return v < 0 ? 0 : v > ch - 1 ? ch - 1 : v;
}
HYDK_CHROMA_FN int32_t hydk_chroma_hx(int filter, int32_t x, int32_t cw) {
    const int32_t h = (x >> 1) + ((x & 1) ? 1 : filter == HYDK_CHROMA_CENTRE ? -1 : 0);
    return h < 0 ? 0 : h > cw - 1 ? cw - 1 : h;
}

/* the vertical mix of one chroma column: near = C[cy][c], far = C[vy][c] */
HYDK_CHROMA_FN uint32_t hydk_chroma_vmix(uint32_t near, uint32_t far) { return 3u * near + far; }

/* the horizontal mix: v0 = vmix at cx, v1 = vmix at hx (unused by left-sited even columns) */
HYDK_CHROMA_FN uint32_t hydk_chroma_hmix(int filter, int x_odd, uint32_t v0, uint32_t v1) {
    if (filter == HYDK_CHROMA_CENTRE)
        return (3u * v0 + v1 + 8u) >> 4;
    return x_odd ? (v0 + v1 + 4u) >> 3 : (v0 + 2u) >> 2;
}

/* U' and V' of pixel x of a picture row, read byte by byte with the clamps.  near, far: the first byte of the PICTURE's
 * chroma rows y >> 1 and hydk_chroma_vy(y, ch), rows of cw (U, V) pairs as NV12 has them.  filter: HYDK_CHROMA_CENTRE or
 * HYDK_CHROMA_LEFT.  The definition pixel by pixel: what the probe flavour's entries run on host and device.  The transform
 * kernel builds a block row's window of six pairs once — by dwords or, at the picture's edges, byte by byte with these
 * clamps — and applies the same hydk_chroma_vy, hydk_chroma_vmix and hydk_chroma_hmix to it. */
HYDK_CHROMA_FN void hydk_chroma_pair(int filter, const uint8_t *near, const uint8_t *far, int32_t cw, int32_t x, uint32_t uv[2]) {
    const int32_t cx = x >> 1, hx = hydk_chroma_hx(filter, x, cw);
    for (int c = 0; c < 2; c++)
        uv[c] = hydk_chroma_hmix(filter, x & 1, hydk_chroma_vmix(near[2 * cx + c], far[2 * cx + c]),
                                 hydk_chroma_vmix(near[2 * hx + c], far[2 * hx + c]));
}

/* subsamplings of the planar forms, HYDK_STORE_YUVP and _YUVPI (HydkLfJob.sub; hyd_sample_fmt.h: ((sample format - 512) >> 2) & 3) */
#define HYDK_PLANAR_420 0
#define HYDK_PLANAR_422 1
#define HYDK_PLANAR_444 2
#define HYDK_PLANAR_SUBS 3
/* log2 of the pixels one chroma sample spans across and down */
HYDK_CHROMA_FN int hydk_planar_sx(int sub) { return sub != HYDK_PLANAR_444; }
HYDK_CHROMA_FN int hydk_planar_sy(int sub) { return sub == HYDK_PLANAR_420; }

/* U' or V' of pixel (x, y) out of ONE plane of a planar picture, read byte by byte with the clamps: the definition pixel by
 * pixel.  plane: the PICTURE's sample (0, 0) of that plane, cw x ch samples, rows `pitch` bytes apart (either sign).  filter:
 * HYDK_CHROMA_NEAREST, _CENTRE or _LEFT; 4:4:4 is nearest whatever it says.  Nothing outside the cw x ch samples is read. */
HYDK_CHROMA_FN uint32_t hydk_planar_sample(int sub, int filter, const uint8_t *plane, long long pitch, int32_t cw, int32_t ch, int32_t x,
                                           int32_t y) {
    const int sx = hydk_planar_sx(sub), sy = hydk_planar_sy(sub);
    const uint8_t *near = plane + (long long)(y >> sy) * pitch;
    if (filter == HYDK_CHROMA_NEAREST || !sx)
        return near[x >> sx];
    /* 4:2:2: the far row is the near row */
    const uint8_t *far = sy ? plane + (long long)hydk_chroma_vy(y, ch) * pitch : near;
    const int32_t cx = x >> 1, hx = hydk_chroma_hx(filter, x, cw);
    return hydk_chroma_hmix(filter, x & 1, hydk_chroma_vmix(near[cx], far[cx]), hydk_chroma_vmix(near[hx], far[hx]));
}

#endif /* HYD_CHROMA_UPSAMPLE_H_ */
