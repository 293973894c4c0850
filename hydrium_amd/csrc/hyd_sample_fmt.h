/*
 * hyd_sample_fmt.h — the sample formats of the encode entry points, in one place for the C host side and the HIP side.
 *
 * 0, 1, 2 are the drop-in API's HYDSampleFormat (include/libhydrium/libhydrium.h); 3 and 4 (include/hydrium_amd.h) name
 * pixels that already sit in device memory as IEEE binary16 or bfloat16.  Half precision is a STORAGE FORM of the float
 * class: a sample is widened exactly on load and from there on is a float32 sample (hip/hydk_half.h).
 *
 * 16 ... 19 (include/hydrium_amd.h) name NV12 pictures in device memory: an 8-bit Y plane and a half-resolution plane of
 * interleaved U, V pairs, under one of four matrices.  NV12 is a storage form of the 8-BIT class: a pixel becomes an
 * ordinary 8-bit RGB pixel right after the load (hip/hydk_yuv.h).  src[0] is the first Y sample, src[1] the first U sample,
 * src[2] == src[1] + 1, the pixel stride is 1 and the row stride is the pitch of both planes in bytes.
 *
 * The NV12 family has a second dimension, the chroma filter: sample format = 16 + matrix + 16 * filter.  Filter 0 (16 ... 19)
 * is nearest neighbour; 1 (32 ... 35) interpolates centre-sited chroma, 2 (48 ... 51) left-sited chroma (hip/hydk_chroma.h).
 * An interpolating format is NV12 in layout, size and origin; what it adds is that a sub-rectangle's pixels depend on the
 * PICTURE around it, which hydamd_encode_lf_group_at carries.
 *
 * The family's third dimension is the sample depth: sample format = 16 + matrix + 16 * filter + 64 * depth.  Depth 0 is the
 * 8-bit NV12 family above.  Depth 1, 2, 3 (P010, P012, P016: 80 ..., 144 ..., 208 ...) name the same two planes in 16-bit WORDS
 * holding 10, 12 or 16 significant bits, MSB-aligned: a storage form of the 16-BIT class (hip/hydk_yuv16.h).  src[2] ==
 * src[1] + 2 bytes, the pixel stride is 1 and the row stride is the pitch of both planes in words.  64 ... 79 name nothing.
 *
 * 512 ... 551 name PLANAR YCbCr in device memory, 8 bits a sample in three planes of their own: sample format = 512 + matrix +
 * 4 * subsampling + 16 * filter.  Subsampling 0 is 4:2:0 (I420; YV12 with src[1] and src[2] swapped), 1 is 4:2:2 (I422), 2 is
 * 4:4:4 (I444, filter 0 only); 3 names nothing.  Matrix and filter are the NV12 family's.  A storage form of the 8-BIT class
 * as NV12 is.  src[0] is the first Y sample, src[1] and src[2] the first U and V samples — independent pointers; the row
 * stride is the pitch of the Y plane, whose pixel stride is 1 by definition, and THE PIXEL STRIDE IS THE ONE PITCH OF BOTH
 * CHROMA PLANES, in bytes, of either sign (hyd_fmt_pitch_ok).  The chroma planes are cw x ch: cw = ceil(W / 2) for 4:2:0 and
 * 4:2:2 and W for 4:4:4, ch = ceil(H / 2) for 4:2:0 and H otherwise.  512 + ... + 64 * depth names nothing: deeper planes are at 2048.
 *
 * 2112 ... 2279 name PLANAR YCbCr OF 16-BIT WORDS (I010, I210, I410, I012 ... I416): sample format = 2048 + matrix + 4 * subsampling +
 * 16 * filter + 64 * depth, depth 1, 2, 3 = 10, 12 or 16 significant bits; depth 0 (2048 ... 2111) names nothing.  The planar
 * family's three planes, pointers and pitches with everything in 16-bit samples, and the words LSB-ALIGNED: a stored word w
 * stands for the P01x sample (w << (16 - n)) & 0xFFFF — bits above the depth are shifted out — and from there the picture is
 * the P01x picture of that depth and matrix on the planar family's geometry (hip/hydk_yuv16.h).  A storage form of the 16-BIT
 * class.  All three addresses sit on 2-byte boundaries (HYD_FMT_PLANAR16_ALIGN_MSG).
 */
#ifndef HYD_SAMPLE_FMT_H_
#define HYD_SAMPLE_FMT_H_

#include <stddef.h>

#define HYD_FMT_UINT8 0
#define HYD_FMT_UINT16 1
#define HYD_FMT_FLOAT32 2
#define HYD_FMT_FLOAT16 3
#define HYD_FMT_BFLOAT16 4
#define HYD_FMT_NV12_BT709 16
#define HYD_FMT_NV12_BT709_FULL 17
#define HYD_FMT_NV12_BT601 18
#define HYD_FMT_NV12_BT601_FULL 19
#define HYD_FMT_NV12C_BT709 32 /* centre-sited chroma, interpolated */
#define HYD_FMT_NV12C_BT709_FULL 33
#define HYD_FMT_NV12C_BT601 34
#define HYD_FMT_NV12C_BT601_FULL 35
#define HYD_FMT_NV12L_BT709 48 /* left-sited chroma, interpolated */
#define HYD_FMT_NV12L_BT709_FULL 49
#define HYD_FMT_NV12L_BT601 50
#define HYD_FMT_NV12L_BT601_FULL 51
#define HYD_FMT_NV12_FILTERS 3
/* P010 / P012 / P016: 16 + matrix + 16 * filter + 64 * depth, depth 1, 2, 3 = 10, 12, 16 significant bits in 16-bit words */
#define HYD_FMT_P010_BT709 80
#define HYD_FMT_P010_BT709_FULL 81
#define HYD_FMT_P010_BT601 82
#define HYD_FMT_P010_BT601_FULL 83
#define HYD_FMT_P010C_BT709 96
#define HYD_FMT_P010C_BT709_FULL 97
#define HYD_FMT_P010C_BT601 98
#define HYD_FMT_P010C_BT601_FULL 99
#define HYD_FMT_P010L_BT709 112
#define HYD_FMT_P010L_BT709_FULL 113
#define HYD_FMT_P010L_BT601 114
#define HYD_FMT_P010L_BT601_FULL 115
#define HYD_FMT_P012_BT709 144
#define HYD_FMT_P012_BT709_FULL 145
#define HYD_FMT_P012_BT601 146
#define HYD_FMT_P012_BT601_FULL 147
#define HYD_FMT_P012C_BT709 160
#define HYD_FMT_P012C_BT709_FULL 161
#define HYD_FMT_P012C_BT601 162
#define HYD_FMT_P012C_BT601_FULL 163
#define HYD_FMT_P012L_BT709 176
#define HYD_FMT_P012L_BT709_FULL 177
#define HYD_FMT_P012L_BT601 178
#define HYD_FMT_P012L_BT601_FULL 179
#define HYD_FMT_P016_BT709 208
#define HYD_FMT_P016_BT709_FULL 209
#define HYD_FMT_P016_BT601 210
#define HYD_FMT_P016_BT601_FULL 211
#define HYD_FMT_P016C_BT709 224
#define HYD_FMT_P016C_BT709_FULL 225
#define HYD_FMT_P016C_BT601 226
#define HYD_FMT_P016C_BT601_FULL 227
#define HYD_FMT_P016L_BT709 240
#define HYD_FMT_P016L_BT709_FULL 241
#define HYD_FMT_P016L_BT601 242
#define HYD_FMT_P016L_BT601_FULL 243
#define HYD_FMT_P016_DEPTHS 3
/* planar YCbCr, 8 bits in three planes: 512 + matrix + 4 * subsampling (0 4:2:0, 1 4:2:2, 2 4:4:4) + 16 * filter */
#define HYD_FMT_I420_BT709 512
#define HYD_FMT_I420_BT709_FULL 513
#define HYD_FMT_I420_BT601 514
#define HYD_FMT_I420_BT601_FULL 515
#define HYD_FMT_I422_BT709 516
#define HYD_FMT_I422_BT709_FULL 517
#define HYD_FMT_I422_BT601 518
#define HYD_FMT_I422_BT601_FULL 519
#define HYD_FMT_I444_BT709 520
#define HYD_FMT_I444_BT709_FULL 521
#define HYD_FMT_I444_BT601 522
#define HYD_FMT_I444_BT601_FULL 523
#define HYD_FMT_I420C_BT709 528
#define HYD_FMT_I420C_BT709_FULL 529
#define HYD_FMT_I420C_BT601 530
#define HYD_FMT_I420C_BT601_FULL 531
#define HYD_FMT_I422C_BT709 532
#define HYD_FMT_I422C_BT709_FULL 533
#define HYD_FMT_I422C_BT601 534
#define HYD_FMT_I422C_BT601_FULL 535
#define HYD_FMT_I420L_BT709 544
#define HYD_FMT_I420L_BT709_FULL 545
#define HYD_FMT_I420L_BT601 546
#define HYD_FMT_I420L_BT601_FULL 547
#define HYD_FMT_I422L_BT709 548
#define HYD_FMT_I422L_BT709_FULL 549
#define HYD_FMT_I422L_BT601 550
#define HYD_FMT_I422L_BT601_FULL 551
/* planar YCbCr of 16-bit words, LSB-aligned: 2048 + matrix + 4 * subsampling + 16 * filter + 64 * depth (1, 2, 3 = 10, 12, 16 bits) */
#define HYD_FMT_I010_BT709 2112
#define HYD_FMT_I010_BT709_FULL 2113
#define HYD_FMT_I010_BT601 2114
#define HYD_FMT_I010_BT601_FULL 2115
#define HYD_FMT_I210_BT709 2116
#define HYD_FMT_I210_BT709_FULL 2117
#define HYD_FMT_I210_BT601 2118
#define HYD_FMT_I210_BT601_FULL 2119
#define HYD_FMT_I410_BT709 2120
#define HYD_FMT_I410_BT709_FULL 2121
#define HYD_FMT_I410_BT601 2122
#define HYD_FMT_I410_BT601_FULL 2123
#define HYD_FMT_I010C_BT709 2128
#define HYD_FMT_I010C_BT709_FULL 2129
#define HYD_FMT_I010C_BT601 2130
#define HYD_FMT_I010C_BT601_FULL 2131
#define HYD_FMT_I210C_BT709 2132
#define HYD_FMT_I210C_BT709_FULL 2133
#define HYD_FMT_I210C_BT601 2134
#define HYD_FMT_I210C_BT601_FULL 2135
#define HYD_FMT_I010L_BT709 2144
#define HYD_FMT_I010L_BT709_FULL 2145
#define HYD_FMT_I010L_BT601 2146
#define HYD_FMT_I010L_BT601_FULL 2147
#define HYD_FMT_I210L_BT709 2148
#define HYD_FMT_I210L_BT709_FULL 2149
#define HYD_FMT_I210L_BT601 2150
#define HYD_FMT_I210L_BT601_FULL 2151
#define HYD_FMT_I012_BT709 2176
#define HYD_FMT_I012_BT709_FULL 2177
#define HYD_FMT_I012_BT601 2178
#define HYD_FMT_I012_BT601_FULL 2179
#define HYD_FMT_I212_BT709 2180
#define HYD_FMT_I212_BT709_FULL 2181
#define HYD_FMT_I212_BT601 2182
#define HYD_FMT_I212_BT601_FULL 2183
#define HYD_FMT_I412_BT709 2184
#define HYD_FMT_I412_BT709_FULL 2185
#define HYD_FMT_I412_BT601 2186
#define HYD_FMT_I412_BT601_FULL 2187
#define HYD_FMT_I012C_BT709 2192
#define HYD_FMT_I012C_BT709_FULL 2193
#define HYD_FMT_I012C_BT601 2194
#define HYD_FMT_I012C_BT601_FULL 2195
#define HYD_FMT_I212C_BT709 2196
#define HYD_FMT_I212C_BT709_FULL 2197
#define HYD_FMT_I212C_BT601 2198
#define HYD_FMT_I212C_BT601_FULL 2199
#define HYD_FMT_I012L_BT709 2208
#define HYD_FMT_I012L_BT709_FULL 2209
#define HYD_FMT_I012L_BT601 2210
#define HYD_FMT_I012L_BT601_FULL 2211
#define HYD_FMT_I212L_BT709 2212
#define HYD_FMT_I212L_BT709_FULL 2213
#define HYD_FMT_I212L_BT601 2214
#define HYD_FMT_I212L_BT601_FULL 2215
#define HYD_FMT_I016_BT709 2240
#define HYD_FMT_I016_BT709_FULL 2241
#define HYD_FMT_I016_BT601 2242
#define HYD_FMT_I016_BT601_FULL 2243
#define HYD_FMT_I216_BT709 2244
#define HYD_FMT_I216_BT709_FULL 2245
#define HYD_FMT_I216_BT601 2246
#define HYD_FMT_I216_BT601_FULL 2247
#define HYD_FMT_I416_BT709 2248
#define HYD_FMT_I416_BT709_FULL 2249
#define HYD_FMT_I416_BT601 2250
#define HYD_FMT_I416_BT601_FULL 2251
#define HYD_FMT_I016C_BT709 2256
#define HYD_FMT_I016C_BT709_FULL 2257
#define HYD_FMT_I016C_BT601 2258
#define HYD_FMT_I016C_BT601_FULL 2259
#define HYD_FMT_I216C_BT709 2260
#define HYD_FMT_I216C_BT709_FULL 2261
#define HYD_FMT_I216C_BT601 2262
#define HYD_FMT_I216C_BT601_FULL 2263
#define HYD_FMT_I016L_BT709 2272
#define HYD_FMT_I016L_BT709_FULL 2273
#define HYD_FMT_I016L_BT601 2274
#define HYD_FMT_I016L_BT601_FULL 2275
#define HYD_FMT_I216L_BT709 2276
#define HYD_FMT_I216L_BT709_FULL 2277
#define HYD_FMT_I216L_BT601 2278
#define HYD_FMT_I216L_BT601_FULL 2279
#define HYD_FMT_PLANAR16_BASE 2048
#define HYD_FMT_PLANAR_420 0
#define HYD_FMT_PLANAR_422 1
#define HYD_FMT_PLANAR_444 2

/* YCbCr 4:2:0 in two planes with nearest-neighbour chroma, and which of the four matrices of hip/hydk_yuv.h (0 ... 3) */
static inline int hyd_fmt_is_nv12(int fmt) { return fmt >= HYD_FMT_NV12_BT709 && fmt <= HYD_FMT_NV12_BT601_FULL; }
static inline int hyd_fmt_nv12_matrix(int fmt) { return fmt - HYD_FMT_NV12_BT709; }
/* the NV12 FAMILY, 16 + matrix + 16 * filter: its layout, size and origin rules; then the filter (0 nearest, 1 centre-sited,
 * 2 left-sited) and the matrix of one of its twelve numbers */
static inline int hyd_fmt_is_nv12_family(int fmt) {
    return fmt >= HYD_FMT_NV12_BT709 && fmt < HYD_FMT_NV12_BT709 + 16 * HYD_FMT_NV12_FILTERS && ((fmt - HYD_FMT_NV12_BT709) & 15) < 4;
}
static inline int hyd_fmt_nv12_filter(int fmt) { return (fmt - HYD_FMT_NV12_BT709) >> 4; }
static inline int hyd_fmt_nv12_family_matrix(int fmt) { return (fmt - HYD_FMT_NV12_BT709) & 3; }
/* the eight whose chroma is interpolated: a sub-rectangle's pixels depend on the picture around it */
static inline int hyd_fmt_is_nv12_interp(int fmt) { return hyd_fmt_is_nv12_family(fmt) && hyd_fmt_nv12_filter(fmt) != 0; }

/* the P016 FAMILY, the thirty-six numbers of depth 1 ... 3: 16-bit words in NV12's two planes.  Its depth index (1, 2, 3), the
 * significant bits that names (10, 12, 16), and filter and matrix as the 8-bit family has them */
static inline int hyd_fmt_is_p016_family(int fmt) {
    return fmt >= HYD_FMT_P010_BT709 && fmt <= HYD_FMT_P016L_BT601_FULL && hyd_fmt_is_nv12_family(fmt & 63);
}
static inline int hyd_fmt_p016_depth(int fmt) { return (fmt - HYD_FMT_NV12_BT709) >> 6; }
static inline int hyd_fmt_p016_bits(int fmt) { return hyd_fmt_p016_depth(fmt) == 1 ? 10 : hyd_fmt_p016_depth(fmt) == 2 ? 12 : 16; }
static inline int hyd_fmt_p016_filter(int fmt) { return ((fmt - HYD_FMT_NV12_BT709) >> 4) & 3; }
static inline int hyd_fmt_p016_matrix(int fmt) { return (fmt - HYD_FMT_NV12_BT709) & 3; }
static inline int hyd_fmt_is_p016_interp(int fmt) { return hyd_fmt_is_p016_family(fmt) && hyd_fmt_p016_filter(fmt) != 0; }
/* 4:2:0 in two planes at any depth (layout and origin rules in samples), and those of them whose chroma is interpolated */
static inline int hyd_fmt_is_yuv420(int fmt) { return hyd_fmt_is_nv12_family(fmt) || hyd_fmt_is_p016_family(fmt); }
static inline int hyd_fmt_is_yuv420_interp(int fmt) { return hyd_fmt_is_nv12_interp(fmt) || hyd_fmt_is_p016_interp(fmt); }


/* the PLANAR family, twenty-eight numbers: its subsampling (HYD_FMT_PLANAR_*), filter and matrix, and the sixteen whose chroma
 * is interpolated.  4:4:4 has nothing to interpolate: filter 0 only */
static inline int hyd_fmt_planar_sub(int fmt) { return ((fmt - HYD_FMT_I420_BT709) >> 2) & 3; }
static inline int hyd_fmt_planar_filter(int fmt) { return (fmt - HYD_FMT_I420_BT709) >> 4; }
static inline int hyd_fmt_planar_matrix(int fmt) { return (fmt - HYD_FMT_I420_BT709) & 3; }
static inline int hyd_fmt_is_planar_yuv(int fmt) {
    return fmt >= HYD_FMT_I420_BT709 && fmt <= HYD_FMT_I422L_BT601_FULL && hyd_fmt_planar_sub(fmt) <= HYD_FMT_PLANAR_444 &&
           (hyd_fmt_planar_sub(fmt) != HYD_FMT_PLANAR_444 || hyd_fmt_planar_filter(fmt) == 0);
}
static inline int hyd_fmt_is_planar_interp(int fmt) { return hyd_fmt_is_planar_yuv(fmt) && hyd_fmt_planar_filter(fmt) != 0; }
/* log2 of the pixels a chroma sample spans across and down */
static inline int hyd_fmt_planar_sx(int fmt) { return hyd_fmt_planar_sub(fmt) != HYD_FMT_PLANAR_444; }
static inline int hyd_fmt_planar_sy(int fmt) { return hyd_fmt_planar_sub(fmt) == HYD_FMT_PLANAR_420; }

/* the PLANAR16 family, eighty-four numbers: the planar family's twenty-eight (subsampling, filter, matrix) at each depth index 1,
 * 2, 3 — 10, 12, 16 significant bits, LSB-aligned in 16-bit words.  hyd_fmt_is_planar_yuv and its helpers keep meaning the
 * 8-bit twenty-eight */
static inline int hyd_fmt_planar16_sub(int fmt) { return ((fmt - HYD_FMT_PLANAR16_BASE) >> 2) & 3; }
static inline int hyd_fmt_planar16_filter(int fmt) { return ((fmt - HYD_FMT_PLANAR16_BASE) >> 4) & 3; }
static inline int hyd_fmt_planar16_matrix(int fmt) { return (fmt - HYD_FMT_PLANAR16_BASE) & 3; }
static inline int hyd_fmt_planar16_depth(int fmt) { return (fmt - HYD_FMT_PLANAR16_BASE) >> 6; }
static inline int hyd_fmt_is_planar16(int fmt) {
    return fmt >= HYD_FMT_I010_BT709 && fmt <= HYD_FMT_I216L_BT601_FULL && hyd_fmt_is_planar_yuv(HYD_FMT_I420_BT709 + (fmt & 63));
}
static inline int hyd_fmt_planar16_bits(int fmt) { return hyd_fmt_planar16_depth(fmt) == 1 ? 10 : hyd_fmt_planar16_depth(fmt) == 2 ? 12 : 16; }
static inline int hyd_fmt_is_planar16_interp(int fmt) { return hyd_fmt_is_planar16(fmt) && hyd_fmt_planar16_filter(fmt) != 0; }
static inline int hyd_fmt_planar16_sx(int fmt) { return hyd_fmt_planar16_sub(fmt) != HYD_FMT_PLANAR_444; }
static inline int hyd_fmt_planar16_sy(int fmt) { return hyd_fmt_planar16_sub(fmt) == HYD_FMT_PLANAR_420; }

/* what an entry point that reads DEVICE pixels takes */
static inline int hyd_fmt_is_device(int fmt) {
    return (fmt >= HYD_FMT_UINT8 && fmt <= HYD_FMT_BFLOAT16) || hyd_fmt_is_yuv420(fmt) || hyd_fmt_is_planar_yuv(fmt) || hyd_fmt_is_planar16(fmt);
}
/* what an entry point that reads HOST pixels takes: the reference's three */
static inline int hyd_fmt_is_host(int fmt) { return fmt >= HYD_FMT_UINT8 && fmt <= HYD_FMT_FLOAT32; }
/* float class: 8-byte token records, 72 histogram bins, the non-finite check */
static inline int hyd_fmt_is_float(int fmt) { return fmt >= HYD_FMT_FLOAT32 && fmt <= HYD_FMT_BFLOAT16; }
/* bytes per sample of a format hyd_fmt_is_device accepts (strides are in samples); 0 for anything else */
static inline size_t hyd_fmt_bytes(int fmt) {
    switch (fmt) {
    case HYD_FMT_UINT8:
    case HYD_FMT_NV12_BT709:
    case HYD_FMT_NV12_BT709_FULL:
    case HYD_FMT_NV12_BT601:
    case HYD_FMT_NV12_BT601_FULL:
    case HYD_FMT_NV12C_BT709:
    case HYD_FMT_NV12C_BT709_FULL:
    case HYD_FMT_NV12C_BT601:
    case HYD_FMT_NV12C_BT601_FULL:
    case HYD_FMT_NV12L_BT709:
    case HYD_FMT_NV12L_BT709_FULL:
    case HYD_FMT_NV12L_BT601:
    case HYD_FMT_NV12L_BT601_FULL:
        return 1;
    case HYD_FMT_UINT16:
    case HYD_FMT_FLOAT16:
    case HYD_FMT_BFLOAT16:
        return 2;
    case HYD_FMT_FLOAT32:
        return 4;
    default:
        return hyd_fmt_is_p016_family(fmt) || hyd_fmt_is_planar16(fmt) ? 2 : hyd_fmt_is_planar_yuv(fmt) ? 1 : 0;
    }
}

/* NV12's layout (all three filters): unit pixel stride and V one byte behind U; every other format takes any layout.  An entry point that
 * finds 0 here fails with HYD_FMT_NV12_LAYOUT_MSG before it enqueues anything. */
#define HYD_FMT_NV12_LAYOUT_MSG "NV12 wants pixel_stride 1 and V one byte behind U"
/* what hydamd_encode_image_multi says to a format with interpolated chroma */
#define HYD_FMT_NV12_SHARDED_MSG "interpolated chroma is not sharded: a shard does not hold its neighbour's chroma rows"
/* the P016 family's: unit pixel stride, V one 16-bit sample behind U, all three addresses on 2-byte boundaries */
#define HYD_FMT_P016_LAYOUT_MSG "P010/P016 wants pixel_stride 1 and V one sample behind U"
/* the planar16 family's: three free pointers as the planar family's, each on a 2-byte boundary */
#define HYD_FMT_PLANAR16_ALIGN_MSG "planar YCbCr of 16-bit words wants its three planes on 2-byte boundaries"
static inline int hyd_fmt_layout_ok(int fmt, const void *const src[3], ptrdiff_t pixel_stride) {
    if (hyd_fmt_is_planar16(fmt))
        return (((size_t)src[0] | (size_t)src[1] | (size_t)src[2]) & 1) == 0;
    if (hyd_fmt_is_p016_family(fmt))
        return pixel_stride == 1 && (const char *)src[2] == (const char *)src[1] + 2 &&
               (((size_t)src[0] | (size_t)src[1]) & 1) == 0;
    return !hyd_fmt_is_nv12_family(fmt) || (pixel_stride == 1 && (const char *)src[2] == (const char *)src[1] + 1);
}
/* The planar families have no layout to hold (three free pointers), but their pixel_stride argument is the chroma planes' pitch
 * in samples: a pitch shorter than a chroma row of the picture the call names, `width` pixels across — the habitual pixel_stride 1 — fails
 * with HYD_FMT_PLANAR_PITCH_MSG before anything is enqueued.  Every other format passes. */
#define HYD_FMT_PLANAR_PITCH_MSG "planar YCbCr wants the chroma planes' pitch in pixel_stride"
static inline int hyd_fmt_pitch_ok(int fmt, ptrdiff_t pixel_stride, size_t width) {
    if (!hyd_fmt_is_planar_yuv(fmt) && !hyd_fmt_is_planar16(fmt))
        return 1;
    const size_t pitch = pixel_stride < 0 ? (size_t)0 - (size_t)pixel_stride : (size_t)pixel_stride;
    return pitch >= (((fmt >> 2) & 3) != HYD_FMT_PLANAR_444 ? (width + 1) >> 1 : width); /* (both bases are multiples of 64) */
}
/* what an entry point says when hyd_fmt_layout_ok is 0 */
static inline const char *hyd_fmt_layout_msg(int fmt) {
    return hyd_fmt_is_planar16(fmt) ? HYD_FMT_PLANAR16_ALIGN_MSG : hyd_fmt_is_p016_family(fmt) ? HYD_FMT_P016_LAYOUT_MSG : HYD_FMT_NV12_LAYOUT_MSG;
}

/* The three origin pointers of the sub-rectangle at pixel (x0, y0) of a picture of a device format — an LF group, a tile, a
 * shard's first row.  Strides are in samples.  NV12: the chroma plane has a row for every two picture rows and two bytes for
 * every two columns, so its origin is row y0 / 2, byte x0; x0 and y0 must be even (every origin the library computes is a
 * multiple of 256).  The P016 family: the same in 16-bit words.  The planar family: Y at row y0, byte x0 of its plane; U and V
 * at row y0 >> sy, byte x0 >> sx of theirs, whose pitch is pixel_stride; x0 must be even, and y0 for 4:2:0.  The planar16
 * family: the same in 16-bit words. */
static inline void hyd_fmt_origin(int fmt, const void *const src[3], ptrdiff_t row_stride, ptrdiff_t pixel_stride, size_t x0,
                                  size_t y0, const void *origin[3]) {
    if (hyd_fmt_is_yuv420(fmt)) {
        const ptrdiff_t bytes = (ptrdiff_t)hyd_fmt_bytes(fmt);
        const ptrdiff_t chroma = ((ptrdiff_t)(y0 / 2) * row_stride + (ptrdiff_t)x0) * bytes;
        origin[0] = (const char *)src[0] + ((ptrdiff_t)y0 * row_stride + (ptrdiff_t)x0) * bytes;
        origin[1] = (const char *)src[1] + chroma;
        origin[2] = (const char *)src[2] + chroma;
        return;
    }
    if (hyd_fmt_is_planar_yuv(fmt)) {
        const ptrdiff_t chroma = (ptrdiff_t)(y0 >> hyd_fmt_planar_sy(fmt)) * pixel_stride + (ptrdiff_t)(x0 >> hyd_fmt_planar_sx(fmt));
        origin[0] = (const char *)src[0] + ((ptrdiff_t)y0 * row_stride + (ptrdiff_t)x0);
        origin[1] = (const char *)src[1] + chroma;
        origin[2] = (const char *)src[2] + chroma;
        return;
    }
    if (hyd_fmt_is_planar16(fmt)) {
        const ptrdiff_t chroma = (ptrdiff_t)(y0 >> hyd_fmt_planar16_sy(fmt)) * pixel_stride + (ptrdiff_t)(x0 >> hyd_fmt_planar16_sx(fmt));
        origin[0] = (const char *)src[0] + ((ptrdiff_t)y0 * row_stride + (ptrdiff_t)x0) * 2;
        origin[1] = (const char *)src[1] + chroma * 2;
        origin[2] = (const char *)src[2] + chroma * 2;
        return;
    }
    const ptrdiff_t off = ((ptrdiff_t)y0 * row_stride + (ptrdiff_t)x0 * pixel_stride) * (ptrdiff_t)hyd_fmt_bytes(fmt);
    for (int c = 0; c < 3; c++)
        origin[c] = (const char *)src[c] + off;
}

#endif /* HYD_SAMPLE_FMT_H_ */
