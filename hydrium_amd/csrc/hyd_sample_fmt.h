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
 * CHROMA PLANES, in bytes, of either sign (hyd_fmt_refusal).  The chroma planes are cw x ch: cw = ceil(W / 2) for 4:2:0 and
 * 4:2:2 and W for 4:4:4, ch = ceil(H / 2) for 4:2:0 and H otherwise.  512 + ... + 64 * depth names nothing: deeper planes are at 2048.
 *
 * 2112 ... 2279 name PLANAR YCbCr OF 16-BIT WORDS (I010, I210, I410, I012 ... I416): sample format = 2048 + matrix + 4 * subsampling +
 * 16 * filter + 64 * depth, depth 1, 2, 3 = 10, 12 or 16 significant bits; depth 0 (2048 ... 2111) names nothing.  The planar
 * family's three planes, pointers and pitches with everything in 16-bit samples, and the words LSB-ALIGNED: a stored word w
 * stands for the P01x sample (w << (16 - n)) & 0xFFFF — bits above the depth are shifted out — and from there the picture is
 * the P01x picture of that depth and matrix on the planar family's geometry (hip/hydk_yuv16.h).  A storage form of the 16-BIT
 * class.  All three addresses sit on 2-byte boundaries (HYD_FMT_PLANAR16_ALIGN_MSG).
 *
 * 8192 ... 8227 name PACKED 4:2:2 YCbCr in device memory (YUY2 / YUYV, UYVY, YVYU, VYUY): sample format = 8192 + matrix + 16 * filter,
 * the subsampling bits 0 and no depth (8192 + 64 * depth names nothing: deeper packed words are at 32768).  One plane of 4-byte groups, each two pixels: two Y
 * bytes, a U and a V.  THE BYTE ORDER IS READ OFF THE POINTERS, not off the number: src[0] is the first Y byte, src[1] and src[2]
 * the U and the V byte of the same group — (src[1] - src[0], src[2] - src[0]) is (1, 3) YUYV, (3, 1) YVYU, (-1, 1) UYVY or
 * (1, -1) VYUY; the pixel stride is 2, the distance of two Y samples, and the row stride the pitch in bytes, of either sign
 * (HYD_FMT_PACKED_LAYOUT_MSG).  A storage form of the 8-BIT class; the picture is the I422 picture of the de-interleaved bytes
 * (hip/hydk_yuy2.h).
 *
 * 32832 ... 32995 name PACKED 4:2:2 YCbCr OF 16-BIT WORDS in device memory (Y210, Y212, Y216): sample format = 32768 + matrix +
 * 16 * filter + 64 * depth, depth 1, 2, 3 = 10, 12 or 16 significant bits, MSB-ALIGNED as P010's are and counted as stored; the
 * subsampling bits are 0 and depth 0 (32768 ... 32831) names nothing.  One plane of groups of four words, each two pixels: two Y
 * words, a U and a V.  THE WORD ORDER IS READ OFF THE POINTERS as the byte order of YUY2 is, with the differences in WORDS:
 * (1, 3) Y210's own order, (3, 1), (-1, 1) or (1, -1); the pixel stride is 2, the row stride the pitch in words, of either sign,
 * and all three addresses sit on 2-byte boundaries (HYD_FMT_PACKED16_LAYOUT_MSG).  A storage form of the 16-BIT class; the picture
 * is the 4:2:2 picture of the de-interleaved words under the P01x conversion of that depth (hip/hydk_y216.h).
 *
 * 131072, 131073 and 131144 ... 131147 name pictures whose PIXEL IS ONE 32-BIT WORD of three 10-bit fields and two spare bits, in
 * device memory (hip/hydk_rgb10.h).  131072 RGB10A2: R in bits 0 ... 9, G in 10 ... 19, B in 20 ... 29 (Vulkan A2B10G10R10, DXGI
 * R10G10B10A2, DRM XBGR2101010); 131073 BGR10A2: B low, R high (Vulkan A2R10G10B10, DRM XRGB2101010) — the two sit at the base's
 * depth-0 corner as 0 ... 4 sit at the bottom of the table.  131144 ... 131147 Y410 (DRM XVYU2101010): 131072 + matrix + 4 * 2
 * (4:4:4) + 64 * 1 (10 bits), U in bits 0 ... 9, Y in 10 ... 19, V in 20 ... 29.  Bits 30 and 31 never matter.  A SAMPLE IS THE
 * DWORD: src[0] == src[1] == src[2], the first dword, on a 4-byte boundary; the pixel stride is 1 and the row stride the pitch in
 * dwords, of either sign (HYD_FMT_DWORD_LAYOUT_MSG).  Storage forms of the 16-BIT class: an RGB field v stands for the 16-bit
 * sample nearest to v / 1023, a Y410 field for the P010 sample v << 6, so that a Y410 picture is the I410 picture of its fields.
 *
 * 524296 ... 524299, 524424 ... 524427 and 524488 ... 524491 name pictures whose PIXEL IS ONE GROUP OF FOUR SAMPLES — Y, U, V and a
 * fourth that is ignored — in device memory, 4:4:4 (hip/hydk_quad.h): 524288 + matrix + 4 * 2 + 64 * depth.  Depth 0, AYUV (VA-API
 * AYUV / XYUV, DRM XYUV8888, ffmpeg vuya / vuyx): a dword of the bytes V, U, Y, A — V in bits 0 ... 7, U in 8 ... 15, Y in 16 ... 23.
 * Depth 2 and 3, Y412 and Y416 (XV36, XV48): a qword of the words U, Y, V, A, MSB-aligned — U in bits 0 ... 15, Y in 16 ... 31, V in
 * 32 ... 47.  Depth 1 names nothing: the 10-bit surface is Y410 at 131144.  A SAMPLE IS THE GROUP: src[0] == src[1] == src[2], the
 * first pixel, on a boundary of the pixel's size (4 or 8 bytes); the pixel stride is 1 and the row stride the pitch in pixels, of
 * either sign (HYD_FMT_QUAD_LAYOUT_MSG).  AYUV is a storage form of the 8-BIT class, the I444 picture of its three bytes; Y412 and
 * Y416 of the 16-BIT class, the words as stored under the P01x conversion of that depth, so a Y416 picture is the I416 picture of
 * its three words.
 *
 * 8388608 and 8388609 name pictures whose PIXEL IS ONE 32-BIT WORD of three UNSIGNED FLOATS, in device memory (hip/hydk_ufloat.h):
 * the float render targets.  8388608 R11G11B10F (DXGI R11G11B10_FLOAT, Vulkan B10G11R11_UFLOAT_PACK32): R in bits 0 ... 10, G in
 * 11 ... 21, B in 22 ... 31, each a 5-bit exponent above 6, 6 and 5 mantissa bits; 8388609 RGB9E5 (DXGI R9G9B9E5_SHAREDEXP, Vulkan
 * E5B9G9R9_UFLOAT_PACK32): three 9-bit mantissas under one 5-bit exponent in bits 27 ... 31.  They are no YCbCr and have no
 * matrix, so they sit at a base of their own as 0 ... 4 sit at the bottom of the table: 2^23.  (2097152, the next of the bases' x 4
 * sequence, and 2^31 - 200 ... 2^31 - 1 were passed over: tests/test_quad_formats.py holds 2097100 ... 2097200 and that top range to
 * naming nothing, and must keep passing as it stands.)  A SAMPLE IS THE DWORD, as RGB10A2's: src[0] == src[1] == src[2], the first
 * dword, on a 4-byte boundary; the pixel stride is 1 and the row stride the pitch in dwords, of either sign
 * (HYD_FMT_UFLOAT_LAYOUT_MSG).  Storage forms of the FLOAT class: a field is widened exactly to float32 on load and is a float32
 * sample from there on, an R11G11B10F infinity or NaN included.
 */
#ifndef HYD_SAMPLE_FMT_H_
#define HYD_SAMPLE_FMT_H_

#include <stddef.h>

/* the five that are no YCbCr picture; every YCbCr number is spelled by hyd_fmt_describe alone (its public name: include/hydrium_amd.h) */
#define HYD_FMT_UINT8 0
#define HYD_FMT_UINT16 1
#define HYD_FMT_FLOAT32 2
#define HYD_FMT_FLOAT16 3
#define HYD_FMT_BFLOAT16 4

/* THE RULE: a YCbCr sample format = base + matrix + 4 * subsampling + 16 * filter + 64 * depth.  The base names the layout and
 * the alignment of the bits in a word: 16 — (U, V) pairs in one plane, MSB-aligned; 512 — a plane each, 8 bits; 2048 — a plane
 * each in 16-bit words, LSB-aligned; 8192 — Y, U and V bytes packed in one plane, 4:2:2 (the subsampling bits are 0, depth 0 only);
 * 32768 — the same groups in 16-bit words, MSB-aligned (the subsampling bits are 0, depth 1 ... 3 only); 131072 — Y, U and V as
 * 10-bit fields of one dword a pixel, 4:4:4 (subsampling 2, filter 0, depth 1 only), and at its depth-0 corner the two RGB orders of
 * the same dword; 524288 — Y, U, V and an ignored fourth sample in one group a pixel, 4:4:4 (subsampling 2, filter 0): bytes in a
 * dword at depth 0, MSB-aligned 16-bit words in a qword at depth 2 and 3 (depth 1 names nothing: that surface is Y410). */
#define HYD_FMT_BASE_PAIRS 16
#define HYD_FMT_BASE_PLANES 512
#define HYD_FMT_BASE_PLANES16 2048
#define HYD_FMT_BASE_PACKED 8192
#define HYD_FMT_BASE_PACKED16 32768
#define HYD_FMT_BASE_DWORD 131072
#define HYD_FMT_BASE_QUAD 524288
#define HYD_FMT_BASE_UFLOAT 8388608 /* no YCbCr base: R11G11B10F and, + 1, RGB9E5 */
/* HydFmt.layout */
#define HYD_LAYOUT_RGB 0    /* three samples a pixel, any strides */
#define HYD_LAYOUT_PAIRS 1  /* a Y plane and a plane of (U, V) pairs */
#define HYD_LAYOUT_PLANES 2 /* Y, U and V planes of their own */
#define HYD_LAYOUT_PACKED 3 /* Y and chroma in one plane: groups of Y, U, Y, V bytes (or 16-bit words: HydFmt.bytes) in one of four orders */
#define HYD_LAYOUT_DWORD 4  /* a pixel is one dword of three 10-bit fields: one pointer three times over, a sample is the dword */
#define HYD_LAYOUT_QUAD 5   /* a pixel is one group of four samples, the fourth ignored (bytes in a dword, or words in a qword: HydFmt.bytes 4 or 8): one pointer three times over, a sample is the group */
#define HYD_LAYOUT_UFLOAT 6 /* a pixel is one dword of three unsigned floats (R11G11B10F) or of three mantissas and their exponent (RGB9E5): one pointer three times over, a sample is the dword */
/* HydFmt.sub */
#define HYD_FMT_SUB_420 0
#define HYD_FMT_SUB_422 1
#define HYD_FMT_SUB_444 2

/* Everything a caller asks of a sample format.  A number that names nothing: all zeros. */
typedef struct HydFmt {
    int device;   /* an entry point that reads DEVICE pixels takes it */
    int host;     /* an entry point that reads HOST pixels takes it: the reference's three */
    int is_float; /* float class: 8-byte token records, 72 histogram bins, the non-finite check */
    int bytes;    /* of a sample; strides are in samples */
    int layout;   /* HYD_LAYOUT_* */
    int matrix;   /* 0 ... 3: BT.709, BT.709 full range, BT.601, BT.601 full range */
    int filter;   /* 0 nearest, 1 centre-sited, 2 left-sited: != 0 — a sub-rectangle's pixels depend on the picture around it */
    int sub;      /* HYD_FMT_SUB_*; pairs are 4:2:0, packed is 4:2:2 */
    int sx, sy;   /* log2 of the pixels a chroma sample spans across and down */
    int depth;    /* 0 ... 3 */
    int bits;     /* significant bits of a sample: 8, 10, 12, 16 by depth; an RGB-like format's are all of its bytes' */
} HydFmt;

#ifdef __cplusplus
#define HYD_FMT_FN constexpr static inline
#else
#define HYD_FMT_FN static inline
#endif

HYD_FMT_FN HydFmt hyd_fmt_describe(int fmt) {
    HydFmt d = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (fmt >= HYD_FMT_UINT8 && fmt <= HYD_FMT_BFLOAT16) {
        d.device = 1;
        d.host = fmt <= HYD_FMT_FLOAT32;
        d.is_float = fmt >= HYD_FMT_FLOAT32;
        d.bytes = fmt == HYD_FMT_UINT8 ? 1 : fmt == HYD_FMT_FLOAT32 ? 4 : 2;
        d.bits = 8 * d.bytes;
        return d;
    }
    if (fmt >= HYD_FMT_BASE_UFLOAT) { /* 8388608 R11G11B10F, 8388609 RGB9E5: float class, a dword a pixel */
        if (fmt > HYD_FMT_BASE_UFLOAT + 1)
            return d;
        d.device = 1;
        d.is_float = 1;
        d.bytes = 4;
        d.layout = HYD_LAYOUT_UFLOAT;
        d.bits = 32;
        return d;
    }
    if (fmt >= HYD_FMT_BASE_QUAD) { /* 524288 + matrix + 4 * 2 + 64 * depth: 4:4:4, no filter, depth 0, 2, 3 */
        const int n = fmt - HYD_FMT_BASE_QUAD, depth = n >> 6;
        if ((n & 60) != 4 * HYD_FMT_SUB_444 || depth == 1 || depth > 3)
            return d;
        d.device = 1;
        d.bytes = depth ? 8 : 4;
        d.layout = HYD_LAYOUT_QUAD;
        d.matrix = n & 3;
        d.sub = HYD_FMT_SUB_444;
        d.depth = depth;
        d.bits = depth == 0 ? 8 : depth == 2 ? 12 : 16;
        return d;
    }
    if (fmt >= HYD_FMT_BASE_DWORD) { /* 131072, 131073: the RGB orders; 131072 + matrix + 4 * 2 + 64 * 1: Y410 */
        const int n = fmt - HYD_FMT_BASE_DWORD;
        if (n > 1 && (n < 72 || n > 75))
            return d;
        d.device = 1;
        d.bytes = 4;
        d.layout = HYD_LAYOUT_DWORD;
        d.bits = 10;
        if (n > 1) {
            d.matrix = n & 3;
            d.sub = HYD_FMT_SUB_444;
            d.depth = 1;
        }
        return d;
    }
    if (fmt >= HYD_FMT_BASE_PACKED16) { /* 32768 + matrix + 16 * filter + 64 * depth: no subsampling bits, depth 1 ... 3 */
        const int n = fmt - HYD_FMT_BASE_PACKED16, depth = n >> 6;
        if ((n & 12) || (n & 48) == 48 || depth < 1 || depth > 3)
            return d;
        d.device = 1;
        d.bytes = 2;
        d.layout = HYD_LAYOUT_PACKED;
        d.matrix = n & 3;
        d.filter = (n >> 4) & 3;
        d.sub = HYD_FMT_SUB_422;
        d.sx = 1;
        d.depth = depth;
        d.bits = depth == 1 ? 10 : depth == 2 ? 12 : 16;
        return d;
    }
    if (fmt >= HYD_FMT_BASE_PACKED) { /* 8192 + matrix + 16 * filter: no subsampling bits, no depth */
        const int n = fmt - HYD_FMT_BASE_PACKED;
        if ((n & 12) || n >= 48)
            return d;
        d.device = 1;
        d.bytes = 1;
        d.layout = HYD_LAYOUT_PACKED;
        d.matrix = n & 3;
        d.filter = n >> 4;
        d.sub = HYD_FMT_SUB_422;
        d.sx = 1;
        d.bits = 8;
        return d;
    }
    const int base = fmt >= HYD_FMT_BASE_PLANES16 ? HYD_FMT_BASE_PLANES16 : fmt >= HYD_FMT_BASE_PLANES ? HYD_FMT_BASE_PLANES : HYD_FMT_BASE_PAIRS;
    const int n = fmt - base, sub = (n >> 2) & 3, filter = (n >> 4) & 3, depth = n >> 6;
    if (n < 0 || depth > 3 || filter > 2 || sub > HYD_FMT_SUB_444 || (sub == HYD_FMT_SUB_444 && filter) ||
        (base == HYD_FMT_BASE_PAIRS && sub) || (base == HYD_FMT_BASE_PLANES && depth) || (base == HYD_FMT_BASE_PLANES16 && !depth))
        return d;
    d.device = 1;
    d.bytes = depth ? 2 : 1;
    d.layout = base == HYD_FMT_BASE_PAIRS ? HYD_LAYOUT_PAIRS : HYD_LAYOUT_PLANES;
    d.matrix = n & 3;
    d.filter = filter;
    d.sub = sub;
    d.sx = sub != HYD_FMT_SUB_444;
    d.sy = sub == HYD_FMT_SUB_420;
    d.depth = depth;
    d.bits = depth == 0 ? 8 : depth == 1 ? 10 : depth == 2 ? 12 : 16;
    return d;
}

/* What an entry point that reads device pixels fails with before it enqueues anything, or NULL: "Invalid Sample Format"; then
 * the layout of src — pairs want unit pixel stride and V one sample behind U (and words on 2-byte boundaries), planes of
 * 16-bit words want their three addresses on 2-byte boundaries, packed 4:2:2 wants pixel stride 2 and U and V in the bytes beside
 * Y in one of the four orders (packed words: the same in words, on 2-byte boundaries), a dword a pixel wants pixel stride 1 and
 * one dword-aligned pointer three times over (three 10-bit fields and three unsigned floats alike), a group of four a pixel the
 * same on a boundary of the group's size (4 or 8 bytes),
 * every other format takes any layout; then
 * the chroma pitch —
 * a plane each has no layout to hold (three free pointers), but its pixel_stride argument is the chroma planes' pitch in
 * samples, of either sign: one shorter than a chroma row of the picture the call names, `width` pixels across — the habitual
 * pixel_stride 1 — is refused.  src NULL: the layout is not looked at (a caller with several pictures holds each to its
 * layout before any to its pitch); width 0: no pitch is too short. */
#define HYD_FMT_NV12_LAYOUT_MSG "NV12 wants pixel_stride 1 and V one byte behind U"
#define HYD_FMT_P016_LAYOUT_MSG "P010/P016 wants pixel_stride 1 and V one sample behind U"
#define HYD_FMT_PLANAR16_ALIGN_MSG "planar YCbCr of 16-bit words wants its three planes on 2-byte boundaries"
#define HYD_FMT_PLANAR_PITCH_MSG "planar YCbCr wants the chroma planes' pitch in pixel_stride"
#define HYD_FMT_PACKED_LAYOUT_MSG "YUY2/UYVY wants pixel_stride 2 and U and V in the bytes beside Y"
#define HYD_FMT_PACKED16_LAYOUT_MSG "Y210/Y216 wants pixel_stride 2 and U and V in the words beside Y"
#define HYD_FMT_DWORD_LAYOUT_MSG "RGB10A2/Y410 wants pixel_stride 1 and three equal pointers on a 4-byte boundary"
#define HYD_FMT_QUAD_LAYOUT_MSG "AYUV/Y416 wants pixel_stride 1 and three equal pointers on a boundary of the pixel's size"
#define HYD_FMT_UFLOAT_LAYOUT_MSG "R11G11B10F/RGB9E5 wants pixel_stride 1 and three equal pointers on a 4-byte boundary"
/* what hydamd_encode_image_multi says to a format with interpolated chroma */
#define HYD_FMT_NV12_SHARDED_MSG "interpolated chroma is not sharded: a shard does not hold its neighbour's chroma rows"
/* The byte order of a packed 4:2:2 picture, read off its pointers: 0 YUYV (U at +1, V at +3), 1 YVYU (+3, +1), 2 UYVY (-1, +1),
 * 3 VYUY (+1, -1) — bit 1: Y is the second byte of a pair, bit 0: V comes before U; -1: no such group.  bytes: of a sample (1 YUY2,
 * 2 Y210 / Y212 / Y216) — the differences are in samples, and every address is a multiple of it. */
#define HYD_PACKED_YUYV 0
#define HYD_PACKED_YVYU 1
#define HYD_PACKED_UYVY 2
#define HYD_PACKED_VYUY 3
static inline int hyd_fmt_packed_order(const void *const src[3], int bytes) {
    /* (the addresses as integers: three pointers that are no group at all need not point into one object) */
    const ptrdiff_t du = (ptrdiff_t)((size_t)src[1] - (size_t)src[0]), dv = (ptrdiff_t)((size_t)src[2] - (size_t)src[0]);
    if (bytes != 1 && (bytes != 2 || (((size_t)src[0] | (size_t)src[1] | (size_t)src[2]) & 1u)))
        return -1;
    const ptrdiff_t u = du / bytes, v = dv / bytes; /* (exact: aligned addresses differ by whole samples) */
    return u == 1 && v == 3 ? HYD_PACKED_YUYV : u == 3 && v == 1 ? HYD_PACKED_YVYU : u == -1 && v == 1 ? HYD_PACKED_UYVY : u == 1 && v == -1 ? HYD_PACKED_VYUY : -1;
}
#ifdef __cplusplus
/* (the order of bytes, as C++ callers of the 8-bit family have spelled it since before there were words) */
static inline int hyd_fmt_packed_order(const void *const src[3]) { return hyd_fmt_packed_order(src, 1); }
#endif
static inline const char *hyd_fmt_refusal(int fmt, const void *const src[3], ptrdiff_t pixel_stride, size_t width) {
    const HydFmt d = hyd_fmt_describe(fmt);
    if (!d.device)
        return "Invalid Sample Format";
    if (src && d.layout == HYD_LAYOUT_PAIRS) {
        if (pixel_stride != 1 || (const char *)src[2] != (const char *)src[1] + d.bytes || (((size_t)src[0] | (size_t)src[1]) & (size_t)(d.bytes - 1)))
            return d.bytes == 2 ? HYD_FMT_P016_LAYOUT_MSG : HYD_FMT_NV12_LAYOUT_MSG;
    } else if (src && d.layout == HYD_LAYOUT_PLANES) {
        if (((size_t)src[0] | (size_t)src[1] | (size_t)src[2]) & (size_t)(d.bytes - 1))
            return HYD_FMT_PLANAR16_ALIGN_MSG;
    } else if (src && d.layout == HYD_LAYOUT_PACKED) {
        if (pixel_stride != 2 || hyd_fmt_packed_order(src, d.bytes) < 0)
            return d.bytes == 2 ? HYD_FMT_PACKED16_LAYOUT_MSG : HYD_FMT_PACKED_LAYOUT_MSG;
    } else if (src && d.layout == HYD_LAYOUT_DWORD) {
        if (pixel_stride != 1 || src[1] != src[0] || src[2] != src[0] || ((size_t)src[0] & 3u))
            return HYD_FMT_DWORD_LAYOUT_MSG;
    } else if (src && d.layout == HYD_LAYOUT_QUAD) {
        if (pixel_stride != 1 || src[1] != src[0] || src[2] != src[0] || ((size_t)src[0] & (size_t)(d.bytes - 1)))
            return HYD_FMT_QUAD_LAYOUT_MSG;
    } else if (src && d.layout == HYD_LAYOUT_UFLOAT) {
        if (pixel_stride != 1 || src[1] != src[0] || src[2] != src[0] || ((size_t)src[0] & 3u))
            return HYD_FMT_UFLOAT_LAYOUT_MSG;
    }
    if (d.layout == HYD_LAYOUT_PLANES) {
        const size_t pitch = pixel_stride < 0 ? (size_t)0 - (size_t)pixel_stride : (size_t)pixel_stride;
        if (pitch < (width + (size_t)d.sx) >> d.sx)
            return HYD_FMT_PLANAR_PITCH_MSG;
    }
    return NULL;
}

/* The three origin pointers of the sub-rectangle at pixel (x0, y0) of a picture of a device format — an LF group, a tile, a
 * shard's first row.  Strides are in samples.  YCbCr: Y at row y0, sample x0 of its plane; the chroma at row y0 >> sy of
 * theirs.  Pairs: the one chroma plane has the Y plane's pitch and two samples for every two columns, so sample x0 of the row.
 * A plane each: the pitch is pixel_stride, sample x0 >> sx.  Packed 4:2:2: all three pointers move by y0 rows and 2 x0 samples
 * (bytes, or 16-bit words), the group of pixel x0.  x0 must be even, and y0 where sy is 1 (every origin the library computes is a multiple of 256).
 * A dword a pixel (of 10-bit fields or of unsigned floats), and a group of four samples a pixel: all three pointers move by y0 rows
 * and x0 pixels (dwords, or qwords); any x0 and y0, since 4:4:4 has no parity to keep. */
static inline void hyd_fmt_origin(int fmt, const void *const src[3], ptrdiff_t row_stride, ptrdiff_t pixel_stride, size_t x0,
                                  size_t y0, const void *origin[3]) {
    const HydFmt d = hyd_fmt_describe(fmt);
    const int pairs = d.layout == HYD_LAYOUT_PAIRS;
    ptrdiff_t luma = (ptrdiff_t)y0 * row_stride + (ptrdiff_t)x0 * pixel_stride, chroma = luma;
    if (d.layout == HYD_LAYOUT_PACKED) {
        luma = chroma = (ptrdiff_t)y0 * row_stride + 2 * (ptrdiff_t)x0;
    } else if (d.layout == HYD_LAYOUT_DWORD || d.layout == HYD_LAYOUT_QUAD || d.layout == HYD_LAYOUT_UFLOAT) {
        luma = chroma = (ptrdiff_t)y0 * row_stride + (ptrdiff_t)x0;
    } else if (d.layout != HYD_LAYOUT_RGB) {
        luma = (ptrdiff_t)y0 * row_stride + (ptrdiff_t)x0;
        chroma = (ptrdiff_t)(y0 >> d.sy) * (pairs ? row_stride : pixel_stride) + (ptrdiff_t)(pairs ? x0 : x0 >> d.sx);
    }
    origin[0] = (const char *)src[0] + luma * d.bytes;
    origin[1] = (const char *)src[1] + chroma * d.bytes;
    origin[2] = (const char *)src[2] + chroma * d.bytes;
}

#endif /* HYD_SAMPLE_FMT_H_ */
