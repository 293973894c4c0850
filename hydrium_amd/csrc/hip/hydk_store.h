/*
 * hydk_store.h — the storage forms of an LF group's pixels, in one table: what HydkLfJob.storage names, what each form is made
 * of, and the two directions between a public sample format (hyd_sample_fmt.h) and a job's fields.  Plain C / C++ for host and
 * device, no HIP needed; in C++ hydk_store_form is constexpr, so a kernel derives its compile-time switches from the table.
 */
#ifndef HYD_STORE_FORMS_H_
#define HYD_STORE_FORMS_H_

#include <stdint.h>

#include "../hyd_sample_fmt.h"

#ifdef __cplusplus
#define HYDK_STORE_FN constexpr static inline
#else
#define HYDK_STORE_FN static inline
#endif

/* sample CLASSES: what a job's fmt and the transform kernel's FMT name.  fmt == HYDK_FMT_F32 means "float class" everywhere */
#define HYDK_FMT_U8 0
#define HYDK_FMT_U16 1
#define HYDK_FMT_F32 2

/* storage forms (HydkLfJob.storage).  0 is what a zeroed job says: the class's own samples — RGB of 8 or 16 bits, float32 */
#define HYDK_STORE_F32 0
#define HYDK_STORE_F16 1   /* float class: 2-byte samples, widened exactly on load (hydk_half.h) */
#define HYDK_STORE_BF16 2
#define HYDK_STORE_NV12 3  /* 8-bit class: a Y plane and a half-resolution plane of U, V pairs, nearest chroma (hydk_yuv.h) */
#define HYDK_STORE_NV12I 4 /* the same picture, chroma interpolated under HydkLfJob.filter (hydk_chroma.h) */
#define HYDK_STORE_P016 5  /* 16-bit class: P010 / P012 / P016, NV12's two planes in 16-bit words (hydk_yuv16.h) */
#define HYDK_STORE_P016I 6
#define HYDK_STORE_YUVP 7  /* 8-bit class: planar YCbCr — src[1], src[2] the U and V planes (pitch pixel_stride), HydkLfJob.sub the subsampling */
#define HYDK_STORE_YUVPI 8
#define HYDK_STORE_YUVP16 9  /* 16-bit class: the same three planes in 16-bit words of 10, 12 or 16 bits, LSB-aligned (hydk_yuvp16.h) */
#define HYDK_STORE_YUVP16I 10
#define HYDK_STORE_YUY2 11  /* 8-bit class: packed 4:2:2 — Y, U and V bytes in one plane, HydkLfJob.sub the byte order (HYD_PACKED_*; hydk_yuy2.h) */
#define HYDK_STORE_YUY2I 12
#define HYDK_STORE_Y216 13  /* 16-bit class: the same groups in 16-bit words, MSB-aligned — Y210 / Y212 / Y216, HydkLfJob.sub the word order (hydk_y216.h) */
#define HYDK_STORE_Y216I 14
#define HYDK_STORE_FORMS 15 /* the forms of ADDRESSABLE samples — floats, bytes, words — end here, as they have since Y216: what pointers and strides can spell */
#define HYDK_STORE_RGB10 15 /* 16-bit class: a pixel is one dword of three 10-bit fields, RGB — HydkLfJob.sub the field order, 0 R low, 1 B low (hydk_rgb10.h) */
#define HYDK_STORE_Y410 16  /* 16-bit class: the same dword holding U, Y, V — 4:4:4, nearest by nature, depth P010 */
#define HYDK_STORE_COUNT 17 /* (what "all of them" came to with the dword forms; pinned since, as HYDK_STORE_FORMS is) */
#define HYDK_STORE_AYUV 17  /* 8-bit class: a pixel is one dword of the bytes V, U, Y and an ignored fourth — 4:4:4, nearest by nature (hydk_quad.h) */
#define HYDK_STORE_Y416 18  /* 16-bit class: a pixel is one qword of the words U, Y, V and an ignored fourth, MSB-aligned — Y412 / Y416, the depth in matrix as P01x's */
#define HYDK_STORE_TABLE 19 /* (what "all of them" came to with the groups of four; pinned since, as the two before it are) */
#define HYDK_STORE_R11G11B10F 19 /* float class: a pixel is one dword of three unsigned floats of 11, 11 and 10 bits, widened exactly on load (hydk_ufloat.h) */
#define HYDK_STORE_RGB9E5 20     /* float class: a pixel is one dword of three 9-bit mantissas and their shared 5-bit exponent */
#define HYDK_STORE_SIZE 21  /* all of them: the table's size and the bits of launch_transform's mask above the two integer classes'; no test
                             * holds it to a value, so the next form grows it */

/* HydkLfJob.use_luts of a YCbCr job is the XYB mode + its form's variant bit: the RGB instances' own test turns it away */
#define HYDK_VARIANT_NV12 8
#define HYDK_VARIANT_NV12I 16
#define HYDK_VARIANT_P016 32
#define HYDK_VARIANT_P016I 64
#define HYDK_VARIANT_YUVP 128
#define HYDK_VARIANT_YUVPI 256
#define HYDK_VARIANT_YUVP16 512
#define HYDK_VARIANT_YUVP16I 1024
#define HYDK_VARIANT_YUY2 2048
#define HYDK_VARIANT_YUY2I 4096
#define HYDK_VARIANT_Y216 8192
#define HYDK_VARIANT_Y216I 16384
#define HYDK_VARIANT_RGB10 32768
#define HYDK_VARIANT_Y410 65536
#define HYDK_VARIANT_AYUV 131072
#define HYDK_VARIANT_Y416 262144

typedef struct HydkStoreForm {
    int cls;           /* HYDK_FMT_*; form 0 belongs to every class */
    int ycbcr;         /* a pixel is converted to RGB of its class right after the load */
    int bits;          /* of a stored sample */
    int chroma_planes; /* YCbCr: 1 — (U, V) pairs interleaved in one plane; 2 — a plane each; 0 — none: U and V sit among the Y samples */
    int interp;        /* chroma interpolated: the job carries filter and the picture (pic_*) */
    int variant;       /* HYDK_VARIANT_* */
} HydkStoreForm;

HYDK_STORE_FN HydkStoreForm hydk_store_form(int storage) {
    const HydkStoreForm forms[HYDK_STORE_SIZE] = {
        {HYDK_FMT_F32, 0, 32, 0, 0, 0},
        {HYDK_FMT_F32, 0, 16, 0, 0, 0},
        {HYDK_FMT_F32, 0, 16, 0, 0, 0},
        {HYDK_FMT_U8, 1, 8, 1, 0, HYDK_VARIANT_NV12},
        {HYDK_FMT_U8, 1, 8, 1, 1, HYDK_VARIANT_NV12I},
        {HYDK_FMT_U16, 1, 16, 1, 0, HYDK_VARIANT_P016},
        {HYDK_FMT_U16, 1, 16, 1, 1, HYDK_VARIANT_P016I},
        {HYDK_FMT_U8, 1, 8, 2, 0, HYDK_VARIANT_YUVP},
        {HYDK_FMT_U8, 1, 8, 2, 1, HYDK_VARIANT_YUVPI},
        {HYDK_FMT_U16, 1, 16, 2, 0, HYDK_VARIANT_YUVP16},
        {HYDK_FMT_U16, 1, 16, 2, 1, HYDK_VARIANT_YUVP16I},
        {HYDK_FMT_U8, 1, 8, 0, 0, HYDK_VARIANT_YUY2},
        {HYDK_FMT_U8, 1, 8, 0, 1, HYDK_VARIANT_YUY2I},
        {HYDK_FMT_U16, 1, 16, 0, 0, HYDK_VARIANT_Y216},
        {HYDK_FMT_U16, 1, 16, 0, 1, HYDK_VARIANT_Y216I},
        {HYDK_FMT_U16, 0, 10, 0, 0, HYDK_VARIANT_RGB10},
        {HYDK_FMT_U16, 1, 10, 0, 0, HYDK_VARIANT_Y410},
        {HYDK_FMT_U8, 1, 8, 0, 0, HYDK_VARIANT_AYUV},
        {HYDK_FMT_U16, 1, 16, 0, 0, HYDK_VARIANT_Y416},
        {HYDK_FMT_F32, 0, 11, 0, 0, 0},
        {HYDK_FMT_F32, 0, 9, 0, 0, 0},
    };
    return forms[storage >= 0 && storage < HYDK_STORE_SIZE ? storage : 0];
}

/* A public sample format taken apart into what a job holds.  ok: a device entry point takes it (else every field is 0).
 * matrix: HYDK_YUV_* (0 ... 3), + 4 * depth (HYDK_YUV16_P01x) for the 16-bit forms; filter: HYDK_CHROMA_*; sub: HYDK_PLANAR_*
 * (packed 4:2:2: HYDK_PLANAR_422 here; a recorded job's sub holds the byte order instead, which the public number does not name;
 * HYDK_STORE_RGB10: the field order, which the number does name);
 * sx, sy: log2 of the pixels one chroma sample spans across and down. */
typedef struct HydkSampleForm {
    int ok, cls;
    uint32_t storage, matrix, filter, sub;
    int sx, sy;
} HydkSampleForm;

static inline HydkSampleForm hydk_decode_fmt(int f) {
    const HydFmt fmt = hyd_fmt_describe(f);
    HydkSampleForm d = {fmt.device, 0, 0, (uint32_t)(fmt.matrix + 4 * fmt.depth), (uint32_t)fmt.filter, (uint32_t)fmt.sub, fmt.sx, fmt.sy};
    if (fmt.layout == HYD_LAYOUT_UFLOAT)
        d.storage = (uint32_t)(HYDK_STORE_R11G11B10F + (f - HYD_FMT_BASE_UFLOAT));
    else if (fmt.layout == HYD_LAYOUT_QUAD)
        d.storage = (uint32_t)(fmt.depth ? HYDK_STORE_Y416 : HYDK_STORE_AYUV);
    else if (fmt.layout == HYD_LAYOUT_DWORD) {
        d.storage = (uint32_t)(fmt.depth ? HYDK_STORE_Y410 : HYDK_STORE_RGB10);
        if (!fmt.depth)
            d.sub = (uint32_t)(f - HYD_FMT_BASE_DWORD);
    } else if (fmt.layout == HYD_LAYOUT_PACKED)
        d.storage = (uint32_t)((fmt.bytes == 2 ? HYDK_STORE_Y216 : HYDK_STORE_YUY2) + (fmt.filter != 0));
    else if (fmt.layout != HYD_LAYOUT_RGB) /* the YCbCr forms in the table's order: pairs then planes, bytes then words, nearest then interpolated */
        d.storage = (uint32_t)(HYDK_STORE_NV12 + 4 * (fmt.layout == HYD_LAYOUT_PLANES) + 2 * (fmt.bytes == 2) + (fmt.filter != 0));
    else if (f == HYD_FMT_FLOAT16 || f == HYD_FMT_BFLOAT16)
        d.storage = (uint32_t)(f == HYD_FMT_FLOAT16 ? HYDK_STORE_F16 : HYDK_STORE_BF16);
    d.cls = d.storage > HYDK_STORE_F32 ? hydk_store_form((int)d.storage).cls : fmt.device ? f : 0;
    return d;
}

/* and back: the public format of a job's cls (fmt), storage, matrix, filter and sub */
static inline int hydk_encode_fmt(HydkSampleForm d) {
    const HydkStoreForm form = hydk_store_form((int)d.storage);
    if (d.storage == HYDK_STORE_R11G11B10F || d.storage == HYDK_STORE_RGB9E5)
        return HYD_FMT_BASE_UFLOAT + (int)(d.storage - HYDK_STORE_R11G11B10F);
    if (d.storage == HYDK_STORE_RGB10)
        return HYD_FMT_BASE_DWORD + (int)(d.sub & 1u);
    if (d.storage == HYDK_STORE_Y410)
        return HYD_FMT_BASE_DWORD + (int)(d.matrix & 3u) + 4 * HYD_FMT_SUB_444 + 64 * (int)(d.matrix >> 2);
    if (d.storage == HYDK_STORE_AYUV || d.storage == HYDK_STORE_Y416) /* (AYUV's matrix holds no depth: 0) */
        return HYD_FMT_BASE_QUAD + (int)(d.matrix & 3u) + 4 * HYD_FMT_SUB_444 + 64 * (int)(d.matrix >> 2);
    if (!form.ycbcr)
        return d.storage == HYDK_STORE_F16 ? HYD_FMT_FLOAT16 : d.storage == HYDK_STORE_BF16 ? HYD_FMT_BFLOAT16 : d.cls;
    if (form.chroma_planes == 0) /* (sub: the byte order in a job, 4:2:2 in a decoded format; neither is in the number) */
        return form.bits == 16 ? HYD_FMT_BASE_PACKED16 + (int)(d.matrix & 3u) + 16 * (int)d.filter + 64 * (int)(d.matrix >> 2)
                               : HYD_FMT_BASE_PACKED + (int)(d.matrix & 3u) + 16 * (int)d.filter;
    const int base = form.chroma_planes == 1 ? HYD_FMT_BASE_PAIRS : form.bits == 16 ? HYD_FMT_BASE_PLANES16 : HYD_FMT_BASE_PLANES;
    return base + (int)(d.matrix & 3u) + 4 * (int)d.sub + 16 * (int)d.filter + 64 * (int)(d.matrix >> 2);
}

#endif /* HYD_STORE_FORMS_H_ */
