/*
 * planar16_formats.cc — the planar YCbCr family of 16-bit words (2112 ...) of csrc/hyd_sample_fmt.h, the storage-form table of
 * csrc/hip/hydk_store.h and the per-pixel definition of csrc/hip/hydk_yuvp16.h as plain C++, no HIP header in sight, built by
 * tests/test_planar16_formats.py with -fsanitize=address,undefined and held to the numpy model (tests/planar16_model.py).  Each
 * mode writes its results to OUT as raw native-endian arrays:
 *
 *   planar16_formats geometry OUT   int64[3 subsamplings][4 sign pairs][3] origin offsets IN BYTES; then int32[2 widths][3 subsamplings]
 *                                   [3 pitches][2 signs] of the pitch rule; then int32[8] of the alignment check, the three planes 0
 *                                   or 1 byte off (bit c of the index: plane c).  What the numbers mean: sample_formats.cc's dump
 *   planar16_formats planes OUT IN  IN: u32 cases, then per case u32 subsampling, filter, depth, matrix, w, h and the Y, U and V
 *                                   planes as 16-bit words; OUT: per case h x w x 3 words
 * Every plane is a malloc of exactly its samples: a tap that leaves the plane meets the redzone.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/hydrium_amd.h"
#include "hyd_sample_fmt.h"
#include "hip/hydk_store.h"
#include "hip/hydk_yuvp16.h"

static void die(const char *what) {
    std::fprintf(stderr, "planar16_formats: %s\n", what);
    std::exit(2);
}

static void put(std::FILE *f, const void *p, size_t n) {
    if (n && std::fwrite(p, 1, n, f) != n)
        die("cannot write");
}

static uint8_t *slurp(const char *path, size_t *size) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f)
        die("cannot open the input");
    std::fseek(f, 0, SEEK_END);
    *size = (size_t)std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    uint8_t *p = (uint8_t *)std::malloc(*size ? *size : 1);
    if (!p || std::fread(p, 1, *size, f) != *size)
        die("cannot read the input");
    std::fclose(f);
    return p;
}

static uint32_t rd32(const uint8_t **p) {
    uint32_t v;
    std::memcpy(&v, *p, 4);
    *p += 4;
    return v;
}

static int pitch_ok(int fmt, ptrdiff_t pitch, size_t width) { return hyd_fmt_refusal(fmt, nullptr, pitch, width) == nullptr; }
static int layout_ok(int fmt, const void *const src[3], ptrdiff_t pixel_stride) { return hyd_fmt_refusal(fmt, src, pixel_stride, 0) == nullptr; }

static void geometry(std::FILE *out) {
    /* origins of the sub-rectangle at (256, 512) of a picture with Y pitch +-1024 and chroma pitch +-520 words: offsets in bytes
     * from the three plane pointers, which sit in allocations of their own */
    const size_t x0 = 256, y0 = 512;
    char *planes[3];
    for (int c = 0; c < 3; c++)
        if (!(planes[c] = (char *)std::malloc(64)))
            die("out of memory");
    const int some[3] = {HYDAMD_I010C_BT601_FULL, HYDAMD_I212L_BT709, HYDAMD_I416_BT601};
    for (int k = 0; k < 3; k++)
        for (int ysign = 1; ysign >= -1; ysign -= 2)
            for (int csign = 1; csign >= -1; csign -= 2) {
                const void *const src[3] = {planes[0], planes[1], planes[2]};
                const void *origin[3];
                hyd_fmt_origin(some[k], src, ysign * 1024, csign * 520, x0, y0, origin);
                for (int c = 0; c < 3; c++) {
                    const int64_t off = (int64_t)((intptr_t)origin[c] - (intptr_t)src[c]);
                    put(out, &off, sizeof(off));
                }
            }
    /* the pitch rule around cw, for an odd and an even width */
    const size_t widths[2] = {199, 200};
    for (int i = 0; i < 2; i++)
        for (int k = 0; k < 3; k++) {
            const ptrdiff_t cw = (ptrdiff_t)(hyd_fmt_describe(some[k]).sub == HYD_FMT_SUB_444 ? widths[i] : (widths[i] + 1) / 2);
            for (ptrdiff_t pitch = cw - 1; pitch <= cw + 1; pitch++)
                for (int sign = 1; sign >= -1; sign -= 2) {
                    const int32_t ok = pitch_ok(some[k], sign * pitch, widths[i]);
                    put(out, &ok, sizeof(ok));
                }
            if (pitch_ok(some[k], 1, widths[i]) || pitch_ok(some[k], 0, widths[i]))
                die("the pitch rule refuses the pixel strides 0 and 1");
        }
    /* the alignment check: every plane on a 2-byte boundary, whatever the pixel stride says */
    for (int k = 0; k < 8; k++) {
        const void *const src[3] = {planes[0] + (k & 1), planes[1] + ((k >> 1) & 1), planes[2] + ((k >> 2) & 1)};
        const int32_t ok = layout_ok(some[k % 3], src, 520) && layout_ok(some[k % 3], src, 1);
        put(out, &ok, sizeof(ok));
        const char *said = hyd_fmt_refusal(some[k % 3], src, 520, 0);
        if ((said && std::strcmp(said, HYD_FMT_PLANAR16_ALIGN_MSG)) || !layout_ok(HYDAMD_I420_BT709, src, 520))
            die("the alignment message is the family's own, and the 8-bit planes have no alignment to hold");
    }
    for (int c = 0; c < 3; c++)
        std::free(planes[c]);
}

/* a malloc of exactly n words holding src's rows in the order given (flip: bottom-up) */
static uint16_t *plane_of(const uint8_t *src, int32_t w, int32_t h, bool flip) {
    uint16_t *p = (uint16_t *)std::malloc((size_t)w * (size_t)h * 2);
    if (!p)
        die("out of memory");
    for (int32_t r = 0; r < h; r++)
        std::memcpy(p + (size_t)(flip ? h - 1 - r : r) * (size_t)w, src + (size_t)r * (size_t)w * 2, (size_t)w * 2);
    return p;
}

static void planes(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const uint8_t *at = raw;
    const uint32_t cases = rd32(&at);
    for (uint32_t k = 0; k < cases; k++) {
        const int sub = (int)rd32(&at), filter = (int)rd32(&at), depth = (int)rd32(&at), matrix = (int)rd32(&at);
        const int32_t w = (int32_t)rd32(&at), h = (int32_t)rd32(&at);
        const int32_t cw = (w + hydk_planar_sx(sub)) >> hydk_planar_sx(sub), ch = (h + hydk_planar_sy(sub)) >> hydk_planar_sy(sub);
        uint16_t *down[3], *up[3];
        const int32_t pw[3] = {w, cw, cw}, ph[3] = {h, ch, ch};
        for (int c = 0; c < 3; c++) {
            down[c] = plane_of(at, pw[c], ph[c], false);
            up[c] = plane_of(at, pw[c], ph[c], true);
            at += (size_t)pw[c] * (size_t)ph[c] * 2;
        }
        uint16_t *row = (uint16_t *)std::malloc((size_t)w * 6);
        if (!row)
            die("out of memory");
        for (int32_t y = 0; y < h; y++) {
            for (int32_t x = 0; x < w; x++) {
                uint32_t a[3], b[3];
                hydk_planar16_pixel(sub, filter, depth, matrix, down[0], w, down[1], down[2], cw, cw, ch, x, y, a);
                /* under negative pitches: the same pixel */
                hydk_planar16_pixel(sub, filter, depth, matrix, up[0] + (size_t)(h - 1) * (size_t)w, -(long long)w,
                                    up[1] + (size_t)(ch - 1) * (size_t)cw, up[2] + (size_t)(ch - 1) * (size_t)cw, -(long long)cw, cw, ch, x, y, b);
                if (a[0] != b[0] || a[1] != b[1] || a[2] != b[2])
                    die("negative pitches give another pixel");
                for (int c = 0; c < 3; c++)
                    row[3 * x + c] = (uint16_t)a[c];
            }
            put(out, row, (size_t)w * 6);
        }
        std::free(row);
        for (int c = 0; c < 3; c++) {
            std::free(down[c]);
            std::free(up[c]);
        }
    }
    if (at != raw + size)
        die("the input has bytes behind its last case");
    std::free(raw);
}

int main(int argc, char **argv) {
    if (argc < 3)
        die("usage: planar16_formats MODE OUT [ARGUMENT]");
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out)
        die("cannot open the output");
    if (!std::strcmp(argv[1], "geometry") && argc == 3)
        geometry(out);
    else if (!std::strcmp(argv[1], "planes") && argc == 4)
        planes(out, argv[3]);
    else
        die("no such mode");
    if (std::fclose(out))
        die("cannot write");
    return 0;
}
