/*
 * planar_formats.cc — the planar YCbCr family (512 ...) of csrc/hyd_sample_fmt.h and the per-pixel definition of
 * csrc/hip/hydk_chroma.h as plain C++, no HIP header in sight, built by tests/test_planar_formats.py with
 * -fsanitize=address,undefined and held to the numpy model (tests/planar_model.py).  Each mode writes its results to OUT as
 * raw native-endian arrays:
 *
 *   planar_formats geometry OUT     int64[3 subsamplings][2 chroma pitches][3] origin offsets; then int32[2 widths][3 subsamplings]
 *                                   [3 pitches][2 signs] of the pitch rule (what the numbers mean: sample_formats.cc's dump)
 *   planar_formats planes OUT IN    IN: u32 cases, then per case u32 subsampling, filter, w, h and ONE chroma plane of ch x cw
 *                                   bytes; OUT: per case h x w bytes
 * Every chroma plane is a malloc of exactly its samples: a tap that leaves the plane meets the redzone.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/hydrium_amd.h"
#include "hyd_sample_fmt.h"
#include "hip/hydk_chroma.h"

static void die(const char *what) {
    std::fprintf(stderr, "planar_formats: %s\n", what);
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

static void geometry(std::FILE *out) {
    /* origins of the sub-rectangle at (256, 512) of a picture with Y pitch 1024 and chroma pitch 520, then -520: offsets from
     * the three plane pointers, which sit in allocations of their own */
    const size_t x0 = 256, y0 = 512;
    char *planes[3];
    for (int c = 0; c < 3; c++)
        if (!(planes[c] = (char *)std::malloc(64)))
            die("out of memory");
    const int some[3] = {HYDAMD_I420C_BT601_FULL, HYDAMD_I422L_BT709, HYDAMD_I444_BT601};
    for (int k = 0; k < 3; k++)
        for (int sign = 1; sign >= -1; sign -= 2) {
            const void *const src[3] = {planes[0], planes[1], planes[2]};
            const void *origin[3];
            hyd_fmt_origin(some[k], src, 1024, sign * 520, x0, y0, origin);
            if (hyd_fmt_refusal(some[k], src, sign * 520, 0) || hyd_fmt_refusal(some[k], src, 1, 0))
                die("hyd_fmt_refusal has no layout to hold a planar picture to");
            for (int c = 0; c < 3; c++) {
                const int64_t off = (int64_t)((intptr_t)origin[c] - (intptr_t)src[c]);
                put(out, &off, sizeof(off));
            }
        }
    for (int c = 0; c < 3; c++)
        std::free(planes[c]);
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
            if (!pitch_ok(HYD_FMT_UINT8, 1, widths[i]) || !pitch_ok(HYDAMD_NV12C_BT709, 1, widths[i]) || !pitch_ok(HYDAMD_P010_BT709, 1, widths[i]) ||
                pitch_ok(some[k], 1, widths[i]) || pitch_ok(some[k], 0, widths[i]))
                die("the pitch rule holds the planar families alone, and refuses them the pixel strides 0 and 1");
        }
}

static void planes(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const uint8_t *at = raw;
    const uint32_t cases = rd32(&at);
    for (uint32_t k = 0; k < cases; k++) {
        const int sub = (int)rd32(&at), filter = (int)rd32(&at);
        const int32_t w = (int32_t)rd32(&at), h = (int32_t)rd32(&at);
        const int32_t cw = (w + hydk_planar_sx(sub)) >> hydk_planar_sx(sub), ch = (h + hydk_planar_sy(sub)) >> hydk_planar_sy(sub);
        const size_t bytes = (size_t)cw * (size_t)ch;
        uint8_t *plane = (uint8_t *)std::malloc(bytes); /* exactly the plane */
        uint8_t *flipped = (uint8_t *)std::malloc(bytes); /* the same plane stored bottom-up */
        uint8_t *row = (uint8_t *)std::malloc((size_t)w);
        if (!plane || !flipped || !row)
            die("out of memory");
        std::memcpy(plane, at, bytes);
        at += bytes;
        for (int32_t r = 0; r < ch; r++)
            std::memcpy(flipped + (size_t)(ch - 1 - r) * (size_t)cw, plane + (size_t)r * (size_t)cw, (size_t)cw);
        for (int32_t y = 0; y < h; y++) {
            for (int32_t x = 0; x < w; x++) {
                const uint32_t down = hydk_planar_sample(sub, filter, plane, cw, cw, ch, x, y);
                /* under a negative pitch: the same sample */
                if (hydk_planar_sample(sub, filter, flipped + (size_t)(ch - 1) * (size_t)cw, -(long long)cw, cw, ch, x, y) != down)
                    die("a negative pitch gives another sample");
                row[x] = (uint8_t)down;
            }
            put(out, row, (size_t)w);
        }
        std::free(row);
        std::free(flipped);
        std::free(plane);
    }
    if (at != raw + size)
        die("the input has bytes behind its last case");
    std::free(raw);
}

int main(int argc, char **argv) {
    if (argc < 3)
        die("usage: planar_formats MODE OUT [ARGUMENT]");
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
