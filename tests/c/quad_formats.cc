/*
 * quad_formats.cc — the formats whose pixel is one group of four samples (AYUV, Y412, Y416) where host and device share their text
 * (csrc/hyd_sample_fmt.h, csrc/hip/hydk_store.h, csrc/hip/hydk_quad.h) as plain C++, no HIP header in sight, built by
 * tests/test_quad_formats.py with -fsanitize=address,undefined and held to tests/quad_model.py.  Each mode writes its results to OUT
 * as raw native-endian arrays:
 *
 *   quad_formats describe OUT LO HI  int32[HI - LO][18]: the twelve fields of hyd_fmt_describe in the struct's order, then of
 *                                    hydk_decode_fmt ok, the format encoded back (-1 where not ok), cls, storage, matrix and the
 *                                    storage form's variant
 *   quad_formats refusals OUT IN     IN: u32 cases, then per case i32 fmt, y, du, dv, pixel_stride, no_src, width — y, du, dv in
 *                                    BYTES: src = {base + y, base + y + du, base + y + dv}, base on a 16-byte boundary; OUT: per
 *                                    case 96 bytes, the message of hyd_fmt_refusal (all zero: NULL), or of src NULL
 *   quad_formats origins OUT IN      IN: u32 cases, then per case i32 fmt, row_stride (pixels), x0, y0; OUT: per case int64[3]: the
 *                                    BYTES hyd_fmt_origin adds to the three pointers
 *   quad_formats pixels OUT IN       IN: u32 cases, then per case u32 depth (0, 2, 3), matrix, w, h, pitch (pixels), flip and the
 *                                    surface, pitch * (h - 1) + w pixels of 4 (depth 0) or 8 bytes; OUT: per case h x w x 3 bytes
 *                                    (depth 0) or words, hydk_quad_pixel of every pixel.  flip: the rows are stored bottom-up and the
 *                                    pitch given to the definition is negative
 * Every surface is a malloc of exactly its pixels, ending with the last pixel of its last row: a read that leaves it meets the redzone.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/hydrium_amd.h"
#include "hyd_sample_fmt.h"
#include "hip/hydk_store.h"
#include "hip/hydk_quad.h"

static void die(const char *what) {
    std::fprintf(stderr, "quad_formats: %s\n", what);
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

static_assert(HYD_FMT_BASE_QUAD == 524288 && HYDAMD_AYUV_BT709 == 524296 && HYDAMD_AYUV_BT709_FULL == 524297 && HYDAMD_AYUV_BT601 == 524298 &&
                  HYDAMD_AYUV_BT601_FULL == 524299 && HYDAMD_Y412_BT709 == 524424 && HYDAMD_Y412_BT709_FULL == 524425 && HYDAMD_Y412_BT601 == 524426 &&
                  HYDAMD_Y412_BT601_FULL == 524427 && HYDAMD_Y416_BT709 == 524488 && HYDAMD_Y416_BT709_FULL == 524489 && HYDAMD_Y416_BT601 == 524490 &&
                  HYDAMD_Y416_BT601_FULL == 524491,
              "the public names are the rule's numbers");
static_assert(hyd_fmt_describe(HYDAMD_AYUV_BT601).layout == HYD_LAYOUT_QUAD && HYD_LAYOUT_QUAD == 5 && hyd_fmt_describe(HYDAMD_AYUV_BT709).bytes == 4 &&
                  hyd_fmt_describe(HYDAMD_Y412_BT709).bytes == 8 && hyd_fmt_describe(HYDAMD_Y412_BT709).bits == 12 && hyd_fmt_describe(HYDAMD_Y416_BT709).bits == 16 &&
                  !hyd_fmt_describe(524288).device && !hyd_fmt_describe(524360).device && !hyd_fmt_describe(524300).device && !hyd_fmt_describe(524492).device,
              "constexpr, as the kernels use it");
static_assert(HYDK_STORE_AYUV == 17 && HYDK_STORE_Y416 == 18 && HYDK_STORE_TABLE == 19 && HYDK_STORE_FORMS == 15 && HYDK_STORE_COUNT == 17 &&
                  HYDK_VARIANT_AYUV == 131072 && HYDK_VARIANT_Y416 == 262144,
              "the two storage forms, their variant bits, and the pinned constants where they were");
static_assert(sizeof(HydFmt) == 12 * sizeof(int), "HydFmt keeps its twelve fields");

static void describe(std::FILE *out, int lo, int hi) {
    for (int fmt = lo; fmt < hi; fmt++) {
        const HydFmt f = hyd_fmt_describe(fmt);
        const HydkSampleForm d = hydk_decode_fmt(fmt);
        const int32_t row[18] = {f.device, f.host, f.is_float, f.bytes, f.layout, f.matrix, f.filter, f.sub, f.sx, f.sy, f.depth, f.bits,
                                 d.ok, d.ok ? hydk_encode_fmt(d) : -1, d.cls, (int32_t)d.storage, (int32_t)d.matrix, hydk_store_form((int)d.storage).variant};
        put(out, row, sizeof(row));
        if (d.ok && f.layout == HYD_LAYOUT_QUAD) {
            const HydkStoreForm form = hydk_store_form((int)d.storage);
            if (form.cls != (f.depth ? HYDK_FMT_U16 : HYDK_FMT_U8) || form.ycbcr != 1 || form.chroma_planes != 0 || form.interp != 0 ||
                form.bits != (f.depth ? 16 : 8))
                die("hydk_decode_fmt: storage form");
            if (d.sub != (uint32_t)HYD_FMT_SUB_444 || d.filter != 0 || d.sx != 0 || d.sy != 0)
                die("hydk_decode_fmt: 4:4:4, nearest");
        }
    }
}

static void refusals(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const uint8_t *at = raw;
    const uint32_t cases = rd32(&at);
    alignas(16) static char buf[8192];
    for (uint32_t k = 0; k < cases; k++) {
        const int fmt = (int)rd32(&at), y = (int)rd32(&at), du = (int)rd32(&at), dv = (int)rd32(&at), ps = (int)rd32(&at), no_src = (int)rd32(&at),
                  width = (int)rd32(&at);
        if (y < -2048 || y > 2048 || du < -2000 || du > 2000 || dv < -2000 || dv > 2000)
            die("no such case");
        const void *const src[3] = {buf + 4096 + y, buf + 4096 + y + du, buf + 4096 + y + dv};
        const char *msg = hyd_fmt_refusal(fmt, no_src ? nullptr : src, ps, (size_t)width);
        char field[96] = {0};
        if (msg) {
            if (std::strlen(msg) >= sizeof(field))
                die("a message longer than its field");
            std::strcpy(field, msg);
        }
        put(out, field, sizeof(field));
    }
    if (at != raw + size)
        die("the input has bytes behind its last case");
    std::free(raw);
}

static void origins(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const uint8_t *at = raw;
    const uint32_t cases = rd32(&at);
    /* (addresses only: nothing is read through them) */
    uint64_t *picture = (uint64_t *)std::malloc((size_t)1 << 27);
    if (!picture)
        die("out of memory");
    for (uint32_t k = 0; k < cases; k++) {
        const int fmt = (int)rd32(&at), pitch = (int)rd32(&at), x0 = (int)rd32(&at), y0 = (int)rd32(&at);
        const uint64_t *base = picture + ((size_t)1 << 23);
        const void *const src[3] = {base, base, base};
        const void *origin[3];
        hyd_fmt_origin(fmt, src, pitch, 1, (size_t)x0, (size_t)y0, origin);
        if (hyd_fmt_refusal(fmt, origin, 1, 0))
            die("an origin that is no such picture");
        for (int c = 0; c < 3; c++) {
            const int64_t off = (const char *)origin[c] - (const char *)src[c];
            put(out, &off, sizeof(off));
        }
    }
    if (at != raw + size)
        die("the input has bytes behind its last case");
    std::free(picture);
    std::free(raw);
}

static void pixels(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const uint8_t *at = raw;
    const uint32_t cases = rd32(&at);
    for (uint32_t k = 0; k < cases; k++) {
        const uint32_t depth = rd32(&at), matrix = rd32(&at), w = rd32(&at), h = rd32(&at), pitch = rd32(&at), flip = rd32(&at);
        if ((depth != 0 && depth != 2 && depth != 3) || matrix > 3u || pitch < w || !w || !h)
            die("no such case");
        const size_t dpp = depth ? 2 : 1; /* dwords a pixel */
        const size_t dwords = ((size_t)pitch * (h - 1) + w) * dpp;
        uint32_t *surface = (uint32_t *)std::malloc(4 * dwords); /* exactly the surface: it ends with the last pixel of its last row */
        if (!surface)
            die("out of memory");
        std::memcpy(surface, at, 4 * dwords);
        at += 4 * dwords;
        const uint32_t *first = flip ? surface + (size_t)pitch * (h - 1) * dpp : surface;
        const size_t sample = depth ? 2 : 1;
        uint8_t *rgb = (uint8_t *)std::malloc((size_t)w * h * 3 * sample);
        if (!rgb)
            die("out of memory");
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                uint32_t px[3];
                hydk_quad_pixel((int)depth, (int)matrix, first, flip ? -(long long)pitch : (long long)pitch, (int32_t)x, (int32_t)y, px);
                for (int c = 0; c < 3; c++) {
                    if (px[c] > (depth ? 65535u : 255u))
                        die("a result that is no sample of its class");
                    const size_t i = ((size_t)y * w + x) * 3 + c;
                    if (depth) {
                        const uint16_t s = (uint16_t)px[c];
                        std::memcpy(rgb + 2 * i, &s, 2);
                    } else
                        rgb[i] = (uint8_t)px[c];
                }
            }
        put(out, rgb, (size_t)w * h * 3 * sample);
        std::free(rgb);
        std::free(surface);
    }
    if (at != raw + size)
        die("the input has bytes behind its last case");
    std::free(raw);
}

int main(int argc, char **argv) {
    if (argc < 3)
        die("usage: quad_formats MODE OUT [ARGUMENTS]");
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out)
        die("cannot open the output");
    if (!std::strcmp(argv[1], "describe") && argc == 5)
        describe(out, std::atoi(argv[3]), std::atoi(argv[4]));
    else if (!std::strcmp(argv[1], "refusals") && argc == 4)
        refusals(out, argv[3]);
    else if (!std::strcmp(argv[1], "origins") && argc == 4)
        origins(out, argv[3]);
    else if (!std::strcmp(argv[1], "pixels") && argc == 4)
        pixels(out, argv[3]);
    else
        die("no such mode");
    if (std::fclose(out))
        die("cannot write");
    return 0;
}
