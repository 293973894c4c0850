/*
 * packed16_formats.cc — the packed 4:2:2 formats of 16-bit words (Y210 / Y212 / Y216) where host and device share their text
 * (csrc/hyd_sample_fmt.h, csrc/hip/hydk_store.h, csrc/hip/hydk_y216.h) as plain C++, no HIP header in sight, built by
 * tests/test_packed16_formats.py with -fsanitize=address,undefined and held to tests/packed16_model.py.  Each mode writes its results
 * to OUT as raw native-endian arrays:
 *
 *   packed16_formats describe OUT LO HI  int32[HI - LO][18]: the twelve fields of hyd_fmt_describe in the struct's order, then of
 *                                        hydk_decode_fmt ok, the format encoded back (-1 where not ok), cls, storage, matrix and the
 *                                        storage form's variant
 *   packed16_formats refusals OUT IN     IN: u32 cases, then per case i32 fmt, y, du, dv, pixel_stride, no_src, width — y, du, dv in
 *                                        BYTES: src = {base + y, base + y + du, base + y + dv}, base on an 8-byte boundary; OUT: per
 *                                        case 96 bytes, the message of hyd_fmt_refusal (all zero: NULL), or of src NULL
 *   packed16_formats origins OUT IN      IN: u32 cases, then per case i32 fmt, du, dv (words), row_stride (words), x0, y0; OUT: per
 *                                        case int64[4]: the BYTES hyd_fmt_origin adds to the three pointers, then the word order
 *                                        they still spell
 *   packed16_formats pixels OUT IN       IN: u32 cases, then per case u32 order, filter, depth, matrix, w, h, pitch (words), flip and
 *                                        the surface, pitch * (h - 1) + 4 * ceil(w / 2) words; OUT: per case h x w x 3 words,
 *                                        hydk_y216_pixel of every pixel.  flip: the rows are stored bottom-up and the pitch given to
 *                                        the definition is negative
 * Every surface is a malloc of exactly its words, ending with the last group of its last row: a read that leaves it meets the redzone.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/hydrium_amd.h"
#include "hyd_sample_fmt.h"
#include "hip/hydk_store.h"
#include "hip/hydk_y216.h"

static void die(const char *what) {
    std::fprintf(stderr, "packed16_formats: %s\n", what);
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

static_assert(HYDAMD_Y210_BT709 == HYD_FMT_BASE_PACKED16 + 64 && HYDAMD_Y210_BT709 == 32832 && HYDAMD_Y212_BT709 == 32896 && HYDAMD_Y216_BT709 == 32960 &&
                  HYDAMD_Y210L_BT601 == 32866 && HYDAMD_Y212C_BT709_FULL == 32913 && HYDAMD_Y216L_BT601_FULL == 32995,
              "the public names are the rule's numbers");
static_assert(hyd_fmt_describe(HYDAMD_Y210L_BT709).layout == HYD_LAYOUT_PACKED && hyd_fmt_describe(HYDAMD_Y212_BT709).bits == 12 &&
                  !hyd_fmt_describe(32768).device && !hyd_fmt_describe(32836).device,
              "constexpr, as the kernels use it");
static_assert(HYDK_STORE_Y216 == 13 && HYDK_STORE_Y216I == 14 && HYDK_STORE_FORMS == 15 && HYDK_VARIANT_Y216 == 8192 && HYDK_VARIANT_Y216I == 16384,
              "the two storage forms and their variant bits");

static void describe(std::FILE *out, int lo, int hi) {
    for (int fmt = lo; fmt < hi; fmt++) {
        const HydFmt f = hyd_fmt_describe(fmt);
        const HydkSampleForm d = hydk_decode_fmt(fmt);
        const int32_t row[18] = {f.device, f.host, f.is_float, f.bytes, f.layout, f.matrix, f.filter, f.sub, f.sx, f.sy, f.depth, f.bits,
                                 d.ok, d.ok ? hydk_encode_fmt(d) : -1, d.cls, (int32_t)d.storage, (int32_t)d.matrix, hydk_store_form((int)d.storage).variant};
        put(out, row, sizeof(row));
        if (d.ok && f.layout == HYD_LAYOUT_PACKED) { /* a recorded job holds the order in sub: whichever it is, the number comes back */
            for (uint32_t order = 0; order < 4; order++) {
                HydkSampleForm j = d;
                j.sub = order;
                if (hydk_encode_fmt(j) != fmt)
                    die("a job's word order changes the format it encodes back to");
            }
            const HydkStoreForm form = hydk_store_form((int)d.storage);
            if (!form.ycbcr || form.chroma_planes != 0 || form.bits != 8 * f.bytes || form.cls != f.bytes - 1 || form.interp != (f.filter != 0))
                die("hydk_decode_fmt: storage form");
        }
    }
}

static void refusals(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const uint8_t *at = raw;
    const uint32_t cases = rd32(&at);
    alignas(8) static char buf[8192];
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
    uint16_t *picture = (uint16_t *)std::malloc((size_t)1 << 25);
    if (!picture)
        die("out of memory");
    for (uint32_t k = 0; k < cases; k++) {
        const int fmt = (int)rd32(&at), du = (int)rd32(&at), dv = (int)rd32(&at), pitch = (int)rd32(&at), x0 = (int)rd32(&at), y0 = (int)rd32(&at);
        const uint16_t *base = picture + ((size_t)1 << 23);
        const void *const src[3] = {base, base + du, base + dv};
        const void *origin[3];
        hyd_fmt_origin(fmt, src, pitch, 2, (size_t)x0, (size_t)y0, origin);
        for (int c = 0; c < 3; c++) {
            const int64_t off = (const char *)origin[c] - (const char *)src[c];
            put(out, &off, sizeof(off));
        }
        const int64_t order = hyd_fmt_packed_order(origin, 2) == hyd_fmt_packed_order(src, 2) ? hyd_fmt_packed_order(origin, 2) : -2;
        put(out, &order, sizeof(order));
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
        const uint32_t order = rd32(&at), filter = rd32(&at), depth = rd32(&at), matrix = rd32(&at), w = rd32(&at), h = rd32(&at), pitch = rd32(&at),
                       flip = rd32(&at);
        const size_t row = 4 * (size_t)((w + 1) / 2), words = (size_t)pitch * (h - 1) + row;
        if (order > 3 || pitch < row || !w || !h)
            die("no such case");
        uint16_t *surface = (uint16_t *)std::malloc(2 * words); /* exactly the surface: it ends with the last group of its last row */
        if (!surface)
            die("out of memory");
        std::memcpy(surface, at, 2 * words);
        at += 2 * words;
        /* the three pointers a caller of that word order gives, at the picture's row 0 */
        const uint16_t *first = flip ? surface + (size_t)pitch * (h - 1) : surface;
        const int yo = hydk_yuy2_y_offset((int)order), c0 = 1 - yo, c1 = 3 - yo;
        const void *const src[3] = {first + yo, first + (hydk_yuy2_v_first((int)order) ? c1 : c0), first + (hydk_yuy2_v_first((int)order) ? c0 : c1)};
        if (hyd_fmt_packed_order(src, 2) != (int)order)
            die("hyd_fmt_packed_order does not read the order back off the pointers");
        if (hyd_fmt_packed_order(src, 1) >= 0)
            die("hyd_fmt_packed_order takes a group of words for a group of bytes");
        uint16_t *rgb = (uint16_t *)std::malloc((size_t)w * h * 6);
        if (!rgb)
            die("out of memory");
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                uint32_t px[3];
                hydk_y216_pixel((int)filter, (int)depth, (int)matrix, (const uint16_t *)src[0], (const uint16_t *)src[1], (const uint16_t *)src[2],
                                flip ? -(long long)pitch : (long long)pitch, (int32_t)w, (int32_t)x, (int32_t)y, px);
                for (int c = 0; c < 3; c++) {
                    if (px[c] > 65535u)
                        die("a result that is no 16-bit sample");
                    rgb[((size_t)y * w + x) * 3 + c] = (uint16_t)px[c];
                }
            }
        put(out, rgb, (size_t)w * h * 6);
        std::free(rgb);
        std::free(surface);
    }
    if (at != raw + size)
        die("the input has bytes behind its last case");
    std::free(raw);
}

int main(int argc, char **argv) {
    if (argc < 3)
        die("usage: packed16_formats MODE OUT [ARGUMENTS]");
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
