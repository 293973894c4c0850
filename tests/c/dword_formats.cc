/*
 * dword_formats.cc — the formats whose pixel is one dword of three 10-bit fields (RGB10A2, BGR10A2, Y410) where host and device share
 * their text (csrc/hyd_sample_fmt.h, csrc/hip/hydk_store.h, csrc/hip/hydk_rgb10.h) as plain C++, no HIP header in sight, built by
 * tests/test_dword_formats.py with -fsanitize=address,undefined and held to tests/dword_model.py.  Each mode writes its results to
 * OUT as raw native-endian arrays:
 *
 *   dword_formats describe OUT LO HI  int32[HI - LO][18]: the twelve fields of hyd_fmt_describe in the struct's order, then of
 *                                     hydk_decode_fmt ok, the format encoded back (-1 where not ok), cls, storage, matrix and the
 *                                     storage form's variant
 *   dword_formats refusals OUT IN     IN: u32 cases, then per case i32 fmt, y, du, dv, pixel_stride, no_src, width — y, du, dv in
 *                                     BYTES: src = {base + y, base + y + du, base + y + dv}, base on an 8-byte boundary; OUT: per
 *                                     case 96 bytes, the message of hyd_fmt_refusal (all zero: NULL), or of src NULL
 *   dword_formats origins OUT IN      IN: u32 cases, then per case i32 fmt, row_stride (dwords), x0, y0; OUT: per case int64[3]: the
 *                                     BYTES hyd_fmt_origin adds to the three pointers
 *   dword_formats widen OUT           uint32[1024][2]: hydk_rgb10_widen(v) and (v * 65535 + 511) / 1023
 *   dword_formats pixels OUT IN       IN: u32 cases, then per case u32 ycbcr, which (the RGB order, or the matrix), w, h, pitch
 *                                     (dwords), flip and the surface, pitch * (h - 1) + w dwords; OUT: per case h x w x 3 words,
 *                                     hydk_dword_pixel of every pixel.  flip: the rows are stored bottom-up and the pitch given to
 *                                     the definition is negative
 * Every surface is a malloc of exactly its dwords, ending with the last dword of its last row: a read that leaves it meets the redzone.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/hydrium_amd.h"
#include "hyd_sample_fmt.h"
#include "hip/hydk_store.h"
#include "hip/hydk_rgb10.h"

static void die(const char *what) {
    std::fprintf(stderr, "dword_formats: %s\n", what);
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

static_assert(HYDAMD_RGB10A2 == HYD_FMT_BASE_DWORD && HYDAMD_RGB10A2 == 131072 && HYDAMD_BGR10A2 == 131073 && HYDAMD_Y410_BT709 == 131144 &&
                  HYDAMD_Y410_BT709_FULL == 131145 && HYDAMD_Y410_BT601 == 131146 && HYDAMD_Y410_BT601_FULL == 131147,
              "the public names are the rule's numbers");
static_assert(hyd_fmt_describe(HYDAMD_Y410_BT601).layout == HYD_LAYOUT_DWORD && hyd_fmt_describe(HYDAMD_BGR10A2).bits == 10 &&
                  hyd_fmt_describe(HYDAMD_RGB10A2).bytes == 4 && !hyd_fmt_describe(131074).device && !hyd_fmt_describe(131148).device,
              "constexpr, as the kernels use it");
static_assert(HYDK_STORE_RGB10 == 15 && HYDK_STORE_Y410 == 16 && HYDK_STORE_COUNT == 17 && HYDK_VARIANT_RGB10 == 32768 && HYDK_VARIANT_Y410 == 65536,
              "the two storage forms and their variant bits");
static_assert(sizeof(HydFmt) == 12 * sizeof(int), "HydFmt keeps its twelve fields");

static void describe(std::FILE *out, int lo, int hi) {
    for (int fmt = lo; fmt < hi; fmt++) {
        const HydFmt f = hyd_fmt_describe(fmt);
        const HydkSampleForm d = hydk_decode_fmt(fmt);
        const int32_t row[18] = {f.device, f.host, f.is_float, f.bytes, f.layout, f.matrix, f.filter, f.sub, f.sx, f.sy, f.depth, f.bits,
                                 d.ok, d.ok ? hydk_encode_fmt(d) : -1, d.cls, (int32_t)d.storage, (int32_t)d.matrix, hydk_store_form((int)d.storage).variant};
        put(out, row, sizeof(row));
        if (d.ok && f.layout == HYD_LAYOUT_DWORD) {
            const HydkStoreForm form = hydk_store_form((int)d.storage);
            if (form.cls != HYDK_FMT_U16 || form.ycbcr != (f.depth != 0) || form.chroma_planes != 0 || form.interp != 0 || form.bits != 10)
                die("hydk_decode_fmt: storage form");
            /* a job's sub carries the field order of the RGB forms, 0 for R low and 1 for B low; Y410's is 4:4:4 */
            if (d.sub != (f.depth ? (uint32_t)HYD_FMT_SUB_444 : (uint32_t)(fmt - HYD_FMT_BASE_DWORD)))
                die("hydk_decode_fmt: sub");
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
    uint32_t *picture = (uint32_t *)std::malloc((size_t)1 << 26);
    if (!picture)
        die("out of memory");
    for (uint32_t k = 0; k < cases; k++) {
        const int fmt = (int)rd32(&at), pitch = (int)rd32(&at), x0 = (int)rd32(&at), y0 = (int)rd32(&at);
        const uint32_t *base = picture + ((size_t)1 << 23);
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

static void widen(std::FILE *out) {
    for (uint32_t v = 0; v < 1024; v++) {
        const uint32_t pair[2] = {hydk_rgb10_widen(v), (v * 65535u + 511u) / 1023u};
        put(out, pair, sizeof(pair));
    }
}

static void pixels(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const uint8_t *at = raw;
    const uint32_t cases = rd32(&at);
    for (uint32_t k = 0; k < cases; k++) {
        const uint32_t ycbcr = rd32(&at), which = rd32(&at), w = rd32(&at), h = rd32(&at), pitch = rd32(&at), flip = rd32(&at);
        const size_t dwords = (size_t)pitch * (h - 1) + w;
        if (ycbcr > 1 || which > (ycbcr ? 3u : 1u) || pitch < w || !w || !h)
            die("no such case");
        uint32_t *surface = (uint32_t *)std::malloc(4 * dwords); /* exactly the surface: it ends with the last dword of its last row */
        if (!surface)
            die("out of memory");
        std::memcpy(surface, at, 4 * dwords);
        at += 4 * dwords;
        const uint32_t *first = flip ? surface + (size_t)pitch * (h - 1) : surface;
        uint16_t *rgb = (uint16_t *)std::malloc((size_t)w * h * 6);
        if (!rgb)
            die("out of memory");
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                uint32_t px[3];
                hydk_dword_pixel((int)ycbcr, (int)which, first, flip ? -(long long)pitch : (long long)pitch, (int32_t)x, (int32_t)y, px);
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
        die("usage: dword_formats MODE OUT [ARGUMENTS]");
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out)
        die("cannot open the output");
    if (!std::strcmp(argv[1], "describe") && argc == 5)
        describe(out, std::atoi(argv[3]), std::atoi(argv[4]));
    else if (!std::strcmp(argv[1], "refusals") && argc == 4)
        refusals(out, argv[3]);
    else if (!std::strcmp(argv[1], "origins") && argc == 4)
        origins(out, argv[3]);
    else if (!std::strcmp(argv[1], "widen") && argc == 3)
        widen(out);
    else if (!std::strcmp(argv[1], "pixels") && argc == 4)
        pixels(out, argv[3]);
    else
        die("no such mode");
    if (std::fclose(out))
        die("cannot write");
    return 0;
}
