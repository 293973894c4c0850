/*
 * ufloat_formats.cc — the formats whose pixel is one dword of three unsigned floats (R11G11B10F, RGB9E5) where host and device share
 * their text (csrc/hyd_sample_fmt.h, csrc/hip/hydk_store.h, csrc/hip/hydk_ufloat.h) as plain C++, no HIP header in sight, built by
 * tests/test_ufloat_formats.py with -fsanitize=address,undefined and held to tests/ufloat_model.py.  Each mode writes its results to
 * OUT as raw native-endian arrays:
 *
 *   ufloat_formats describe OUT LO HI  int32[HI - LO][18]: the twelve fields of hyd_fmt_describe in the struct's order, then of
 *                                      hydk_decode_fmt ok, the format encoded back (-1 where not ok), cls, storage, matrix and the
 *                                      storage form's variant
 *   ufloat_formats refusals OUT IN     IN: u32 cases, then per case i32 fmt, y, du, dv, pixel_stride, no_src, width — y, du, dv in
 *                                      BYTES: src = {base + y, base + y + du, base + y + dv}, base on a 16-byte boundary; OUT: per
 *                                      case 96 bytes, the message of hyd_fmt_refusal (all zero: NULL), or of src NULL
 *   ufloat_formats origins OUT IN      IN: u32 cases, then per case i32 fmt, row_stride (dwords), x0, y0; OUT: per case int64[3]: the
 *                                      BYTES hyd_fmt_origin adds to the three pointers
 *   ufloat_formats widen OUT           uint32[2048] the float32 bits of every 11-bit field, uint32[1024] of every 10-bit field,
 *                                      uint32[32][512] of every RGB9E5 (exponent, mantissa) pair
 *   ufloat_formats pixels OUT IN       IN: u32 cases, then per case u32 which (0 R11G11B10F, 1 RGB9E5), w, h, pitch (dwords), flip and
 *                                      the surface, pitch * (h - 1) + w dwords; OUT: per case h x w x 3 uint32, hydk_ufloat_pixel of
 *                                      every pixel.  flip: the rows are stored bottom-up and the pitch given to the definition is
 *                                      negative
 * Every surface is a malloc of exactly its dwords, ending with the last dword of its last row: a read that leaves it meets the redzone.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/hydrium_amd.h"
#include "hyd_sample_fmt.h"
#include "hip/hydk_store.h"
#include "hip/hydk_ufloat.h"

static void die(const char *what) {
    std::fprintf(stderr, "ufloat_formats: %s\n", what);
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

static_assert(HYD_FMT_BASE_UFLOAT == 8388608 && HYDAMD_R11G11B10F == 8388608 && HYDAMD_RGB9E5 == 8388609, "the public names are the base and the base + 1");
static_assert(hyd_fmt_describe(HYDAMD_R11G11B10F).layout == HYD_LAYOUT_UFLOAT && HYD_LAYOUT_UFLOAT == 6 && hyd_fmt_describe(HYDAMD_RGB9E5).is_float == 1 &&
                  hyd_fmt_describe(HYDAMD_RGB9E5).bytes == 4 && !hyd_fmt_describe(HYDAMD_R11G11B10F).host && !hyd_fmt_describe(8388610).device &&
                  !hyd_fmt_describe(8388607).device && !hyd_fmt_describe(2097152).device,
              "constexpr, as the kernels use it");
static_assert(HYDK_STORE_R11G11B10F == 19 && HYDK_STORE_RGB9E5 == 20 && HYDK_STORE_SIZE > HYDK_STORE_RGB9E5 && HYDK_STORE_TABLE == 19 && HYDK_STORE_FORMS == 15 &&
                  HYDK_STORE_COUNT == 17 && HYDK_STORE_R11G11B10F + HYDK_UFLOAT_RGB9E5 == HYDK_STORE_RGB9E5,
              "the two storage forms' own numbers inside the table, whatever its size comes to, and the older pinned constants where they were");
static_assert(hydk_store_form(HYDK_STORE_R11G11B10F).cls == HYDK_FMT_F32 && hydk_store_form(HYDK_STORE_RGB9E5).cls == HYDK_FMT_F32 &&
                  hydk_store_form(HYDK_STORE_RGB9E5).variant == 0 && hydk_store_form(HYDK_STORE_R11G11B10F).ycbcr == 0,
              "float class, no YCbCr, no variant bit");
static_assert(sizeof(HydFmt) == 12 * sizeof(int), "HydFmt keeps its twelve fields");

static void describe(std::FILE *out, int lo, int hi) {
    for (int fmt = lo; fmt < hi; fmt++) {
        const HydFmt f = hyd_fmt_describe(fmt);
        const HydkSampleForm d = hydk_decode_fmt(fmt);
        const int32_t row[18] = {f.device, f.host, f.is_float, f.bytes, f.layout, f.matrix, f.filter, f.sub, f.sx, f.sy, f.depth, f.bits,
                                 d.ok, d.ok ? hydk_encode_fmt(d) : -1, d.cls, (int32_t)d.storage, (int32_t)d.matrix, hydk_store_form((int)d.storage).variant};
        put(out, row, sizeof(row));
        if (d.ok && f.layout == HYD_LAYOUT_UFLOAT) {
            const HydkStoreForm form = hydk_store_form((int)d.storage);
            if (form.cls != HYDK_FMT_F32 || form.ycbcr != 0 || form.chroma_planes != 0 || form.interp != 0 || form.variant != 0)
                die("hydk_decode_fmt: storage form");
            if (d.sub != 0 || d.filter != 0 || d.sx != 0 || d.sy != 0 || d.matrix != 0)
                die("hydk_decode_fmt: nothing of YCbCr");
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
    for (uint32_t v = 0; v < 2048; v++) {
        const uint32_t w = hydk_ufloat_widen_field(v, 6);
        put(out, &w, 4);
    }
    for (uint32_t v = 0; v < 1024; v++) {
        const uint32_t w = hydk_ufloat_widen_field(v, 5);
        put(out, &w, 4);
    }
    for (uint32_t e = 0; e < 32; e++)
        for (uint32_t m = 0; m < 512; m++) {
            const uint32_t w = hydk_rgb9e5_widen(m, e);
            put(out, &w, 4);
        }
}

static void pixels(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const uint8_t *at = raw;
    const uint32_t cases = rd32(&at);
    for (uint32_t k = 0; k < cases; k++) {
        const uint32_t which = rd32(&at), w = rd32(&at), h = rd32(&at), pitch = rd32(&at), flip = rd32(&at);
        if (which > 1u || pitch < w || !w || !h)
            die("no such case");
        const size_t dwords = (size_t)pitch * (h - 1) + w;
        uint32_t *surface = (uint32_t *)std::malloc(4 * dwords); /* exactly the surface: it ends with the last dword of its last row */
        if (!surface)
            die("out of memory");
        std::memcpy(surface, at, 4 * dwords);
        at += 4 * dwords;
        const uint32_t *first = flip ? surface + (size_t)pitch * (h - 1) : surface;
        uint32_t *rgb = (uint32_t *)std::malloc((size_t)w * h * 12);
        if (!rgb)
            die("out of memory");
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++)
                hydk_ufloat_pixel((int)which, first, flip ? -(long long)pitch : (long long)pitch, (int32_t)x, (int32_t)y, rgb + ((size_t)y * w + x) * 3);
        put(out, rgb, (size_t)w * h * 12);
        std::free(rgb);
        std::free(surface);
    }
    if (at != raw + size)
        die("the input has bytes behind its last case");
    std::free(raw);
}

int main(int argc, char **argv) {
    if (argc < 3)
        die("usage: ufloat_formats MODE OUT [ARGUMENTS]");
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
