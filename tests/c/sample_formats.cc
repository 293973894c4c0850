/*
 * sample_formats.cc — the sample-format headers that host and device share (csrc/hyd_sample_fmt.h, csrc/hip/hydk_half.h,
 * hydk_yuv.h, hydk_yuv16.h, hydk_chroma.h, hydk_store.h) as plain C++, no HIP header in sight, built by tests/test_host_sanitizers.py with
 * -fsanitize=address,undefined and held to the numpy models (tests/yuv_model.py, p016_model.py, chroma_model.py,
 * pixel_layouts.widen_half_bits).  Each mode writes its results to OUT as raw native-endian arrays:
 *
 *   sample_formats half OUT            uint32[65536] binary16 widened, then uint32[65536] bfloat16 widened
 *   sample_formats yuv8 OUT MATRIX     uint8[2^24][3]: R, G, B of every (Y, U, V), Y slowest
 *   sample_formats yuv16 OUT IN        IN: uint16[n][3]; OUT: uint16[n][3] for each of the twelve table rows, depth slowest
 *   sample_formats chroma OUT IN       IN: u32 cases, then per case u32 bits (8, 16), filter, w, h and the chroma plane
 *                                      ceil(h / 2) x ceil(w / 2) x 2 samples; OUT: per case h x w x 2 samples
 *   sample_formats formats OUT         int32[FMT_HI - FMT_LO][18] for every number -8 ... 4100: the twelve fields of hyd_fmt_describe
 *                                      in the struct's order, then of hydk_decode_fmt ok, the format encoded back (-1 where not
 *                                      ok), cls, storage, matrix and the storage form's variant; then int64[cases][3] origin
 *                                      offsets; before it writes, the round trip of csrc/hip/hydk_store.h and the cases of
 *                                      hyd_fmt_refusal
 * Every chroma plane is a malloc of exactly its samples: a tap that leaves the plane meets the redzone.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/hydrium_amd.h"
#include "hyd_sample_fmt.h"
#include "hip/hydk_half.h"
#include "hip/hydk_yuv.h"
#include "hip/hydk_chroma.h"
#include "hip/hydk_yuv16.h"
#include "hip/hydk_store.h"

static void die(const char *what) {
    std::fprintf(stderr, "sample_formats: %s\n", what);
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

static void half(std::FILE *out) {
    for (int storage = HYDK_STORE_F16; storage <= HYDK_STORE_BF16; storage++)
        for (uint32_t bits = 0; bits < 65536u; bits++) {
            const uint32_t wide = hydk_widen_half(storage, bits);
            put(out, &wide, sizeof(wide));
        }
}

static void yuv8(std::FILE *out, int matrix) {
    const HydkYuvMatrix m = hydk_yuv_matrix(matrix);
    uint8_t *row = (uint8_t *)std::malloc(256 * 256 * 3);
    if (!row)
        die("out of memory");
    for (uint32_t y = 0; y < 256; y++) {
        for (uint32_t u = 0; u < 256; u++)
            for (uint32_t v = 0; v < 256; v++) {
                uint32_t rgb[3];
                hydk_yuv_to_rgb(m, y, u, v, rgb);
                for (int c = 0; c < 3; c++)
                    row[(u * 256 + v) * 3 + c] = (uint8_t)rgb[c];
            }
        put(out, row, 256 * 256 * 3);
    }
    std::free(row);
}

static void yuv16(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const size_t n = size / 6;
    uint16_t *yuv = (uint16_t *)std::malloc(n ? n * 6 : 1), *res = (uint16_t *)std::malloc(n ? n * 6 : 1);
    if (!yuv || !res)
        die("out of memory");
    std::memcpy(yuv, raw, n * 6);
    for (int depth = HYDK_YUV16_P010; depth <= HYDK_YUV16_P016; depth++)
        for (int matrix = 0; matrix < HYDK_YUV_MATRICES; matrix++) {
            const HydkYuvMatrix m = hydk_yuv16_matrix(depth, matrix), j = hydk_yuv16_job_matrix((uint32_t)(matrix + 4 * depth));
            if (std::memcmp(&m, &j, sizeof(m)))
                die("hydk_yuv16_job_matrix disagrees with hydk_yuv16_matrix");
            for (size_t i = 0; i < n; i++) {
                uint32_t rgb[3];
                hydk_yuv16_to_rgb(m, yuv[3 * i], yuv[3 * i + 1], yuv[3 * i + 2], rgb);
                for (int c = 0; c < 3; c++)
                    res[3 * i + c] = (uint16_t)rgb[c];
            }
            put(out, res, n * 6);
        }
    std::free(yuv);
    std::free(res);
    std::free(raw);
}

static uint32_t rd32(const uint8_t **p) {
    uint32_t v;
    std::memcpy(&v, *p, 4);
    *p += 4;
    return v;
}

static void chroma(std::FILE *out, const char *in) {
    size_t size = 0;
    uint8_t *raw = slurp(in, &size);
    const uint8_t *at = raw;
    const uint32_t cases = rd32(&at);
    for (uint32_t k = 0; k < cases; k++) {
        const uint32_t bits = rd32(&at), filter = rd32(&at), w = rd32(&at), h = rd32(&at);
        const int32_t cw = (int32_t)((w + 1) / 2), ch = (int32_t)((h + 1) / 2);
        const size_t bytes = (size_t)cw * (size_t)ch * 2 * (bits / 8);
        uint8_t *plane = (uint8_t *)std::malloc(bytes); /* exactly the plane */
        if (!plane)
            die("out of memory");
        std::memcpy(plane, at, bytes);
        at += bytes;
        for (int32_t y = 0; y < (int32_t)h; y++)
            for (int32_t x = 0; x < (int32_t)w; x++) {
                const int32_t vy = hydk_chroma_vy(y, ch);
                uint32_t uv[2];
                if (bits == 8) {
                    hydk_chroma_pair((int)filter, plane + (size_t)(y >> 1) * cw * 2, plane + (size_t)vy * cw * 2, cw, x, uv);
                    const uint8_t two[2] = {(uint8_t)uv[0], (uint8_t)uv[1]};
                    put(out, two, sizeof(two));
                } else {
                    const uint16_t *words = (const uint16_t *)plane;
                    hydk_chroma16_pair((int)filter, words + (size_t)(y >> 1) * cw * 2, words + (size_t)vy * cw * 2, cw, x, uv);
                    const uint16_t two[2] = {(uint16_t)uv[0], (uint16_t)uv[1]};
                    put(out, two, sizeof(two));
                }
            }
        std::free(plane);
    }
    if (at != raw + size)
        die("the input has bytes behind its last case");
    std::free(raw);
}

enum { FMT_LO = -8, FMT_HI = 4101 };

/* csrc/hip/hydk_store.h: every format a device entry point takes encodes back to itself after the decode, and every other
 * number of -8 ... 4100 is refused.  A job's fields are the descriptor's, for every family (the descriptor itself is held to
 * tests/format_model.py, number by number, by the Python side) */
static void round_trip() {
    for (int fmt = FMT_LO; fmt < FMT_HI; fmt++) {
        const HydFmt f = hyd_fmt_describe(fmt);
        const HydkSampleForm d = hydk_decode_fmt(fmt);
        if (!f.device) {
            if (d.ok || d.cls || d.storage || d.matrix || d.filter || d.sub || d.sx || d.sy)
                die("hydk_decode_fmt takes a number that names no device format");
            continue;
        }
        if (d.ok != 1 || hydk_encode_fmt(d) != fmt)
            die("a device format does not come back from hydk_decode_fmt and hydk_encode_fmt");
        const HydkStoreForm form = hydk_store_form((int)d.storage);
        const int yuv = f.layout != HYD_LAYOUT_RGB;
        if (d.cls != (f.is_float ? HYDK_FMT_F32 : f.bytes == 1 ? HYDK_FMT_U8 : HYDK_FMT_U16) || (d.storage != HYDK_STORE_F32 && form.cls != d.cls))
            die("hydk_decode_fmt: class");
        if (form.ycbcr != yuv || form.interp != (f.filter != 0) || (yuv && form.bits != 8 * f.bytes) || (yuv && form.chroma_planes != f.layout) ||
            (!yuv && d.storage != (uint32_t)(fmt == HYD_FMT_FLOAT16 ? HYDK_STORE_F16 : fmt == HYD_FMT_BFLOAT16 ? HYDK_STORE_BF16 : HYDK_STORE_F32)))
            die("hydk_decode_fmt: storage form");
        if (d.matrix != (uint32_t)(f.matrix + 4 * f.depth) || d.filter != (uint32_t)f.filter || d.sub != (uint32_t)f.sub || d.sx != f.sx || d.sy != f.sy)
            die("hydk_decode_fmt: a job's YCbCr fields are the descriptor's");
        if (f.layout == HYD_LAYOUT_PAIRS && (d.sub || d.sx != 1 || d.sy != 1))
            die("hydk_decode_fmt: 4:2:0 fields");
        if (!yuv && (d.matrix || d.filter || d.sub || d.sx || d.sy))
            die("hydk_decode_fmt: an RGB format has no YCbCr fields");
    }
}

/* hyd_fmt_refusal: one case per family for each rule it can break alone, and the one family that can break two */
static void want(const char *got, const char *message, const char *what) {
    if (got != message && (!got || !message || std::strcmp(got, message)))
        die(what);
}

static void refusals() {
    alignas(8) static char buf[64];
    const void *const rgb[3] = {buf, buf + 1, buf + 2}, *const nv12[3] = {buf, buf + 32, buf + 33}, *const p016[3] = {buf, buf + 32, buf + 34};
    const void *const planes[3] = {buf, buf + 16, buf + 32}, *const odd[3] = {buf, buf + 16, buf + 33};
    want(hyd_fmt_refusal(5, rgb, 3, 200), "Invalid Sample Format", "a number that names nothing");
    want(hyd_fmt_refusal(2111, nullptr, 0, 0), "Invalid Sample Format", "a number that names nothing, asked of the format alone");
    for (int fmt = HYD_FMT_UINT8; fmt <= HYDAMD_BFLOAT16; fmt++)
        want(hyd_fmt_refusal(fmt, odd, 0, 200), nullptr, "an RGB-like format takes any layout");
    want(hyd_fmt_refusal(HYDAMD_NV12C_BT601, nv12, 1, 200), nullptr, "NV12 as it should be");
    want(hyd_fmt_refusal(HYDAMD_NV12C_BT601, nv12, 2, 200), HYD_FMT_NV12_LAYOUT_MSG, "NV12: pixel stride");
    want(hyd_fmt_refusal(HYDAMD_NV12_BT709, p016, 1, 200), HYD_FMT_NV12_LAYOUT_MSG, "NV12: V two bytes behind U");
    want(hyd_fmt_refusal(HYDAMD_NV12_BT709, p016, 1, 0), HYD_FMT_NV12_LAYOUT_MSG, "NV12: the layout alone");
    want(hyd_fmt_refusal(HYDAMD_NV12_BT709, nullptr, 2, 200), nullptr, "NV12: no layout asked, and no pitch to hold");
    want(hyd_fmt_refusal(HYDAMD_P010L_BT709, p016, 1, 200), nullptr, "P010 as it should be");
    want(hyd_fmt_refusal(HYDAMD_P010L_BT709, p016, 2, 200), HYD_FMT_P016_LAYOUT_MSG, "P010: pixel stride");
    want(hyd_fmt_refusal(HYDAMD_P016_BT601_FULL, nv12, 1, 200), HYD_FMT_P016_LAYOUT_MSG, "P016: V one byte behind U");
    const void *const p016_odd[3] = {buf + 1, buf + 32, buf + 34}, *const p016_odd_uv[3] = {buf, buf + 33, buf + 35};
    want(hyd_fmt_refusal(HYDAMD_P012_BT709, p016_odd, 1, 200), HYD_FMT_P016_LAYOUT_MSG, "P012: an odd Y address");
    want(hyd_fmt_refusal(HYDAMD_P012_BT709, p016_odd_uv, 1, 200), HYD_FMT_P016_LAYOUT_MSG, "P012: an odd chroma address");
    want(hyd_fmt_refusal(HYDAMD_I422C_BT709, odd, 100, 200), nullptr, "planar 8-bit: any three addresses");
    want(hyd_fmt_refusal(HYDAMD_I422C_BT709, odd, 99, 200), HYD_FMT_PLANAR_PITCH_MSG, "planar 8-bit: pitch");
    want(hyd_fmt_refusal(HYDAMD_I444_BT709, planes, -199, 200), HYD_FMT_PLANAR_PITCH_MSG, "planar 4:4:4: pitch");
    want(hyd_fmt_refusal(HYDAMD_I444_BT709, planes, -199, 0), nullptr, "planar: no width, no pitch too short");
    want(hyd_fmt_refusal(HYDAMD_I210_BT601, planes, 100, 200), nullptr, "planar16 as it should be");
    want(hyd_fmt_refusal(HYDAMD_I210_BT601, odd, 100, 200), HYD_FMT_PLANAR16_ALIGN_MSG, "planar16: alignment");
    want(hyd_fmt_refusal(HYDAMD_I210_BT601, planes, 99, 200), HYD_FMT_PLANAR_PITCH_MSG, "planar16: pitch");
    want(hyd_fmt_refusal(HYDAMD_I210_BT601, odd, 99, 200), HYD_FMT_PLANAR16_ALIGN_MSG, "planar16, an odd address and a short pitch: the alignment message wins");
    want(hyd_fmt_refusal(HYDAMD_I210_BT601, nullptr, 99, 200), HYD_FMT_PLANAR_PITCH_MSG, "planar16: the pitch alone");
}

static void formats(std::FILE *out) {
    round_trip();
    refusals();
    for (int fmt = FMT_LO; fmt < FMT_HI; fmt++) {
        const HydFmt f = hyd_fmt_describe(fmt);
        const HydkSampleForm d = hydk_decode_fmt(fmt);
        const int32_t row[18] = {f.device, f.host,   f.is_float, f.bytes, f.layout, f.matrix, f.filter, f.sub, f.sx, f.sy, f.depth, f.bits,
                                 d.ok, d.ok ? hydk_encode_fmt(d) : -1, d.cls, (int32_t)d.storage, (int32_t)d.matrix, hydk_store_form((int)d.storage).variant};
        put(out, row, sizeof(row));
    }
    /* origins of the sub-rectangle at (256, 512) of a picture of pitch 1024: offsets from the three plane pointers */
    const size_t x0 = 256, y0 = 512;
    const ptrdiff_t pitch = 1024, pixel = 3;
    char *picture = (char *)std::malloc((size_t)pitch * 1024 * 3 * 4);
    if (!picture)
        die("out of memory");
    const int some[] = {HYD_FMT_UINT8, HYD_FMT_UINT16, HYD_FMT_FLOAT32, HYDAMD_FLOAT16, HYDAMD_BFLOAT16, HYDAMD_NV12_BT601, HYDAMD_NV12L_BT709,
                        HYDAMD_P010_BT709, HYDAMD_P016L_BT601_FULL};
    for (size_t k = 0; k < sizeof(some) / sizeof(some[0]); k++) {
        const HydFmt f = hyd_fmt_describe(some[k]);
        const int yuv = f.layout == HYD_LAYOUT_PAIRS;
        const void *const src[3] = {picture, picture + 64, picture + 64 + f.bytes};
        const void *origin[3];
        hyd_fmt_origin(some[k], src, pitch, yuv ? 1 : pixel, x0, y0, origin);
        if (hyd_fmt_refusal(some[k], src, yuv ? 1 : pixel, 0) || (yuv && !hyd_fmt_refusal(some[k], src, 2, 0)))
            die("hyd_fmt_refusal: the layout");
        for (int c = 0; c < 3; c++) {
            const int64_t off = (const char *)origin[c] - (const char *)src[c];
            put(out, &off, sizeof(off));
        }
    }
    std::free(picture);
}

int main(int argc, char **argv) {
    if (argc < 3)
        die("usage: sample_formats MODE OUT [ARGUMENT]");
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out)
        die("cannot open the output");
    if (!std::strcmp(argv[1], "half") && argc == 3)
        half(out);
    else if (!std::strcmp(argv[1], "yuv8") && argc == 4)
        yuv8(out, std::atoi(argv[3]));
    else if (!std::strcmp(argv[1], "yuv16") && argc == 4)
        yuv16(out, argv[3]);
    else if (!std::strcmp(argv[1], "chroma") && argc == 4)
        chroma(out, argv[3]);
    else if (!std::strcmp(argv[1], "formats") && argc == 3)
        formats(out);
    else
        die("no such mode");
    if (std::fclose(out))
        die("cannot write");
    return 0;
}
