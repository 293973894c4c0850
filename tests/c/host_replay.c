/*
 * host_replay.c — the host glue's test hooks (csrc/host/, -DHYD_TEST_HOOKS) called from a program of its own, so that the
 * address and undefined-behaviour sanitizers see them: tests/test_host_sanitizers.py compiles this file with all of
 * csrc/host and -fsanitize=address,undefined, writes one record per hook call it made through the ctypes flavour, and
 * compares what comes back here, byte for byte.
 *
 *   host_replay RECORDS RESULTS REPORT     replay every record
 *   host_replay --device-call              call the first device function the link stubbed: must end the program
 *
 * Every input buffer is a malloc of exactly the bytes the hook may read (a zero-length input is malloc(0)), every output
 * buffer one of exactly its capacity: the allocator's redzone starts at the first byte a hook has no business with.  A
 * record that holds byte streams (blobs, payloads, LF bit streams, ICC profiles) runs a second time with each of them at an
 * odd address.  Everything else has the alignment of its element type, as C gives it to the caller of the hook.
 *
 * File formats (native byte order; written and read by tests/host_replay.py, never committed):
 *   records: "HYDRPLY1", u32 count, then per record u32 hook, u32 nargs and per argument u32 kind, u32 flags, u64 a, u64 b
 *            and the payload of its kind (below)
 *   results: per record and pass u32 index, u32 pass, i32 return code, the error text (u32 length or 0xffffffff, bytes), then
 *            per K_OUT argument its bytes and per K_OUTPTR argument u64 length (all ones: none) and the bytes
 *   report:  one line "name calls" per hook
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hydrium_amd.h"
#include "planbuf.h"

/* ---- the hooks (the files of csrc/host under HYD_TEST_HOOKS; they have no header of their own) ---- */
int hydt_frame_from_stages(const HYDImageMetadata *md, int write_header, int is_last, size_t lfg_count, const uint32_t *tile_xy,
                           const int32_t *const *dc, const uint32_t *freq, const uint32_t *alphabet, const uint32_t *group_bits,
                           unsigned max_alphabet, const uint8_t *payload, size_t payload_len, const uint8_t *icc, size_t icc_size,
                           uint8_t **out, size_t *out_len, const char **err);
void hydt_free(void *p);
int hydt_code_lengths(const uint32_t *freq, uint32_t *lengths, uint32_t n, int max_depth);
int hydt_small_code_lengths(const uint32_t *freq, uint32_t *lengths, uint32_t n, int max_depth);
int hydt_icc_mangled(const uint8_t *icc, size_t icc_size, uint8_t **out, size_t *out_len);
int hydt_lf_group(const int32_t *dc, size_t vbw, size_t vbh, uint8_t **out, size_t *out_len);
int hydt_lf_group_coded(size_t vbw, size_t vbh, const uint8_t *lengths, uint32_t alphabet, uint32_t run_pairs, const uint8_t *bits,
                        uint64_t bit_count, uint8_t **out, size_t *out_len);
int hydt_blob_class(const void *blob, size_t size, size_t expected_slots);
int hydt_batch_from_streams(const HYDImageMetadata *md, size_t nframes, const HydAmdLfStream *lf, const uint32_t *freq,
                            const uint32_t *alphabet, const uint32_t *group_bits, const uint32_t *max_alphabet, const uint8_t *payload,
                            size_t payload_len, uint64_t *frame_offsets, uint8_t **out, size_t *out_len, const char **err);
int hydt_tiles_from_streams(const HYDImageMetadata *md, size_t nframes, const HydAmdLfStream *lf, const uint32_t *freq,
                            const uint32_t *alphabet, const uint32_t *group_bits, const uint32_t *max_alphabet, const uint8_t *payload,
                            size_t payload_len, uint64_t *frame_offsets, uint8_t **out, size_t *out_len, const char **err);
int hydt_mixed_from_streams(size_t n, const uint32_t *widths, const uint32_t *heights, const HydAmdLfStream *lf, const uint32_t *freq,
                            const uint32_t *alphabet, const uint32_t *group_bits, const uint32_t *max_alphabet, const uint8_t *payload,
                            size_t payload_len, uint64_t *frame_offsets, uint8_t **out, size_t *out_len, const char **err);
int hydt_mixed_from_streams_skip(size_t n, const uint32_t *widths, const uint32_t *heights, const HydAmdLfStream *lf,
                                 const uint32_t *freq, const uint32_t *alphabet, const uint32_t *group_bits, const uint32_t *max_alphabet,
                                 const uint8_t *payload, size_t payload_len, const uint32_t *flags, uint64_t *frame_offsets,
                                 uint32_t *status, uint64_t *piece_bits, uint8_t **out, size_t *out_len, const char **err);
int hydt_mixed_plan_counts(size_t n, const uint32_t *widths, const uint32_t *heights, uint32_t *nshapes, size_t *plan_bytes);
int hydt_mixed_plan_describe(size_t n, const uint32_t *widths, const uint32_t *heights, int max_frames, int max_slots,
                             uint32_t *per_frame, uint32_t *counts, uint32_t *parts, uint64_t *fixed, uint64_t *caps, uint8_t **plan_out,
                             size_t *plan_len, const char **err);
int hydt_mixed_frame_plan_alone(uint32_t w, uint32_t h, uint8_t **plan_out, size_t *plan_len, const char **err);
int hydt_compose_pieces(const uint64_t *dst_bit, const uint64_t *nbits, const uint64_t *src_off, uint32_t np, const uint8_t *src,
                        uint64_t lo, uint64_t bytes, uint8_t *out);
int hydt_lf_head_host(const uint8_t *lengths, uint32_t alphabet0, uint32_t run_pairs, uint8_t *out, size_t cap, uint64_t *nbits);
int hydt_lf_head_sections(const uint8_t *lengths, uint32_t alphabet0, uint32_t run_pairs, uint8_t *out, size_t cap, uint64_t *nbits);
int hydt_lf_head_wave(const uint8_t *lengths, uint32_t alphabet0, uint32_t run_pairs, uint8_t *out, size_t cap, uint64_t *nbits);
int hydt_ans_distribution_host(const uint32_t *freq, uint32_t alphabet, uint8_t *out, size_t cap, uint64_t *nbits);
int hydt_ans_distribution_sections(const uint32_t *freq, uint32_t alphabet, uint8_t *out, size_t cap, uint64_t *nbits);
int hydt_toc_entry_check(uint64_t size);
int hydt_shard_checks(int reset, int mode, int n, const int *keys, int assembling, int latch, int *check_view, int *check_floor);

/* the order of tests/host_replay.py's HOOKS */
enum {
    H_FRAME_FROM_STAGES, H_FRAME_FROM_STREAMS, H_LF_GROUP, H_LF_GROUP_CODED, H_CODE_LENGTHS, H_SMALL_CODE_LENGTHS, H_ICC_MANGLED,
    H_BLOB_CLASS, H_LAYOUT_FROM_STREAMS, H_LAYOUT_FROM_STREAMS_SKIP, H_MIXED_FROM_STREAMS, H_MIXED_FROM_STREAMS_SKIP,
    H_MIXED_PLAN_COUNTS, H_MIXED_PLAN_DESCRIBE, H_MIXED_FRAME_PLAN_ALONE, H_TILES_FROM_STREAMS, H_BATCH_FROM_STREAMS,
    H_COMPOSE_PIECES, H_ANS_DISTRIBUTION_HOST, H_ANS_DISTRIBUTION_SECTIONS, H_LF_HEAD_HOST, H_LF_HEAD_SECTIONS, H_LF_HEAD_WAVE,
    H_TOC_ENTRY_CHECK, H_SHARD_CHECKS, H_FREE, H_BLOB_CLASS_PREFIXES, H_COUNT
};
static const char *const kNames[H_COUNT] = {
    "hydt_frame_from_stages", "hydamd_frame_from_streams", "hydt_lf_group", "hydt_lf_group_coded", "hydt_code_lengths",
    "hydt_small_code_lengths", "hydt_icc_mangled", "hydt_blob_class", "hydt_layout_from_streams", "hydt_layout_from_streams_skip",
    "hydt_mixed_from_streams", "hydt_mixed_from_streams_skip", "hydt_mixed_plan_counts", "hydt_mixed_plan_describe",
    "hydt_mixed_frame_plan_alone", "hydt_tiles_from_streams", "hydt_batch_from_streams", "hydt_compose_pieces",
    "hydt_ans_distribution_host", "hydt_ans_distribution_sections", "hydt_lf_head_host", "hydt_lf_head_sections", "hydt_lf_head_wave",
    "hydt_toc_entry_check", "hydt_shard_checks", "hydt_free", "hydt_blob_class:prefixes"};
static unsigned long g_calls[H_COUNT];

/* the layout hooks have no export of their own: mixed.c and batch.c call them across files, and the link (--wrap) routes
 * those calls through here, where they are counted.  They run on the plans the product's own planners just made. */
int __real_hydt_layout_from_streams(const uint8_t *plan, const struct HydkTileFrame *frames, const struct HydkTileShape *shapes,
                                    size_t nframes, const struct HydAmdLfStream *lf, const uint32_t *freq, const uint32_t *alphabet,
                                    const uint32_t *group_bits, const uint32_t *max_alphabet, const uint8_t *payload, size_t payload_len,
                                    uint64_t *frame_offsets, uint8_t **out, size_t *out_len, const char **err);
int __wrap_hydt_layout_from_streams(const uint8_t *plan, const struct HydkTileFrame *frames, const struct HydkTileShape *shapes,
                                    size_t nframes, const struct HydAmdLfStream *lf, const uint32_t *freq, const uint32_t *alphabet,
                                    const uint32_t *group_bits, const uint32_t *max_alphabet, const uint8_t *payload, size_t payload_len,
                                    uint64_t *frame_offsets, uint8_t **out, size_t *out_len, const char **err) {
    g_calls[H_LAYOUT_FROM_STREAMS]++;
    return __real_hydt_layout_from_streams(plan, frames, shapes, nframes, lf, freq, alphabet, group_bits, max_alphabet, payload,
                                           payload_len, frame_offsets, out, out_len, err);
}
int __real_hydt_layout_from_streams_skip(const uint8_t *plan, const struct HydkTileFrame *frames, const struct HydkTileShape *shapes,
                                         size_t nframes, const struct HydAmdLfStream *lf, const uint32_t *freq, const uint32_t *alphabet,
                                         const uint32_t *group_bits, const uint32_t *max_alphabet, const uint8_t *payload,
                                         size_t payload_len, const uint32_t *flags, uint64_t *frame_offsets, uint32_t *status,
                                         uint64_t *piece_bits, uint8_t **out, size_t *out_len, const char **err);
int __wrap_hydt_layout_from_streams_skip(const uint8_t *plan, const struct HydkTileFrame *frames, const struct HydkTileShape *shapes,
                                         size_t nframes, const struct HydAmdLfStream *lf, const uint32_t *freq, const uint32_t *alphabet,
                                         const uint32_t *group_bits, const uint32_t *max_alphabet, const uint8_t *payload,
                                         size_t payload_len, const uint32_t *flags, uint64_t *frame_offsets, uint32_t *status,
                                         uint64_t *piece_bits, uint8_t **out, size_t *out_len, const char **err) {
    g_calls[H_LAYOUT_FROM_STREAMS_SKIP]++;
    return __real_hydt_layout_from_streams_skip(plan, frames, shapes, nframes, lf, freq, alphabet, group_bits, max_alphabet, payload,
                                                payload_len, flags, frame_offsets, status, piece_bits, out, out_len, err);
}

/* ---- what a device function's stand-in calls (the stubs are written at test time, one per symbol the link misses) ---- */
void hydt_replay_device_call(const char *name) {
    fprintf(stderr, "host_replay: a replayed hook reached the device function %s\n", name);
    fflush(stderr);
    _Exit(3);
}
void hydt_replay_first_stub(void);

static void die(const char *what) {
    fprintf(stderr, "host_replay: %s\n", what);
    exit(2);
}

/* ---- records ---- */
enum { K_SCALAR, K_IN, K_OUT, K_OUTPTR, K_OUTLEN, K_ERR, K_LFARR, K_PTRARR };
enum { F_NULL = 1, F_STREAM = 2 };
#define MAX_ARGS 24
#define NONE (~UINT64_C(0))

typedef struct Arg {
    uint32_t kind, flags;
    uint64_t a, b;
    const uint8_t *payload; /* in the records' image */
    void *ptr;              /* what the hook is handed in this pass */
    uint8_t *out;           /* K_OUTPTR */
    size_t out_len;         /* K_OUTLEN */
    const char *err;        /* K_ERR */
} Arg;

static void *g_owned[3 * 256 + 4 * MAX_ARGS];
static size_t g_nowned;

static void *own(void *p) {
    if (!p)
        die("out of memory");
    if (g_nowned == sizeof(g_owned) / sizeof(g_owned[0]))
        die("too many buffers in one record");
    return g_owned[g_nowned++] = p;
}

/* n bytes of their own; `odd`: at an odd address */
static void *exact(const uint8_t *src, uint64_t n, int odd) {
    uint8_t *p = own(malloc((size_t)n + (odd ? 1 : 0)));
    if (odd)
        p++;
    if (n)
        memcpy(p, src, (size_t)n);
    return p;
}

static uint64_t rd64(const uint8_t **p) {
    uint64_t v;
    memcpy(&v, *p, 8);
    *p += 8;
    return v;
}
static uint32_t rd32(const uint8_t **p) {
    uint32_t v;
    memcpy(&v, *p, 4);
    *p += 4;
    return v;
}

/* reads one argument's payload; with `make`, allocates what the hook gets */
static void argument(Arg *a, const uint8_t **at, int make, int odd) {
    const uint8_t *p = *at;
    const int null = a->flags & F_NULL, stream = odd && (a->flags & F_STREAM);
    a->ptr = NULL;
    switch (a->kind) {
    case K_IN:
    case K_OUT:
        if (!null) {
            if (make)
                a->ptr = exact(p, a->a, stream);
            p += a->a;
        }
        break;
    case K_OUTPTR:
        a->out = NULL;
        a->ptr = null ? NULL : (void *)&a->out;
        break;
    case K_OUTLEN:
        a->out_len = 0;
        a->ptr = null ? NULL : (void *)&a->out_len;
        break;
    case K_ERR:
        a->err = NULL;
        a->ptr = null ? NULL : (void *)&a->err;
        break;
    case K_LFARR:
        if (!null) {
            HydAmdLfStream *lf = make ? own(malloc((size_t)a->a * sizeof(*lf))) : NULL;
            for (uint64_t i = 0; i < a->a; i++) {
                const uint32_t alphabet = rd32(&p), run_pairs = rd32(&p);
                const uint64_t bit_count = rd64(&p), nl = rd64(&p);
                const uint8_t *lengths = p;
                p += nl == NONE ? 0 : nl;
                const uint64_t nb = rd64(&p);
                const uint8_t *bits = p;
                p += nb == NONE ? 0 : nb;
                if (make) {
                    lf[i].alphabet = alphabet;
                    lf[i].run_pairs = run_pairs;
                    lf[i].bit_count = bit_count;
                    lf[i].lengths = nl == NONE ? NULL : exact(lengths, nl, 0);
                    lf[i].bits = nb == NONE ? NULL : exact(bits, nb, odd); /* a bit stream: any byte address */
                }
            }
            a->ptr = lf;
        }
        break;
    case K_PTRARR:
        if (!null) {
            void **v = make ? own(malloc((size_t)a->a * sizeof(*v))) : NULL;
            for (uint64_t i = 0; i < a->a; i++) {
                const uint64_t n = rd64(&p);
                if (make)
                    v[i] = n == NONE ? NULL : exact(p, n, 0);
                p += n == NONE ? 0 : n;
            }
            a->ptr = v;
        }
        break;
    default:
        break;
    }
    *at = p;
}

#define S(i, T) ((T)A[i].a)
#define P(i, T) ((T)A[i].ptr)

static int call(uint32_t hook, Arg *A, uint32_t n) {
    static const uint32_t want[H_COUNT] = {17, 17, 5, 9, 4, 4, 4, 3, 0, 0, 14, 17, 5, 13, 5, 13, 13, 8, 5, 5, 6, 6, 6, 1, 8, 0, 3};
    if (hook >= H_COUNT || n != want[hook] || hook == H_LAYOUT_FROM_STREAMS || hook == H_LAYOUT_FROM_STREAMS_SKIP || hook == H_FREE)
        die("a record names a hook with other arguments than it has");
    g_calls[hook]++;
    switch (hook) {
    case H_FRAME_FROM_STAGES:
        return hydt_frame_from_stages(P(0, const HYDImageMetadata *), S(1, int), S(2, int), S(3, size_t), P(4, const uint32_t *),
                                      P(5, const int32_t *const *), P(6, const uint32_t *), P(7, const uint32_t *), P(8, const uint32_t *),
                                      S(9, unsigned), P(10, const uint8_t *), S(11, size_t), P(12, const uint8_t *), S(13, size_t),
                                      P(14, uint8_t **), P(15, size_t *), P(16, const char **));
    case H_FRAME_FROM_STREAMS:
        return hydamd_frame_from_streams(P(0, const HYDImageMetadata *), S(1, int), S(2, int), S(3, size_t), P(4, const uint32_t *),
                                         P(5, const HydAmdLfStream *), P(6, const uint32_t *), P(7, const uint32_t *),
                                         P(8, const uint32_t *), S(9, unsigned), P(10, const uint8_t *), S(11, size_t),
                                         P(12, const uint8_t *), S(13, size_t), P(14, uint8_t **), P(15, size_t *), P(16, const char **));
    case H_LF_GROUP:
        return hydt_lf_group(P(0, const int32_t *), S(1, size_t), S(2, size_t), P(3, uint8_t **), P(4, size_t *));
    case H_LF_GROUP_CODED:
        return hydt_lf_group_coded(S(0, size_t), S(1, size_t), P(2, const uint8_t *), S(3, uint32_t), S(4, uint32_t), P(5, const uint8_t *),
                                   S(6, uint64_t), P(7, uint8_t **), P(8, size_t *));
    case H_CODE_LENGTHS:
        return hydt_code_lengths(P(0, const uint32_t *), P(1, uint32_t *), S(2, uint32_t), S(3, int));
    case H_SMALL_CODE_LENGTHS:
        return hydt_small_code_lengths(P(0, const uint32_t *), P(1, uint32_t *), S(2, uint32_t), S(3, int));
    case H_ICC_MANGLED:
        return hydt_icc_mangled(P(0, const uint8_t *), S(1, size_t), P(2, uint8_t **), P(3, size_t *));
    case H_BLOB_CLASS:
        return hydt_blob_class(P(0, const void *), S(1, size_t), S(2, size_t));
    case H_MIXED_FROM_STREAMS:
        return hydt_mixed_from_streams(S(0, size_t), P(1, const uint32_t *), P(2, const uint32_t *), P(3, const HydAmdLfStream *),
                                       P(4, const uint32_t *), P(5, const uint32_t *), P(6, const uint32_t *), P(7, const uint32_t *),
                                       P(8, const uint8_t *), S(9, size_t), P(10, uint64_t *), P(11, uint8_t **), P(12, size_t *),
                                       P(13, const char **));
    case H_MIXED_FROM_STREAMS_SKIP:
        return hydt_mixed_from_streams_skip(S(0, size_t), P(1, const uint32_t *), P(2, const uint32_t *), P(3, const HydAmdLfStream *),
                                            P(4, const uint32_t *), P(5, const uint32_t *), P(6, const uint32_t *), P(7, const uint32_t *),
                                            P(8, const uint8_t *), S(9, size_t), P(10, const uint32_t *), P(11, uint64_t *),
                                            P(12, uint32_t *), P(13, uint64_t *), P(14, uint8_t **), P(15, size_t *), P(16, const char **));
    case H_MIXED_PLAN_COUNTS:
        return hydt_mixed_plan_counts(S(0, size_t), P(1, const uint32_t *), P(2, const uint32_t *), P(3, uint32_t *), P(4, size_t *));
    case H_MIXED_PLAN_DESCRIBE:
        return hydt_mixed_plan_describe(S(0, size_t), P(1, const uint32_t *), P(2, const uint32_t *), S(3, int), S(4, int), P(5, uint32_t *),
                                        P(6, uint32_t *), P(7, uint32_t *), P(8, uint64_t *), P(9, uint64_t *), P(10, uint8_t **),
                                        P(11, size_t *), P(12, const char **));
    case H_MIXED_FRAME_PLAN_ALONE:
        return hydt_mixed_frame_plan_alone(S(0, uint32_t), S(1, uint32_t), P(2, uint8_t **), P(3, size_t *), P(4, const char **));
    case H_TILES_FROM_STREAMS:
        return hydt_tiles_from_streams(P(0, const HYDImageMetadata *), S(1, size_t), P(2, const HydAmdLfStream *), P(3, const uint32_t *),
                                       P(4, const uint32_t *), P(5, const uint32_t *), P(6, const uint32_t *), P(7, const uint8_t *),
                                       S(8, size_t), P(9, uint64_t *), P(10, uint8_t **), P(11, size_t *), P(12, const char **));
    case H_BATCH_FROM_STREAMS:
        return hydt_batch_from_streams(P(0, const HYDImageMetadata *), S(1, size_t), P(2, const HydAmdLfStream *), P(3, const uint32_t *),
                                       P(4, const uint32_t *), P(5, const uint32_t *), P(6, const uint32_t *), P(7, const uint8_t *),
                                       S(8, size_t), P(9, uint64_t *), P(10, uint8_t **), P(11, size_t *), P(12, const char **));
    case H_COMPOSE_PIECES:
        return hydt_compose_pieces(P(0, const uint64_t *), P(1, const uint64_t *), P(2, const uint64_t *), S(3, uint32_t),
                                   P(4, const uint8_t *), S(5, uint64_t), S(6, uint64_t), P(7, uint8_t *));
    case H_ANS_DISTRIBUTION_HOST:
        return hydt_ans_distribution_host(P(0, const uint32_t *), S(1, uint32_t), P(2, uint8_t *), S(3, size_t), P(4, uint64_t *));
    case H_ANS_DISTRIBUTION_SECTIONS:
        return hydt_ans_distribution_sections(P(0, const uint32_t *), S(1, uint32_t), P(2, uint8_t *), S(3, size_t), P(4, uint64_t *));
    case H_LF_HEAD_HOST:
        return hydt_lf_head_host(P(0, const uint8_t *), S(1, uint32_t), S(2, uint32_t), P(3, uint8_t *), S(4, size_t), P(5, uint64_t *));
    case H_LF_HEAD_SECTIONS:
        return hydt_lf_head_sections(P(0, const uint8_t *), S(1, uint32_t), S(2, uint32_t), P(3, uint8_t *), S(4, size_t), P(5, uint64_t *));
    case H_LF_HEAD_WAVE:
        return hydt_lf_head_wave(P(0, const uint8_t *), S(1, uint32_t), S(2, uint32_t), P(3, uint8_t *), S(4, size_t), P(5, uint64_t *));
    case H_TOC_ENTRY_CHECK:
        return hydt_toc_entry_check(S(0, uint64_t));
    case H_SHARD_CHECKS:
        return hydt_shard_checks(S(0, int), S(1, int), S(2, int), P(3, const int *), S(4, int), S(5, int), P(6, int *), P(7, int *));
    default:
        die("no such hook");
    }
    return 0;
}

static void put(FILE *f, const void *p, size_t n) {
    if (n && fwrite(p, 1, n, f) != n)
        die("cannot write the results");
}

/* H_BLOB_CLASS_PREFIXES (blob, expected_slots, classes [len + 1]): every truncation of the blob, 0 bytes to all of it, each
 * in an allocation of exactly its length, at an even and at an odd address; classes[k] = the class of the first k bytes */
static int blob_prefixes(Arg *A, int odd) {
    const uint8_t *blob = A[0].ptr;
    uint8_t *classes = A[2].ptr;
    g_calls[H_BLOB_CLASS_PREFIXES]++;
    for (uint64_t k = 0; k <= A[0].a; k++) {
        uint8_t *base = malloc((size_t)k + (odd ? 1 : 0)), *p = base + (odd ? 1 : 0);
        if (!base)
            die("out of memory");
        if (k)
            memcpy(p, blob, (size_t)k);
        g_calls[H_BLOB_CLASS]++;
        classes[k] = (uint8_t)hydt_blob_class(p, (size_t)k, S(1, size_t));
        free(base);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--device-call")) {
        hydt_replay_first_stub();
        return 0; /* a stub that came back: the test fails on this status */
    }
    if (argc != 4)
        die("usage: host_replay RECORDS RESULTS REPORT | --device-call");
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        die("cannot open the records");
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *image = malloc((size_t)size + 1);
    if (!image || fread(image, 1, (size_t)size, f) != (size_t)size)
        die("cannot read the records");
    fclose(f);
    if (size < 12 || memcmp(image, "HYDRPLY1", 8))
        die("not a records file");
    FILE *res = fopen(argv[2], "wb");
    if (!res)
        die("cannot open the results");
    const uint8_t *at = image + 8;
    const uint32_t count = rd32(&at);
    for (uint32_t r = 0; r < count; r++) {
        Arg A[MAX_ARGS];
        const uint32_t hook = rd32(&at), n = rd32(&at);
        if (n > MAX_ARGS)
            die("too many arguments");
        const uint8_t *first = at;
        int streams = 0;
        for (int pass = 0; pass < 1 + streams; pass++) {
            at = first;
            for (uint32_t i = 0; i < n; i++) {
                A[i].kind = rd32(&at);
                A[i].flags = rd32(&at);
                A[i].a = rd64(&at);
                A[i].b = rd64(&at);
                argument(&A[i], &at, 1, pass);
                if (!pass && !(A[i].flags & F_NULL) && ((A[i].flags & F_STREAM) || A[i].kind == K_LFARR))
                    streams = 1;
            }
            const int ret = hook == H_BLOB_CLASS_PREFIXES ? blob_prefixes(A, pass) : call(hook, A, n);
            const uint32_t head[2] = {r, (uint32_t)pass};
            put(res, head, sizeof(head));
            put(res, &ret, sizeof(ret));
            const char *err = NULL;
            for (uint32_t i = 0; i < n; i++)
                if (A[i].kind == K_ERR)
                    err = A[i].err;
            const uint32_t elen = err ? (uint32_t)strlen(err) : ~0u;
            put(res, &elen, sizeof(elen));
            if (err)
                put(res, err, elen);
            for (uint32_t i = 0; i < n; i++) {
                if (A[i].kind == K_OUT && A[i].ptr)
                    put(res, A[i].ptr, (size_t)A[i].a);
                if (A[i].kind == K_OUTPTR) {
                    size_t len = 0;
                    for (uint32_t j = i + 1; j < n && !len; j++)
                        if (A[j].kind == K_OUTLEN)
                            len = A[j].out_len;
                    const uint64_t told = !ret && A[i].out ? (uint64_t)len : NONE;
                    put(res, &told, sizeof(told));
                    if (told != NONE)
                        put(res, A[i].out, len);
                    if (A[i].out) {
                        g_calls[H_FREE]++;
                        hydt_free(A[i].out);
                    }
                }
            }
            while (g_nowned)
                free(g_owned[--g_nowned]);
        }
    }
    if (at != image + size)
        die("the records file has bytes behind its last record");
    if (fclose(res))
        die("cannot write the results");
    FILE *rep = fopen(argv[3], "w");
    if (!rep)
        die("cannot open the report");
    for (int h = 0; h < H_COUNT; h++)
        fprintf(rep, "%s %lu\n", kNames[h], g_calls[h]);
    if (fclose(rep))
        die("cannot write the report");
    free(image);
    return 0;
}
