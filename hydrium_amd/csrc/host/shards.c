/*
 * shards.c — the ONE closing stage of a frame whose LF groups sit on n >= 1 device contexts (shard d: slots[d] LF groups
 * in send order).  Per shard what the reference does per frame (encoder.c:928-957), with two crossings, both device-side:
 *     alphabet floor of shard d from shards 0 .. d-1 by peer read (entropy.c:459-460)  ->  hydamd_finish_frame per shard
 *     ->  every shard's blob as a view  ->  the assembling shard's stream waits for the others  ->  (checksums of the
 *     views, where written and where read)  ->  the assembler reads all blobs in place and writes the file into its HBM
 * hyd_shards_enqueue does that and returns; hyd_shards_wait syncs, sends the shards behind one that outgrew its buffers
 * (and reran inside its sync) round again, assembles again where a blob was stale or the file outgrew its buffer, verifies
 * the peer reads it chose to check and latches the pairs that passed.  The callers — encoder.c for hyd_send_tile's frames
 * (n = 1 included), multi.c for device-resident ones — describe the frame and act on the outcome.
 *
 * Two open matters now have this one home: the order the shards are synced in (the assembling shard last), and the error
 * paths' drains — they return while other shards hold enqueued work and the assembling stream may still read their views.
 */
#define _POSIX_C_SOURCE 200809L /* clock_gettime under -std=c99 */
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "shards.h"
#include "libhydrium/libhydrium.h"

static double now_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

int hyd_verify_peers_mode(void) {
    static int mode = -1;
    if (mode < 0) {
        const char *v = getenv("HYDAMD_VERIFY_PEERS");
        mode = !v || !*v ? VERIFY_FIRST_USE : *v == '0' ? VERIFY_NEVER : VERIFY_ALWAYS;
    }
    return mode;
}

/* has this pair been seen to read correctly (set: it has, from now on)?  Keys outside the table: never */
static int pair_ok(HydPairLatch *t, int reader, int owner, int set) {
    if (reader < 0 || owner < 0 || reader >= HYD_PAIR_KEYS || owner >= HYD_PAIR_KEYS)
        return 0;
    pthread_mutex_lock(&t->lock);
    const int ok = t->ok[reader][owner] |= set;
    pthread_mutex_unlock(&t->lock);
    return ok;
}

/* the assembling shard reads every other shard's view; shard d's floor kernel reads shards 0 .. d-1 */
void hyd_shards_choose_checks(HydShardFrame *f, int mode) {
    const int a = f->assembling;
    f->checking = 0;
    for (int d = 0; d < f->n; d++) {
        f->check_view[d] = d != a && mode != VERIFY_NEVER && (mode == VERIFY_ALWAYS || !pair_ok(f->latch, f->key[a], f->key[d], 0));
        f->check_floor[d] = 0;
        for (int p = 0; p < d; p++)
            f->check_floor[d] |= mode != VERIFY_NEVER && (mode == VERIFY_ALWAYS || !pair_ok(f->latch, f->key[d], f->key[p], 0));
        f->checking |= f->check_view[d] | f->check_floor[d];
    }
}

/* every peer read this frame checked was seen to return what its owner wrote: those pairs are trusted from here on */
void hyd_shards_latch(const HydShardFrame *f) {
    for (int d = 0; d < f->n; d++) {
        if (f->check_view[d])
            pair_ok(f->latch, f->key[f->assembling], f->key[d], 1);
        for (int p = 0; p < d && f->check_floor[d]; p++)
            pair_ok(f->latch, f->key[d], f->key[p], 1);
    }
}

static int attempts(int n) { return n > 1 ? 4 + 2 * n : 4; } /* every shard may rerun once and send the later ones round again */

/* the blobs are views: the file's size comes from the contexts' capacities plus what the assembler itself adds per LF group
 * (head bits, TOC entries) and per frame (prefix, HFGlobal); should a frame still exceed it, the assembler says how many bytes
 * it needs and the frame is assembled again into a buffer of that size */
static size_t output_bound(const HydShardFrame *f) {
    size_t groups = 0, cap = 256u << 10;
    for (int d = 0; d < f->n; d++) {
        groups += f->slots[d];
        cap += hydamd_blob_bound(f->ctx[d], (int)f->slots[d]);
    }
    return cap + 4096 * groups;
}

static int done(HydShardOutcome *o, int kind, int code, int shard, const char *msg) {
    o->kind = kind;
    o->code = code;
    o->shard = shard;
    o->msg = msg;
    return kind;
}
#define DEVICE_TRY(call, d, what)                                                   \
    for (const int st_ = (call); st_;)                                              \
        return done(o, SHARDS_DEVICE, st_, (d), (what)) /* shard d's context holds the detail */

/* every shard's view, the assembling shard waiting for the others, the checksums, the assembly itself */
static int assemble(HydShardFrame *f, HydShardOutcome *o) {
    const int a = f->assembling;
    const void *blob[HYDAMD_MAX_PEERS];
    size_t cap[HYDAMD_MAX_PEERS];
    for (int d = 0; d < f->n; d++)
        DEVICE_TRY(hydamd_export_frame_owned(f->ctx[d], (int)f->slots[d], &blob[d], &cap[d]), d, "export");
    for (int d = 0; d < f->n; d++) /* the assembling GPU's stream waits for the other shards' exports and may read their memory */
        if (d != a)
            DEVICE_TRY(hydamd_wait_for(f->ctx[a], f->ctx[d]), a, "cross-device wait");
    for (int d = 0; d < f->n; d++)
        if (f->check_view[d]) { /* summed where it was written and where it is about to be read */
            DEVICE_TRY(hydamd_verify_enqueue(f->ctx[d], f->ctx[d], (int)f->slots[d], 0), d, "checksum on the owning device");
            DEVICE_TRY(hydamd_verify_enqueue(f->ctx[a], f->ctx[d], (int)f->slots[d], d), a, "checksum through peer reads");
        }
    HydAmdAssembler *as = hydamd_context_assembler(f->ctx[a]);
    const int st = hydamd_assembler_run(as, blob, cap, hydamd_get_stream(f->ctx[a]), NULL, f->out_cap);
    return st ? done(o, SHARDS_DEVICE, st, a, hydamd_assembler_error(as)) : 0;
}

int hyd_shards_enqueue(HydShardFrame *f, HydShardOutcome *o) {
    const int a = f->assembling;
    memset(o, 0, sizeof(*o));
    f->t0 = now_ms();
    hyd_shards_choose_checks(f, hyd_verify_peers_mode());
    for (int d = 1; d < f->n; d++) /* shard d's tables start from the maximum over shards 0 .. d-1 (entropy.c:459-460) */
        DEVICE_TRY(hydamd_alphabet_floor_from_peers(f->ctx[d], d, f->ctx), d, "alphabet floor from the earlier shards");
    for (int d = 0; d < f->n; d++) {
        DEVICE_TRY(hydamd_finish_frame(f->ctx[d], (int)f->slots[d]), d, "closing stage");
        f->reruns[d] = hydamd_overflow_reruns(f->ctx[d]);
    }
    HydAmdAssembler *as = hydamd_context_assembler(f->ctx[a]);
    if (!as)
        return done(o, SHARDS_DEVICE, HYD_INTERNAL_ERROR, a, "frame assembler could not be created");
    const int st = hydamd_assembler_plan(as, f->md, f->write_header, 1, (size_t)f->n, f->slots, f->lf_ids, NULL, 0);
    if (st) /* once per frame: what is assembled again is the same frame */
        return done(o, SHARDS_PLAN, st, a, hydamd_assembler_error(as));
    if (!f->out_cap)
        f->out_cap = output_bound(f);
    return assemble(f, o);
}

/* f's peer reads against what their owners hold; -> 0, or the outcome that ends the frame */
static int verify(HydShardFrame *f, HydShardOutcome *o) {
    const int a = f->assembling;
    for (int d = 0; d < f->n; d++) {
        if (f->check_floor[d]) {
            int ok = 0;
            DEVICE_TRY(hydamd_verify_floor(f->ctx[d], d, f->ctx, &ok), d, "floor verification");
            if (!ok) {
                o->reader = d, o->owner = -1, o->is_floor = 1;
                return done(o, SHARDS_MISMATCH, HYD_INTERNAL_ERROR, d, "peer read mismatch");
            }
        }
        if (f->check_view[d]) {
            unsigned long long written = 0, seen = 0;
            DEVICE_TRY(hydamd_verify_read(f->ctx[d], 0, &written), d, "view verification");
            DEVICE_TRY(hydamd_verify_read(f->ctx[a], d, &seen), a, "view verification");
            if (written != seen) {
                o->reader = a, o->owner = d, o->is_floor = 0;
                return done(o, SHARDS_MISMATCH, HYD_INTERNAL_ERROR, d, "peer read mismatch");
            }
        }
    }
    return 0;
}

int hyd_shards_wait(HydShardFrame *f, HydShardOutcome *o) {
    const int a = f->assembling, n = f->n;
    HydAmdAssembler *as = hydamd_context_assembler(f->ctx[a]);
    memset(o, 0, sizeof(*o));
    for (int attempt = 0; attempt < attempts(n); attempt++) {
        const int last = attempt + 1 == attempts(n);
        for (int k = 1; k <= n; k++) { /* a shard whose frame outgrew its buffers reruns it in here: its blob is then stale */
            const int d = (a + k) % n; /* the assembling shard last: its stream carries the assembly */
            DEVICE_TRY(hydamd_sync(f->ctx[d]), d, "shard");
        }
        /* a shard that reran its frame had left PARTIAL alphabet maxima the first time (a group that runs out of token
         * space stops counting): the later shards read their floor from those.  They read it again and run again. */
        int stale_from = 0;
        for (int d = 0; d < n; d++) {
            const unsigned now = hydamd_overflow_reruns(f->ctx[d]);
            if (now != f->reruns[d] && !stale_from && d + 1 < n)
                stale_from = d + 1;
            f->reruns[d] = now;
        }
        size_t size = 0;
        int again = stale_from != 0;
        const char *asm_failed = NULL;
        for (int d = stale_from; again && !last && d < n; d++) {
            DEVICE_TRY(hydamd_alphabet_floor_from_peers(f->ctx[d], d, f->ctx), d, "replay behind a rerun shard");
            DEVICE_TRY(hydamd_replay_frame(f->ctx[d]), d, "replay behind a rerun shard");
        }
        if (!again) {
            o->hot_ms = now_ms() - f->t0;
            const int st = hydamd_assembler_result(as, &size);
            const char *e = st ? hydamd_assembler_error(as) : NULL;
            if (st == HYD_NEED_MORE_OUTPUT && size > f->out_cap) {
                f->out_cap = size;
                again = 1;
            } else if (e && strstr(e, "incomplete")) { /* a blob of a shard that reran: its results are exported again */
                again = 1;
            } else if (e && strstr(e, "NaN")) { /* the caller's input, whatever the peer reads did */
                return done(o, SHARDS_NAN, HYD_API_ERROR, a, "Invalid NaN Float");
            } else if (st) {
                asm_failed = e ? e : "GPU frame assembly failed";
                if (!f->checking)
                    return done(o, SHARDS_ASSEMBLY, st < HYD_ERROR_START ? st : HYD_INTERNAL_ERROR, a, asm_failed);
                /* else an assembler that may have read garbage through a bad peer mapping: the checks name the pair */
            }
        }
        if (again) {
            if (!last && assemble(f, o))
                return o->kind;
            continue;
        }
        if (f->checking) {
            const double tv = now_ms();
            if (verify(f, o))
                return o->kind;
            o->verify_ms = now_ms() - tv;
            if (asm_failed) /* the peer reads were fine: the assembly failed for a reason of its own */
                return done(o, SHARDS_ASSEMBLY, HYD_INTERNAL_ERROR, a, asm_failed);
            hyd_shards_latch(f);
        }
        o->size = size;
        return SHARDS_OK;
    }
    return done(o, SHARDS_NO_FIT, HYD_INTERNAL_ERROR, a, "frame still does not fit after enlarging its buffers");
}

#ifdef HYD_TEST_HOOKS
/* the choice of checks and the latching, on a table of the hook's own (CPU only): one image of n shards with `keys`;
 * -> the ordered pairs latched so far.  reset: forget them first; latch: the image passed its checks */
__attribute__((visibility("default"))) int hydt_shard_checks(int reset, int mode, int n, const int *keys, int assembling, int latch,
                                                             int *check_view, int *check_floor) {
    static HydPairLatch table = HYD_PAIR_LATCH_INIT;
    HydShardFrame f = {.n = n, .assembling = assembling, .latch = &table};
    int pairs = 0;
    if (n < 1 || n > HYDAMD_MAX_PEERS)
        return -1;
    if (reset)
        memset(table.ok, 0, sizeof(table.ok));
    memcpy(f.key, keys, (size_t)n * sizeof(*keys));
    hyd_shards_choose_checks(&f, mode);
    memcpy(check_view, f.check_view, (size_t)n * sizeof(*check_view));
    memcpy(check_floor, f.check_floor, (size_t)n * sizeof(*check_floor));
    if (latch)
        hyd_shards_latch(&f);
    for (int r = 0; r < HYD_PAIR_KEYS; r++)
        for (int w = 0; w < HYD_PAIR_KEYS; w++)
            pairs += table.ok[r][w];
    return pairs;
}
#endif
