/* shards.h — the closing stage of a frame whose LF groups sit on n >= 1 device contexts (shards.c).  Internal. */
#ifndef HYD_SHARDS_H
#define HYD_SHARDS_H

#include <pthread.h>

#include "hydrium_amd.h"

/* HYDAMD_VERIFY_PEERS: unset = peer reads are checked at first use of a pair, 1 = on every frame, 0 = never */
enum { VERIFY_NEVER = 0, VERIFY_ALWAYS = 1, VERIFY_FIRST_USE = 2 };
int hyd_verify_peers_mode(void);

/* peer reads seen to return what their owner wrote: ok[reading key][owning key].  What a key is belongs to the table's
 * user; a key outside the table is never known and never latched, so its reads are checked every time */
#define HYD_PAIR_KEYS 16
typedef struct HydPairLatch {
    pthread_mutex_t lock;
    unsigned char ok[HYD_PAIR_KEYS][HYD_PAIR_KEYS];
} HydPairLatch;
#define HYD_PAIR_LATCH_INIT {PTHREAD_MUTEX_INITIALIZER, {{0}}}

typedef struct HydShardFrame {
    /* the frame, from the caller */
    int n, assembling;  /* shards; the one whose device assembles the file */
    int write_header;
    HydAmdContext *ctx[HYDAMD_MAX_PEERS];
    uint32_t slots[HYDAMD_MAX_PEERS]; /* LF groups per shard, in send order across the shards */
    int key[HYDAMD_MAX_PEERS];        /* each shard's key in `latch` */
    HydPairLatch *latch;
    const HYDImageMetadata *md;
    const uint32_t *lf_ids; /* raster id of every LF group, in send order */
    size_t out_cap;         /* 0: hyd_shards_enqueue sets the bound; a frame that needs more grows it */
    /* this frame's state, the closer's */
    unsigned reruns[HYDAMD_MAX_PEERS];
    int check_view[HYDAMD_MAX_PEERS], check_floor[HYDAMD_MAX_PEERS], checking;
    double t0;
} HydShardFrame;

enum {
    SHARDS_OK = 0,
    SHARDS_NAN,       /* the caller's samples */
    SHARDS_MISMATCH,  /* a peer read did not return what its owner wrote */
    SHARDS_PLAN,      /* the assembler rejected the frame's description: code, msg = its message */
    SHARDS_ASSEMBLY,  /* the assembler failed on the frame: code, msg = its message */
    SHARDS_DEVICE,    /* a device call failed: shard (its context holds the detail), code, msg = the step */
    SHARDS_NO_FIT
};
typedef struct HydShardOutcome {
    int kind, code; /* code: the HYDStatusCode that goes with kind */
    size_t size;    /* SHARDS_OK: bytes of the file in the assembling device's memory */
    int shard;      /* SHARDS_DEVICE: the failing shard.  SHARDS_MISMATCH: the shard whose floor or view was misread, ... */
    int reader, owner, is_floor; /* ... the reading shard, the owning one (-1: the earlier shards), and which read it was */
    const char *msg;
    double hot_ms, verify_ms; /* > 0: the hot path was done that long after enqueue / this frame's peer reads were verified */
} HydShardOutcome;

/* which of the frame's peer reads are checked (-> f->check_view, check_floor, checking), and the latching of those
 * after a frame that passed */
void hyd_shards_choose_checks(HydShardFrame *f, int mode);
void hyd_shards_latch(const HydShardFrame *f);

/* floors, closing stage per shard, views, waits, checksums, the assembler: everything enqueued, nothing waited for */
int hyd_shards_enqueue(HydShardFrame *f, HydShardOutcome *o);
/* waits; reruns and re-assembles what a shard that outgrew its buffers invalidated; verifies; latches.  -> o->kind */
int hyd_shards_wait(HydShardFrame *f, HydShardOutcome *o);

#endif
