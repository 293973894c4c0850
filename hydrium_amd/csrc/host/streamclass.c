/* streamclass.c — the placement rule of the contexts' own streams.
 *
 * The HIP runtime deals streams to hardware queues in rotation, and keeps one pool of queues PER STREAM PRIORITY (low,
 * normal, high), each capped at GPU_MAX_HW_QUEUES.  A hardware queue runs its kernels one after the other, so with the
 * runtime's default of four queues sixteen contexts have four kernels on the card at a time, and a queue that hosts the 32
 * wavefronts of a chain launch keeps three other contexts' transform kernels waiting.  Contexts beyond the first `pool`
 * are therefore created in the other priority classes: up to three times as many queues, by a plain HIP call, and no
 * change for a process with few contexts or for one that exports a queue count large enough to need none of it.
 * (profiles/stream_classes_ab.txt) */
#include "streamclass.h"

#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

/* classes in use, in the order they are dealt: all three.  Normal and high alone were measured beside it and lost:
 * 127.8 against 133.7 Gpixel/s on pools of four (profiles/stream_classes_ab.txt) */
#define HYD_STREAM_CLASSES 3

/* the test flavour of the library shows the four functions as they are, for tests without a device */
#ifdef HYD_TEST_HOOKS
#define HYD_SC_API __attribute__((visibility("default")))
#else
#define HYD_SC_API
#endif

HYD_SC_API int hyd_queue_pool_size(const char *env_value) {
    if (!env_value || !*env_value)
        return 4;
    char *end = NULL;
    const long v = strtol(env_value, &end, 10);
    if (end == env_value || v < 1)
        return 4;
    return v > 1 << 20 ? 1 << 20 : (int)v;
}

HYD_SC_API int hyd_stream_class(int live_index, int pool) {
    /* three pools of more than eight queues pass the 22-24 queues in use above which the firmware time-slices them;
     * a deployment that exports 20-22 keeps every stream normal */
    if (pool > 8 || pool < 1 || live_index < 0)
        return HYD_STREAM_NORMAL;
    return (live_index / pool) % HYD_STREAM_CLASSES; /* normal, high, low */
}

static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;
static uint64_t g_held[HYD_STREAM_DEVICES][HYD_STREAM_SLOTS / 64];

HYD_SC_API int hyd_stream_slot_take(int device) {
    int got = -1;
    if (device < 0 || device >= HYD_STREAM_DEVICES)
        return -1;
    pthread_mutex_lock(&g_lock);
    for (int w = 0; w < HYD_STREAM_SLOTS / 64 && got < 0; w++) {
        const uint64_t held = g_held[device][w];
        if (held == UINT64_MAX)
            continue;
        int b = 0;
        while (held >> b & 1)
            b++;
        g_held[device][w] = held | (uint64_t)1 << b;
        got = w * 64 + b;
    }
    pthread_mutex_unlock(&g_lock);
    return got;
}

HYD_SC_API void hyd_stream_slot_release(int device, int live_index) {
    if (device < 0 || device >= HYD_STREAM_DEVICES || live_index < 0 || live_index >= HYD_STREAM_SLOTS)
        return;
    pthread_mutex_lock(&g_lock);
    g_held[device][live_index / 64] &= ~((uint64_t)1 << (live_index % 64));
    pthread_mutex_unlock(&g_lock);
}
