/* streamclass_main.c — csrc/host/streamclass.c alone, as a stand-alone host program: the class table, the environment
 * parser, slot reuse, and eight threads taking and releasing slots.  tests/test_stream_class.py compiles it twice, with
 * -fsanitize=address,undefined and with -fsanitize=thread, and runs both.  Prints "ok". */
#include <pthread.h>
#include <stdatomic.h>
#include <stdio.h>

#include "streamclass.h"

static atomic_int owners[HYD_STREAM_SLOTS], twice;

static void *worker(void *arg) {
    (void)arg;
    for (int i = 0; i < 1000; i++) {
        const int a = hyd_stream_slot_take(1), b = hyd_stream_slot_take(1);
        if (a < 0 || b < 0 || atomic_fetch_add(&owners[a], 1) || atomic_fetch_add(&owners[b], 1))
            atomic_fetch_add(&twice, 1);
        atomic_fetch_sub(&owners[b], 1);
        hyd_stream_slot_release(1, b);
        atomic_fetch_sub(&owners[a], 1);
        hyd_stream_slot_release(1, a);
    }
    return NULL;
}

int main(void) {
    int bad = 0;
    static const char *const text[] = {NULL, "", "abc", "0", "-3", "4", "22"};
    static const int pools[] = {4, 4, 4, 4, 4, 4, 22};
    for (int i = 0; i < 7; i++)
        bad += hyd_queue_pool_size(text[i]) != pools[i];
    for (int i = 0; i < 64; i++) {
        bad += hyd_stream_class(i, 4) != (i / 4) % 3 || hyd_stream_class(i, 8) != (i / 8) % 3;
        bad += hyd_stream_class(i, 9) != 0 || hyd_stream_class(i, 22) != 0 || hyd_stream_class(i, 1) != i % 3;
    }
    bad += hyd_stream_class(-1, 4) != 0 || hyd_stream_class(3, 0) != 0;
    for (int i = 0; i < 5; i++)
        bad += hyd_stream_slot_take(0) != i;
    hyd_stream_slot_release(0, 1);
    hyd_stream_slot_release(0, 3);
    bad += hyd_stream_slot_take(0) != 1 || hyd_stream_slot_take(0) != 3 || hyd_stream_slot_take(0) != 5;
    bad += hyd_stream_slot_take(-1) != -1 || hyd_stream_slot_take(HYD_STREAM_DEVICES) != -1;
    hyd_stream_slot_release(0, -1); /* ignored, as a context that never got a slot hands back */
    hyd_stream_slot_release(0, HYD_STREAM_SLOTS);
    for (int i = 6; i < HYD_STREAM_SLOTS; i++) /* the table full: no slot, and the next context is normal */
        bad += hyd_stream_slot_take(0) != i;
    bad += hyd_stream_slot_take(0) != -1;
    hyd_stream_slot_release(0, 700);
    bad += hyd_stream_slot_take(0) != 700;
    pthread_t t[8];
    for (int i = 0; i < 8; i++)
        pthread_create(&t[i], NULL, worker, NULL);
    for (int i = 0; i < 8; i++)
        pthread_join(t[i], NULL);
    bad += atomic_load(&twice) != 0 || hyd_stream_slot_take(1) != 0;
    if (bad) {
        printf("%d checks failed\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
