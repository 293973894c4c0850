/* streamclass.h — which of the runtime's hardware-queue pools a context's stream is created in (streamclass.c).
 * Host C with no GPU in it.  Internal. */
#ifndef HYD_STREAMCLASS_H
#define HYD_STREAMCLASS_H

#ifdef __cplusplus
extern "C" {
#endif

enum { HYD_STREAM_NORMAL = 0, HYD_STREAM_HIGH = 1, HYD_STREAM_LOW = 2 };

/* devices with a slot table of their own, and live contexts each table counts; a context beyond either is normal */
#define HYD_STREAM_DEVICES 64
#define HYD_STREAM_SLOTS 1024

/* the runtime's hardware queues per priority pool, from the text of GPU_MAX_HW_QUEUES: unset, empty, not a number or
 * below 1 -> 4 (HIP's default) */
int hyd_queue_pool_size(const char *env_value);

/* the class of the live_index-th context of a device whose pools hold `pool` queues each */
int hyd_stream_class(int live_index, int pool);

/* the lowest live index of `device` that no context holds, now held (-1: none left, or no such table), and its return */
int hyd_stream_slot_take(int device);
void hyd_stream_slot_release(int device, int live_index);

#ifdef __cplusplus
}
#endif

#endif
