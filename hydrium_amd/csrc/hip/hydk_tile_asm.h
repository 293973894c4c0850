/*
 * hydk_tile_asm.h — private interface between the host side of device-resident tile-mode images (csrc/host/tiled.c,
 * C99) and the device-side tile assembler (csrc/hip/assemble_tiles.hip), which includes it too: a prototype that drifts
 * from its definition does not compile.  Nothing here is exported from the library.
 */
#ifndef HYD_TILE_ASM_H_
#define HYD_TILE_ASM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct HydkTileAsm HydkTileAsm;

/* all int results are HYDStatusCode-compatible; hydk_tiles_error() describes the last failure */
/* scratch for launch groups of up to `max_frames` frames; the plan (hydk_tiles.h) is copied to the device */
int hydk_tiles_create(int device, int max_frames, const void *plan, size_t plan_bytes, HydkTileAsm **out);
void hydk_tiles_destroy(HydkTileAsm *a);
const char *hydk_tiles_error(HydkTileAsm *a);
/* enqueue the assembly of frames [first_frame, first_frame + frames) of the plan on `stream`, behind whatever fills the
 * view `blob` and its extents; first_group: the file starts here */
int hydk_tiles_run(HydkTileAsm *a, uint32_t first_frame, uint32_t frames, const void *blob, const void *extents, int first_group, void *stream);
/* after the stream has been synchronised: the device's error word (HYDK_ASM_E_*), the bytes of the file behind this
 * group, and the bytes the output buffer must hold for it */
int hydk_tiles_result(HydkTileAsm *a, uint32_t *err, uint64_t *file_bytes, uint64_t *needed);
/* the output buffer holds at least `bytes`; its first `keep` bytes survive a move, which waits for `stream` */
int hydk_tiles_reserve(HydkTileAsm *a, uint64_t bytes, uint64_t keep, void *stream);
const uint8_t *hydk_tiles_out(HydkTileAsm *a);
uint64_t hydk_tiles_out_capacity(HydkTileAsm *a);
int hydk_tiles_wait(HydkTileAsm *a, void *stream);
int hydk_tiles_read(HydkTileAsm *a, uint8_t *dst, size_t n);
/* free device memory right now (what an object holds = the difference around its creation) */
uint64_t hydk_tiles_device_free(int device);

#ifdef __cplusplus
}
#endif

#endif /* HYD_TILE_ASM_H_ */
