/*
 * hydrium_amd.h — additive C-ABI of the MI355X build of libhydrium (not present in the reference).
 *
 * The drop-in boundary is include/libhydrium/libhydrium.h (the reference's nine hyd_* functions).
 * The functions below expose the layer underneath it — the HIP hot path of one LF group at a
 * time — so that callers which already hold pixels in HBM (bench.py, multi-GPU sharding, a video
 * pipeline) can skip the host-pointer API the reference's hyd_send_tile imposes
 * (reference src/include/libhydrium/libhydrium.h:260-262, SURVEY.md §8b "additive extension").
 *
 * One HydAmdContext drives one GPU through one HIP stream.  All calls are asynchronous with
 * respect to the GPU unless stated; hydamd_sync() is the only blocking point.  Plain pointers and
 * sizes only: no C++ or torch types cross this boundary.
 *
 * What each call replaces in the reference (file:line relative to /root/reference/src/libhydrium/):
 *   hydamd_encode_lf_group*   hyd_populate_xyb_buffer (format.c:142), forward_dct (encoder.c:631),
 *                             the HF quantiser (encoder.c:783-823), the LF ints of write_lf_group
 *                             (encoder.c:573,582), initialize_hf_coeffs (encoder.c:689),
 *                             hyd_ans_prepare_frequencies (entropy.c:943) and the per-group
 *                             hyd_ans_write_stream_symbols loop (encoder.c:940-950, entropy.c:1064)
 *   hydamd_finish_frame       the byte-padding + concatenation of encoder.c:973-981
 *   (LF coder, on by default) the LF-coefficient stream of write_lf_group (encoder.c:560-596) with its
 *                             LZ77-as-RLE symbol buffering (entropy.c:473-524), Huffman code construction
 *                             (entropy.c:577-707) and symbol write-out (entropy.c:1003-1021)
 */
#ifndef HYDRIUM_AMD_H_
#define HYDRIUM_AMD_H_

#include <stddef.h>
#include <stdint.h>

#include "libhydrium/libhydrium.h"

#if defined(__GNUC__) || defined(__clang__)
#define HYDAMD_EXPORT __attribute__((visibility("default")))
#else
#define HYDAMD_EXPORT
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define HYDAMD_MAX_CLUSTERS 9      /* clusters owned by one preset */
#define HYDAMD_ALPHABET 128        /* row pitch of the frequency tables */
#define HYDAMD_GROUPS_PER_LFG 64   /* group slots per LF group (8 x 8) */
#define HYDAMD_MAX_LF_GROUPS 255   /* the reference cannot code 256 presets (entropy.c:99) */

typedef struct HydAmdContext HydAmdContext;

#define HYDAMD_LF_CODES 384        /* compact token space of the LF-coefficient stream: [0,256) literals, [256,384) token 16384 + (i - 256) */

/* Kernel classes timed by the optional profiler. */
enum { HYDAMD_K_TRANSFORM = 0, HYDAMD_K_TABLES = 1, HYDAMD_K_RANS = 2, HYDAMD_K_PACK = 3, HYDAMD_K_LF = 4, HYDAMD_K_COUNT = 5 };

/* Number of usable HIP devices (0 when there is none; never fails). */
HYDAMD_EXPORT int hydamd_device_count(void);

/* memcpy on the library's staging threads (HYDAMD_STAGE_THREADS) for moves of several megabytes; plain memcpy below 4 MB */
HYDAMD_EXPORT void hydamd_host_copy(void *dst, const void *src, size_t n);

/*
 * Create a context on `device` with room for `max_lf_groups` LF groups in flight (one frame's
 * worth: every LF group of a one-frame image, or 1 for tile mode).  `linear_light` selects the
 * input transfer LUTs (HYDImageMetadata.linear_light).  `debug_planes` != 0 additionally
 * allocates the XYB / DCT / quantised dump planes used by the parity tests.
 * Returns NULL on failure; *status (if non-NULL) receives a HYDStatusCode-compatible value and
 * hydamd_error(NULL) a description.
 */
HYDAMD_EXPORT HydAmdContext *hydamd_create(int device, int max_lf_groups, int linear_light, int debug_planes, int *status);
HYDAMD_EXPORT void hydamd_destroy(HydAmdContext *ctx);
HYDAMD_EXPORT const char *hydamd_error(HydAmdContext *ctx);

/* Run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL restores the context's own. */
HYDAMD_EXPORT int hydamd_set_stream(HydAmdContext *ctx, void *hip_stream);
HYDAMD_EXPORT void *hydamd_get_stream(HydAmdContext *ctx);
/* The hardware-queue pool of the context's own stream: 0 normal, 1 high, 2 low stream priority.  The HIP runtime keeps
 * GPU_MAX_HW_QUEUES queues per priority; with 8 or fewer (its default is 4) a device's live contexts are dealt to the
 * pools GPU_MAX_HW_QUEUES at a time (normal, high, low, normal, ...), so that more of them can have a kernel on the card
 * at once; with more than 8 every context is normal.  A caller's own stream (hydamd_set_stream) is never touched. */
HYDAMD_EXPORT int hydamd_stream_class(const HydAmdContext *ctx);

/* 1 if K1 evaluates the format.c LUTs in registers (verified bit-exact at creation), 0 if it gathers from them. */
HYDAMD_EXPORT int hydamd_uses_register_luts(HydAmdContext *ctx);
/* Force the LUT-gather (1) or register (0) variant; for A/B measurements. */
HYDAMD_EXPORT int hydamd_force_luts(HydAmdContext *ctx, int use_luts);
/* XYB evaluation mode of the integer pixel path: 0 registers with v_rcp + one fused Newton step,
 * 1 registers with IEEE division, 2 LUT gathers.  Only modes that reproduced all 65536 LUT entries
 * bit for bit in the creation-time self-test can be selected; the fastest such mode is the default. */
HYDAMD_EXPORT int hydamd_xyb_mode(HydAmdContext *ctx);
HYDAMD_EXPORT int hydamd_set_xyb_mode(HydAmdContext *ctx, int mode);

/* One of a pixel's six transfer / bias curves is read from the uploaded table through the texture path instead of being
 * evaluated in registers (the values are the reference's own table entries either way): faster for photographic and smooth
 * content, slower for pixels that scatter over the whole table (noise).  0 (default): decided per frame from the density
 * of the frame this context finished last (more than 0.75 bytes of HF sections per pixel: registers); 1: always gather
 * (rounds 1-4); 2: never. */
HYDAMD_EXPORT int hydamd_set_curve_gathers(HydAmdContext *ctx, int mode);
/* The density the default choice goes by is that of the last frame hydamd_sync waited for on this context (bytes and pixels
 * of ONE frame, taken together); hydamd_forget_content clears it — what the drop-in API does when it takes a parked context
 * for another image. */
HYDAMD_EXPORT int hydamd_forget_content(HydAmdContext *ctx);

/* Form of the entropy (rANS) stage.  The recurrence is serial per group, so the forms trade the
 * latency of one frame against how much of the GPU the stage occupies while it runs:
 *   4   one wavefront per group, 4 groups per workgroup (default): lowest single-frame latency
 *   5   one LANE per group: a single wavefront walks the 64 chains of an LF group and a second, wave-
 *       parallel kernel writes the bits straight into the payload; a fifteenth of the instructions and
 *       a sixty-fourth of the wavefronts of form 4 — best when many frames are in flight.  LF groups
 *       with float samples are still coded by form 4.
 *   6   (rounds 3-4: form 5 with its coding tables packed into a byte and a nibble plane, 62 KB of LDS per chain
 *       instead of 80.)  Since round 5 the lane form's tables are sized by the frame's clustering scheme (9 / 3 / 2 / 1
 *       clusters per preset: 79.5 / 26.5 / 17.7 / 8.8 KB) and its step is hand-scheduled; packed and plain tables measured
 *       equal in a pipelined loop, so the packed variant is gone and 6 is accepted as another name of 5.
 * Integer frames: forms 4 and 5 both leave the bits to a second, wave-parallel kernel (k_rans_emit); float frames are
 * coded by form 4's self-emitting variant.
 * Round 1's row forms 1-3 are gone: asking for one of them (here or through HYDAMD_RANS_WAVES) selects
 * form 5, which replaced them, and says so once on stderr. */
HYDAMD_EXPORT int hydamd_set_rans_waves(HydAmdContext *ctx, int waves);

/* Start a frame of `num_presets` presets (= LF groups, at most 255): clears histograms and the running alphabet. */
HYDAMD_EXPORT int hydamd_begin_frame(HydAmdContext *ctx, unsigned num_presets);

/*
 * Half-precision DEVICE pixels: two sample formats beside the drop-in API's HYD_UINT8 (0), HYD_UINT16 (1) and
 * HYD_FLOAT32 (2), which include/libhydrium/libhydrium.h keeps as the reference has them.  What a network or a GPU image
 * pipeline leaves in device memory goes in as it is, without a float32 copy.
 *   HYDAMD_FLOAT16   IEEE binary16 (torch.float16)
 *   HYDAMD_BFLOAT16  bfloat16: the upper half of a float32 (torch.bfloat16)
 * A sample is 2 bytes and strides stay in samples.  The file is byte for byte what the reference writes for the same
 * picture given as HYD_FLOAT32 with every sample widened exactly (both widenings are lossless).  A non-finite sample
 * (binary16 exponent 31, bfloat16 exponent 255) is what a non-finite float32 sample is: "Invalid NaN Float" for the frame
 * or batch, or that image's HYDAMD_IMAGE_BAD_SAMPLE under hydamd_*_set_image_errors.
 * Accepted wherever a sample_fmt names device pixels: hydamd_encode_lf_group, hydamd_encode_image,
 * hydamd_encode_image_batch, hydamd_encode_batch, hydamd_encode_mixed, hydamd_encode_mixed_formats,
 * hydamd_encode_image_tiled, hydamd_encode_image_multi and hydamd_debug_transform_footprint.  Entry points that read HOST
 * pointers — hyd_send_tile, hydamd_encode_lf_group_host — refuse both with "Invalid Sample Format", as they and every
 * other entry point refuse anything that is neither 0..4 nor of the NV12 family (16..19, 32..35, 48..51, below) nor of the
 * P010 / P012 / P016 family (80..83, 96..99, 112..115, 144..147, 160..163, 176..179, 208..211, 224..227, 240..243, below)
 * nor of the planar YCbCr family (512..523, 528..535, 544..551, below) nor of the planar YCbCr family of 16-bit words
 * (2112..2151, 2176..2215, 2240..2279 less the planar family's gaps, below).
 */
#define HYDAMD_FLOAT16 3
#define HYDAMD_BFLOAT16 4

/*
 * NV12 DEVICE pixels: what a hardware video or JPEG decoder leaves in device memory — a full-resolution 8-bit Y plane and a
 * half-resolution plane of interleaved U, V pairs (YCbCr 4:2:0) — read by the transform kernel as it is, without an RGB
 * copy.  Four formats, by matrix and range:
 *   HYDAMD_NV12_BT709       BT.709 matrix, limited range (Y 16..235, U and V 16..240): HD video
 *   HYDAMD_NV12_BT709_FULL  BT.709 matrix, full range
 *   HYDAMD_NV12_BT601       BT.601 matrix, limited range: SD video
 *   HYDAMD_NV12_BT601_FULL  BT.601 matrix, full range: what a JPEG decoder leaves (JFIF)
 * (the numbers start at 16: 5..15, 20..31, 36..47, 52..79 and whatever else no section here names stay "Invalid Sample
 * Format"; 32..35 and 48..51 are the same pictures with interpolated chroma, 80 and up in 16-bit words, both further down).
 *
 * The file is byte for byte what the reference writes for the HYD_UINT8 picture this conversion produces.  For pixel (x, y):
 * Y = luma[y][x]; U, V = the chroma pair at (x >> 1, y >> 1) (nearest neighbour: every 2 x 2 block shares one pair);
 * c = Y - yo, d = U - 128, e = V - 128 in 32-bit integers, >> an arithmetic shift:
 *   R = clamp((cy*c         + crv*e + 8192) >> 14, 0, 255)
 *   G = clamp((cy*c - cgu*d - cgv*e + 8192) >> 14, 0, 255)
 *   B = clamp((cy*c + cbu*d         + 8192) >> 14, 0, 255)
 *                 yo     cy    crv    cgu    cgv    cbu
 *   BT709         16  19077  29372   3494   8731  34610
 *   BT709_FULL     0  16384  25802   3069   7670  30402
 *   BT601         16  19077  26149   6419  13320  33050
 *   BT601_FULL     0  16384  22970   5638  11700  29032
 * — round(v * 2^14) of the real coefficients; within 0.51 of the clamped real-valued conversion for every (Y, U, V).
 *
 * How an NV12 picture is named, wherever a sample_fmt names device pixels (the list above) and in sample_fmts[k] of
 * hydamd_encode_mixed_formats:
 *   src[0]        the first Y sample of the picture or LF group
 *   src[1]        the first U sample of its chroma row 0;  src[2] must equal src[1] + 1
 *   pixel_stride  must be 1
 *   row_stride    the pitch in bytes of BOTH planes, as NV12 defines it; may be negative.  Width and height may be odd: the
 *                 chroma plane then holds ceil(w / 2) x ceil(h / 2) pairs, a chroma row 2 * ceil(w / 2) bytes.
 * A bad src[2] or pixel_stride is HYD_API_ERROR "NV12 wants pixel_stride 1 and V one byte behind U", nothing enqueued.
 * The library finds an LF group, tile or shard at pixel (x0, y0) at src[0] + y0 * row_stride + x0 and
 * src[1] + (y0 / 2) * row_stride + x0; its own origins are multiples of 256.  A caller's own crop (a HydAmdImageDesc, or an
 * LF group given to hydamd_encode_lf_group) must start on EVEN coordinates x0, y0 of the surface, or its pixels meet
 * their neighbours' chroma: this cannot be checked.
 * Entry points that read HOST pointers — hyd_send_tile, hydamd_encode_lf_group_host — refuse all four with "Invalid
 * Sample Format".
 * Out of scope: NV21; host-pointer NV12; any colour description other than the four above.
 * (10- to 16-bit P010 / P012 / P016 have a fixed-point derivation and formats of their own, further down; so have planar
 * I420, I422 and I444.)
 */
#define HYDAMD_NV12_BT709 16
#define HYDAMD_NV12_BT709_FULL 17
#define HYDAMD_NV12_BT601 18
#define HYDAMD_NV12_BT601_FULL 19

/*
 * NV12 with INTERPOLATED chroma: sample_fmt = 16 + matrix + 16 * filter.  Filter 0 is the nearest-neighbour family above;
 *   HYDAMD_NV12C_* (32..35)  centre-sited: the chroma sample sits in the middle of its 2 x 2 luma block (JPEG / JFIF, MPEG-1)
 *   HYDAMD_NV12L_* (48..51)  left-sited: co-sited with even luma columns, midway between two luma rows (MPEG-2, and
 *                            chroma_sample_loc_type 0: the default of H.264, HEVC and most AV1)
 * with the four matrices in the same order.  Layout, strides, odd sizes, negative pitch and the layout error are NV12's.
 *
 * The file is byte for byte what the reference writes for the HYD_UINT8 picture this produces.  The PICTURE is W x H with a
 * chroma plane of cw = ceil(W / 2) by ch = ceil(H / 2) pairs.  For pixel (x, y) in picture coordinates: cx = x >> 1,
 * cy = y >> 1, vy = clamp(cy + (y odd ? 1 : -1), 0, ch - 1), and for U and V separately, C the component's plane:
 *   centre, hx = clamp(cx + (x odd ? 1 : -1), 0, cw - 1):
 *       C' = (9*C[cy][cx] + 3*C[cy][hx] + 3*C[vy][cx] + C[vy][hx] + 8) >> 4
 *   left, x even:  C' = (3*C[cy][cx] + C[vy][cx] + 2) >> 2
 *   left, x odd, hx = min(cx + 1, cw - 1):
 *       C' = (3*(C[cy][cx] + C[cy][hx]) + C[vy][cx] + C[vy][hx] + 4) >> 3
 * then R, G, B from Y[y][x], U', V' exactly as above.
 *
 * Clamping is at the edges of the PICTURE, not of an LF group or tile: inside a picture an LF group or tile reads its
 * neighbours' chroma, and nothing is ever read outside the picture's chroma rows 0 ... ch - 1, bytes 0 ... 2 * cw - 1, or its
 * Y rectangle.  A picture is what the caller names: the image of hydamd_encode_image, hydamd_encode_image_batch and
 * hydamd_encode_batch; each HydAmdImageDesc of hydamd_encode_mixed* (a crop of a larger surface is a picture: its edges
 * replicate although real neighbours exist in memory); the whole image of hydamd_encode_image_tiled (tiles are frames, the
 * chroma is continuous across them).  hydamd_encode_lf_group_at names the picture of one LF group; plain
 * hydamd_encode_lf_group treats the LF group as a picture of its own.
 *
 * Refused: hydamd_encode_image_multi ("interpolated chroma is not sharded: ..." — a shard's buffer is only promised to hold
 * its own rows, and the filter would read a neighbouring shard's chroma row), and the host-pointer entry points as for NV12.
 * Out of scope: top-left siting (BT.2020), other two-plane layouts (NV21, NV16), cross-shard chroma, host-pointer input.
 * (Planar I420 and I422 take the same two filters: HYDAMD_I420C_* ... further down.)
 */
#define HYDAMD_NV12C_BT709 32
#define HYDAMD_NV12C_BT709_FULL 33
#define HYDAMD_NV12C_BT601 34
#define HYDAMD_NV12C_BT601_FULL 35
#define HYDAMD_NV12L_BT709 48
#define HYDAMD_NV12L_BT709_FULL 49
#define HYDAMD_NV12L_BT601 50
#define HYDAMD_NV12L_BT601_FULL 51

/*
 * P010 / P012 / P016 DEVICE pixels: what a hardware decoder leaves for anything deeper than 8 bits (HEVC Main10, 10-bit AV1
 * and VP9, 12-bit profiles) — NV12's two planes in 16-bit WORDS, the significant bits MSB-aligned (10 bits with 6 low bits
 * zero, 12 with 4) — read by the transform kernel as they are, without an RGB16 copy.
 *   sample_fmt = 16 + matrix + 16 * filter + 64 * depth
 * matrix 0..3 and filter 0..2 as in the NV12 family (depth 0, whose numbers do not change); depth 1, 2, 3 = 10, 12, 16
 * significant bits:
 *                    nearest     centre (..C_)   left (..L_)
 *   HYDAMD_P010_*    80..83       96..99         112..115
 *   HYDAMD_P012_*   144..147     160..163        176..179
 *   HYDAMD_P016_*   208..211     224..227        240..243
 * 64..79, and every number in between that the table leaves out, stay "Invalid Sample Format".
 *
 * The file is byte for byte what the reference writes for the HYD_UINT16 picture this conversion produces.  U, V of a pixel
 * are the pair at (x >> 1, y >> 1), or U', V' by the taps of the section above on 16-bit samples (clamped at the PICTURE's
 * edges and continuous across LF groups and tiles, as there); then with the 16-bit words AS STORED — low bits are not masked,
 * so a surface that carries noise below its depth is read as it stands —
 *   c = Y - yo, d = U - 32768, e = V - 32768
 *   R = clamp((cy*c         + crv*e + 2^19) >> 20, 0, 65535)
 *   G = clamp((cy*c - cgu*d - cgv*e + 2^19) >> 20, 0, 65535)
 *   B = clamp((cy*c + cbu*d         + 2^19) >> 20, 0, 65535)
 * in 64-bit two's complement, >> an arithmetic shift.  The coefficients are floor(v * 2^20 + 0.5) of cy = sy, crv = 2(1-Kr) sc,
 * cbu = 2(1-Kb) sc, cgu = 2(1-Kb) Kb/Kg sc, cgv = 2(1-Kr) Kr/Kg sc (Kr, Kb = 0.2126, 0.0722 or 0.299, 0.114; Kg = 1 - Kr - Kb).
 * Limited range, at every depth (the standards scale the range with the depth, so MSB-aligned words need no depth):
 * yo = 4096, sy = 65535 / (219 * 256), sc = 65535 / (224 * 256).  Full range: yo = 0, sy = sc = 65535 / ((2^n - 1) * 2^(16 - n))
 * for n significant bits — 1 for n = 16.  The depth matters only there: it makes 10-bit code 1023 white.
 *                      yo       cy      crv     cgu     cgv      cbu
 *   BT709 (any depth)  4096  1225714  1887168  224481  560979  2223666
 *   BT601 (any depth)  4096  1225714  1680093  412397  855788  2123484
 *   P010 BT709_FULL       0  1049585  1652886  196613  491336  1947610
 *   P010 BT601_FULL       0  1049585  1471518  361200  749547  1859865
 *   P012 BT709_FULL       0  1048816  1651676  196469  490976  1946183
 *   P012 BT601_FULL       0  1048816  1470440  360936  748998  1858502
 *   P016 BT709_FULL       0  1048576  1651297  196424  490864  1945738
 *   P016 BT601_FULL       0  1048576  1470104  360853  748826  1858077
 * A coefficient is off by at most 2^-21, together at most 65535 * 2^-21 + 2 * 32768 * 2^-21 = 0.0625; with half a code of
 * rounding the result is within 0.5625 of the clamped real-valued conversion for every (Y, U, V).
 *
 * How such a picture is named: as an NV12 picture, in 16-bit samples —
 *   src[0]        the first Y word;  src[1] the first U word of chroma row 0;  src[2] must equal src[1] + 2 bytes
 *   pixel_stride  must be 1
 *   row_stride    the one pitch of both planes IN SAMPLES (16-bit words), as every stride of this API is; may be negative.
 *                 Width and height may be odd: the chroma plane is ceil(h / 2) rows of ceil(w / 2) pairs.
 * All three addresses are 2-byte aligned.  A bad layout is HYD_API_ERROR "P010/P016 wants pixel_stride 1 and V one sample
 * behind U", nothing enqueued.  The library finds an LF group, tile or shard at even (x0, y0) at word y0 * row_stride + x0 of
 * the Y plane and word (y0 / 2) * row_stride + x0 of the chroma plane.
 *
 * Accepted wherever NV12 is.  hydamd_encode_image_multi takes the nearest forms and refuses the interpolated 24 as it does
 * NV12's; the host-pointer entry points refuse all 36 with "Invalid Sample Format".
 * Out of scope: BT.2020 and the PQ / HLG transfer curves — the codestream this encoder writes signals sRGB or linear sRGB
 * only, so HDR10 content would be mis-described whatever the matrix; two-plane 16-bit 4:2:2 and 4:4:4 (P210, P410: the planar
 * forms I210 ... I416 are further down, HYDAMD_I010_* ...); host-pointer P010.
 */
#define HYDAMD_P010_BT709 80
#define HYDAMD_P010_BT709_FULL 81
#define HYDAMD_P010_BT601 82
#define HYDAMD_P010_BT601_FULL 83
#define HYDAMD_P010C_BT709 96
#define HYDAMD_P010C_BT709_FULL 97
#define HYDAMD_P010C_BT601 98
#define HYDAMD_P010C_BT601_FULL 99
#define HYDAMD_P010L_BT709 112
#define HYDAMD_P010L_BT709_FULL 113
#define HYDAMD_P010L_BT601 114
#define HYDAMD_P010L_BT601_FULL 115
#define HYDAMD_P012_BT709 144
#define HYDAMD_P012_BT709_FULL 145
#define HYDAMD_P012_BT601 146
#define HYDAMD_P012_BT601_FULL 147
#define HYDAMD_P012C_BT709 160
#define HYDAMD_P012C_BT709_FULL 161
#define HYDAMD_P012C_BT601 162
#define HYDAMD_P012C_BT601_FULL 163
#define HYDAMD_P012L_BT709 176
#define HYDAMD_P012L_BT709_FULL 177
#define HYDAMD_P012L_BT601 178
#define HYDAMD_P012L_BT601_FULL 179
#define HYDAMD_P016_BT709 208
#define HYDAMD_P016_BT709_FULL 209
#define HYDAMD_P016_BT601 210
#define HYDAMD_P016_BT601_FULL 211
#define HYDAMD_P016C_BT709 224
#define HYDAMD_P016C_BT709_FULL 225
#define HYDAMD_P016C_BT601 226
#define HYDAMD_P016C_BT601_FULL 227
#define HYDAMD_P016L_BT709 240
#define HYDAMD_P016L_BT709_FULL 241
#define HYDAMD_P016L_BT601 242
#define HYDAMD_P016L_BT601_FULL 243

/*
 * PLANAR YCbCr DEVICE pixels: I420, I422 and I444 — 8 bits a sample, Y, U and V each in a plane of its own.  What rocJPEG's
 * planar output, rocDecode's 4:4:4 surfaces and every software decoder (yuv420p, yuvj422p, yuv444p) leave; YV12 is I420 with
 * src[1] and src[2] swapped.  Read by the transform kernel as they are, without an RGB or NV12 copy.
 *   sample_fmt = 512 + matrix + 4 * subsampling + 16 * filter
 * matrix 0..3 and filter 0..2 as in the NV12 family; subsampling 0 = 4:2:0, 1 = 4:2:2, 2 = 4:4:4 (filter 0 only):
 *                     nearest      centre-sited   left-sited
 *   HYDAMD_I420_*    512..515     528..531 (C)    544..547 (L)
 *   HYDAMD_I422_*    516..519     532..535 (C)    548..551 (L)
 *   HYDAMD_I444_*    520..523
 * 28 numbers.  524..527, 536..543, 552 and up name nothing, 512 + ... + 64 * depth included: planes deeper than 8 bits have
 * numbers of their own at 2048 (HYDAMD_I010_* ..., the next section).
 * A JPEG is BT601_FULL, centre-sited: HYDAMD_I420C_BT601_FULL, HYDAMD_I422C_BT601_FULL or HYDAMD_I444_BT601_FULL.
 *
 * How such a picture is named, wherever a sample_fmt names device pixels and in a HydAmdImageDesc:
 *   src[0]        the first Y sample
 *   src[1], [2]   the first U and the first V sample: independent pointers, possibly in separate allocations
 *   row_stride    the pitch of the Y plane in bytes; may be negative.  Y's pixel stride is 1 by definition
 *   pixel_stride  THE ONE PITCH OF BOTH CHROMA PLANES in bytes; may be negative, independently of row_stride
 * The chroma planes are cw x ch samples: cw = ceil(W / 2) for 4:2:0 and 4:2:2 and W for 4:4:4; ch = ceil(H / 2) for 4:2:0 and
 * H otherwise.  Odd sizes work as NV12's.  |pixel_stride| < cw of the picture the call names (the LF group's width for plain
 * hydamd_encode_lf_group) is HYD_API_ERROR "planar YCbCr wants the chroma planes' pitch in pixel_stride", nothing enqueued:
 * that is what the habitual pixel_stride 1 meets.
 * The library finds an LF group, tile or shard at pixel (x0, y0) at src[0] + y0 * row_stride + x0 and, with sx = 0 for 4:4:4
 * and 1 otherwise, sy = 1 for 4:2:0 and 0 otherwise, at src[1 or 2] + (y0 >> sy) * pixel_stride + (x0 >> sx).  A caller's own
 * crop must start on even x0, and on even y0 for 4:2:0, as NV12's.
 *
 * The file is byte for byte what the reference writes for the HYD_UINT8 picture this conversion produces.  Nearest: U and V
 * of pixel (x, y) are C[y >> sy][x >> sx] of each plane.  4:2:0 with filter 1 or 2: the taps of the NV12C / NV12L section,
 * applied to each plane as it stands.  4:2:2: the horizontal taps alone, with cx = x >> 1 —
 *   centre-sited, hx = clamp(cx + (x odd ? 1 : -1), 0, cw - 1):   C' = (3 C[y][cx] + C[y][hx] + 2) >> 2
 *   left-sited, x even:                                           C' = C[y][cx]
 *   left-sited, x odd, hx = min(cx + 1, cw - 1):                  C' = (C[y][cx] + C[y][hx] + 1) >> 1
 * (the 4:2:0 taps with the far row equal to the near one).  Then R, G, B by the NV12 section's formula and table, within 0.51
 * of the real-valued conversion of (Y, U', V').  Clamping is at the edges of the PICTURE: chroma is continuous across LF
 * groups and tiles, hydamd_encode_lf_group_at carries the picture, and nothing outside a plane's cw x ch samples or the Y
 * rectangle is ever read.
 *
 * Accepted wherever NV12 is, and beside NV12, P010 and RGB pictures in one hydamd_encode_mixed_formats launch group.
 * hydamd_encode_image_multi takes the 12 nearest forms and refuses the 16 interpolated ones as it does NV12's (a 4:2:2 window
 * also crosses into an LF group another shard owns); the host-pointer entry points refuse all 28 with "Invalid Sample Format".
 * Out of scope: NV21 and NV16; U and V planes of different pitches; top-left siting; host-pointer
 * input; cross-shard interpolation.  (I010 and deeper planes: the next section; packed YUY2 / UYVY: the one after it.)
 */
#define HYDAMD_I420_BT709 512
#define HYDAMD_I420_BT709_FULL 513
#define HYDAMD_I420_BT601 514
#define HYDAMD_I420_BT601_FULL 515
#define HYDAMD_I422_BT709 516
#define HYDAMD_I422_BT709_FULL 517
#define HYDAMD_I422_BT601 518
#define HYDAMD_I422_BT601_FULL 519
#define HYDAMD_I444_BT709 520
#define HYDAMD_I444_BT709_FULL 521
#define HYDAMD_I444_BT601 522
#define HYDAMD_I444_BT601_FULL 523
#define HYDAMD_I420C_BT709 528
#define HYDAMD_I420C_BT709_FULL 529
#define HYDAMD_I420C_BT601 530
#define HYDAMD_I420C_BT601_FULL 531
#define HYDAMD_I422C_BT709 532
#define HYDAMD_I422C_BT709_FULL 533
#define HYDAMD_I422C_BT601 534
#define HYDAMD_I422C_BT601_FULL 535
#define HYDAMD_I420L_BT709 544
#define HYDAMD_I420L_BT709_FULL 545
#define HYDAMD_I420L_BT601 546
#define HYDAMD_I420L_BT601_FULL 547
#define HYDAMD_I422L_BT709 548
#define HYDAMD_I422L_BT709_FULL 549
#define HYDAMD_I422L_BT601 550
#define HYDAMD_I422L_BT601_FULL 551

/*
 * PLANAR YCbCr DEVICE pixels OF 16-BIT WORDS: I010, I210, I410, I012, I212, I412, I016, I216 and I416 — the planar family's three
 * planes with 10, 12 or 16 significant bits a sample, LSB-ALIGNED in 16-bit words.  What every software decoder leaves for HEVC
 * Main10, 10-bit AV1 and VP9 and ProRes (yuv420p10le, yuv422p10le, yuv444p12le ...) and how rocDecode hands out 4:4:4 surfaces
 * above 8 bits; the first 16-bit route for 4:2:2 and 4:4:4 of any layout.  Read by the transform kernel as they are.
 *   sample_fmt = 2048 + matrix + 4 * subsampling + 16 * filter + 64 * depth
 * matrix 0..3, subsampling 0..2 and filter 0..2 as in the planar family; depth 1, 2, 3 = 10, 12, 16 significant bits as in the
 * P010 family:
 *                     nearest       centre-sited    left-sited
 *   HYDAMD_I010_*    2112..2115    2128..2131 (C)   2144..2147 (L)
 *   HYDAMD_I210_*    2116..2119    2132..2135 (C)   2148..2151 (L)
 *   HYDAMD_I410_*    2120..2123
 *   HYDAMD_I012_*    2176..2179    2192..2195 (C)   2208..2211 (L)
 *   HYDAMD_I212_*    2180..2183    2196..2199 (C)   2212..2215 (L)
 *   HYDAMD_I412_*    2184..2187
 *   HYDAMD_I016_*    2240..2243    2256..2259 (C)   2272..2275 (L)
 *   HYDAMD_I216_*    2244..2247    2260..2263 (C)   2276..2279 (L)
 *   HYDAMD_I416_*    2248..2251
 * 84 numbers, 28 a depth; the gaps are the planar family's.  2048..2111 (depth 0) name nothing — 8-bit planes stay at 512 — nor
 * does 2280 and up.
 *
 * How such a picture is named: as a planar picture, everything in SAMPLES (16-bit words), as every stride of this API is —
 *   src[0], [1], [2]  the first Y, U and V word: independent pointers, each 2-byte aligned
 *   row_stride        the pitch of the Y plane in words; may be negative
 *   pixel_stride      THE ONE PITCH OF BOTH CHROMA PLANES in words; may be negative, independently of row_stride
 * Plane sizes, odd sizes, crop rules, the origin of an LF group, tile or shard (in words) and what a picture is for the
 * interpolating forms are the planar family's.  |pixel_stride| < cw is HYD_API_ERROR "planar YCbCr wants the chroma planes'
 * pitch in pixel_stride"; an address that is not 2-byte aligned is HYD_API_ERROR "planar YCbCr of 16-bit words wants its three
 * planes on 2-byte boundaries"; nothing is enqueued by either.
 *
 * The file is byte for byte what the reference writes for the HYD_UINT16 picture this produces.  A stored word w of a picture of
 * n significant bits stands for the sample
 *   s = (w << (16 - n)) & 0xFFFF
 * — bits above the depth are shifted out and not trusted, so every word means something; depth 16 takes the word as stored,
 * so an MSB-aligned planar surface of any depth and limited range goes in as HYDAMD_I*16_*.  From there the picture is the
 * P010 / P012 / P016 picture of the same depth and matrix on the planar family's geometry: nearest takes C[y >> sy][x >> sx] of
 * each plane; filters 1 and 2 apply the taps of the NV12C / NV12L section to the SHIFTED samples of each plane by itself, 4:2:2
 * with the far row equal to the near one; then R, G, B by the P010 section's formula and table, unchanged.
 *
 * Accepted wherever the planar family is, and beside every other family in one hydamd_encode_mixed_formats launch group.
 * hydamd_encode_image_multi takes the 36 nearest forms and refuses the 48 interpolated ones as it does NV12's; the host-pointer
 * entry points refuse all 84 with "Invalid Sample Format".
 * Out of scope: BT.2020 and PQ / HLG (see the P010 section); MSB-aligned planes with full range at 10 or 12 bits; U and V planes
 * of different pitches; NV16 / NV21 (packed 8-bit YUY2 / UYVY: the next section; packed Y210 / Y216: the one after it); top-left siting; host-pointer input;
 * cross-shard interpolation.
 */
#define HYDAMD_I010_BT709 2112
#define HYDAMD_I010_BT709_FULL 2113
#define HYDAMD_I010_BT601 2114
#define HYDAMD_I010_BT601_FULL 2115
#define HYDAMD_I210_BT709 2116
#define HYDAMD_I210_BT709_FULL 2117
#define HYDAMD_I210_BT601 2118
#define HYDAMD_I210_BT601_FULL 2119
#define HYDAMD_I410_BT709 2120
#define HYDAMD_I410_BT709_FULL 2121
#define HYDAMD_I410_BT601 2122
#define HYDAMD_I410_BT601_FULL 2123
#define HYDAMD_I010C_BT709 2128
#define HYDAMD_I010C_BT709_FULL 2129
#define HYDAMD_I010C_BT601 2130
#define HYDAMD_I010C_BT601_FULL 2131
#define HYDAMD_I210C_BT709 2132
#define HYDAMD_I210C_BT709_FULL 2133
#define HYDAMD_I210C_BT601 2134
#define HYDAMD_I210C_BT601_FULL 2135
#define HYDAMD_I010L_BT709 2144
#define HYDAMD_I010L_BT709_FULL 2145
#define HYDAMD_I010L_BT601 2146
#define HYDAMD_I010L_BT601_FULL 2147
#define HYDAMD_I210L_BT709 2148
#define HYDAMD_I210L_BT709_FULL 2149
#define HYDAMD_I210L_BT601 2150
#define HYDAMD_I210L_BT601_FULL 2151
#define HYDAMD_I012_BT709 2176
#define HYDAMD_I012_BT709_FULL 2177
#define HYDAMD_I012_BT601 2178
#define HYDAMD_I012_BT601_FULL 2179
#define HYDAMD_I212_BT709 2180
#define HYDAMD_I212_BT709_FULL 2181
#define HYDAMD_I212_BT601 2182
#define HYDAMD_I212_BT601_FULL 2183
#define HYDAMD_I412_BT709 2184
#define HYDAMD_I412_BT709_FULL 2185
#define HYDAMD_I412_BT601 2186
#define HYDAMD_I412_BT601_FULL 2187
#define HYDAMD_I012C_BT709 2192
#define HYDAMD_I012C_BT709_FULL 2193
#define HYDAMD_I012C_BT601 2194
#define HYDAMD_I012C_BT601_FULL 2195
#define HYDAMD_I212C_BT709 2196
#define HYDAMD_I212C_BT709_FULL 2197
#define HYDAMD_I212C_BT601 2198
#define HYDAMD_I212C_BT601_FULL 2199
#define HYDAMD_I012L_BT709 2208
#define HYDAMD_I012L_BT709_FULL 2209
#define HYDAMD_I012L_BT601 2210
#define HYDAMD_I012L_BT601_FULL 2211
#define HYDAMD_I212L_BT709 2212
#define HYDAMD_I212L_BT709_FULL 2213
#define HYDAMD_I212L_BT601 2214
#define HYDAMD_I212L_BT601_FULL 2215
#define HYDAMD_I016_BT709 2240
#define HYDAMD_I016_BT709_FULL 2241
#define HYDAMD_I016_BT601 2242
#define HYDAMD_I016_BT601_FULL 2243
#define HYDAMD_I216_BT709 2244
#define HYDAMD_I216_BT709_FULL 2245
#define HYDAMD_I216_BT601 2246
#define HYDAMD_I216_BT601_FULL 2247
#define HYDAMD_I416_BT709 2248
#define HYDAMD_I416_BT709_FULL 2249
#define HYDAMD_I416_BT601 2250
#define HYDAMD_I416_BT601_FULL 2251
#define HYDAMD_I016C_BT709 2256
#define HYDAMD_I016C_BT709_FULL 2257
#define HYDAMD_I016C_BT601 2258
#define HYDAMD_I016C_BT601_FULL 2259
#define HYDAMD_I216C_BT709 2260
#define HYDAMD_I216C_BT709_FULL 2261
#define HYDAMD_I216C_BT601 2262
#define HYDAMD_I216C_BT601_FULL 2263
#define HYDAMD_I016L_BT709 2272
#define HYDAMD_I016L_BT709_FULL 2273
#define HYDAMD_I016L_BT601 2274
#define HYDAMD_I016L_BT601_FULL 2275
#define HYDAMD_I216L_BT709 2276
#define HYDAMD_I216L_BT709_FULL 2277
#define HYDAMD_I216L_BT601 2278
#define HYDAMD_I216L_BT601_FULL 2279

/*
 * PACKED 4:2:2 YCbCr DEVICE pixels: YUY2 (YUYV), UYVY, YVYU and VYUY — 8 bits a sample, Y, U and V in ONE plane of 4-byte groups,
 * two pixels a group.  What rocJPEG's native output is for a 4:2:2 JPEG ("for ROCJPEG_CSS_422 write YUYV (packed) to first
 * channel"), what capture cards and V4L2 devices deliver and what rocDecode's YUYV surfaces hold.  Read by the transform kernel
 * as it is, without a planar or RGB copy.
 *   sample_fmt = 8192 + matrix + 16 * filter
 * matrix 0..3 and filter 0..2 as in the NV12 family:
 *                     nearest       centre-sited    left-sited
 *   HYDAMD_YUY2_*    8192..8195    8208..8211 (C)   8224..8227 (L)
 * 12 numbers.  The subsampling bits (4 *) are 0: 8196..8207, 8212..8223 and 8228..8239 name nothing; nor does 8240 and up (filter 3,
 * and 64 * depth: packed words of 10 to 16 bits have a base of their own, 32768, the next section).  A 4:2:2 JPEG is HYDAMD_YUY2C_BT601_FULL; video is left-sited.
 *
 * How such a picture is named — THE BYTE ORDER IS READ OFF THE POINTERS, not off the number:
 *   src[0]        the first Y byte
 *   src[1], [2]   the first U and the first V byte, both of the group src[0] lies in:
 *                 (src[1] - src[0], src[2] - src[0]) = (1, 3) YUYV / YUY2, (3, 1) YVYU, (-1, 1) UYVY, (1, -1) VYUY
 *   pixel_stride  2, the distance between two Y samples
 *   row_stride    the pitch of the surface in bytes; may be negative
 * Anything else is HYD_API_ERROR "YUY2/UYVY wants pixel_stride 2 and U and V in the bytes beside Y", nothing enqueued.
 * A row is 4 * ceil(W / 2) bytes: for odd W the last group's second Y byte belongs to the row, may be read and is no pixel.
 * Nothing outside those bytes of rows 0 .. H - 1 is ever read.  The library finds an LF group, tile or shard at pixel (x0, y0)
 * by adding y0 * row_stride + 2 * x0 to ALL THREE pointers; a caller's own crop must start on even x0.
 *
 * The picture is the HYDAMD_I422* picture whose planes are the de-interleaved bytes: Y[y][x] is the byte at 2 x from src[0] in
 * row y, U[y][cx] and V[y][cx] the bytes at 4 cx from src[1] and src[2], cw = ceil(W / 2).  Nearest chroma and the centre- and
 * left-sited horizontal taps are the planar section's, the conversion and its 0.51 bound the NV12 section's.  Clamping is at the
 * edges of the PICTURE: chroma is continuous across LF groups and tiles, hydamd_encode_lf_group_at carries the picture, and plain
 * hydamd_encode_lf_group treats the LF group as a picture of its own.  The file is byte for byte what the reference writes for the
 * HYD_UINT8 picture this produces, and so what this library writes for the same planes given as HYDAMD_I422*.
 *
 * Accepted wherever NV12 is, and beside every other family — and pictures of different byte orders — in one
 * hydamd_encode_mixed_formats launch group.  hydamd_encode_image_multi takes the 4 nearest forms and refuses the 8 interpolated
 * ones as it does I422C / I422L; the host-pointer entry points refuse all 12 with "Invalid Sample Format".
 * Out of scope: 4:4:0 planes, rocJPEG's other native form
 * (subsampling 3 of the planar family names nothing); host-pointer input; cross-shard interpolation.
 */
#define HYDAMD_YUY2_BT709 8192
#define HYDAMD_YUY2_BT709_FULL 8193
#define HYDAMD_YUY2_BT601 8194
#define HYDAMD_YUY2_BT601_FULL 8195
#define HYDAMD_YUY2C_BT709 8208
#define HYDAMD_YUY2C_BT709_FULL 8209
#define HYDAMD_YUY2C_BT601 8210
#define HYDAMD_YUY2C_BT601_FULL 8211
#define HYDAMD_YUY2L_BT709 8224
#define HYDAMD_YUY2L_BT709_FULL 8225
#define HYDAMD_YUY2L_BT601 8226
#define HYDAMD_YUY2L_BT601_FULL 8227

/*
 * PACKED 4:2:2 YCbCr OF 16-BIT WORDS, DEVICE pixels: Y210, Y212 and Y216 — 10, 12 or 16 significant bits a sample, MSB-aligned as
 * P010's are, Y, U and V in ONE plane of groups of four words, two pixels a group.  What a VA-API or D3D decoder leaves for 4:2:2
 * 10-bit HEVC, ffmpeg's y210le / y212le / y216le, the layout of 10-bit capture and broadcast ingest.  Read by the transform kernel
 * as it is, without a de-interleaved or RGB copy.
 *   sample_fmt = 32768 + matrix + 16 * filter + 64 * depth
 * matrix 0..3 and filter 0..2 as in the NV12 family, depth 1, 2, 3 = 10, 12, 16 bits as in the P010 family:
 *                     nearest         centre-sited      left-sited
 *   HYDAMD_Y210_*    32832..32835    32848..32851 (C)   32864..32867 (L)
 *   HYDAMD_Y212_*    32896..32899    32912..32915 (C)   32928..32931 (L)
 *   HYDAMD_Y216_*    32960..32963    32976..32979 (C)   32992..32995 (L)
 * 36 numbers.  Depth 0 (32768..32831: the 8-bit family stays at 8192), the subsampling bits (4 *), filter 3 and 33024 and up name
 * nothing.  HEVC, H.264 and AV1 video is left-sited.
 *
 * How such a picture is named — everything in 16-BIT SAMPLES, and THE WORD ORDER IS READ OFF THE POINTERS, not off the number:
 *   src[0]        the first Y word
 *   src[1], [2]   the first U and the first V word, both of the group src[0] lies in: (src[1] - src[0], src[2] - src[0]) in words
 *                 = (1, 3) Y210's own order Y U Y V, (3, 1) Y V Y U, (-1, 1) U Y V Y, (1, -1) V Y U Y
 *   pixel_stride  2, the distance between two Y words
 *   row_stride    the pitch of the surface in words; may be negative
 * All three addresses sit on 2-byte boundaries.  Anything else is HYD_API_ERROR "Y210/Y216 wants pixel_stride 2 and U and V in the
 * words beside Y", nothing enqueued.  A row is 4 * ceil(W / 2) words: for odd W the last group's second Y word belongs to the row,
 * may be read and is no pixel.  Nothing outside those words of rows 0 .. H - 1 is ever read.  The library finds an LF group, tile or
 * shard at pixel (x0, y0) by adding y0 * row_stride + 2 * x0 words to ALL THREE pointers; a caller's own crop must start on even x0.
 *
 * The words count AS STORED — the low 6 (Y210) or 4 (Y212) bits are not masked, the P010 section's rule — and the picture is the
 * 4:2:2 picture of the de-interleaved words: Y[y][x] is the word at 2 x from src[0] in row y, U[y][cx] and V[y][cx] the words at
 * 4 cx from src[1] and src[2], cw = ceil(W / 2).  Nearest chroma and the centre- and left-sited horizontal taps are the planar
 * section's, the conversion, its depth-dependent full-range matrices and its 0.5625 bound the P010 section's.  So a Y216 picture is
 * the HYDAMD_I216* picture of its de-interleaved words, and a Y210 picture whose low six bits are zero the HYDAMD_I210* picture of
 * the words shifted right by six.  Clamping is at the edges of the PICTURE, as for YUY2.  The file is byte for byte what the
 * reference writes for the HYD_UINT16 picture this produces.
 *
 * Accepted wherever YUY2 is, and beside every other family — and pictures of different word orders — in one
 * hydamd_encode_mixed_formats launch group.  hydamd_encode_image_multi takes the 12 nearest forms and refuses the 24 interpolated
 * ones as it does YUY2C / YUY2L; the host-pointer entry points refuse all 36 with "Invalid Sample Format".
 * Out of scope: v210; NV16 / NV24 / P210; LSB-aligned packed words; host-pointer input;
 * cross-shard interpolation.
 */
#define HYDAMD_PACKED16_STEM(P, F, D) \
    HYDAMD_##P##_BT709 = 32768 + 16 * (F) + 64 * (D), HYDAMD_##P##_BT709_FULL, HYDAMD_##P##_BT601, HYDAMD_##P##_BT601_FULL
enum {
    HYDAMD_PACKED16_STEM(Y210, 0, 1), HYDAMD_PACKED16_STEM(Y210C, 1, 1), HYDAMD_PACKED16_STEM(Y210L, 2, 1),
    HYDAMD_PACKED16_STEM(Y212, 0, 2), HYDAMD_PACKED16_STEM(Y212C, 1, 2), HYDAMD_PACKED16_STEM(Y212L, 2, 2),
    HYDAMD_PACKED16_STEM(Y216, 0, 3), HYDAMD_PACKED16_STEM(Y216C, 1, 3), HYDAMD_PACKED16_STEM(Y216L, 2, 3)
};
#undef HYDAMD_PACKED16_STEM

/*
 * ONE DWORD A PIXEL, DEVICE pixels: RGB10A2, BGR10A2 and Y410 — a pixel is one 32-bit word of three 10-bit fields and two spare
 * bits.  RGB10A2 is the render-target and scan-out format of HDR and deep-colour pipelines (Vulkan A2B10G10R10_UNORM_PACK32, DXGI
 * R10G10B10A2_UNORM, DRM XBGR2101010), BGR10A2 its other order (Vulkan A2R10G10B10_UNORM_PACK32, DRM XRGB2101010), Y410 (DRM
 * XVYU2101010) what a VA-API or D3D decoder leaves for 4:4:4 10-bit HEVC.  Read by the transform kernel as it is, without an
 * unpacked RGB16 copy of three times the bytes.
 *   HYDAMD_RGB10A2   131072          R in bits 0..9, G in 10..19, B in 20..29
 *   HYDAMD_BGR10A2   131073          B in bits 0..9, G in 10..19, R in 20..29
 *   HYDAMD_Y410_*    131144..131147  = 131072 + matrix + 4 * 2 (4:4:4) + 64 * 1 (10 bits); U in bits 0..9, Y in 10..19, V in 20..29
 * Six numbers; every other number from 131072 up to 524287 names nothing.  Bits 30 and 31 are ignored.
 *
 * How such a picture is named — A SAMPLE IS THE DWORD:
 *   src[0] == src[1] == src[2]   the first dword, on a 4-byte boundary
 *   pixel_stride                 1
 *   row_stride                   the pitch of the surface in dwords; may be negative
 * Anything else is HYD_API_ERROR "RGB10A2/Y410 wants pixel_stride 1 and three equal pointers on a 4-byte boundary", nothing
 * enqueued.  A row is W dwords and nothing outside the W dwords of rows 0 .. H - 1 is ever read.  The library finds an LF group, tile
 * or shard at pixel (x0, y0) by adding y0 * row_stride + x0 dwords to all three pointers; a caller's own crop may start anywhere.
 *
 * Both are storage forms of the 16-bit class.  An RGB field v (0..1023) stands for the HYD_UINT16 sample nearest to v / 1023,
 * (v * 65535 + 511) / 1023 in integers — 0 is 0, 1023 is 65535, no value is a tie — and the picture is the HYD_UINT16 picture of
 * those samples.  A Y410 field v stands for the P010 sample v << 6, and from there the conversion, its matrices and its 0.5625 bound
 * are the P010 section's: a Y410 picture is the HYDAMD_I410_* picture of its three fields.  The file is byte for byte what the
 * reference writes for the HYD_UINT16 picture this produces.  An HDR10 swap chain's PQ-coded numbers would be coded AS sRGB, as the
 * P010 section says of BT.2020 video: the codestream this encoder writes signals sRGB or linear sRGB and nothing else.
 *
 * Accepted wherever Y210 is, and beside every other family in one hydamd_encode_mixed_formats launch group.  There is no chroma
 * filter, so hydamd_encode_image_multi takes all six; the host-pointer entry points refuse all six with "Invalid Sample Format".
 * Out of scope: v210; PQ / HLG / BT.2020; an alpha in bits 30..31; host-pointer input.  (R11G11B10F, the float render target of
 * the same size, is the section after the next.)  (The 8-, 12- and 16-bit
 * siblings of Y410 — AYUV, Y412, Y416 — are the next section.)
 */
enum {
    HYDAMD_RGB10A2 = 131072,
    HYDAMD_BGR10A2 = 131073,
    HYDAMD_Y410_BT709 = 131072 + 4 * 2 + 64 * 1,
    HYDAMD_Y410_BT709_FULL,
    HYDAMD_Y410_BT601,
    HYDAMD_Y410_BT601_FULL
};

/*
 * FOUR SAMPLES A PIXEL, DEVICE pixels: AYUV, Y412 and Y416 — packed 4:4:4 YCbCr, a pixel is one group of Y, U, V and a fourth
 * sample that is ignored.  AYUV (DXGI AYUV, VA-API AYUV / XYUV, DRM XYUV8888, ffmpeg vuya / vuyx) is what a decoder leaves for
 * 4:4:4 8-bit video, Y412 (XV36, DRM XVYU12_16161616) and Y416 (XV48, DRM XVYU16161616) for 12 and 16 bits; with Y410 of the section
 * above they are the packed 4:4:4 surfaces DXGI, VA-API, DRM and AMF hand out.  Read by the transform kernel as they are, without a
 * de-interleave pass into three planes.
 *   HYDAMD_AYUV_*   524296..524299  = 524288 + matrix + 4 * 2 (4:4:4)           one DWORD: V in bits 0..7, U in 8..15, Y in 16..23
 *                                                                                (bytes V, U, Y, A); bits 24..31 ignored
 *   HYDAMD_Y412_*   524424..524427  = 524288 + matrix + 4 * 2 + 64 * 2 (12 bits) one QWORD: U in bits 0..15, Y in 16..31, V in 32..47
 *                                                                                (words U, Y, V, A), MSB-aligned; bits 48..63 ignored
 *   HYDAMD_Y416_*   524488..524491  = 524288 + matrix + 4 * 2 + 64 * 3 (16 bits) the same qword, 16 significant bits
 * Twelve numbers; depth 1 (524360..524363) names nothing — the 10-bit surface is Y410 at 131144 — and so does every other number
 * from 524288 up to 8388607.
 *
 * How such a picture is named — A SAMPLE IS THE GROUP, exactly as Y410's sample is the dword:
 *   src[0] == src[1] == src[2]   the first pixel, on a boundary of the pixel's size: 4 bytes for AYUV, 8 bytes for Y412 / Y416
 *   pixel_stride                 1
 *   row_stride                   the pitch of the surface in pixels (dwords or qwords respectively); may be negative
 * Anything else is HYD_API_ERROR "AYUV/Y416 wants pixel_stride 1 and three equal pointers on a boundary of the pixel's size",
 * nothing enqueued.  A row is W pixels and nothing outside the W pixels of rows 0 .. H - 1 is ever read.  The library finds an LF
 * group, tile or shard at pixel (x0, y0) by adding y0 * row_stride + x0 pixels to all three pointers; a caller's own crop may start
 * anywhere.
 *
 * AYUV is a storage form of the 8-bit class: the HYDAMD_I444_* picture of its three bytes, under the NV12 section's conversion.
 * Y412 and Y416 are storage forms of the 16-bit class: the words count as stored — low bits are not masked, the P010 section's rule
 * — under that section's conversion at 12 or 16 bits.  A Y416 picture is the HYDAMD_I416_* picture of its three words, and a Y412
 * picture whose low four bits are zero the HYDAMD_I412_* picture of the words >> 4.  The fourth sample never matters.  The file is
 * byte for byte what the reference writes for the HYD_UINT8 or HYD_UINT16 picture this produces.
 *
 * Accepted wherever Y410 is, and beside every other family in one hydamd_encode_mixed_formats launch group.  There is no chroma
 * filter, so hydamd_encode_image_multi takes all twelve; the host-pointer entry points refuse all twelve with "Invalid Sample
 * Format".
 * Out of scope: other byte orders (ffmpeg ayuv, uyva, ayuv64le, 3-byte vyu444); an alpha channel; v210; NV16 / NV24 / P210;
 * host-pointer input; PQ / HLG / BT.2020.
 */
enum {
    HYDAMD_AYUV_BT709 = 524288 + 4 * 2,
    HYDAMD_AYUV_BT709_FULL,
    HYDAMD_AYUV_BT601,
    HYDAMD_AYUV_BT601_FULL,
    HYDAMD_Y412_BT709 = 524288 + 4 * 2 + 64 * 2,
    HYDAMD_Y412_BT709_FULL,
    HYDAMD_Y412_BT601,
    HYDAMD_Y412_BT601_FULL,
    HYDAMD_Y416_BT709 = 524288 + 4 * 2 + 64 * 3,
    HYDAMD_Y416_BT709_FULL,
    HYDAMD_Y416_BT601,
    HYDAMD_Y416_BT601_FULL
};

/*
 * THREE UNSIGNED FLOATS IN ONE DWORD, DEVICE pixels: R11G11B10F and RGB9E5 — the float render targets that pack a pixel into 32 bits.
 * R11G11B10F (DXGI R11G11B10_FLOAT, Vulkan B10G11R11_UFLOAT_PACK32, GL R11F_G11F_B10F) is the usual HDR scene and post-processing
 * buffer of real-time renderers and what game and screen capture hands over for HDR content; RGB9E5 (DXGI R9G9B9E5_SHAREDEXP, Vulkan
 * E5B9G9R9_UFLOAT_PACK32, GL RGB9_E5) holds HDR textures, light maps and environment maps.  Read by the transform kernel as they are,
 * without an unpacked float32 copy of three times the bytes.
 *   HYDAMD_R11G11B10F   8388608   R in bits 0..10, G in 11..21, B in 22..31; a field has no sign, a 5-bit exponent e (bias 15) above
 *                                 M = 6, 6, 5 mantissa bits m: e = 1..30 is 2^(e-15) * (1 + m / 2^M), e = 0 is m * 2^(-14-M)
 *                                 (subnormals and zero), e = 31 is +Inf (m = 0) or NaN
 *   HYDAMD_RGB9E5       8388609   R's mantissa in bits 0..8, G's in 9..17, B's in 18..26, the shared exponent E in 27..31; a channel is
 *                                 m * 2^(E-24), no implicit leading one; every dword is a finite picture
 * Two numbers; every other number from 8388608 up names nothing.
 *
 * How such a picture is named — A SAMPLE IS THE DWORD, exactly as RGB10A2's is:
 *   src[0] == src[1] == src[2]   the first dword, on a 4-byte boundary
 *   pixel_stride                 1
 *   row_stride                   the pitch of the surface in dwords; may be negative
 * Anything else is HYD_API_ERROR "R11G11B10F/RGB9E5 wants pixel_stride 1 and three equal pointers on a 4-byte boundary", nothing
 * enqueued.  A row is W dwords and nothing outside the W dwords of rows 0 .. H - 1 is ever read.  The library finds an LF group, tile
 * or shard at pixel (x0, y0) by adding y0 * row_stride + x0 dwords to all three pointers; a caller's own crop may start anywhere.
 *
 * Both are storage forms of the FLOAT class, as HYDAMD_FLOAT16 is.  A sample is widened EXACTLY to float32 on load — every value
 * of both formats is a float32 normal or zero, the smallest 2^-20 and 2^-24 — and from there on the pixel is a float32 pixel: the
 * file is byte for byte what the reference writes for the HYD_FLOAT32 picture of the widened samples, values above 1.0 included.
 * An R11G11B10F field that is Inf or NaN is whatever a non-finite HYD_FLOAT32 sample is on the same entry point: the same error on a
 * context, the same status word of its image in a batch.  The samples are taken as sRGB-coded, or as linear light where the
 * encoder is set to linear_light, as every float sample is: a renderer's scene-referred buffer wants linear_light = 1.
 *
 * Accepted wherever HYDAMD_FLOAT16 is, and beside every other family in one hydamd_encode_mixed_formats launch group.  There is no
 * chroma filter, so hydamd_encode_image_multi takes both; the host-pointer entry points refuse both with "Invalid Sample Format".
 * Out of scope: signed or 16-bit-per-channel float packings other than what strides already spell (R16G16B16A16_FLOAT is
 * HYDAMD_FLOAT16 with pixel_stride 4); an alpha; PQ / HLG / BT.2020; host-pointer input.  (RGB10A2, the unsigned-normalised
 * render target of the same size, is two sections up.)
 */
enum {
    HYDAMD_R11G11B10F = 8388608,
    HYDAMD_RGB9E5 = 8388609
};

/*
 * Enqueue the whole hot path for the LF group stored in `slot` (0 <= slot < max_lf_groups; slots
 * are coded into the frame in the order they are submitted).  src/strides/fmt mean exactly what
 * hyd_send_tile's buffer/row_stride/pixel_stride/sample_fmt mean (strides in samples, src[c]
 * pointing at the LF group's first pixel), except that the pointers are DEVICE pointers and that sample_fmt may also be
 * HYDAMD_FLOAT16, HYDAMD_BFLOAT16 or one of the HYDAMD_NV12_*, HYDAMD_P01x_*, HYDAMD_I4xx_*, HYDAMD_Ixnn_*, HYDAMD_YUY2_*, HYDAMD_Y21x_*, HYDAMD_RGB10A2, HYDAMD_BGR10A2, HYDAMD_Y410_*, HYDAMD_AYUV_*, HYDAMD_Y412_*, HYDAMD_Y416_* formats, HYDAMD_R11G11B10F or HYDAMD_RGB9E5 (whose src and strides are
 * described above).  With an interpolating format (HYDAMD_NV12C_*, HYDAMD_NV12L_*, their P01x and I42x forms) the LF group is a
 * picture of its own: its chroma clamps at its own edges.
 */
HYDAMD_EXPORT int hydamd_encode_lf_group(HydAmdContext *ctx, int slot, const void *const src[3], ptrdiff_t row_stride,
                                         ptrdiff_t pixel_stride, int sample_fmt, size_t width, size_t height,
                                         unsigned preset);

/* The same for the width x height LF group at pixel (x0, y0) of a pic_width x pic_height PICTURE whose first pixel src
 * names (for NV12: its first Y and U samples).  For every format this finds the LF group's origin as the library does and
 * is hydamd_encode_lf_group from there; for the interpolating formats (above) it also records the picture, whose chroma the
 * filter reads across the LF group's edges and at whose edges it clamps.  HYD_API_ERROR: x0 or y0 no multiple of 256, or a
 * rectangle that does not lie inside the picture. */
HYDAMD_EXPORT int hydamd_encode_lf_group_at(HydAmdContext *ctx, int slot, const void *const src[3], ptrdiff_t row_stride,
                                            ptrdiff_t pixel_stride, int sample_fmt, size_t pic_width, size_t pic_height,
                                            size_t x0, size_t y0, size_t width, size_t height, unsigned preset);

/* A whole device-resident image in ONE call: hydamd_begin_frame, hydamd_encode_lf_group for every LF group in raster
 * order (slot = raster index = preset: the one-frame layout of the reference for tiles sent in raster order,
 * libhydrium.c:172-203) and hydamd_finish_frame.  src/strides/fmt as above, for the image's first pixel.  Asynchronous. */
HYDAMD_EXPORT int hydamd_encode_image(HydAmdContext *ctx, const void *const src[3], ptrdiff_t row_stride,
                                      ptrdiff_t pixel_stride, int sample_fmt, size_t width, size_t height);

/* A BATCH of `frames` independent images of one shape as ONE launch group (for a queue of frames: the serial rANS chains
 * of the batch run side by side, so a stream is held for one chain's duration per batch instead of per frame; bench.py
 * codes two 8192x8192 frames per group).  hydamd_begin_batch = hydamd_begin_frame with frame k in slots k * num_presets ...
 * (k + 1) * num_presets - 1, presets 0 .. num_presets - 1 in each; hydamd_encode_image_batch = hydamd_encode_image for
 * src[3 k .. 3 k + 2] of every frame, then hydamd_finish_frame over all slots.  Results per slot as usual
 * (hydamd_read_sections, hydamd_read_tables, hydamd_read_lf_streams); frame k's sections follow frame k - 1's in the
 * payload.  A batch is not exported as a blob (hydamd_export_frame*: HYD_API_ERROR): hydamd_export_batch_owned gives its
 * results as a view, and hydamd_batch_* (below) turns a batch into finished files on the device. */
HYDAMD_EXPORT int hydamd_begin_batch(HydAmdContext *ctx, unsigned num_presets, int frames);
/* `frames` independent images of DIFFERENT shapes as one launch group: image k of lf_groups[k] LF groups (1..28 each: the
 * nine-cluster scheme, which keeps the cluster count launch-wide), in slots first_k .. first_k + lf_groups[k] - 1 with
 * first_k = sum of lf_groups[0 .. k - 1]; presets and the running alphabet maximum restart with every image.  Then
 * hydamd_encode_lf_group per slot (preset: the LF group's raster index inside its image), hydamd_finish_frame and
 * hydamd_export_batch_owned over all slots, as for hydamd_begin_batch.  HYD_API_ERROR: frames < 1, a null pointer, a count
 * of 0 or above 28, more LF groups in all than the context has slots. */
#define HYDAMD_BATCH_FRAME_LF_GROUPS 28
HYDAMD_EXPORT int hydamd_begin_batch_frames(HydAmdContext *ctx, int frames, const unsigned *lf_groups);
HYDAMD_EXPORT int hydamd_encode_image_batch(HydAmdContext *ctx, int frames, const void *const *src, ptrdiff_t row_stride,
                                            ptrdiff_t pixel_stride, int sample_fmt, size_t width, size_t height);

/* Same, from HOST pointers: the samples are gathered into pinned staging (the caller's buffers may
 * be reused as soon as this returns, as after hyd_send_tile) and copied to the GPU on the stream.  sample_fmt is one of
 * HYD_UINT8, HYD_UINT16, HYD_FLOAT32: the half-precision and NV12 formats name device pixels only. */
HYDAMD_EXPORT int hydamd_encode_lf_group_host(HydAmdContext *ctx, int slot, const void *const src[3],
                                              ptrdiff_t row_stride, ptrdiff_t pixel_stride, int sample_fmt,
                                              size_t width, size_t height, unsigned preset);

/* Optional: enqueue the transform stage of the LF group in `slot` right away instead of at
 * hydamd_finish_frame (slots in order, one at a time).  hyd_send_tile uses it so that the GPU works
 * on LF group n while the host is still staging tile n + 1; hydamd_finish_frame then runs what is
 * left (the entropy stage and the LF coder, batched over the frame) and packs. */
HYDAMD_EXPORT int hydamd_submit_lf_group(HydAmdContext *ctx, int slot);

/* Optional: enqueue the LF coder for the slots not yet LF-coded below `num_slots` right here in the
 * context's stream (their transform stage must be enqueued); with `last` != 0 the frame's LF streams
 * are also packed, and hydamd_sync_lf() then waits for just that — so a caller can read the LF streams
 * (hydamd_read_lf_streams / hydamd_read_lf_payload) and build the LF sections on the host while
 * the entropy stage enqueued behind it is still running.  hyd_send_tile does. */
HYDAMD_EXPORT int hydamd_run_lf_coder(HydAmdContext *ctx, int num_slots, int last);
HYDAMD_EXPORT int hydamd_sync_lf(HydAmdContext *ctx);

/* Enqueue whatever of the hot path is still outstanding for slots [0, num_slots) — transform stage,
 * LF coder, ANS tables, rANS — and the packing of the HF sections: byte-padded, slot-major, raster
 * inside a slot.  Asynchronous. */
HYDAMD_EXPORT int hydamd_finish_frame(HydAmdContext *ctx, int num_slots);

/* Block until everything enqueued so far has run; reports device-side failures (non-finite float
 * sample -> HYD_API_ERROR, table construction failure -> HYD_INTERNAL_ERROR). */
HYDAMD_EXPORT int hydamd_sync(HydAmdContext *ctx);

/* Where a non-finite float sample is recorded.  Off (default): bit 0 of the launch-wide status word — hydamd_sync fails with
 * "Invalid NaN Float" and a view's header carries the bit: the LF group cannot be named.  On: one flag per SLOT, cleared and
 * rerun with the frame's other accumulators; the sample is coded as 0.0 (the slot's results are those of an ordinary picture
 * and can neither fail nor rerun its launch group), the status word and the view's header stay clean and hydamd_sync returns
 * HYD_OK.  The switch holds for LF groups recorded after the call: set it between frames.
 * hydamd_read_bad_slots waits for the frame and copies `count` flags from slot `first_slot` on (non-zero: flagged; all zero
 * while the switch is off); in a view the flag travels in each slot's record (HydAmdBlobSlot.reserved[0]). */
HYDAMD_EXPORT int hydamd_set_bad_sample_per_slot(HydAmdContext *ctx, int on);
HYDAMD_EXPORT int hydamd_read_bad_slots(HydAmdContext *ctx, int first_slot, int count, uint32_t *flags);

/* ---- results; valid after hydamd_sync() ---- */
HYDAMD_EXPORT size_t hydamd_payload_size(HydAmdContext *ctx);
/* The device pointer may change when a frame outgrows its buffers (see below): fetch it after hydamd_sync(). */
HYDAMD_EXPORT const uint8_t *hydamd_payload_device(HydAmdContext *ctx);
/* Buffers are sized for typical content (1.5 symbols and 1 byte of sections per pixel) rather than for
 * the format's hard maximum.  A frame that needs more is detected on the device; hydamd_sync() then
 * enlarges the arrays and runs the frame again before it returns — transparent to the caller except
 * for the time it takes and for device pointers fetched earlier.  These report the current sizes and
 * how often that happened (a context that met one such frame stays enlarged). */
HYDAMD_EXPORT size_t hydamd_payload_capacity(HydAmdContext *ctx);
HYDAMD_EXPORT unsigned hydamd_token_capacity(HydAmdContext *ctx);
HYDAMD_EXPORT unsigned hydamd_overflow_reruns(HydAmdContext *ctx);
/* Once any context of the process has rerun a frame for that reason, the others take the hint: hydamd_begin_frame enlarges
 * an IDLE context's arrays ahead of its next frame (a queue of frames is of one kind as a rule); a busy context keeps what
 * it has and finds out by itself.  How often that happened for this context: */
HYDAMD_EXPORT unsigned hydamd_grown_ahead(HydAmdContext *ctx);
HYDAMD_EXPORT int hydamd_read_payload(HydAmdContext *ctx, uint8_t *dst, size_t capacity);
/* bits[g] = exact bit length of group g's section (0 for absent groups), offsets[g] = byte offset in the payload */
HYDAMD_EXPORT int hydamd_read_sections(HydAmdContext *ctx, int slot, uint32_t bits[HYDAMD_GROUPS_PER_LFG],
                                       uint64_t offsets[HYDAMD_GROUPS_PER_LFG]);
HYDAMD_EXPORT int hydamd_read_tables(HydAmdContext *ctx, int slot, uint32_t freq[HYDAMD_MAX_CLUSTERS][HYDAMD_ALPHABET],
                                     uint32_t alphabet[HYDAMD_MAX_CLUSTERS], uint32_t *log_alphabet_size,
                                     uint32_t *running_max_alphabet);
/* LF ints, dst[c][by][bx] with row pitch vbw, channel order X, Y, B */
HYDAMD_EXPORT int hydamd_read_dc(HydAmdContext *ctx, int slot, int32_t *dst, size_t vbw, size_t vbh);

/* ---- LF-group coder: the LF-coefficient sub-stream of every submitted LF group is coded on the
 * GPU alongside the HF entropy stage (on by default; 0 leaves the LF ints to a host coder via
 * hydamd_read_dc).  Results are valid after hydamd_sync(). ---- */
/* on_device: 0 off; 1 (default) on a side stream beside the HF entropy stage — lowest frame latency;
 * 2 at the end of the context's own stream — no second stream per context, for many frames in flight */
HYDAMD_EXPORT int hydamd_set_lf_coder(HydAmdContext *ctx, int on_device);
HYDAMD_EXPORT int hydamd_lf_coder(HydAmdContext *ctx);
/* code length per compact token, largest token + 1, number of (run, distance) pairs, bits of symbol data */
HYDAMD_EXPORT int hydamd_read_lf_stream(HydAmdContext *ctx, int slot, uint8_t lengths[HYDAMD_LF_CODES], uint32_t *alphabet,
                                        uint32_t *run_pairs, uint32_t *bit_count);
/* the symbol bits, LSB first; capacity >= (bit_count + 7) / 8; bytes of dst beyond the stream's end are zero */
HYDAMD_EXPORT int hydamd_read_lf_bits(HydAmdContext *ctx, int slot, uint8_t *dst, size_t capacity);
/* The frame's LF streams in two copies instead of two per slot: the per-slot records (with the byte
 * offset of each slot's symbol data) and the symbol data of all slots back to back, 4-byte aligned,
 * in slot order.  hydamd_lf_payload_device() is what a multi-GPU job all-gathers. */
typedef struct HydAmdLfInfo {
    uint32_t bit_count, alphabet, run_pairs, error, offset, reserved[3];
    uint8_t lengths[HYDAMD_LF_CODES];
} HydAmdLfInfo;
HYDAMD_EXPORT int hydamd_read_lf_streams(HydAmdContext *ctx, int first_slot, int count, HydAmdLfInfo *dst);
HYDAMD_EXPORT size_t hydamd_lf_payload_size(HydAmdContext *ctx);
HYDAMD_EXPORT const uint8_t *hydamd_lf_payload_device(HydAmdContext *ctx);
HYDAMD_EXPORT int hydamd_read_lf_payload(HydAmdContext *ctx, uint8_t *dst, size_t capacity);
/* unit-test entry: run the device's code construction on one histogram over the compact token space */
HYDAMD_EXPORT int hydamd_debug_lf_code(HydAmdContext *ctx, const uint32_t hist[HYDAMD_LF_CODES],
                                       uint8_t lengths[HYDAMD_LF_CODES], uint32_t codes[HYDAMD_LF_CODES],
                                       uint32_t *alphabet, uint32_t *error);

/* Resource footprint of the transform kernel instance that serves `sample_fmt` on this context (the XYB mode the
 * context runs): static LDS bytes and registers per thread.  LDS is allocated in granules of 1280 bytes and two
 * transform workgroups share a CU with one entropy-stage workgroup only at <= 26 granules: a test holds that line. */
HYDAMD_EXPORT int hydamd_debug_transform_footprint(HydAmdContext *ctx, int sample_fmt, int *lds_bytes, int *registers);
/* the shader clock in MHz as a 20 us single-wavefront kernel on a stream of its own sees it (s_memtime against the 100 MHz
 * s_memrealtime); blocks the caller for those 20 us plus the launch, not the context's stream */
HYDAMD_EXPORT int hydamd_debug_shader_clock_mhz(HydAmdContext *ctx, double *mhz);

/* ---- parity / debug read-backs ---- */
HYDAMD_EXPORT int hydamd_read_symbol_counts(HydAmdContext *ctx, int slot, uint32_t counts[HYDAMD_GROUPS_PER_LFG]);
/* token records of one group: lo = token | cluster<<8 | residue_bits<<16, hi = residue */
HYDAMD_EXPORT int hydamd_read_tokens(HydAmdContext *ctx, int slot, int group, uint64_t *dst, size_t capacity);
/* which: 0 XYB, 1 DCT (float), 2 quantised (int32); dst[c][y][x] with row pitch `pitch` elements */
HYDAMD_EXPORT int hydamd_read_debug_plane(HydAmdContext *ctx, int which, void *dst, size_t pitch, size_t rows);

/* ---- multi-GPU: only the entropy tables of LF group n depend on earlier LF groups, through the
 * running maximum alphabet (reference entropy.c:459-460,952).  A rank that codes LF groups
 * k..k+m of a frame runs the transform stage, exchanges the per-LF-group maxima, sets the maximum
 * over LF groups 0..k-1 as its floor, then runs the entropy stage.  hydamd_finish_frame() is the
 * two stages back to back with floor 0. ---- */
HYDAMD_EXPORT int hydamd_run_transform(HydAmdContext *ctx, int num_slots);
HYDAMD_EXPORT int hydamd_read_alphabet_max(HydAmdContext *ctx, int slot, uint32_t *max_token_plus_one);
HYDAMD_EXPORT int hydamd_set_alphabet_floor(HydAmdContext *ctx, uint32_t floor);
HYDAMD_EXPORT int hydamd_run_entropy(HydAmdContext *ctx, int num_slots);

/* The same exchange without the host in the loop: the per-slot maxima as they sit in device memory
 * ([max_lf_groups] uint32, complete once the transform kernels enqueued so far have run — order your
 * reads behind the context's stream), and a device location the table kernel reads the floor from when
 * it runs (the larger of it and hydamd_set_alphabet_floor's value counts; NULL clears; reset by
 * hydamd_begin_frame).  A job that all-gathers the maxima with RCCL writes its floor there. */
HYDAMD_EXPORT const uint32_t *hydamd_alphabet_max_device(HydAmdContext *ctx);
HYDAMD_EXPORT int hydamd_set_alphabet_floor_device(HydAmdContext *ctx, const uint32_t *floor_on_device);

/* One frame on several devices of ONE process (what hyd_send_tile does when HYDAMD_DEVICES names more than one; no
 * collective library involved): every device's context owns a run of consecutive LF groups in send order.
 *   hydamd_wait_for                   ctx's stream waits, on the device, for everything enqueued so far on peer's
 *                                     stream; peer access from ctx's device to peer's is enabled (xGMI reads).
 *   hydamd_alphabet_floor_from_peers  the floor of ctx's LF groups = the largest token + 1 over the LF groups of the
 *                                     `npeers` contexts that hold the LF groups sent BEFORE ctx's (their transform
 *                                     stages enqueued): a single-wave kernel in ctx's stream reads the peers' maxima
 *                                     in place, behind their transform kernels, and leaves the floor where ctx's
 *                                     table kernel reads it.  Then hydamd_run_entropy / hydamd_finish_frame.
 * The assembler (below) reads blobs of other devices in place: hydamd_wait_for(assembling ctx, peer) first. */
#define HYDAMD_MAX_PEERS 8
HYDAMD_EXPORT int hydamd_context_device(HydAmdContext *ctx);
HYDAMD_EXPORT int hydamd_wait_for(HydAmdContext *ctx, HydAmdContext *peer);
/* 1 if every device of the list can read every other one's memory (hipDeviceCanAccessPeer for every ordered pair of distinct
 * devices; an index that repeats is its own peer), else 0.  hyd_send_tile asks before it deals a frame out to several
 * devices and keeps the frame on one device when the answer is no. */
HYDAMD_EXPORT int hydamd_peers_reachable(const int *devices, int n);
/* Insurance for the peer reads (what HYDAMD_VERIFY_PEERS=1 makes hyd_send_tile do for every sharded frame): a checksum of
 * everything `owner`'s exported view names (view, packed LF streams, HF sections), computed in `reader`'s stream — on the
 * owning device when reader == owner, through peer reads otherwise (hydamd_wait_for(reader, owner) first) — into the
 * reader's result `index` (0 .. HYDAMD_MAX_PEERS - 1); hydamd_verify_read waits for the reader's stream and returns it.
 * The owner's and a reader's sums of one view are equal exactly when the reader saw the bytes the owner wrote. */
HYDAMD_EXPORT int hydamd_verify_enqueue(HydAmdContext *reader, HydAmdContext *owner, int num_slots, int index);
HYDAMD_EXPORT int hydamd_verify_read(HydAmdContext *reader, int index, unsigned long long *sum);
HYDAMD_EXPORT int hydamd_alphabet_floor_from_peers(HydAmdContext *ctx, int npeers, HydAmdContext *const *peers);
/* The other peer read of a sharded frame, checked the same way: *ok = 1 when the floor hydamd_alphabet_floor_from_peers left
 * for ctx's table kernel equals the maximum over the peers' per-LF-group maxima as the HOST copies them from each peer's own
 * device (no peer access involved).  Waits for the frames of ctx and of the peers. */
HYDAMD_EXPORT int hydamd_verify_floor(HydAmdContext *ctx, int npeers, HydAmdContext *const *peers, int *ok);
/* Enqueue the current frame's stages again from the job descriptors the context still holds (pixels stay borrowed), after
 * waiting for what was enqueued before — for a caller that changed an input of the closing stage (hydamd_set_alphabet_floor,
 * hydamd_set_alphabet_floor_device) after hydamd_finish_frame.  hyd_send_tile's through-the-host fallback uses it when a
 * sharded frame's peer reads fail their first-use verification.  Not for batches. */
HYDAMD_EXPORT int hydamd_replay_frame(HydAmdContext *ctx);

/*
 * One self-describing byte string with everything a frame assembler needs from this context's LF
 * groups, built by a kernel in the context's stream right behind the entropy stage: no host
 * synchronisation, one buffer to gather.  Layout: HydAmdBlobHeader, num_slots x HydAmdBlobSlot, the
 * packed LF streams (lf_bytes), then at the next multiple of 16 the packed HF sections (hf_bytes).
 * The LF coder must be on.  `capacity` is the size of the caller's device buffer; a blob that does not
 * fit, or a frame that outgrew the context's buffers, has HYDAMD_BLOB_RETRY set in header.status: call
 * hydamd_sync() (it enlarges and reruns the frame) and export again, into a larger buffer if
 * total_bytes says so.  hydamd_blob_bound() is an upper bound for the context's current capacities.
 */
typedef struct HydAmdBlobHeader {
    uint32_t magic;       /* "HYDB" */
    uint32_t version;     /* 1 */
    uint32_t num_slots;
    uint32_t status;      /* device status word; & HYDAMD_BLOB_RETRY: incomplete, see above; & 1: non-finite float sample */
    uint64_t hf_bytes, lf_bytes, total_bytes;
    uint32_t lf_coded;    /* the slot records carry device-coded LF streams */
    uint32_t reserved[5];
} HydAmdBlobHeader;
#define HYDAMD_BLOB_RETRY 0xEu
typedef struct HydAmdBlobSlot {
    uint32_t preset;                /* = raster id of the LF group in its frame */
    uint32_t running_max_alphabet, log_alphabet_size, table_error;
    uint32_t alphabet[HYDAMD_MAX_CLUSTERS];
    uint32_t reserved[3];           /* [0]: non-zero when the slot held a non-finite float sample (hydamd_set_bad_sample_per_slot on; else 0) */
    uint32_t group_bits[HYDAMD_GROUPS_PER_LFG];
    uint32_t freq[HYDAMD_MAX_CLUSTERS][HYDAMD_ALPHABET];
    HydAmdLfInfo lf;                /* lf.offset is relative to the blob's LF byte string */
} HydAmdBlobSlot;
HYDAMD_EXPORT size_t hydamd_blob_bound(HydAmdContext *ctx, int num_slots);
HYDAMD_EXPORT int hydamd_export_frame(HydAmdContext *ctx, int num_slots, void *device_dst, size_t capacity);
/* The same blob through a device buffer and a pinned host buffer of the context's own: stage (enqueued on the context's
 * stream, behind hydamd_finish_frame), hydamd_sync, read — ONE device-to-host copy of exactly the blob's bytes; *host_blob
 * stays valid until the context's next staged read; *size = 0 (and a blob whose header carries HYDAMD_BLOB_RETRY) when the frame
 * was rerun with larger buffers after it was staged: read the results the separate way then.  What hyd_send_tile uses for the frames it assembles on the host
 * (tile mode): six small read-backs became one. */
HYDAMD_EXPORT int hydamd_stage_frame_blob(HydAmdContext *ctx, int num_slots);
HYDAMD_EXPORT int hydamd_read_frame_blob(HydAmdContext *ctx, int num_slots, const void **host_blob, size_t *size);
/* Host only: a whole one-frame codestream from the blobs of the contexts (ranks) that coded its LF
 * groups, in any order; every LF group of the image must appear exactly once.  *out as for
 * hydamd_frame_from_streams. */
HYDAMD_EXPORT int hydamd_frame_from_blobs(const HYDImageMetadata *md, int write_header, int is_last, size_t nblobs,
                                          const void *const *blobs, const size_t *blob_sizes, const uint8_t *icc,
                                          size_t icc_size, uint8_t **out, size_t *out_len, const char **err);

/*
 * The same assembly ON THE DEVICE: the blobs stay where hydamd_export_frame (or an RCCL gather) left
 * them, kernels write every section into place — LF group sections around their coefficient streams
 * (reference encoder.c:539-629), HFGlobal's histograms (encoder.c:959-967), the TOC (encoder.c:992-1005)
 * — and the finished one-frame codestream lands in one buffer: one copy to the host instead of
 * per-section read-backs and a host-side splice.  The host contributes the bytes that do not depend on
 * the pixels (file and frame header, LFGlobal, constant sub-streams), once per frame description.
 *   hydamd_assembler_plan    describe the frame: which LF groups (raster ids, `lf_ids`) each of the
 *                            `nblobs` blobs carries, blob by blob, slot by slot — this order becomes the
 *                            frame's section order.  Cheap when the description repeats.
 *   hydamd_assembler_run     enqueue the assembly on `hip_stream` (behind whatever fills the blobs):
 *                            `blobs_dev[b]` is a device pointer to blob b (`blob_caps[b]` readable bytes),
 *                            `out` any device-accessible buffer of `out_cap` bytes (device memory, or
 *                            pinned host memory for frames that should land on the host directly).
 *                            Alignment: `out` 4 bytes, every blob 16 bytes (the copy kernel moves whole
 *                            words and 16-byte records); anything else is HYD_API_ERROR.
 *   hydamd_assembler_result  after the stream has been synchronised: the frame's size; HYD_NEED_MORE_OUTPUT
 *                            (with *size = bytes needed) if `out_cap` was too small; HYD_API_ERROR for a
 *                            blob that is malformed, incomplete (rerun the shard) or carries NaN input.
 * Frames of a single 256x256 group are one bit-contiguous section and stay with hydamd_frame_from_blobs.
 * One assembler serves one frame at a time (its scratch is reused by the next hydamd_assembler_run).
 */
typedef struct HydAmdAssembler HydAmdAssembler;
HYDAMD_EXPORT HydAmdAssembler *hydamd_assembler_create(int device, int *status);
HYDAMD_EXPORT void hydamd_assembler_destroy(HydAmdAssembler *a);
HYDAMD_EXPORT const char *hydamd_assembler_error(HydAmdAssembler *a);
HYDAMD_EXPORT int hydamd_assembler_plan(HydAmdAssembler *a, const HYDImageMetadata *md, int write_header, int is_last,
                                        size_t nblobs, const uint32_t *blob_slots, const uint32_t *lf_ids, const uint8_t *icc,
                                        size_t icc_size);
HYDAMD_EXPORT int hydamd_assembler_run(HydAmdAssembler *a, const void *const *blobs_dev, const size_t *blob_caps, void *hip_stream,
                                       void *out, size_t out_cap);
HYDAMD_EXPORT int hydamd_assembler_result(HydAmdAssembler *a, size_t *size);
/* `out` == NULL in hydamd_assembler_run: the frame goes to a device buffer the assembler owns — of `out_cap` bytes, or,
 * with out_cap == 0, sized from the blob capacities (self-contained blobs only: a view's capacity says nothing about
 * its frame; hydamd_blob_bound() of the exporting context is an upper bound for it) — and this copies it to host
 * memory once hydamd_assembler_result has said how large it is. */
HYDAMD_EXPORT int hydamd_assembler_read(HydAmdAssembler *a, uint8_t *dst, size_t capacity);
/* A context's own way to both: the blob of slots [0, num_slots) as a VIEW — header and slot records in a small device
 * buffer the context keeps, the packed LF streams and HF sections left where the context has them, their addresses in
 * the header (lf_coded = 0x101) — for an assembler on the same device and stream, valid until the context's next frame:
 * nothing of the frame's bulk is copied.  hydamd_frame_from_blobs does not take views.  *capacity receives the readable
 * bytes at *blob_dev.  And an assembler that lives and is parked with the context.  hyd_send_tile builds its frames
 * with these. */
HYDAMD_EXPORT int hydamd_export_frame_owned(HydAmdContext *ctx, int num_slots, const void **blob_dev, size_t *capacity);
HYDAMD_EXPORT HydAmdAssembler *hydamd_context_assembler(HydAmdContext *ctx);
/* The results of a BATCH of frames (hydamd_begin_batch(ctx, n, frames): n = 1 for tile-mode frames, the LF groups of the
 * shape for hydamd_encode_image_batch) as such a view: one header, the slot records of all `num_slots` = frames x n slots —
 * frame k's at k n .. k n + n - 1 —, the packed LF streams and HF sections left in place.  Where slot s's bytes sit in those
 * two strings follows from every slot before it, so the view states it: *extents_dev is a device array of num_slots
 * HydAmdBatchExtent, written by a kernel behind the export in the context's stream; a frame's HF sections reach from its
 * first slot's hf_offset to its last slot's hf_offset + hf_bytes.  Valid until the context's next frame.
 * hydamd_export_frame* keeps refusing batches. */
typedef struct HydAmdBatchExtent {
    uint64_t lf_offset, lf_bytes; /* in the packed LF streams (= the slot record's lf.offset, and its bit count rounded up) */
    uint64_t hf_offset, hf_bytes; /* in the packed HF sections: the slot's byte-padded group sections, raster order */
} HydAmdBatchExtent;
HYDAMD_EXPORT int hydamd_export_batch_owned(HydAmdContext *ctx, int num_slots, const void **blob_dev, size_t *capacity,
                                            const void **extents_dev);

/*
 * Wrap LF-group results — from this or other GPUs — into codestream bytes (host only, no GPU).
 *   md            image metadata, as for hyd_set_metadata (one-frame mode: every LF group must be present)
 *   tile_xy       [lfg_count][2] tile coordinates, in the order the sections appear in `payload`
 *   dc            [lfg_count] pointers to LF ints as hydamd_read_dc returns them
 *   freq/alphabet [lfg_count][9][128] / [lfg_count][9] as hydamd_read_tables returns them
 *   group_bits    [lfg_count][64] as hydamd_read_sections returns them
 *   max_alphabet  final running maximum (largest running_max_alphabet of any LF group)
 *   payload       the packed HF sections of all LF groups, concatenated in the same order
 * On success *out is a malloc'ed buffer (release with hydamd_free) holding the file header (if
 * write_header) and the frame.
 */
HYDAMD_EXPORT int hydamd_frame_from_results(const HYDImageMetadata *md, int write_header, int is_last, size_t lfg_count,
                                            const uint32_t *tile_xy, const int32_t *const *dc, const uint32_t *freq,
                                            const uint32_t *alphabet, const uint32_t *group_bits, unsigned max_alphabet,
                                            const uint8_t *payload, size_t payload_len, const uint8_t *icc,
                                            size_t icc_size, uint8_t **out, size_t *out_len, const char **err);
/* The same with LF groups whose coefficient streams were coded on the GPU (hydamd_read_lf_stream /
 * hydamd_read_lf_bits) instead of LF ints: what a multi-GPU job gathers when the LF coder is on. */
typedef struct HydAmdLfStream {
    const uint8_t *lengths;  /* [HYDAMD_LF_CODES] */
    uint32_t alphabet, run_pairs;
    const uint8_t *bits;     /* (bit_count + 7) / 8 bytes */
    uint64_t bit_count;
} HydAmdLfStream;
HYDAMD_EXPORT int hydamd_frame_from_streams(const HYDImageMetadata *md, int write_header, int is_last, size_t lfg_count,
                                            const uint32_t *tile_xy, const HydAmdLfStream *lf, const uint32_t *freq,
                                            const uint32_t *alphabet, const uint32_t *group_bits, unsigned max_alphabet,
                                            const uint8_t *payload, size_t payload_len, const uint8_t *icc,
                                            size_t icc_size, uint8_t **out, size_t *out_len, const char **err);
/* Releases a buffer returned by hydamd_frame_from_*.  The library may keep it for the next frame it
 * assembles (mapped pages: a fresh 50 MB buffer costs 8 ms of page faults): up to four buffers of 1 MB to
 * 256 MB each per process, i.e. at most 1 GB of host memory; the next frame or encoder takes the smallest
 * one that fits it.  The buffer behind *out may therefore be larger than out_len.  hydamd_trim_cache()
 * lets go of all of them. */
HYDAMD_EXPORT void hydamd_free(void *p);

/* hyd_encoder_destroy parks its device context (device memory, pinned staging, streams) for the next
 * encoder of the same shape instead of freeing it — up to HYDAMD_CONTEXT_CACHE contexts (default 16, at most 32) and
 * HYDAMD_CONTEXT_CACHE_MB megabytes (default 8192) per process.  This releases whatever is parked, and the spare
 * frame buffers hydamd_free may have kept. */
HYDAMD_EXPORT void hydamd_trim_cache(void);

/* ---- knobs of the drop-in encoder (HYDEncoder of libhydrium.h) that the reference has no counterpart for ----
 * Tile mode (tile_size_shift >= 0): every tile is a frame, and by default — as in the reference
 * (src/libhydrium/libhydrium.c:147-203, encoder.c:339-378) — hyd_send_tile returns with that frame complete.
 * hydamd_set_tile_pipeline(e, depth) lets up to `depth` (2..8) tile frames be in flight instead: a call launches
 * its tile and collects the frame launched `depth` calls earlier, the final tile's call collects the rest; the
 * bytes are the same, in the same order, up to depth - 1 calls later (4-5x the tile rate: a tile costs 2-3 ms of
 * latency however small it is), a NaN or device error is reported by the call that collects the frame, and an
 * encoder destroyed before its final tile drops what is still in flight.  depth 1 = the reference's timing;
 * 0 = the process default (environment HYDAMD_TILE_PIPELINE, else 1).  HYD_API_ERROR while frames are in flight. */
HYDAMD_EXPORT int hydamd_set_tile_pipeline(HYDEncoder *encoder, int depth);
HYDAMD_EXPORT int hydamd_get_tile_pipeline(const HYDEncoder *encoder);

/* ---- optional per-kernel timing with HIP events on the context's stream ---- */
HYDAMD_EXPORT int hydamd_profile(HydAmdContext *ctx, int enable);
/* accumulated milliseconds and launch counts per kernel class since the last call; resets the counters */
HYDAMD_EXPORT int hydamd_profile_read(HydAmdContext *ctx, double ms[HYDAMD_K_COUNT], uint64_t launches[HYDAMD_K_COUNT]);

/*
 * ONE frame whose pixels already sit in HBM, on N devices of ONE process (csrc/host/multi.c; the composition of the calls
 * above that hyd_send_tile's multi-device scheduler makes for host tiles — reference libhydrium.c:172-203,
 * encoder.c:928-957 — without the uploads, which bound that path at any N).  No collective library, no process group:
 * LF groups dealt in raster runs (shard d: groups d * total / N .. (d + 1) * total / N - 1), the alphabet floor by peer
 * read, every shard's blob a view, the assembling shard's GPU reading all of them in place (the other devices' over xGMI)
 * and writing the finished FILE (header included) into its own memory.
 *   hydamd_multi_create        contexts for the image's shape, one per entry of `devices` (an index may repeat: several
 *                              shards on one GPU); HYD_INTERNAL_ERROR in *status when the devices cannot read each other.
 *   hydamd_encode_image_multi  enqueue one frame; returns without waiting.  `src` holds three pointers per shard
 *                              ([shard][channel]) in THAT shard's device memory: where pixel (0, 0) of the image would sit
 *                              in the shard's buffer — only the pixels of the shard's own LF groups are read, so a slab of
 *                              rows [y0, y1) passes slab - y0 * row_stride.  Strides in samples, sample_fmt as
 *                              hyd_send_tile's.  `assembling_shard` picks the GPU that builds the file (rotate it per frame:
 *                              the file's copy to the host then leaves through another GPU's link each time).
 *   hydamd_multi_result        wait for the frame; reruns what a shard that outgrew its buffers invalidated (its own frame
 *                              inside hydamd_sync, the later shards' floors and frames, the assembly).  *size = bytes of
 *                              the file.  A peer read that fails its first-use verification (see HYDAMD_VERIFY_PEERS in
 *                              INTEGRATION.md) is HYD_INTERNAL_ERROR with the device pair in hydamd_multi_error.
 *   hydamd_multi_read          the file to host memory, one copy from the assembling device.
 * One frame in flight per HydAmdMulti; keep several for a queue of frames (bench.py's shard_16k_inprocess leg keeps four).
 */
typedef struct HydAmdMulti HydAmdMulti;
HYDAMD_EXPORT HydAmdMulti *hydamd_multi_create(int n, const int *devices, const HYDImageMetadata *md, int *status);
HYDAMD_EXPORT void hydamd_multi_destroy(HydAmdMulti *m);
HYDAMD_EXPORT const char *hydamd_multi_error(HydAmdMulti *m);
HYDAMD_EXPORT HydAmdContext *hydamd_multi_context(HydAmdMulti *m, int shard);
HYDAMD_EXPORT int hydamd_multi_shard_lf_groups(HydAmdMulti *m, int shard, size_t *first, size_t *count);
HYDAMD_EXPORT int hydamd_encode_image_multi(HydAmdMulti *m, const void *const *src, ptrdiff_t row_stride, ptrdiff_t pixel_stride,
                                            int sample_fmt, int assembling_shard);
HYDAMD_EXPORT int hydamd_multi_result(HydAmdMulti *m, size_t *size);
HYDAMD_EXPORT int hydamd_multi_read(HydAmdMulti *m, uint8_t *dst, size_t capacity);

/*
 * A TILE-MODE image whose pixels already sit in HBM, frames built on the GPU (csrc/host/tiled.c, csrc/hip/assemble_tiles.hip).
 * Tile mode (both tile_size_shift_x/y 0..3: tiles of 256..2048 pixels, reference libhydrium.c:147-203) codes every tile
 * as a Frame of its own and is the only way to code an image one frame cannot hold (more than 255 LF groups, or 128).
 * A tile is one LF group, so the tiles are coded in LAUNCH GROUPS of up to `tiles_per_launch` independent frames
 * (hydamd_begin_batch(ctx, 1, n)); one launch sequence behind each group's entropy stage writes its frames — header, TOC,
 * LF group, HFGlobal, HF sections; frames of a single 256x256 group as one bit-contiguous section — back to back behind
 * the frames of the groups before it, at a running offset kept in device memory.  The host contributes the bytes that do
 * not depend on the pixels, once per object, and waits once per launch group (never per tile).
 *   hydamd_tiled_create        md: the image, both shifts 0..3.  tiles_per_launch: 0 = default (32), at most 255; an
 *                              LF-group slot of the context costs 70-100 MB whatever the tile size, so the default
 *                              object holds about 3 GB plus the output buffer.  One device per object.
 *   hydamd_encode_image_tiled  src / strides / sample_fmt as hydamd_encode_image's (device pointers, strides in samples),
 *                              for the image's first pixel; tiles in raster order, edge tiles clipped as hyd_send_tile
 *                              clips them, the file header in front of tile 0, is_last on the final tile.  Enqueues the
 *                              first launch group and returns; the pixels stay borrowed until hydamd_tiled_result.
 *   hydamd_tiled_result        runs the remaining launch groups and waits; *size = bytes of the finished FILE, which sits
 *                              in device memory (hydamd_tiled_device).  A launch group that outgrew the context's buffers
 *                              is rerun inside hydamd_sync and assembled again before the next group starts, so later
 *                              frames land where its real sizes put them; an output buffer that proves too small is grown
 *                              and the group's assembly repeated (never HYD_NEED_MORE_OUTPUT).  A non-finite float sample:
 *                              HYD_API_ERROR "Invalid NaN Float"; the stream is drained and the object stays usable.
 *   hydamd_tiled_read          the file to host memory, one copy.
 * HYD_API_ERROR: a shift of -1, a null pointer, a bad sample format, a second encode while an image is in flight,
 * result or read without an image.  (An ICC profile belongs to one-frame mode only, as in the reference: there is no way
 * to pass one.)  hydamd_tiled_overflow_reruns: launch groups run twice because a buffer was too small.
 */
typedef struct HydAmdTiled HydAmdTiled;
HYDAMD_EXPORT HydAmdTiled *hydamd_tiled_create(int device, const HYDImageMetadata *md, int tiles_per_launch, int *status);
HYDAMD_EXPORT void hydamd_tiled_destroy(HydAmdTiled *t);
HYDAMD_EXPORT const char *hydamd_tiled_error(HydAmdTiled *t);
HYDAMD_EXPORT int hydamd_encode_image_tiled(HydAmdTiled *t, const void *const src[3], ptrdiff_t row_stride, ptrdiff_t pixel_stride,
                                            int sample_fmt);
HYDAMD_EXPORT int hydamd_tiled_result(HydAmdTiled *t, size_t *size);
HYDAMD_EXPORT int hydamd_tiled_read(HydAmdTiled *t, uint8_t *dst, size_t capacity);
HYDAMD_EXPORT const uint8_t *hydamd_tiled_device(HydAmdTiled *t);
HYDAMD_EXPORT unsigned hydamd_tiled_overflow_reruns(HydAmdTiled *t);
/* device memory the object holds right now (context arrays are estimated from its capacities; output buffer exact) */
HYDAMD_EXPORT size_t hydamd_tiled_device_bytes(HydAmdTiled *t);

/*
 * A BATCH of one-frame images whose pixels already sit in HBM, every one a finished FILE, built on the GPU
 * (csrc/host/batch.c, csrc/hip/assemble_batch.hip) — for a queue of 4K/8K frames in device memory of which each must
 * become a .jxl (a video pipeline).  hydamd_encode_image_batch codes `frames` independent pictures of one shape as one
 * launch group, their serial rANS chains side by side; one launch sequence behind its entropy stage then writes every
 * frame — file header, frame header with is_last, TOC, LFGlobal, LF groups, HFGlobal, HF sections; frames of a single
 * 256x256 group as one bit-contiguous section — exactly as the reference writes that picture alone, the files back to
 * back at byte granularity in ONE device buffer the object owns, with the table of their offsets beside it.  The host
 * contributes the bytes that do not depend on the pixels, once per object, and waits once per batch.
 *   hydamd_batch_create          md: a one-frame image (both tile_size_shift -1) of n = LF groups; max_frames: frames a batch
 *                                may hold, max_frames x n <= 255 (the slots of the object's one context; n = 128 and
 *                                n > 255 cannot be one frame).  icc: optional profile, written into every file as
 *                                hydamd_assembler_plan writes it.  One device and one stream per object.
 *   hydamd_encode_batch          `frames` <= max_frames pictures of the object's shape: src[3 k .. 3 k + 2] are frame k's
 *                                channel pointers (device memory), strides in samples and sample_fmt as
 *                                hydamd_encode_image_batch's.  Enqueues the batch and its assembly and returns; the
 *                                pixels stay borrowed until hydamd_batch_result.  (An object's first batch allocates
 *                                the output buffer, for max_frames, before it enqueues anything.)
 *   hydamd_batch_result          waits; *total_bytes = bytes of all files.  A batch that outgrew the context's buffers is
 *                                rerun inside hydamd_sync and exported and assembled again first; the output buffer is
 *                                sized from the context's capacities (never HYD_NEED_MORE_OUTPUT).  By default a non-finite
 *                                float sample ANYWHERE fails the WHOLE batch — HYD_API_ERROR "Invalid NaN Float" (see
 *                                hydamd_batch_set_image_errors).  After a failure the stream is drained and the object
 *                                stays usable.
 *   hydamd_batch_set_image_errors  per_image != 0: an outcome per image instead.  The context records non-finite samples
 *                                per slot (hydamd_set_bad_sample_per_slot) and the assembly gives an image ANY of whose LF
 *                                groups is flagged no bytes: hydamd_batch_result returns HYD_OK, *total_bytes counts the
 *                                delivered files only (0 when every image is flagged), offsets[k + 1] == offsets[k] and
 *                                hydamd_batch_read copies 0 bytes for such an image, and the files on both sides of it
 *                                still meet at byte granularity.  Every other error fails the batch as before.  0
 *                                (default): as above.  HYD_API_ERROR while a batch is in flight.
 *   hydamd_batch_image_status    after hydamd_batch_result: status[k] for the batch's `frames` images, 0 = a file,
 *                                HYDAMD_IMAGE_BAD_SAMPLE = a non-finite sample, no bytes.  All zeros with the switch off.
 *   hydamd_batch_image_status_device  the same words (uint32, `frames` of them) in device memory, beside the offsets table.
 *   hydamd_batch_offsets         offsets[k] .. offsets[k + 1] bound file k; offsets[0] = 0, offsets[frames] = total.
 *   hydamd_batch_device,         the files and the same table (frames + 1 entries) in device memory, for a consumer
 *   hydamd_batch_offsets_device  that never leaves the GPU.  Everything is valid until the object's next hydamd_encode_batch.
 *   hydamd_batch_read            file `frame` (or, with -1, all of them back to back) to host memory, one copy.
 * HYD_API_ERROR: a shift other than -1, max_frames out of range, a null pointer, a bad sample format, `frames` out of
 * range, a second encode while a batch is in flight, result / offsets / read without a batch, a destination that is too
 * small.  hydamd_batch_overflow_reruns: batches run twice because a buffer was too small.  Keep several objects for a
 * deeper queue (scripts/batch_files_probe.py keeps four).
 */
typedef struct HydAmdBatch HydAmdBatch;
HYDAMD_EXPORT HydAmdBatch *hydamd_batch_create(int device, const HYDImageMetadata *md, int max_frames, const uint8_t *icc, size_t icc_size,
                                               int *status);
HYDAMD_EXPORT void hydamd_batch_destroy(HydAmdBatch *b);
HYDAMD_EXPORT const char *hydamd_batch_error(HydAmdBatch *b);
HYDAMD_EXPORT int hydamd_encode_batch(HydAmdBatch *b, int frames, const void *const *src, ptrdiff_t row_stride, ptrdiff_t pixel_stride,
                                      int sample_fmt);
HYDAMD_EXPORT int hydamd_batch_result(HydAmdBatch *b, size_t *total_bytes);
HYDAMD_EXPORT int hydamd_batch_offsets(HydAmdBatch *b, uint64_t *offsets);
HYDAMD_EXPORT const uint8_t *hydamd_batch_device(HydAmdBatch *b);
HYDAMD_EXPORT const uint64_t *hydamd_batch_offsets_device(HydAmdBatch *b);
HYDAMD_EXPORT int hydamd_batch_read(HydAmdBatch *b, int frame, uint8_t *dst, size_t capacity);
HYDAMD_EXPORT unsigned hydamd_batch_overflow_reruns(HydAmdBatch *b);
#define HYDAMD_IMAGE_BAD_SAMPLE 1u
HYDAMD_EXPORT int hydamd_batch_set_image_errors(HydAmdBatch *b, int per_image);
HYDAMD_EXPORT int hydamd_batch_image_status(HydAmdBatch *b, uint32_t *status);
HYDAMD_EXPORT const uint32_t *hydamd_batch_image_status_device(HydAmdBatch *b);

/*
 * A batch of one-frame images EACH OF ITS OWN SIZE whose pixels already sit in HBM, every one a finished FILE, built on
 * the GPU (csrc/host/mixed.c, csrc/hip/assemble_batch.hip) — for a queue of pictures of many sizes in device memory
 * (thumbnails, product shots, crops, the output of a GPU decoder), which hydamd_batch_* would need one object per shape
 * for.  Every image is at most 2048 x 2048 pixels, ONE LF group (hydamd_mixed_create), or up to 28 LF groups — 117
 * Mpixel, e.g. 14336 x 8192 — (hydamd_mixed_create_slots); the images of a batch are coded as one launch group
 * (hydamd_begin_batch(ctx, 1, frames), each LF group of its own size, as a tile-mode image's ragged tiles are;
 * hydamd_begin_batch_frames where images may hold several LF groups), and the
 * launch sequence behind hydamd_batch_*'s entropy stage writes every frame — file header, frame header with is_last, TOC,
 * LFGlobal, LF group, HFGlobal, HF sections; images of a single 256x256 group as one bit-contiguous section — exactly as
 * the reference writes that picture alone with tile_size_shift_x = tile_size_shift_y = -1, the files back to back at byte
 * granularity in ONE device buffer the object owns, with the table of their offsets beside it.  The host contributes
 * the bytes that do not depend on the pixels — a plan per batch, a record per distinct size and one per image, uploaded
 * in the stream; a batch whose list of sizes equals the previous batch's reuses the plan on the device — and waits once
 * per batch.  The protocol is hydamd_batch_*'s, call for call.
 *   hydamd_mixed_create          max_frames: images a batch may hold, 1..255 (the slots of the object's one context),
 *                                0 = default (32); an LF-group slot of the context costs 70-100 MB of device memory
 *                                whatever the image sizes, so the default object holds about 3 GB plus the output
 *                                buffer, one of 255 about 22 GB.  linear_light: as HYDImageMetadata's, for every image.
 *                                One device and one stream per object.
 *   hydamd_mixed_create_slots    as hydamd_mixed_create, with max_lf_groups (max_frames..255) slots in the object's context:
 *                                an image may then hold up to 28 LF groups, a batch up to max_frames images and
 *                                max_lf_groups LF groups in all.  28: up to there a frame clusters nine ways whatever its
 *                                LF-group count, so one chain launch serves frames of 1, 4 and 9 LF groups side by side;
 *                                what differs per frame (the width of the preset field, where the alphabet maximum
 *                                restarts, the frame's plan) travels per slot and per frame.
 *   hydamd_encode_mixed          `frames` <= max_frames images: images[k].src are image k's channel pointers (device
 *                                memory, its first pixel), row_stride / pixel_stride in samples as hyd_send_tile's,
 *                                width and height 1..2048 (hydamd_mixed_create_slots: at least 1, at most 28 LF groups of
 *                                2048 x 2048, the batch's LF groups at most max_lf_groups); one sample_fmt for the whole call
 *                                (hydamd_encode_mixed_formats: one per image).  Enqueues the batch and
 *                                its assembly and returns; the pixels stay borrowed until hydamd_mixed_result, the
 *                                descriptors only for the call.  The output buffer is sized before anything is
 *                                enqueued, from the batch's plan and the context's capacities.
 *   hydamd_encode_mixed_formats  the same with image k's samples in sample_fmts[k] (HYD_UINT8 / HYD_UINT16 / HYD_FLOAT32 / HYDAMD_FLOAT16 / HYDAMD_BFLOAT16 / HYDAMD_NV12_* / HYDAMD_P01x_* / HYDAMD_I4xx_*):
 *                                8-bit, 16-bit and float pictures side by side in one launch group, every file what the
 *                                reference writes for that picture in its format.  A bad entry is HYD_API_ERROR "Invalid
 *                                Sample Format" with nothing enqueued.  The plan and its reuse depend on sizes only.
 *   hydamd_mixed_result          waits; *total_bytes = bytes of all files.  A batch that outgrew the context's buffers is
 *                                rerun inside hydamd_sync and exported and assembled again first (never
 *                                HYD_NEED_MORE_OUTPUT).  By default a non-finite float sample ANYWHERE fails the WHOLE
 *                                batch — HYD_API_ERROR "Invalid NaN Float".  After a failure the stream is drained and
 *                                the object stays usable.
 *   hydamd_mixed_set_image_errors, hydamd_mixed_image_status, hydamd_mixed_image_status_device
 *                                an outcome per image, exactly as hydamd_batch_set_image_errors and its companions: an
 *                                image with a non-finite sample in ANY of its LF groups yields no bytes and status
 *                                HYDAMD_IMAGE_BAD_SAMPLE, the others their files; the rerun of a batch that outgrew its
 *                                buffers arrives at the same outcomes.
 *   hydamd_mixed_offsets         offsets[k] .. offsets[k + 1] bound file k; offsets[0] = 0, offsets[frames] = total.
 *   hydamd_mixed_device,         the files and the same table (frames + 1 entries) in device memory.  Everything is
 *   hydamd_mixed_offsets_device  valid until the object's next hydamd_encode_mixed.
 *   hydamd_mixed_read            file `frame` (or, with -1, all of them back to back) to host memory, one copy.
 * HYD_API_ERROR: max_frames or max_lf_groups out of range, a null descriptor array or channel pointer, a width or height of
 * 0 or above 2048 (hydamd_mixed_create_slots: an image of more than 28 LF groups, a batch of more LF groups than
 * max_lf_groups), `frames` outside 1..max_frames, a bad sample format, a second encode while a batch is in flight, result / offsets
 * / read without a batch, a destination that is too small.  No usable device at creation: HYD_INTERNAL_ERROR.
 * hydamd_mixed_overflow_reruns: batches run twice because a buffer was too small.  Keep several objects for a deeper
 * queue (scripts/mixed_batch_probe.py keeps four).
 * OUT OF SCOPE: images of more than 28 LF groups (other cluster schemes would need chain launches per cluster count: such
 * images go through one hydamd_batch_* object per shape, or hydamd_encode_image); an ICC profile (it would sit in
 * every frame's prefix); several devices per object; outcomes per image for hydamd_tiled_* and hydamd_multi_* (one image, one
 * outcome);
 * closing the throughput gap to the padded-classes upper reference that profiles/mixed_batch.txt records.
 */
typedef struct HydAmdImageDesc {
    const void *src[3];                 /* device pointers: R, G, B of the image's first pixel (HYDAMD_NV12_*: Y, U, U + 1; planar YCbCr: Y, U, V, and pixel_stride the chroma pitch) */
    ptrdiff_t row_stride, pixel_stride; /* in samples, as hyd_send_tile's */
    size_t width, height;               /* 1..2048 each; hydamd_mixed_create_slots: >= 1, at most 28 LF groups of 2048 x 2048 */
} HydAmdImageDesc;
typedef struct HydAmdMixed HydAmdMixed;
HYDAMD_EXPORT HydAmdMixed *hydamd_mixed_create(int device, int max_frames, int linear_light, int *status);
HYDAMD_EXPORT HydAmdMixed *hydamd_mixed_create_slots(int device, int max_frames, int max_lf_groups, int linear_light, int *status);
HYDAMD_EXPORT void hydamd_mixed_destroy(HydAmdMixed *m);
HYDAMD_EXPORT const char *hydamd_mixed_error(HydAmdMixed *m);
HYDAMD_EXPORT int hydamd_encode_mixed(HydAmdMixed *m, int frames, const HydAmdImageDesc *images, int sample_fmt);
HYDAMD_EXPORT int hydamd_encode_mixed_formats(HydAmdMixed *m, int frames, const HydAmdImageDesc *images, const int *sample_fmts);
HYDAMD_EXPORT int hydamd_mixed_result(HydAmdMixed *m, size_t *total_bytes);
HYDAMD_EXPORT int hydamd_mixed_offsets(HydAmdMixed *m, uint64_t *offsets);
HYDAMD_EXPORT const uint8_t *hydamd_mixed_device(HydAmdMixed *m);
HYDAMD_EXPORT const uint64_t *hydamd_mixed_offsets_device(HydAmdMixed *m);
HYDAMD_EXPORT int hydamd_mixed_read(HydAmdMixed *m, int frame, uint8_t *dst, size_t capacity);
HYDAMD_EXPORT unsigned hydamd_mixed_overflow_reruns(HydAmdMixed *m);
HYDAMD_EXPORT int hydamd_mixed_set_image_errors(HydAmdMixed *m, int per_image);
HYDAMD_EXPORT int hydamd_mixed_image_status(HydAmdMixed *m, uint32_t *status);
HYDAMD_EXPORT const uint32_t *hydamd_mixed_image_status_device(HydAmdMixed *m);

#ifdef __cplusplus
}
#endif

#endif /* HYDRIUM_AMD_H_ */
