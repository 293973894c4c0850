/*
 * lf_coder.hip — the LF-group coder on the GPU.
 *
 * What it replaces (file:line relative to /root/reference/src/libhydrium/): the LF-coefficient
 * sub-stream of write_lf_group (encoder.c:560-596): clamped-gradient prediction of the LF ints,
 * hyd_entropy_send_symbol with LZ77 used as run-length coding (entropy.c:473-524), the
 * depth-limited Huffman construction with its selection order (entropy.c:577-662), canonical code
 * assignment (entropy.c:664-707) and the symbol write-out (entropy.c:1003-1021).  The constant
 * sub-streams around it (MA tree, HF metadata) and the code-length header stay on the host
 * (csrc/host/frame.c), which receives the code lengths and the packed symbol bits from here.
 *
 * The stream is one value sequence per LF group: channels Y, X, B, raster inside a channel,
 * n = 3 * vbw * vbh <= 196608 values.  Everything is cut into windows that one 256-thread workgroup
 * handles, so that an LF group is hundreds of small, short-lived workgroups that fit beside whatever
 * else the GPU is running (a 1024-thread workgroup per LF group, as in round 1, had to wait for a
 * compute unit with sixteen free wave slots and then held half of its registers for a millisecond:
 * 16 % of the pipelined frame rate for 1.5 % of its instructions):
 *
 *   k_lf_tokens   one workgroup per 896 values: residuals -> run structure -> one 8-byte record per
 *                 value + token histogram.  A maximal run of equal values is cut into chunks of 128:
 *                 the chunk's first value is a literal; the r <= 127 repeats behind it become one (run
 *                 token r - 3, distance) pair when r > 3 and r literals otherwise.  What a position
 *                 emits therefore depends only on its offset in its run and on at most 127 values
 *                 ahead: the workgroup looks at a window of 1024 values and finds the run its first
 *                 value continues by a (parallel) backward scan.
 *   k_lf_huffman  one wavefront per LF group: the reference's O(n^2) selection loop with the two
 *                 smallest candidates found by a wave-wide minimum over a total order that reproduces
 *                 its comparator and slot-visiting order; subtree depth recursion replaced by subtree
 *                 heights and a parent walk.  Runs in a compact slot space (only the slots the
 *                 16509-entry alphabet can ever touch) with all candidates held in registers: no
 *                 LDS traffic or barrier inside the merge loop.
 *                 The same wavefront then turns the code lengths into the bits of each window (its
 *                 token histogram times the lengths, plus its residue bits) and their exclusive prefix
 *                 sum (lf_huffman.h lf_window_offsets_wave): no kernel of its own does that.
 *   k_lf_pack     one workgroup per window: per-value bit strings (<= 59 bits) ORed into an LDS
 *                 window at the window's bit offset, whole words stored; of the two words a window may
 *                 share with its neighbours it replaces exactly its own bits (a bit mask: atomic AND,
 *                 then atomic OR), so nothing clears them first; LSB-first like HYDBitWriter
 *                 (bitwriter.c:110-124).
 *   k_lf_gather   one workgroup per LF group: the slot's staged words (lf_bits) copied behind those of
 *                 the slots in front of it, 4-byte aligned (lf_packed).
 *
 * The window work itself (what a token and a pack workgroup do) lives in lf_windows.h, because the
 * frame loop does not launch these kernels: when one entropy launch codes all LF groups of a lane-form
 * launch group with the in-stream coder, the token workgroups ride in the table kernel's launch and
 * the pack workgroups in the emit kernel's (kernels.hip k_build_tables, k_rans_emit<true>), and the
 * pack workgroups write straight into lf_packed at the offsets the bit counts give: no staging, no
 * gather.  The kernels here serve the routes that code LF groups on their own or a few at a time —
 * hydamd_run_lf_coder's growing calls, the side stream, the late coder of a frame's closing stage,
 * wave-form and float frames — which stage every slot's stream in lf_bits and gather once the frame's
 * last LF group is coded, and HYDAMD_LF_CODES_RIDE=tables, whose code builders in the table launch need
 * k_lf_tokens finished in front of it.
 *
 * The work is small (<= 196608 values per 4.2 Mpx LF group); it exists so that a frame's sections are
 * complete on the device and the host's per-frame serial work disappears.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hydk_common.h"

namespace {

#include "lf_huffman.h"
#include "lf_windows.h" /* HYDK_LF_WPB, HYDK_LF_PROBE; the token and the pack role */

/* ==========================================================================================
 * The kernels.  All workgroups are 256 threads and live for microseconds.
 * ======================================================================================== */
/* grid = (windows of 896 values, LF groups); hist_all must be zero on entry */
__global__ __launch_bounds__(kLfThreads) void k_lf_tokens(const HydkLfJob *__restrict__ jobs,
                                                          unsigned long long *__restrict__ recs_all,
                                                          uint32_t *__restrict__ hist_all, LfWork *__restrict__ work) {
    __shared__ LfTokenLds s_lds;
    const int slot = blockIdx.y;
    lf_tokens_role(jobs[slot], recs_all + (size_t)slot * HYDK_LF_SYMBOLS, hist_all + (size_t)slot * HYDK_LF_CODES, work[slot],
                   (int)blockIdx.x, s_lds);
}

/* grid = LF groups, block = 64: code lengths + canonical codes of each LF group's histogram */
__global__ __launch_bounds__(64) void k_lf_codes(const HydkLfJob *__restrict__ jobs, const uint32_t *__restrict__ hist_all,
                                                 HydkLfStream *__restrict__ streams, LfWork *__restrict__ work) {
    if (!(HYDK_LF_PROBE & 1))
        __builtin_amdgcn_s_setprio(3); /* late work of a frame whose stream holds nothing else: see kernels.hip HYDK_URGENT */
    __shared__ LfHuffScratch s_huff;
    const int slot = blockIdx.x;
    lf_code_and_offsets_wave(hist_all + (size_t)slot * HYDK_LF_CODES, work[slot], streams + slot, jobs[slot], s_huff, (int)threadIdx.x);
}

/* grid = (windows of 896 values, LF groups): every slot's stream staged in its own HYDK_LF_BITWORDS words */
__global__ __launch_bounds__(kLfThreads) void k_lf_pack(const HydkLfJob *__restrict__ jobs,
                                                        const unsigned long long *__restrict__ recs_all,
                                                        const LfWork *__restrict__ work,
                                                        const HydkLfStream *__restrict__ streams, uint32_t *__restrict__ bits_all) {
    __shared__ LfPackLds s_lds;
    const int slot = blockIdx.y;
    lf_pack_role(jobs[slot], recs_all + (size_t)slot * HYDK_LF_SYMBOLS, work[slot], streams[slot],
                 bits_all + (size_t)slot * HYDK_LF_BITWORDS, (uint32_t)HYDK_LF_BITWORDS, (int)blockIdx.x, s_lds);
}

/* The LF groups' symbol data, 4-byte aligned, back to back in slot order: one copy (or one
 * all-gather) moves a frame's LF streams.  grid = LF groups, block = 256. */
__global__ __launch_bounds__(256) void k_lf_gather(HydkLfStream *__restrict__ streams, const uint32_t *__restrict__ bits_all,
                                                   uint32_t *__restrict__ packed, unsigned long long *__restrict__ total,
                                                   int num_slots) {
    const int slot = blockIdx.x, tid = threadIdx.x;
    __shared__ uint32_t s_off;
    if (tid < 64) {
        uint32_t mine = 0;
        for (int s = tid; s < slot; s += 64)
            mine += (streams[s].bit_count + 31u) >> 5;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            mine += __shfl_xor(mine, d);
        if (tid == 0)
            s_off = mine;
    }
    __syncthreads();
    const uint32_t off = s_off, words = (streams[slot].bit_count + 31u) >> 5;
    const uint32_t *src = bits_all + (size_t)slot * HYDK_LF_BITWORDS;
    for (uint32_t w = tid; w < words; w += 256)
        packed[off + w] = src[w];
    if (tid == 0) {
        streams[slot].offset = off * 4u;
        if (slot == num_slots - 1)
            *total = (unsigned long long)(off + words) * 4ull;
    }
}

/* unit-test entry: the code construction alone, on a histogram in global memory */
__global__ __launch_bounds__(64) void k_lf_huffman(const uint32_t *__restrict__ hist, HydkLfStream *__restrict__ stream_out,
                                                   uint32_t *__restrict__ codes) {
    __shared__ LfHuffScratch s_huff;
    uint32_t len6[kEntries];
    lf_huffman_wave(hist, codes, stream_out, s_huff, (int)threadIdx.x, len6);
}

} // namespace

namespace hydk {

/* bytes of scratch per LF group (device_api.hip allocates it) */
size_t lf_work_bytes() { return sizeof(LfWork); }

/* The LF coder for `num_slots` LF groups in three steps (every pointer addresses the first of the LF
 * groups): tokens; code construction with the windows' offsets; pack.  The middle step may instead ride in the entropy
 * stage's launch (kernels.hip k_rans_lanes), which is why it can be left out here. */
hipError_t launch_lf_front(const HydkLfJob *d_jobs, unsigned long long *recs, uint32_t *hist, void *work, int num_slots,
                           hipStream_t stream) {
    /* hist is zero on entry: it lives in the arena k_frame_begin clears once per frame */
    hipLaunchKernelGGL(k_lf_tokens, dim3(kLfWorkgroups, num_slots), dim3(kLfThreads), 0, stream, d_jobs, recs, hist, (LfWork *)work);
    return hipGetLastError();
}

hipError_t launch_lf_codes(const HydkLfJob *d_jobs, const uint32_t *hist, HydkLfStream *streams, void *work, int num_slots,
                           hipStream_t stream) {
    hipLaunchKernelGGL(k_lf_codes, dim3(num_slots), dim3(64), 0, stream, d_jobs, hist, streams, (LfWork *)work);
    return hipGetLastError();
}

hipError_t launch_lf_back(const HydkLfJob *d_jobs, const unsigned long long *recs, HydkLfStream *streams, uint32_t *bits,
                          void *work, int num_slots, hipStream_t stream) {
    LfWork *w = (LfWork *)work;
    hipLaunchKernelGGL(k_lf_pack, dim3(kLfWorkgroups, num_slots), dim3(kLfThreads), 0, stream, d_jobs, recs, w, streams, bits);
    return hipGetLastError();
}

hipError_t launch_lf_coder(const HydkLfJob *d_jobs, unsigned long long *recs, uint32_t *hist, HydkLfStream *streams,
                           uint32_t *bits, void *work, int num_slots, hipStream_t stream) {
    hipError_t e = launch_lf_front(d_jobs, recs, hist, work, num_slots, stream);
    if (e == hipSuccess)
        e = launch_lf_codes(d_jobs, hist, streams, work, num_slots, stream);
    if (e == hipSuccess)
        e = launch_lf_back(d_jobs, recs, streams, bits, work, num_slots, stream);
    return e;
}

/* once per frame, over all of its LF groups */
hipError_t launch_lf_gather(HydkLfStream *streams, const uint32_t *bits, uint32_t *packed, unsigned long long *total,
                            int num_slots, hipStream_t stream) {
    hipLaunchKernelGGL(k_lf_gather, dim3(num_slots), dim3(256), 0, stream, streams, bits, packed, total, num_slots);
    return hipGetLastError();
}

/* debug / unit-test entry: code lengths and codes for one caller-supplied histogram (device pointers) */
hipError_t launch_lf_huffman_only(const uint32_t *hist, HydkLfStream *stream_out, uint32_t *codes, hipStream_t stream) {
    hipLaunchKernelGGL(k_lf_huffman, dim3(1), dim3(64), 0, stream, hist, stream_out, codes);
    return hipGetLastError();
}

} // namespace hydk
