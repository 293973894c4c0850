/*
 * hydk_tiles.h — tile-mode frames assembled many at a time: the plan the host writes, the data-dependent
 * fields of one tile frame and where its bit strings go.  Like
 * hydk_sections.h the same source runs on the GPU (csrc/hip/assemble_tiles.hip: one wavefront per frame,
 * then one thread per output word) and on the host (csrc/host/tiled.c under HYD_TEST_HOOKS: the CPU tests
 * hold it to the host assembler, frame.c, byte for byte).  Include hydrium_amd.h first (HydAmdBlobSlot).
 *
 * A tile is at most 2048 x 2048 pixels: ONE LF group, one preset, nine clusters, up to 64 groups.  Two layouts
 * (reference encoder.c:380-398 and 968-1005):
 *   one group       frame header | TOC (one entry) | LFGlobal LFGroup HFGlobal group — one bit-contiguous section,
 *                   padded once at its end.  Four bit strings: [LFGlobal + fixed LF head + prefix codes] (HEAD),
 *                   the LF coefficient stream, [LF tail + HFGlobal] (MID), the group's rANS bits.
 *   several groups  frame header with the TOC permutation | TOC | LFGlobal | LFGroup | HFGlobal | groups, each padded
 *                   to a byte.  HEAD holds the fixed LF head + prefix codes, MID holds HFGlobal.
 * A frame is a list of HYDK_TILE_PIECES pieces (hydk_pieces.h); the pieces of all frames of a launch group form one
 * sorted list, from which every output word is composed.
 */
#ifndef HYD_TILE_LAYOUT_H_
#define HYD_TILE_LAYOUT_H_

#include <stdint.h>

#include "hydk_asm_common.h"

#define HYDK_TILE_MAGIC 0x4C495448u /* "HTIL" */
#define HYDK_TILE_MAX_SHAPES 4      /* interior, right edge, bottom edge, corner */
#define HYDK_TILE_PIECES 8
#define HYDK_TILE_HEAD_WORDS 704    /* LFGlobal + <= 384 x 45 bits of prefix codes + fixed fields */
#define HYDK_TILE_MID_WORDS 3072    /* LF tail + nine histograms of <= 73 words + the cluster map */
#define HYDK_TILE_TOC_WORDS 80      /* <= 67 entries of <= 32 bits */
#define HYDK_TILE_CLUSTERS 9
#define HYDK_TILE_MAX_FRAMES 255    /* frames of one launch group (= LF-group slots of a context) */

typedef struct HydkTileShape {
    uint32_t ngroups;                      /* 256 x 256 groups of the tile; 1: the bit-contiguous layout */
    uint32_t pre_off, pre_bits;            /* what opens HEAD: (LFGlobal, one group only) + the LF group's fixed fields */
    uint32_t lfglobal_off, lfglobal_bytes; /* the byte-padded LFGlobal section (several groups) */
    uint32_t tail_off, tail_bits;          /* geometry-only bits that close the LF group */
    uint32_t hfpre_off, hfpre_bits;        /* HFGlobal up to and including "ANS, not prefix codes" */
    uint32_t pad[3];
} HydkTileShape;

typedef struct HydkTileFrame { /* one tile, raster order */
    uint32_t prefix_off, prefix_bytes; /* (file header, tile 0) + frame header with origin, size, is_last, TOC permutation */
    uint32_t shape, pad;
} HydkTileFrame;

typedef struct HydkTilePlan { /* header of the plan buffer; offsets in bytes from its start, 16-byte aligned */
    uint32_t magic, total_bytes, num_frames, nshapes;
    HydkTileShape shapes[HYDK_TILE_MAX_SHAPES];
    uint32_t frames_off, pad[3];
} HydkTilePlan;

/* A MIXED plan (csrc/host/mixed.c): one-frame images of different sizes side by side, every frame with a prefix of its own
 * (its file header, its frame header) and any number of shapes — the shape records live in the buffer, `nshapes` of them
 * at `shapes_off`, a frame's `shape` indexing them.  Offsets inside the records count from the start of the plan, as above. */
#define HYDK_MIXED_MAGIC 0x58494D48u /* "HMIX" */
typedef struct HydkMixedPlan {
    uint32_t magic, total_bytes, num_frames, nshapes;
    uint32_t shapes_off, frames_off, pad[2];
} HydkMixedPlan;

/* A FRAMES plan (csrc/host/mixed.c, hydamd_mixed_create_slots): one-frame images of different sizes AND different LF-group
 * counts side by side.  A frame record says which kind its frame is: one LF group — `one`, the mixed plan's record, and the
 * shape it names — or several — `plan_off`, where in this buffer a complete HydkAsmPlan of that image lies (hydk_assemble.h:
 * one blob, the LF groups in raster order, file header, is_last; images of one size share one).  Either way the record
 * names the frame's slots in the batch view and its part of each of the assembler's scratch arrays, prefix sums the host
 * computes: heads, head bits and HF byte counts are indexed by slot, HFGlobal, TOC, section sizes and pieces per frame.
 * `parts` maps a workgroup of k_batch_prepare_frames to (frame << 8 | part) over the frames of several LF groups. */
#define HYDK_FRAMES_MAGIC 0x46584D48u /* "HMXF" */
#define HYDK_FRAMES_MAX_LF_GROUPS 28  /* of one image: up to here a frame clusters nine ways (HYDAMD_BATCH_FRAME_LF_GROUPS) */
typedef struct HydkBatchFrame {
    HydkTileFrame one;             /* one LF group: the frame's prefix and shape */
    uint32_t plan_off;             /* several: the frame's HydkAsmPlan; 0: one LF group */
    uint32_t first_slot, lf_groups;
    uint32_t piece_base;           /* sum of 3 n + 5 over the frames before it */
    uint32_t hfg_off, hfg_words;   /* in words */
    uint32_t toc_off, toc_words;
    uint32_t sizes_off, pad[3];    /* in entries of 8 bytes; a frame of several LF groups has toc_n of them */
} HydkBatchFrame;

typedef struct HydkFramesPlan {
    uint32_t magic, total_bytes, num_frames, nshapes;
    uint32_t shapes_off, frames_off, parts_off, nparts; /* HydkTileShape[], HydkBatchFrame[], uint32_t[] */
    uint32_t num_slots, npieces, nplans, pad;           /* LF groups and pieces of the batch; distinct HydkAsmPlans */
} HydkFramesPlan;

/* what the assembler's scratch arrays hold for batches of up to F frames and N LF groups in all, whatever the sizes: a
 * slot's head is the larger of the two layouts'; a frame of n LF groups has 3 n + 5 pieces, a TOC of 2 + n + (<= 64 n)
 * entries and an HFGlobal of (hfpre_bits + 2 + 9 C) / 32 + 73 C + 2 words with C = 9 n, where hfpre holds the cluster map
 * of 1485 n contexts at no more than 16 bits each; a frame of one LF group the tile layout's fixed arrays.  The planner
 * holds every batch against these (mixed.c), the device each frame against its own share (HYDK_ASM_E_SCRATCH). */
#define HYDK_FRAMES_HEAD_STRIDE HYDK_TILE_HEAD_WORDS
#define HYDK_FRAMES_HFG_CAP(F, N) ((size_t)(F) * HYDK_TILE_MID_WORDS + (size_t)(N) * (743u + 660u))
#define HYDK_FRAMES_TOC_CAP(F, N) ((size_t)(F) * HYDK_TILE_TOC_WORDS + (size_t)(N) * 65u)
#define HYDK_FRAMES_SIZES_CAP(F, N) ((size_t)(F) * 2u + (size_t)(N) * 65u)
#define HYDK_FRAMES_PIECES_CAP(F, N) ((size_t)(F) * 5u + (size_t)(N) * 3u)

/* ---- an outcome per image (hydamd_*_set_image_errors): what k_batch_place (assemble_batch.hip) does with a frame whose
 * context flagged one of its slots, in the words the host build (tiled.c, HYD_TEST_HOOKS) runs too ---- */
/* is any of the frame's n slot records flagged?  (HydAmdBlobSlot.reserved[0]: hydamd_set_bad_sample_per_slot) */
HYDK_HD uint32_t hydk_frame_flagged(const HydAmdBlobSlot *rec, uint32_t n) {
    uint32_t any = 0;
    for (uint32_t i = 0; i < n; i++)
        any |= rec[i].reserved[0] != 0;
    return any;
}
/* one piece of a frame that starts at byte `at` of the output, as its preparation left it (counted from the frame's first
 * byte): moved there — or, the frame skipped, made an EMPTY piece at `at`, which is also where the next frame starts.  The
 * list keeps its length and its order, its ends stay monotone (what hydk_pieces_word's search needs), no bit is covered. */
HYDK_HD void hydk_place_piece(HydkPiece *p, uint64_t at, uint32_t skip) {
    if (skip)
        *p = hydk_piece(at * 8u, (const void *)0, 0);
    else
        p->dst_bit += at * 8u;
}

typedef struct HydkTileSizes { /* what the preparation of one frame leaves */
    uint32_t head_bits, mid_bits, toc_bits, err;
    uint64_t lfsec_bytes, hfg_bytes; /* several groups: the two padded sections */
    uint64_t hf_bytes;               /* the frame's extent in the packed HF sections */
    uint64_t frame_bytes;
} HydkTileSizes;

typedef struct HydkTileExtent { /* a batch's results, frame by frame: where its bytes sit in the two packed strings */
    uint64_t lf_off, lf_bytes, hf_off, hf_bytes;
} HydkTileExtent;

typedef struct HydkTileScratch {
    HydkLfHeadScratch lf;
    uint32_t hist_bits[HYDK_TILE_CLUSTERS];
    uint32_t err;
} HydkTileScratch;

/* `nbits` bits of the zero-padded words `src` into the sink at bit `at`, dealt over the lanes */
#define HYDK_TILE_COPY_BITS(words, cap, at, src, nbits)                                      \
    HKS_LANES(l) {                                                                           \
        for (uint32_t i_ = (uint32_t)l; i_ * 32u < (nbits); i_ += 64u) {                     \
            HydkSink sk_ = {(words), (uint64_t)(at) + (uint64_t)i_ * 32u, (cap), 0, 1};      \
            const uint32_t left_ = (nbits) - i_ * 32u;                                       \
            hks_put(&sk_, (src)[i_], left_ < 32u ? left_ : 32u);                             \
            if (sk_.overflow)                                                                \
                S->err = HYDK_ASM_E_SCRATCH;                                                 \
        }                                                                                    \
    }

/* Called by the 64 lanes of one wavefront (device) / once (host).  head, mid and toc are zeroed arrays of
 * HYDK_TILE_*_WORDS words; `lengths` = rec->lf.lengths (on the device a copy in LDS).  Lane 0 / the caller fills *out. */
HYDK_HD void hydk_tile_prepare(const uint8_t *planb, const HydkTileFrame *fr, const HydkTileShape *sh, const HydAmdBlobSlot *rec,
                               const uint8_t *lengths, uint64_t lf_capacity, uint32_t *head, uint32_t *mid, uint32_t *toc,
                               HydkTileScratch *S, HydkTileSizes *out) {
    const int single = sh->ngroups == 1;
    uint32_t e = hydk_slot_check(rec, 0, lf_capacity);
    for (uint32_t g = sh->ngroups; g < HYDAMD_GROUPS_PER_LFG; g++)
        if (rec->group_bits[g])
            e |= HYDK_ASM_E_SIZE; /* a group the tile's geometry does not have */
    HKS_LANES(l) {
        if (l == 0)
            S->err = 0;
    }
    HKS_SYNC();
    if (e) {
        HKS_LANES(l) {
            if (l == 0) {
                HydkTileSizes z = {0, 0, 0, 0, 0, 0, 0, 0};
                z.err = e;
                *out = z;
            }
        }
        return;
    }
    /* HEAD: the constant bits, then the LF stream header's data-dependent part */
    const uint64_t head_cap = (uint64_t)HYDK_TILE_HEAD_WORDS * 32u, mid_cap = (uint64_t)HYDK_TILE_MID_WORDS * 32u;
    HYDK_TILE_COPY_BITS(head, head_cap, 0, (const uint32_t *)(planb + sh->pre_off), sh->pre_bits)
    HKS_SYNC();
    uint64_t head_end = 0;
    const int hret = hydk_lf_prefix_codes_wave(head, head_cap, sh->pre_bits, lengths, rec->lf.alphabet, rec->lf.run_pairs, &S->lf, &head_end);
    /* MID: (the LF group's tail, one group only), HFGlobal's fixed fields, then what the tables decide (encoder.c:959-967) */
    const uint32_t tail_here = single ? sh->tail_bits : 0u;
    if (single)
        HYDK_TILE_COPY_BITS(mid, mid_cap, 0, (const uint32_t *)(planb + sh->tail_off), sh->tail_bits)
    HYDK_TILE_COPY_BITS(mid, mid_cap, tail_here, (const uint32_t *)(planb + sh->hfpre_off), sh->hfpre_bits)
    HKS_LANES(l) {
        if (l < HYDK_TILE_CLUSTERS) {
            HydkSink count = {(uint32_t *)0, 0, ~(uint64_t)0, 0, 0};
            const uint32_t a = rec->alphabet[l] > HYDAMD_ALPHABET ? HYDAMD_ALPHABET : rec->alphabet[l];
            hydk_put_ans_distribution(&count, rec->freq[l], a);
            S->hist_bits[l] = (uint32_t)count.pos;
        }
    }
    HKS_SYNC();
    int log_alpha = 0;
    const uint32_t cfg_bits = hydk_put_hf_config((HydkSink *)0, rec->running_max_alphabet, &log_alpha);
    const uint64_t cfg_at = (uint64_t)tail_here + sh->hfpre_bits + 2u;
    const uint64_t hist_at = cfg_at + (uint64_t)HYDK_TILE_CLUSTERS * cfg_bits;
    uint64_t mid_end = hist_at;
    for (int i = 0; i < HYDK_TILE_CLUSTERS; i++)
        mid_end += S->hist_bits[i];
    HKS_LANES(l) {
        if (l < HYDK_TILE_CLUSTERS && log_alpha <= 8 && mid_end <= mid_cap) {
            HydkSink sink = {mid, cfg_at - 2u, mid_cap, 0, 1};
            if (l == 0)
                hks_put(&sink, (uint32_t)(log_alpha - 5), 2);
            sink.pos = cfg_at + (uint64_t)l * cfg_bits;
            hydk_put_hf_config(&sink, rec->running_max_alphabet, &log_alpha);
            uint64_t at = hist_at;
            for (int i = 0; i < l; i++)
                at += S->hist_bits[i];
            sink.pos = at;
            const uint32_t a = rec->alphabet[l] > HYDAMD_ALPHABET ? HYDAMD_ALPHABET : rec->alphabet[l];
            hydk_put_ans_distribution(&sink, rec->freq[l], a);
        }
    }
    HKS_SYNC();
    /* sizes and the TOC (encoder.c:992-1005): a handful of entries, one lane */
    HKS_LANES(l) {
        if (l == 0) {
            HydkTileSizes z = {0, 0, 0, 0, 0, 0, 0, 0};
            z.err = S->err | (hret ? HYDK_ASM_E_HEAD : 0u) | (log_alpha > 8 || mid_end > mid_cap ? HYDK_ASM_E_SCRATCH : 0u);
            z.head_bits = (uint32_t)head_end;
            z.mid_bits = (uint32_t)mid_end;
            HydkSink sink = {toc, 0, (uint64_t)HYDK_TILE_TOC_WORDS * 32u, 0, 0};
            uint64_t v = 0, body = 0;
            uint32_t w = 1;
            if (single) {
                const uint64_t bits = head_end + rec->lf.bit_count + mid_end + rec->group_bits[0];
                body = (bits + 7) >> 3;
                z.hf_bytes = ((uint64_t)rec->group_bits[0] + 7) >> 3;
                w = hydk_toc_entry(body, &v);
                hks_put64(&sink, v, w);
            } else {
                z.lfsec_bytes = (head_end + rec->lf.bit_count + sh->tail_bits + 7) >> 3;
                z.hfg_bytes = (mid_end + 7) >> 3;
                for (uint32_t i = 0; i < 3 + sh->ngroups && w; i++) {
                    const uint64_t n = i == 0 ? sh->lfglobal_bytes : i == 1 ? z.lfsec_bytes : i == 2 ? z.hfg_bytes : ((uint64_t)rec->group_bits[i - 3] + 7) >> 3;
                    if (i >= 3)
                        z.hf_bytes += n;
                    body += n;
                    w = hydk_toc_entry(n, &v);
                    hks_put64(&sink, v, w);
                }
            }
            if (!w || sink.overflow)
                z.err |= HYDK_ASM_E_SIZE;
            z.toc_bits = (uint32_t)sink.pos;
            z.frame_bytes = (uint64_t)fr->prefix_bytes + ((sink.pos + 7) >> 3) + body;
            *out = z;
        }
    }
}

/* the frame's pieces, in output order, for a frame that starts at byte `at` of the output */
HYDK_HD void hydk_tile_pieces(const uint8_t *planb, const HydkTileFrame *fr, const HydkTileShape *sh, const HydkTileSizes *z,
                              const HydAmdBlobSlot *rec, const uint32_t *head, const uint32_t *mid, const uint32_t *toc,
                              const uint8_t *lf_src, const uint8_t *hf_src, uint64_t at, HydkPiece *P) {
    uint64_t bit = at * 8u;
    P[0] = hydk_piece(bit, planb + fr->prefix_off, (uint64_t)fr->prefix_bytes * 8u);
    bit += (uint64_t)fr->prefix_bytes * 8u;
    P[1] = hydk_piece(bit, toc, z->toc_bits);
    bit += (((uint64_t)z->toc_bits + 7) >> 3) * 8u;
    if (sh->ngroups == 1) {
        P[2] = hydk_piece(bit, head, z->head_bits);
        bit += z->head_bits;
        P[3] = hydk_piece(bit, lf_src, rec->lf.bit_count);
        bit += rec->lf.bit_count;
        P[4] = hydk_piece(bit, mid, z->mid_bits);
        bit += z->mid_bits;
        P[5] = hydk_piece(bit, hf_src, rec->group_bits[0]);
        bit += rec->group_bits[0];
        P[6] = hydk_piece(bit, head, 0);
        P[7] = hydk_piece(bit, head, 0);
        return;
    }
    P[2] = hydk_piece(bit, planb + sh->lfglobal_off, (uint64_t)sh->lfglobal_bytes * 8u);
    bit += (uint64_t)sh->lfglobal_bytes * 8u;
    const uint64_t lfsec = bit;
    P[3] = hydk_piece(bit, head, z->head_bits);
    bit += z->head_bits;
    P[4] = hydk_piece(bit, lf_src, rec->lf.bit_count);
    bit += rec->lf.bit_count;
    P[5] = hydk_piece(bit, planb + sh->tail_off, sh->tail_bits);
    bit = lfsec + z->lfsec_bytes * 8u;
    P[6] = hydk_piece(bit, mid, z->mid_bits);
    bit += z->hfg_bytes * 8u;
    P[7] = hydk_piece(bit, hf_src, z->hf_bytes * 8u);
}

#if defined(__HIPCC__)
/* One workgroup of 64 threads (one wavefront): hydk_tile_prepare for the frame `fr` of the plan from slot record `rec`,
 * through LDS, the strings copied out to head / mid / toc (device arrays of HYDK_TILE_*_WORDS words).  Every lane
 * gets the frame's sizes.  What k_tiles_prepare (assemble_tiles.hip) and k_batch_prepare_one (assemble_batch.hip) run. */
static __device__ __forceinline__ HydkTileSizes hydk_tile_prepare_wave(const uint8_t *planb, const HydkTileFrame *fr, const HydkTileShape *sh,
                                                                       const HydAmdBlobSlot *rec, uint64_t lf_capacity, uint32_t *head,
                                                                       uint32_t *mid, uint32_t *toc) {
    __shared__ uint32_t s_head[HYDK_TILE_HEAD_WORDS];
    __shared__ uint32_t s_mid[HYDK_TILE_MID_WORDS];
    __shared__ uint32_t s_toc[HYDK_TILE_TOC_WORDS];
    __shared__ uint8_t s_len[HYDK_LF_CODES];
    __shared__ HydkTileScratch s_scratch;
    __shared__ HydkTileSizes s_sizes;
    const int t = threadIdx.x;
    for (int i = t; i < HYDK_TILE_HEAD_WORDS; i += 64)
        s_head[i] = 0;
    for (int i = t; i < HYDK_TILE_MID_WORDS; i += 64)
        s_mid[i] = 0;
    for (int i = t; i < HYDK_TILE_TOC_WORDS; i += 64)
        s_toc[i] = 0;
    for (int i = t; i < HYDK_LF_CODES; i += 64)
        s_len[i] = rec->lf.lengths[i];
    __syncthreads();
    hydk_tile_prepare(planb, fr, sh, rec, s_len, lf_capacity, s_head, s_mid, s_toc, &s_scratch, &s_sizes);
    __syncthreads();
    const HydkTileSizes z = s_sizes;
    for (uint32_t i = t; i < (z.head_bits + 31u) >> 5; i += 64)
        head[i] = s_head[i];
    for (uint32_t i = t; i < (z.mid_bits + 31u) >> 5; i += 64)
        mid[i] = s_mid[i];
    for (uint32_t i = t; i < (z.toc_bits + 31u) >> 5; i += 64)
        toc[i] = s_toc[i];
    return z;
}
#endif

#endif /* HYD_TILE_LAYOUT_H_ */
