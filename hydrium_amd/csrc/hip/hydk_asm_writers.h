/*
 * hydk_asm_writers.h — the data-dependent parts of a one-frame codestream, written on the GPU: what the frame assembler
 * (assemble.hip, k_asm_prepare: one frame from shard blobs) and the batch assembler (assemble_batch.hip, k_batch_prepare:
 * the frames of a batch view, side by side) do for ONE frame, in one source.  asm_frame is the body of both kernels; the
 * kernels differ in which frame a workgroup belongs to (AsmFrame) and in whose scratch it writes (Scratch).
 * For the two .hip files only; include hydrium_amd.h, hydk_asm_common.h and hydk_common.h first.
 */
#ifndef HYD_ASM_WRITERS_H_
#define HYD_ASM_WRITERS_H_

namespace {

constexpr int kHeadWords = 640;         /* bits in front of an LF group's symbols: <= 384 x 45 + fixed fields */

struct BlobArgs {
    const uint8_t *p[HYDK_ASM_MAX_BLOBS];
    uint64_t cap[HYDK_ASM_MAX_BLOBS];
};

/* which frame of a batch view a workgroup works on; all zero: the plan's own blobs hold one frame */
struct AsmFrame {
    uint32_t slot_base;  /* the frame's first slot record inside the view */
    uint32_t view_slots; /* slot records the view holds (0: what the plan says of each blob) */
    const uint8_t *hf;   /* the frame's HF sections inside the view's packed string (null: each blob's own, whole) */
    uint64_t hf_bytes;
};

struct Scratch { /* device pointers: one frame's */
    uint32_t *head;       /* [slots][kHeadWords] */
    uint32_t *head_bits;  /* [slots] */
    uint64_t *sizes;      /* [toc_n] section sizes in physical (TOC) order */
    uint64_t *slot_hf;    /* [slots] bytes of each LF group's HF sections */
    uint32_t *hfg;        /* [hfg_words] */
    uint32_t *toc;        /* [toc_words] */
    HydkPiece *pieces;    /* [4 + 3 slots + blobs] */
    uint32_t *npieces;    /* [1] */
    uint32_t *err;        /* [1] */
    uint32_t *done;       /* [1] workgroups of the frame that have finished their part */
    uint64_t *result;     /* [4] error word, 0, bytes of the frame (what k_pieces_copy reads), HFGlobal's bit count */
    uint32_t hfg_words, toc_words; /* what hfg and toc hold */
};

/* header sane and consistent with the plan?  (0, or HYDK_ASM_E_* bits; nothing behind the header is touched) */
__device__ __forceinline__ uint32_t blob_check(const uint8_t *blob, uint64_t cap, uint32_t want_slots) {
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    if (cap < sizeof(HydAmdBlobHeader))
        return HYDK_ASM_E_BLOB;
    const uint32_t e = blob_ident(h, want_slots);
    if (e)
        return e;
    const uint64_t lf_off = sizeof(HydAmdBlobHeader) + (uint64_t)h->num_slots * sizeof(HydAmdBlobSlot);
    if (h->lf_coded == kLfCodedView) {
        if (h->total_bytes != lf_off || lf_off > cap || !(h->reserved[1] | h->reserved[2]) || !(h->reserved[3] | h->reserved[4]) ||
            ((h->reserved[1] | h->reserved[3]) & 15u))
            return HYDK_ASM_E_BLOB;
        return 0;
    }
    const uint64_t hf_off = (lf_off + h->lf_bytes + 15ull) & ~15ull;
    if (h->lf_coded != 1 || h->total_bytes > cap || lf_off > h->total_bytes || h->lf_bytes > h->total_bytes || h->hf_bytes > h->total_bytes ||
        hf_off + h->hf_bytes != h->total_bytes)
        return HYDK_ASM_E_BLOB;
    return 0;
}

__device__ __forceinline__ const HydkAsmPlan *plan_of(const uint8_t *plan) { return (const HydkAsmPlan *)plan; }

/* ---- one LF group (workgroup s of the frame, 256 threads; the header itself is one wavefront's work) ---- */
__device__ void asm_slot(const uint8_t *__restrict__ planb, const BlobArgs &blobs, const Scratch &S, const AsmFrame &F, int s) {
    const HydkAsmPlan *plan = plan_of(planb);
    const int t = threadIdx.x;
    const HydkAsmSlot sl = ((const HydkAsmSlot *)(planb + plan->slots_off))[s];
    __shared__ uint32_t s_head[kHeadWords];
    __shared__ uint8_t s_len[HYDK_LF_CODES];
    __shared__ HydkLfHeadScratch s_scratch;
    __shared__ uint32_t s_bits, s_err;
    const uint8_t *blob = blobs.p[sl.blob];
    const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blob;
    uint32_t e = blob_check(blob, blobs.cap[sl.blob], F.view_slots ? F.view_slots : plan->blob_slots[sl.blob]);
    if (!e && F.slot_base + sl.index >= h->num_slots)
        e = HYDK_ASM_E_BLOB;
    const HydAmdBlobSlot *rec = (const HydAmdBlobSlot *)(blob + sizeof(HydAmdBlobHeader)) + F.slot_base + sl.index;
    if (!e)
        e = hydk_slot_check(rec, sl.preset, h->lf_bytes);
    if (e) {
        if (t == 0) {
            atomicOr(S.err, e);
            S.head_bits[s] = 0;
            S.slot_hf[s] = 0;
            S.sizes[1 + s] = 0;
        }
        for (uint32_t g = t; g < sl.ngroups; g += 256)
            S.sizes[2 + plan->num_slots + sl.group_base + g] = 0;
        return;
    }
    for (int i = t; i < kHeadWords; i += 256)
        s_head[i] = 0;
    for (int i = t; i < HYDK_LF_CODES; i += 256)
        s_len[i] = rec->lf.lengths[i];
    if (t == 0)
        s_err = 0;
    __syncthreads();
    {
        /* the plan's constant bits first (whole words; the bits of the last one beyond lfpre_bits are zero), then the
         * stream header's data-dependent part, written by one wavefront (hydk_sections.h) */
        const uint32_t *pre = (const uint32_t *)(planb + plan->lfpre_off);
        for (uint32_t i = t; i < (plan->lfpre_bits + 31u) >> 5; i += 256)
            s_head[i] = pre[i];
    }
    __syncthreads();
    uint64_t hf = 0;
    uint32_t bad = 0;
    if (t < 64) {
        uint64_t end = 0;
        const int ret = hydk_lf_prefix_codes_wave(s_head, (uint64_t)kHeadWords * 32u, plan->lfpre_bits, s_len, rec->lf.alphabet,
                                                  rec->lf.run_pairs, &s_scratch, &end);
        if (t == 0) {
            if (ret)
                s_err = HYDK_ASM_E_HEAD;
            s_bits = ret ? 0u : (uint32_t)end;
        }
        /* TOC sizes of this LF group's sections */
        const uint32_t b = rec->group_bits[t];
        if ((uint32_t)t < sl.ngroups) {
            const uint64_t n = ((uint64_t)b + 7u) >> 3;
            S.sizes[2 + plan->num_slots + sl.group_base + t] = n;
            hf = n;
        } else if (b) {
            bad = 1; /* a group the frame's geometry does not have */
        }
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            hf += __shfl_xor(hf, d);
            bad |= (uint32_t)__shfl_xor((int)bad, d);
        }
    }
    __syncthreads();
    const uint32_t head_bits = s_bits;
    uint32_t *dst = S.head + (size_t)s * kHeadWords;
    for (uint32_t i = t; i < (head_bits + 31u) >> 5; i += 256)
        dst[i] = s_head[i];
    if (t == 0) {
        const uint64_t sec_bits = (uint64_t)head_bits + rec->lf.bit_count + plan->tail_bits[sl.tail];
        S.head_bits[s] = head_bits;
        S.sizes[1 + s] = (sec_bits + 7) >> 3;
        S.slot_hf[s] = hf;
        const uint32_t ee = s_err | (bad ? HYDK_ASM_E_SIZE : 0u);
        if (ee)
            atomicOr(S.err, ee);
    }
}

__device__ __forceinline__ const HydAmdBlobSlot *slot_record(const uint8_t *planb, const BlobArgs &blobs, const AsmFrame &F, uint32_t s) {
    const HydkAsmPlan *plan = plan_of(planb);
    const HydkAsmSlot sl = ((const HydkAsmSlot *)(planb + plan->slots_off))[s];
    return (const HydAmdBlobSlot *)(blobs.p[sl.blob] + sizeof(HydAmdBlobHeader)) + F.slot_base + sl.index;
}

/* ---- HFGlobal (the workgroup behind the frame's LF groups', 256 threads) ---- */
__device__ void asm_hfglobal(const uint8_t *__restrict__ planb, const BlobArgs &blobs, const Scratch &S, const AsmFrame &F) {
    const HydkAsmPlan *plan = plan_of(planb);
    __shared__ uint64_t s_wave[4];
    __shared__ uint32_t s_max;
    const int t = threadIdx.x;
    {
        /* the LF groups' workgroups run beside this one: it checks the headers it is about to follow itself */
        uint32_t e = 0;
        if ((uint32_t)t < plan->num_blobs)
            e = blob_check(blobs.p[t], blobs.cap[t], F.view_slots ? F.view_slots : plan->blob_slots[t]);
        if (e)
            atomicOr(S.err, e);
        if (__syncthreads_or((int)e))
            return;
    }
    const uint32_t per = plan->clusters_per_preset, C = plan->num_presets * per;
    if (t == 0)
        s_max = 0;
    __syncthreads();
    uint32_t mx = 0;
    for (uint32_t s = t; s < plan->num_slots; s += 256)
        mx = max(mx, slot_record(planb, blobs, F, s)->running_max_alphabet);
    if (mx)
        atomicMax(&s_max, mx);
    /* pass 1: how long each histogram is */
    const uint32_t *freq = nullptr;
    uint32_t alphabet = 0;
    uint64_t nb = 0;
    if ((uint32_t)t < C) {
        const uint32_t p = (uint32_t)t / per, k = (uint32_t)t % per;
        const uint32_t slot = ((const uint32_t *)(planb + plan->preset_slot_off))[p];
        const HydAmdBlobSlot *rec = slot_record(planb, blobs, F, slot);
        freq = rec->freq[k];
        alphabet = rec->alphabet[k] > HYDAMD_ALPHABET ? HYDAMD_ALPHABET : rec->alphabet[k];
        HydkSink count = {nullptr, 0, ~0ull, 0, 0};
        hydk_put_ans_distribution(&count, freq, alphabet);
        nb = count.pos;
    }
    uint64_t total = 0;
    const uint64_t off = scan256(nb, s_wave, &total);
    int log_alpha = 0;
    const uint32_t cfg_bits = hydk_put_hf_config(nullptr, s_max, &log_alpha);
    const uint64_t base = (uint64_t)plan->hfpre_bits + 2u + (uint64_t)C * cfg_bits;
    const uint64_t bits = base + total;
    const uint64_t words = (bits + 31) >> 5;
    if (words > (uint64_t)S.hfg_words || log_alpha > 8) {
        if (t == 0)
            atomicOr(S.err, HYDK_ASM_E_SCRATCH);
        return;
    }
    for (uint64_t i = t; i < words; i += 256)
        S.hfg[i] = 0;
    __threadfence();
    __syncthreads();
    HydkSink sink = {S.hfg, 0, (uint64_t)S.hfg_words * 32u, 0, 1};
    if (t == 0) {
        const uint32_t *pre = (const uint32_t *)(planb + plan->hfpre_off);
        for (uint32_t done = 0; done < plan->hfpre_bits; done += 32)
            hks_put(&sink, pre[done >> 5], plan->hfpre_bits - done < 32 ? plan->hfpre_bits - done : 32);
        hks_put(&sink, (uint32_t)(log_alpha - 5), 2);
        S.sizes[1 + plan->num_slots] = (bits + 7) >> 3;
        S.result[3] = bits; /* for the layout */
    }
    if ((uint32_t)t < C) {
        sink.pos = (uint64_t)plan->hfpre_bits + 2u + (uint64_t)t * cfg_bits;
        hydk_put_hf_config(&sink, s_max, &log_alpha);
        sink.pos = base + off;
        hydk_put_ans_distribution(&sink, freq, alphabet);
    }
}

/* ---- TOC and layout (the workgroup of the frame that finishes last, 256 threads); the pieces' positions count from the
 * frame's first byte ---- */
__device__ void asm_layout(const uint8_t *__restrict__ planb, const BlobArgs &blobs, const Scratch &S, const AsmFrame &F, uint64_t out_cap,
                           uint64_t *h_result /* pinned host [2], or null */) {
    const HydkAsmPlan *plan = plan_of(planb);
    __shared__ uint64_t s_wave[4];
    const int t = threadIdx.x;
    const uint32_t n = plan->toc_n, nslots = plan->num_slots;
    /* what the copy kernel (S.result) and the host (h_result: size, error) read */
    auto finish = [&](uint64_t size, uint32_t e) {
        if (t == 0) {
            S.result[0] = e;
            S.result[1] = 0;
            S.result[2] = e ? 0 : size;
            if (h_result) {
                h_result[0] = size;
                h_result[1] = e;
            }
        }
    };
    const uint32_t err = *S.err;
    if (err) {
        finish(0, err);
        return;
    }
    const uint64_t hfg_bits = S.result[3];
    if (t == 0)
        S.sizes[0] = plan->lfglobal_bytes;
    __threadfence();
    __syncthreads();
    /* TOC: entry widths, where each goes, the entries */
    const uint32_t per = (n + 255u) / 256u;
    const uint32_t lo = min(n, (uint32_t)t * per), hi = min(n, lo + per);
    uint64_t mine = 0;
    uint32_t bad = 0;
    for (uint32_t i = lo; i < hi; i++) {
        uint64_t v;
        const uint32_t w = hydk_toc_entry(S.sizes[i], &v);
        bad |= w == 0;
        mine += w;
    }
    uint64_t toc_bits = 0;
    const uint64_t start = scan256(mine, s_wave, &toc_bits);
    const uint64_t toc_words = (toc_bits + 31) >> 5;
    if (toc_words > (uint64_t)S.toc_words)
        bad |= 2;
    if (__syncthreads_or((int)bad)) {
        finish(0, (bad & 2) ? HYDK_ASM_E_SCRATCH : HYDK_ASM_E_SIZE);
        return;
    }
    for (uint64_t i = t; i < toc_words; i += 256)
        S.toc[i] = 0;
    __threadfence();
    __syncthreads();
    {
        HydkSink sink = {S.toc, start, (uint64_t)S.toc_words * 32u, 0, 1};
        for (uint32_t i = lo; i < hi; i++) {
            uint64_t v;
            const uint32_t w = hydk_toc_entry(S.sizes[i], &v);
            hks_put64(&sink, v, w);
        }
    }
    const uint64_t toc_bytes = (toc_bits + 7) >> 3;
    const uint64_t body = (uint64_t)plan->prefix_bytes + toc_bytes;
    /* LF group sections: thread t owns slot t */
    uint64_t lf_mine = (uint32_t)t < nslots ? S.sizes[1 + t] : 0, lf_total = 0;
    const uint64_t lf_off = scan256(lf_mine, s_wave, &lf_total);
    const uint64_t lf_base = body + plan->lfglobal_bytes;
    const uint64_t hfg_dst = lf_base + lf_total, hfg_bytes = (hfg_bits + 7) >> 3;
    /* HF sections: one piece per blob, in blob order; each blob's byte count must be what its slots add up to */
    uint64_t hf_mine = 0;
    uint32_t mismatch = 0;
    if ((uint32_t)t < plan->num_blobs) {
        const HydAmdBlobHeader *h = (const HydAmdBlobHeader *)blobs.p[t];
        hf_mine = F.hf ? F.hf_bytes : h->hf_bytes;
        uint64_t sum = 0;
        for (uint32_t s = plan->blob_first[t]; s < plan->blob_first[t] + plan->blob_slots[t]; s++)
            sum += S.slot_hf[s];
        mismatch = sum != hf_mine;
    }
    uint64_t hf_total = 0;
    const uint64_t hf_off = scan256(hf_mine, s_wave, &hf_total);
    const uint64_t hf_base = hfg_dst + hfg_bytes;
    const uint64_t total = hf_base + hf_total;
    /* the pieces, in output order: bits, where the sections are measured in bytes */
    HydkPiece *P = S.pieces;
    if (t == 0) {
        P[0] = hydk_piece(0, planb + plan->prefix_off, (uint64_t)plan->prefix_bytes * 8u);
        P[1] = hydk_piece((uint64_t)plan->prefix_bytes * 8u, S.toc, toc_bits);
        P[2] = hydk_piece(body * 8u, planb + plan->lfglobal_off, (uint64_t)plan->lfglobal_bytes * 8u);
        P[3 + 3 * nslots] = hydk_piece(hfg_dst * 8u, S.hfg, hfg_bits);
        *S.npieces = 4 + 3 * nslots + plan->num_blobs;
    }
    if ((uint32_t)t < nslots) {
        const HydkAsmSlot sl = ((const HydkAsmSlot *)(planb + plan->slots_off))[t];
        const uint8_t *blob = blobs.p[sl.blob];
        const HydAmdBlobSlot *rec = (const HydAmdBlobSlot *)(blob + sizeof(HydAmdBlobHeader)) + F.slot_base + sl.index;
        const uint64_t at = (lf_base + lf_off) * 8u, head_bits = S.head_bits[t];
        P[3 + 3 * t] = hydk_piece(at, S.head + (size_t)t * kHeadWords, head_bits);
        P[4 + 3 * t] = hydk_piece(at + head_bits, blob_lf_bytes(blob) + rec->lf.offset, rec->lf.bit_count);
        P[5 + 3 * t] = hydk_piece(at + head_bits + rec->lf.bit_count, planb + plan->tail_off[sl.tail], plan->tail_bits[sl.tail]);
    }
    if ((uint32_t)t < plan->num_blobs)
        P[4 + 3 * nslots + t] = hydk_piece((hf_base + hf_off) * 8u, F.hf ? F.hf : blob_hf_bytes(blobs.p[t]), hf_mine * 8u);
    const int any_mismatch = __syncthreads_or((int)mismatch);
    const uint32_t e = any_mismatch ? HYDK_ASM_E_SIZE : total > out_cap ? HYDK_ASM_E_SPACE : 0u;
    finish(e == HYDK_ASM_E_SIZE ? 0 : total, e); /* out of space: the bytes the frame needs */
}

/* ---- one frame: `parts` = LF groups + 1 workgroups of 256 threads.  Part s < LF groups: that LF group (asm_slot); the one
 * behind them: HFGlobal; whichever finishes last: TOC and layout, then the frame's counters back to zero for the next
 * launch — one launch where three kernels and a memset used to sit in the stream (in a pipelined loop every launch of
 * a frame costs latency in a GPU full of other frames' workgroups: export + five launches took 13 % of the frame rate
 * for 1 % of its instructions) ---- */
__device__ __forceinline__ void asm_frame(const uint8_t *__restrict__ planb, const BlobArgs &blobs, const Scratch &S, const AsmFrame &F,
                                          uint32_t part, uint32_t parts, uint64_t out_cap, uint64_t *h_result) {
    __shared__ int s_last;
    if (part + 1 < parts)
        asm_slot(planb, blobs, S, F, (int)part);
    else
        asm_hfglobal(planb, blobs, S, F);
    __threadfence(); /* this workgroup's results before its tick */
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = atomicAdd(S.done, 1u) == parts - 1;
    __syncthreads();
    if (!s_last)
        return;
    __threadfence(); /* everyone else's results after the last tick */
    asm_layout(planb, blobs, S, F, out_cap, h_result);
    __syncthreads();
    if (threadIdx.x == 0) { /* ready for the next frame */
        *S.done = 0;
        *S.err = 0;
    }
}

} // namespace

#endif /* HYD_ASM_WRITERS_H_ */
