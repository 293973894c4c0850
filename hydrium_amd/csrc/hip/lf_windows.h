/*
 * lf_windows.h — the LF coder's window work: what one 256-thread workgroup does to windows of 896 values of an LF group's
 * coefficient stream, as a token workgroup (residuals -> run structure -> records + token histogram) and as a pack workgroup
 * (records + prefix code -> bits).  Included by lf_coder.hip, whose k_lf_tokens / k_lf_pack are these roles as kernels of
 * their own, and by kernels.hip, where the same roles ride as extra workgroups in the table kernel's and the emit kernel's
 * launches (k_build_tables, k_rans_emit<true>): a role depends only on launches that ended before its own began, never on
 * the workgroups beside it.  Everything here is internal linkage (include it inside an anonymous namespace).
 */
#pragma once

#include "lf_huffman.h"

/* HYDK_LF_WPB: windows a token / pack workgroup takes, one after another (1: 220 workgroups per LF group and role) */
#ifndef HYDK_LF_WPB
#define HYDK_LF_WPB 1
#endif
/* HYDK_LF_PROBE (timing only, wrong LF streams): 1 no s_setprio in the LF roles; 2 token workgroups leave no histograms (no global
 * atomics); 4 token workgroups store no records; 8 token workgroups return at once (what do 7 040 workgroups cost by existing?) */
#ifndef HYDK_LF_PROBE
#define HYDK_LF_PROBE 0
#endif

constexpr int kLfPlane = HYDK_DC_PITCH * HYDK_DC_PITCH;
constexpr int kLfWorkgroups = (kMaxWindows + HYDK_LF_WPB - 1) / HYDK_LF_WPB; /* token / pack workgroups per LF group */

/* record: bits 0-31 value, bit 32 "emit a literal", bits 33-39 run length r (0: no run pair) */
#define LF_REC(v, lit, r) ((unsigned long long)(v) | ((unsigned long long)((uint32_t)(lit) | ((uint32_t)(r) << 1)) << 32))

struct LfShape {
    int vbw, blocks, n;
    uint32_t vbw_magic; /* ceil(2^32 / vbw): rem / vbw = mulhi(rem, magic) for rem < 2^16 (vbw = 1: handled apart) */
};

__device__ __forceinline__ LfShape lf_shape(const HydkLfJob &job) {
    LfShape sh;
    sh.vbw = (job.width + 7) >> 3;
    sh.blocks = sh.vbw * ((job.height + 7) >> 3);
    sh.n = lf_values_of(job); /* 3 * blocks */
    sh.vbw_magic = sh.vbw > 1 ? (uint32_t)(0xFFFFFFFFu / (uint32_t)sh.vbw) + 1u : 0u;
    return sh;
}

/* rem / vbw for 0 <= rem < 65536 without the 30-instruction integer division: the multiply-high by
 * ceil(2^32 / vbw) overshoots rem / vbw by less than 2^-16, never across an integer (vbw <= 256) */
__device__ __forceinline__ int lf_row_of(const LfShape &sh, int rem) {
    return sh.vbw > 1 ? (int)__umulhi((uint32_t)rem, sh.vbw_magic) : rem;
}

/* hybrid-uint config (split 7, msb 1, lsb 1), entropy.c:427-444 */
__device__ __forceinline__ void lf_hybrid(uint32_t v, uint32_t &token, uint32_t &nbits, uint32_t &residue) {
    if (v < 128u) {
        token = v;
        nbits = 0;
        residue = 0;
        return;
    }
    const uint32_t nb = (31u - (uint32_t)__clz(v)) - 2u;
    residue = (v >> 1) & ((1u << nb) - 1u);
    token = 128u + (((nb - 5u) << 2) | (((v >> (nb + 1u)) & 1u) << 1) | (v & 1u));
    nbits = nb;
}

#define LF_DPP_KEEP(v, ctrl, rmask) ((uint32_t)__builtin_amdgcn_update_dpp((int)(v), (int)(v), ctrl, rmask, 0xF, false))

/* inclusive maximum over the wavefront: row_shr 1/2/4/8 inside each row of 16, then row_bcast 15 / 31 (the inclusive sum is
 * lf_huffman.h lf_wave_incl_sum) */
__device__ __forceinline__ int wave_incl_max(int v) {
    int t;
    t = (int)LF_DPP_KEEP(v, 0x111, 0xF);
    v = v > t ? v : t;
    t = (int)LF_DPP_KEEP(v, 0x112, 0xF);
    v = v > t ? v : t;
    t = (int)LF_DPP_KEEP(v, 0x114, 0xF);
    v = v > t ? v : t;
    t = (int)LF_DPP_KEEP(v, 0x118, 0xF);
    v = v > t ? v : t;
    t = (int)LF_DPP_KEEP(v, 0x142, 0xA);
    v = v > t ? v : t;
    t = (int)LF_DPP_KEEP(v, 0x143, 0xC);
    v = v > t ? v : t;
    return v;
}

/* ==========================================================================================
 * tokens: residuals -> run structure -> records + token histogram, one window per workgroup.
 * Thread t owns window positions 4t .. 4t+3.
 * ======================================================================================== */
struct LfTokenScratch {
    int wtot[kLfWaves];       /* per wave: last run head inside it (absolute index) or -1 */
    uint32_t lastv[kLfWaves]; /* per wave: its last value (the next wave's lane 0 compares against it) */
    int head[kLfWaves];       /* backward scan: nearest run head each wave found, or -1 */
    uint32_t first;           /* the window's first value */
};

/* value of the stream at plane c, block (y, x): pack_signed(lf - clamped_gradient(w, n, nw)),
 * encoder.c:574-594, in 32-bit wrap-around arithmetic (as the reference's int32 code behaves on the
 * targets it runs on) */
__device__ __forceinline__ uint32_t lf_predict(int32_t cur, int32_t w, int32_t n, int32_t nw) {
    const int32_t lo = w < n ? w : n, hi = w < n ? n : w;
    int32_t pred = (int32_t)((uint32_t)w + (uint32_t)n - (uint32_t)nw);
    pred = pred < lo ? lo : pred > hi ? hi : pred;
    const uint32_t d = (uint32_t)cur - (uint32_t)pred;
    return (d << 1) ^ (0u - (d >> 31));
}

__device__ __forceinline__ uint32_t lf_residual_at(const int32_t *dc, int c, int y, int x) {
    const int idx = c * kLfPlane + y * HYDK_DC_PITCH + x;
    const int iw = x ? idx - 1 : y ? idx - HYDK_DC_PITCH : idx;
    const int in = y ? idx - HYDK_DC_PITCH : iw;
    const int inw = x && y ? idx - HYDK_DC_PITCH - 1 : iw;
    const int32_t cur = dc[idx];
    int32_t w = dc[iw], n = dc[in], nw = dc[inw];
    if (!(x | y)) /* top-left block: all three neighbours count as 0 */
        w = n = nw = 0;
    return lf_predict(cur, w, n, nw);
}

/* the stream's value at position i (0 <= i < n) */
__device__ __forceinline__ uint32_t lf_value_at(const int32_t *dc, const LfShape &sh, int i) {
    const int visit = (i >= sh.blocks) + (i >= 2 * sh.blocks);
    const int rem = i - visit * sh.blocks;
    const int y = lf_row_of(sh, rem), x = rem - y * sh.vbw;
    return lf_residual_at(dc, visit < 2 ? 1 - visit : 2, y, x);
}

/* the thread's four consecutive values from stream position i0 on.  The usual case — all four in one
 * block row — shares its neighbours: ten loads instead of sixteen, no per-value address arithmetic. */
__device__ __forceinline__ void lf_fetch(const int32_t *dc, const LfShape &sh, int i0, uint32_t (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++)
        v[j] = 0;
    if (i0 >= sh.n)
        return;
    int visit = (i0 >= sh.blocks) + (i0 >= 2 * sh.blocks);
    const int rem = i0 - visit * sh.blocks;
    int y = lf_row_of(sh, rem), x = rem - y * sh.vbw;
    if (x + 3 < sh.vbw) { /* same row, hence same channel and inside the stream */
        const int c = visit < 2 ? 1 - visit : 2; /* Y, X, B */
        const int32_t *row = dc + c * kLfPlane + y * HYDK_DC_PITCH + x;
        const int32_t *up = y ? row - HYDK_DC_PITCH : row;
        const int32_t c0 = row[0], c1 = row[1], c2 = row[2], c3 = row[3];
        const int32_t u0 = up[0], u1 = up[1], u2 = up[2], u3 = up[3];
        const int32_t left = row[x ? -1 : 0], upleft = up[x ? -1 : 0];
        const int32_t w0 = x ? left : y ? u0 : 0;
        v[0] = lf_predict(c0, w0, y ? u0 : w0, y && x ? upleft : w0);
        v[1] = lf_predict(c1, c0, y ? u1 : c0, y ? u0 : c0);
        v[2] = lf_predict(c2, c1, y ? u2 : c1, y ? u1 : c1);
        v[3] = lf_predict(c3, c2, y ? u3 : c2, y ? u2 : c2);
        return;
    }
    const int vbh = sh.blocks / sh.vbw;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (visit < 3)
            v[j] = lf_residual_at(dc, visit < 2 ? 1 - visit : 2, y, x);
        if (++x == sh.vbw) {
            x = 0;
            if (++y == vbh) {
                y = 0;
                visit++;
            }
        }
    }
}

/* Start of the run that position `from` (>= 0) belongs to: the largest h <= from with h == 0 or
 * value[h] != value[h - 1].  All threads of the workgroup scan backwards together, 256 positions per
 * step; photographic content stops in the first step, a flat plane walks all of it (768 steps at most). */
__device__ __forceinline__ int lf_run_start(const int32_t *dc, const LfShape &sh, int from, LfTokenScratch &S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int top = from; top >= 0; top -= kLfThreads) {
        const int p = top - tid;
        int head = -1;
        if (p >= 0)
            head = (p == 0 || lf_value_at(dc, sh, p) != lf_value_at(dc, sh, p - 1)) ? p : -1;
        head = wave_incl_max(head);
        if (lane == 63)
            S.head[wave] = head;
        __syncthreads();
        int best = -1;
#pragma unroll
        for (int w = 0; w < kLfWaves; w++)
            best = best > S.head[w] ? best : S.head[w];
        __syncthreads();
        if (best >= 0)
            return best;
    }
    return 0;
}

/* returns the residue bits of the literals this thread sent */
__device__ __forceinline__ uint32_t lf_tokens_window(const HydkLfJob &job, const LfShape &sh, unsigned long long *__restrict__ recs,
                                                     int tb, int *s_rs /* [kScanSpan] */, uint32_t *s_hist, LfTokenScratch &S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t *dc = job.dc;
    const int q0 = tid * 4;

    for (int i = tid; i < HYDK_LF_CODES; i += kLfThreads)
        s_hist[i] = 0;
    uint32_t v[4];
    lf_fetch(dc, sh, tb + q0, v);
    /* what lies in front of the window: the value at tb - 1 and — only if the window's first value continues its run,
     * which photographic content hardly ever does — the start of that run (a backward scan by the whole workgroup:
     * until round 3 every window paid for it, a third of this kernel's instructions) */
    const uint32_t tailv = tb > 0 ? lf_value_at(dc, sh, tb - 1) : 0u;
    if (lane == 63)
        S.lastv[wave] = v[3];
    if (tid == 0)
        S.first = v[0];
    __syncthreads();
    const bool continues = tb > 0 && tb < sh.n && S.first == tailv; /* the same for every thread */
    const int carry = continues ? lf_run_start(dc, sh, tb - 1, S) : 0;

    /* start of the run each position belongs to (absolute index): max-scan of run heads */
    uint32_t prev = LF_DPP_KEEP(v[3], 0x138, 0xF); /* wave_shr:1 — the previous lane's last value */
    if (lane == 0)
        prev = wave ? S.lastv[wave - 1] : tailv;
    int rs[4];
    int last = -1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = tb + q0 + j;
        last = (i == 0 || i >= sh.n || v[j] != prev) ? i : last;
        rs[j] = last;
        prev = v[j];
    }
    const int inc = wave_incl_max(last);
    if (lane == 63)
        S.wtot[wave] = inc;
    __syncthreads();
    int pre = carry;
    for (int w = 0; w < wave; w++) {
        const int t = S.wtot[w];
        pre = pre > t ? pre : t;
    }
    {
        int excl = (int)LF_DPP_KEEP(inc, 0x138, 0xF);
        excl = lane ? excl : -1;
        pre = pre > excl ? pre : excl;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        rs[j] = rs[j] < 0 ? pre : rs[j];
    *(int4 *)&s_rs[q0] = make_int4(rs[0], rs[1], rs[2], rs[3]);
    __syncthreads();

    /* what each position sends, without divergent control flow: offset c inside the run's current
     * 128-chunk; "same4" = the chunk has a fifth value, i.e. more than 3 repeats behind its first */
    const int last_q = sh.n - 1 - tb; /* window-relative index of the stream's last value */
    uint32_t lit[4], r[4];
    bool need[4], any_need = false;
    int s4v[4], hq[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int q = q0 + j;
        const bool valid = q < kEmitSpan && q <= last_q;
        /* The symbol 0xFFFFFFFF (the residual of an LF int of INT_MIN, which only float input reaches) is the one the
         * reference's run detector cannot tell from "no symbol yet": it keeps last_symbol = symbol + 1, 0 for none
         * (entropy.c:508,520).  So up to 3 repeats behind such a literal are not written at all (entropy.c:489 sends them
         * only if last_symbol is set), and a stream that STARTS with it takes its first values for repeats of a value
         * in front of the stream: the run's chunks count from position -1, whose literal nobody sends and whose run
         * pair — when more than 3 values follow it — position 0 sends. */
        const bool wraps = v[j] == 0xFFFFFFFFu;
        const bool phantom = wraps && tb + q == 0;
        const int c = (tb + q - rs[j] + (wraps && rs[j] == 0 ? 1 : 0)) & 127;
        const int s4 = q - c + 4;
        const bool same4 = c <= 3 && s4 <= last_q && s_rs[s4 < kScanSpan ? s4 : kScanSpan - 1] == rs[j];
        lit[j] = valid && (c == 0 || (c <= 3 && !same4 && !wraps));
        need[j] = valid && (c == 0 || phantom) && same4;
        r[j] = 0;
        s4v[j] = s4;
        hq[j] = q - c; /* the chunk's head: q itself, or -1 in front of the stream */
        any_need |= need[j];
    }
    if (__any(any_need)) { /* some chunk head has a run behind it: how long, up to 127 (7 halvings) */
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int lo = need[j] ? s4v[j] : 0, hi = hq[j] + 127 < last_q ? hq[j] + 127 : last_q;
            hi = need[j] ? hi : 0;
#pragma unroll
            for (int it = 0; it < 7; it++) {
                const int mid = (lo + hi + 1) >> 1;
                const bool in_run = s_rs[mid] == rs[j];
                lo = in_run ? mid : lo;
                hi = in_run ? hi : mid - 1;
            }
            r[j] = need[j] ? (uint32_t)(lo - hq[j]) : 0u;
        }
    }
    uint32_t residue_bits = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (lit[j]) {
            uint32_t token, nb, res;
            lf_hybrid(v[j], token, nb, res);
            atomicAdd(&s_hist[token], 1u);
            residue_bits += nb;
        }
        if (r[j])
            atomicAdd(&s_hist[256u + r[j] - 3u], 1u);
    }
    if (!(HYDK_LF_PROBE & 4) && q0 < kEmitSpan && q0 <= last_q) { /* a thread's four records are 32 contiguous bytes; the tail of the stream is padded, never read */
        ulonglong2 *dst = (ulonglong2 *)(recs + tb + q0);
        dst[0] = make_ulonglong2(q0 + 0 <= last_q ? LF_REC(v[0], lit[0], r[0]) : 0ull, q0 + 1 <= last_q ? LF_REC(v[1], lit[1], r[1]) : 0ull);
        dst[1] = make_ulonglong2(q0 + 2 <= last_q ? LF_REC(v[2], lit[2], r[2]) : 0ull, q0 + 3 <= last_q ? LF_REC(v[3], lit[3], r[3]) : 0ull);
    }
    __syncthreads();
    return residue_bits;
}

/* a token workgroup's LDS */
struct LfTokenLds {
    __attribute__((aligned(16))) int rs[kScanSpan];
    uint32_t hist[HYDK_LF_CODES];
    LfTokenScratch tok;
    uint32_t rbits;
};

/* The token role: workgroup `wg` (0 .. kLfWorkgroups - 1) of one LF group takes HYDK_LF_WPB windows, one after another.
 * recs / hist / w are the LF group's own; hist must be zero before the launch */
__device__ __forceinline__ void lf_tokens_role(const HydkLfJob &job, unsigned long long *__restrict__ recs, uint32_t *__restrict__ hist,
                                               LfWork &w, int wg, LfTokenLds &L) {
    if (!(HYDK_LF_PROBE & 1))
        __builtin_amdgcn_s_setprio(3); /* late work of a frame whose stream holds nothing else: see kernels.hip HYDK_URGENT */
    if (HYDK_LF_PROBE & 8)
        return;
    const int tid = threadIdx.x;
    const LfShape sh = lf_shape(job);
    for (int win = wg * HYDK_LF_WPB; win < (wg + 1) * HYDK_LF_WPB && win < kMaxWindows; win++) {
        const int tb = win * kEmitSpan;
        if (tb >= sh.n)
            return;
        if (tid == 0)
            L.rbits = 0;
        uint32_t rb = lf_tokens_window(job, sh, recs, tb, L.rs, L.hist, L.tok);
        rb = lf_wave_incl_sum(rb);
        if ((tid & 63) == 63 && rb)
            atomicAdd(&L.rbits, rb);
        __syncthreads();
        for (int i = tid; i < HYDK_LF_CODES && !(HYDK_LF_PROBE & 2); i += kLfThreads) {
            const uint32_t c = L.hist[i];
            w.win_hist[win][i] = (uint16_t)c; /* at most 896 + 7 per window */
            if (c)
                atomicAdd(&hist[i], c);
        }
        if (tid == 0)
            w.win_residue_bits[win] = L.rbits;
        if (HYDK_LF_WPB > 1)
            __syncthreads(); /* the next window reuses the scratch */
    }
}

/* ==========================================================================================
 * pack: per-value bit strings -> bits at the window's offset.  A window is 1024 values
 * (four per thread); a value takes at most 59 bits.
 * ======================================================================================== */
constexpr int kPackWords = (31 + kEmitSpan * 59) / 32 + 2;

/* the bit string (value, length) each of the thread's four records sends under the LF group's code;
 * returns their total length */
__device__ __forceinline__ uint32_t lf_window_strings(const LfShape &sh, const unsigned long long *__restrict__ recs, int tb,
                                                      const uint32_t *s_code, unsigned long long (&val)[4], uint32_t (&len)[4]) {
    const int i0 = tb + (int)threadIdx.x * 4;
    unsigned long long rec[4] = {0, 0, 0, 0};
    const bool mine_window = (int)threadIdx.x * 4 < kEmitSpan; /* the last 32 threads have no values of this window */
    if (mine_window && i0 < sh.n) { /* records are stored in padded groups of four */
        const ulonglong2 a = ((const ulonglong2 *)(recs + i0))[0], b = ((const ulonglong2 *)(recs + i0))[1];
        rec[0] = a.x;
        rec[1] = a.y;
        rec[2] = b.x;
        rec[3] = b.y;
    }
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        val[j] = 0;
        len[j] = 0;
        if (mine_window && i0 + j < sh.n) {
            const uint32_t v = (uint32_t)rec[j], lit = (uint32_t)(rec[j] >> 32) & 1u, r = (uint32_t)(rec[j] >> 33) & 127u;
            if (lit) {
                uint32_t token, nb, res;
                lf_hybrid(v, token, nb, res);
                const uint32_t e = s_code[token];
                val[j] = (e & 0xFFFFu) | ((unsigned long long)res << (e >> 16));
                len[j] = (e >> 16) + nb;
            }
            if (r) {
                const uint32_t e = s_code[256u + r - 3u];
                val[j] |= (unsigned long long)(e & 0xFFFFu) << len[j];
                len[j] += e >> 16;
            }
        }
        mine += len[j];
    }
    return mine;
}

/* a pack workgroup's LDS */
struct LfPackLds {
    uint32_t bits[kPackWords];
    uint32_t code[HYDK_LF_CODES];
    uint32_t wsum[kLfWaves];
    uint32_t slot_off; /* lf_packed_slot_offset */
};

/* The pack role: workgroup `wg` of one LF group ORs the bit strings of HYDK_LF_WPB windows into an LDS window each and
 * stores whole words from `dst`, the first word of the LF group's stream, on; a stream never reaches beyond dst[room - 1]
 * (room <= HYDK_LF_BITWORDS).  The code builder has left w.codes, w.win_off and st.bit_count. */
__device__ __forceinline__ void lf_pack_role(const HydkLfJob &job, const unsigned long long *__restrict__ recs, const LfWork &w,
                                             const HydkLfStream &st, uint32_t *__restrict__ dst, uint32_t room, int wg, LfPackLds &L) {
    if (!(HYDK_LF_PROBE & 1))
        __builtin_amdgcn_s_setprio(3); /* late work of a frame whose stream holds nothing else: see kernels.hip HYDK_URGENT */
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LfShape sh = lf_shape(job);
    if (wg * HYDK_LF_WPB * kEmitSpan >= sh.n)
        return;
    for (int i = tid; i < HYDK_LF_CODES; i += kLfThreads)
        L.code[i] = w.codes[i];
    for (int win = wg * HYDK_LF_WPB; win < (wg + 1) * HYDK_LF_WPB && win < kMaxWindows; win++) {
        const int tb = win * kEmitSpan;
        if (tb >= sh.n)
            return;
        if (win != wg * HYDK_LF_WPB)
            __syncthreads(); /* the window before has left L.bits and L.wsum */
        for (int i = tid; i < kPackWords; i += kLfThreads)
            L.bits[i] = 0;
        __syncthreads();
        unsigned long long val[4];
        uint32_t len[4];
        const uint32_t mine = lf_window_strings(sh, recs, tb, L.code, val, len);
        const uint32_t inc = lf_wave_incl_sum(mine);
        if (lane == 63)
            L.wsum[wave] = inc;
        __syncthreads();
        const uint32_t gbits = w.win_off[win]; /* bits in front of this window */
        uint32_t pos = (gbits & 31u) + inc - mine, total = 0;
        for (int i = 0; i < kLfWaves; i++) {
            const uint32_t t = L.wsum[i];
            if (i < wave)
                pos += t;
            total += t;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!len[j])
                continue;
            const uint32_t at = pos >> 5, shl = pos & 31u;
            const unsigned long long lo = val[j] << shl;
            const uint32_t hi = shl ? (uint32_t)(val[j] >> (64u - shl)) : 0u;
            if ((uint32_t)lo)
                atomicOr(&L.bits[at], (uint32_t)lo);
            if ((uint32_t)(lo >> 32))
                atomicOr(&L.bits[at + 1], (uint32_t)(lo >> 32));
            if (hi)
                atomicOr(&L.bits[at + 2], hi);
            pos += len[j];
        }
        __syncthreads();
        /* whole words are stored; the first and the last word of the span may be shared with the neighbouring windows, whose
         * workgroups run in any order and find whatever an earlier frame left: each replaces exactly its own bits of such a word
         * (the masks of neighbours are disjoint, so their ANDs and ORs commute).  The window that ends the stream owns the rest
         * of its last word, which stays zero */
        if (!total)
            continue;
        const uint32_t end = (gbits & 31u) + total, last = (end - 1u) >> 5;
        if ((gbits >> 5) + last >= room)
            continue; /* offsets no code builder wrote (a measurement build that leaves the builder out): never outside the stream's words */
        const bool ends_stream = gbits + total == st.bit_count;
        uint32_t *out = dst + (gbits >> 5);
        for (uint32_t i = tid; i <= last; i += kLfThreads) {
            uint32_t mask = 0xFFFFFFFFu;
            if (i == 0)
                mask <<= gbits & 31u;
            if (i == last && (end & 31u) && !ends_stream)
                mask &= (1u << (end & 31u)) - 1u;
            if (mask == 0xFFFFFFFFu)
                out[i] = L.bits[i];
            else {
                atomicAnd(&out[i], ~mask);
                atomicOr(&out[i], L.bits[i]);
            }
        }
    }
}

/* Where LF group `slot`'s stream starts in the packed area, in words, when the pack workgroups write there at once: the LF
 * groups' streams lie back to back in slot order, each from a 4-byte boundary, so two never share a word.  Every bit count
 * is known when the launch begins (the code builders ran in the launch before): the first wavefront sums the words of the at
 * most 254 slots in front.  The workgroup of the slot's window 0 writes the stream's byte offset, whether the stream holds
 * bits or not, and the last slot's the total.  Called by all threads of the workgroup, before anything returns. */
__device__ __forceinline__ uint32_t lf_packed_slot_offset(HydkLfStream *streams, int slot, int num_slots,
                                                          unsigned long long *total, int wg, LfPackLds &L) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        uint32_t mine = 0;
        for (int s = tid; s < slot; s += 64)
            mine += (streams[s].bit_count + 31u) >> 5;
        mine = lf_wave_incl_sum(mine);
        if (tid == 63)
            L.slot_off = mine;
    }
    __syncthreads();
    const uint32_t off = L.slot_off;
    if (wg == 0 && tid == 0) {
        streams[slot].offset = off * 4u;
        if (slot == num_slots - 1)
            *total = (unsigned long long)(off + ((streams[slot].bit_count + 31u) >> 5)) * 4ull;
    }
    return off;
}
