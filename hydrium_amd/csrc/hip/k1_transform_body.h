/*
 * k1_transform_body.h — the body of the transform kernel (kernels.hip, K1), included into k_transform_tokenize, into
 * k_transform_tokenize_p016, into k_transform_tokenize_planar, into k_transform_tokenize_yuvp16, into k_transform_tokenize_yuy2, into k_transform_tokenize_y216, into k_transform_tokenize_dword, into k_transform_tokenize_quad and into k_transform_tokenize_ufloat and nowhere else.  In scope where it is included: the template parameters or constants FMT, XMODE
 * and STORE, the kernel's parameters jobs, status, part_info and plog, and everything kernels.hip defines above its K1 section.
 * No include guard: it is function-body text, meant to be included once per kernel.
 */
    /* What STORE is made of (hydk_store.h).  YUV: a YCbCr form — a pixel becomes an RGB pixel of its class right after the load.
     * TWO_PLANES: U and V in planes of their own, whose pitch is job.pixel_stride, subsampled as job.sub says (planar YCbCr);
     * else (U, V) pairs in one half-resolution plane of the Y plane's pitch (NV12; P010 / P012 / P016 in 16-bit words).
     * PK: no chroma plane at all — packed 4:2:2, U and V among the Y bytes of one plane in the byte order job.sub names (hydk_yuy2.h),
     * or among the Y words of one plane of 16-bit words (hydk_y216.h).
     * INTERP: chroma interpolated (hydk_chroma.h) — job.filter says centre- or left-sited, and the job knows the picture it is
     * cut from, since a pixel's chroma neighbours may lie in another LF group or tile of it.  HALF: 2-byte floats, widened on load.
     * DW: a pixel is one dword of three 10-bit fields (hydk_rgb10.h) — RGB10, which is no YCbCr form, and Y410, which is one with
     * neither planes nor groups: every pixel carries its own chroma.
     * QD: a pixel is one group of four samples, the fourth ignored (hydk_quad.h) — AYUV, bytes in a dword, and Y416, words in a qword:
     * YCbCr 4:4:4 as Y410 is, of whole samples, so neither PK nor DW.
     * UF: a pixel is one dword of three unsigned floats (hydk_ufloat.h) — R11G11B10F and RGB9E5, storage forms of the float class as
     * the half-precision ones are: widened exactly on load, float32 samples from there on */
    constexpr HydkStoreForm FORM = hydk_store_form(STORE);
    static_assert(STORE == HYDK_STORE_F32 || FORM.cls == FMT,
                  "the float class has the half-precision storage forms, R11G11B10F and RGB9E5, the 8-bit class NV12, NV12I, YUVP, YUVPI, YUY2 and YUY2I, the 16-bit class P016, P016I, YUVP16, YUVP16I, Y216, Y216I, RGB10 and Y410; AYUV is of the 8-bit class and Y416 of the 16-bit class");
    constexpr bool DW = STORE == HYDK_STORE_RGB10 || STORE == HYDK_STORE_Y410;
    constexpr bool QD = STORE == HYDK_STORE_AYUV || STORE == HYDK_STORE_Y416;
    constexpr bool YUV = FORM.ycbcr, TWO_PLANES = FORM.chroma_planes == 2, PK = YUV && FORM.chroma_planes == 0 && !DW && !QD, INTERP = FORM.interp;
    constexpr bool UF = STORE == HYDK_STORE_R11G11B10F || STORE == HYDK_STORE_RGB9E5;
    constexpr bool HALF = FMT == HYDK_FMT_F32 && STORE != HYDK_STORE_F32 && !UF;
    /* the two-plane forms by name: YUVPI keeps a prefetch, an edge fill and an interpolate loop of its own (through the shared
     * ones its instances measured a few tenths of a percent slower, profiles/ycbcr_loader.txt) */
    constexpr bool YUVP = TWO_PLANES && !INTERP && FMT == HYDK_FMT_U8, YUVPI = TWO_PLANES && INTERP && FMT == HYDK_FMT_U8;
    /* the two-plane forms of 16-bit words, nearest and interpolated: windows of their own beside the 8-bit ones (hydk_yuvp16.h) */
    constexpr bool YP16 = TWO_PLANES && FMT == HYDK_FMT_U16;
    /* packed 4:2:2 by sample size: bytes (YUY2, YUY2I) unpack into YUVP's and YUVPI's registers, words (Y216, Y216I) into YP16's */
    constexpr bool PK8 = PK && FMT == HYDK_FMT_U8, PK16 = PK && FMT == HYDK_FMT_U16;
    typedef typename std::conditional<HALF, uint16_t, typename SampleOf<FMT>::type>::type sample_t;
    constexpr bool LUTS = XMODE == kXybGather;
    constexpr int kWords = FMT == HYDK_FMT_U8 ? 6 : 12; /* dwords holding 8 packed RGB pixels */
    /* dwords of the prefetched block row: QD keeps its eight pixels as stored, the fourth sample with them — 8 dwords of bytes, 16 of
     * words — and drops it at use; every other form's window is the kWords of the packed row */
    constexpr int kWin = QD ? (FMT == HYDK_FMT_U8 ? 8 : 16) : kWords;
#if HYDK_K1_PRIO
    __builtin_amdgcn_s_setprio(HYDK_K1_PRIO);
#endif
    /* plog > 0 (launches of one or two LF groups: a tile-mode frame, the drop-in API's closing tile): a group is walked by
     * 1 << plog workgroups, a run of strips each, so that 64 or 128 groups still fill 256 compute units; every part leaves
     * its symbols in its own share of the group's token array and k_join_parts closes the gaps (round 5) */
    const unsigned bid = blockIdx.x >> plog, part = blockIdx.x & ((1u << plog) - 1u);
    const HydkLfJob job = jobs[bid >> 6];
    /* (a YCbCr job names its variant as mode + its form's variant bit: the RGB instances' own test turns it away as it stands) */
    if (job.fmt != FMT || (FMT != HYDK_FMT_F32 && job.use_luts != xyb_arith(XMODE) + FORM.variant) ||
        (FMT == HYDK_FMT_F32 && job.storage != (uint32_t)STORE))
        return; /* another template instance of this launch round owns this LF group */
    if ((int)(bid & 63) >= job.gcols * job.grows)
        return;
    if (FMT == HYDK_FMT_F32 && job.rec_bytes != 8) {
        /* the context's token arrays are laid out for 4-byte records; the host widens them before it
         * records a float LF group, so this is unreachable — kept so that a host bug cannot corrupt memory */
        if (threadIdx.x == 0) {
            atomicOr(status, HYDK_STATUS_LAYOUT);
            job.sym_count[bid & 63] = 0;
            job.rbits_total[bid & 63] = 0;
            if (plog)
                part_info[blockIdx.x] = uint2{0u, 0u};
        }
        return;
    }

#if HYDK_K1_CHANSEQ
    static_assert(HYDK_K1_WAVELOCAL, "the channels share one row-pass buffer: a wavefront must read only what it wrote");
    /* [block][kv][kh]: ONE channel's row-pass output at a time, 9.0 KiB; [c][block][kh][kv]: quantised coefficients, 12.0 KiB
     * (integer input: |q| < 2^13, see store_record; float input keeps 32-bit coefficients) */
    typedef typename std::conditional<FMT == HYDK_FMT_F32, int32_t, int16_t>::type coef_t;
    constexpr int kQBlock = 64;
    __shared__ float s_rowpass[kS0Chan];
    __shared__ __attribute__((aligned(16))) coef_t s_q[3 * 32 * kQBlock];
#else
    /* [c][block][kv][kh]: row-pass output, overwritten in place by the quantised coefficients, 27.0 KiB */
    __shared__ float s_rowpass[3 * kS0Chan];
#endif
    /* exclusive prefix sums of the blocks' symbol counts + strip total.  Every wave computes and writes the same
     * 33 values (no barrier needed before it reads them back: its own stores are ordered before its loads) */
    __shared__ uint32_t s_boff[33];
    __shared__ uint32_t s_rbits;                      /* residue bits of the group's symbols */
    /* integer input cannot produce a token above 35 (see store_record): 40 bins per cluster suffice.  LDS is
     * handed out in granules of 1280 bytes (measured: a 33 284-byte build lost the co-residency a 33 232-byte
     * one has): at <= 26 granules two of these workgroups fit beside an entropy-stage workgroup (75 granules) */
    constexpr int kHistW = FMT == HYDK_FMT_F32 ? 72 : (int)HYDK_REC32_TOKENS; /* float input: the (4,1,0) configuration ends at token 71 */
    __shared__ uint32_t s_hist[HYDK_MAX_CLUSTERS * kHistW];
    __shared__ uint16_t s_lut8[256];
    __shared__ uint8_t s_nnz3[64];                    /* coefficient-count context offset (encoder.c:60-66) mod 3 */
    __shared__ uint16_t s_jinfo[64];                  /* zig-zag position j -> natural index kv*8+kh | (frequency context (encoder.c:53-58) mod 3) << 8 */
    /* per (varblock, visit = Y, X, B): {non-zero bitmap by zig-zag position (2 words), symbols | non-zeros << 8,
     * word offset of the block's coefficients in s_rowpass}.  The walk's last step reads one entry past the end
     * and never uses it (whatever follows in LDS, or zero) */
    __shared__ uint4 s_seg[32 * 3];
    __shared__ uint32_t s_blen[32];                   /* symbols of the block's Y | X << 8 | B << 16 runs */
    __shared__ __attribute__((aligned(16))) float s_wq[3 * 64]; /* quantisation weight [channel][kh][kv]: a thread's eight in two 16-byte reads */

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const int g = (int)(bid & 63);
    const int gx = g % job.gcols, gy = g / job.gcols;
    const int px0 = gx << 8, py0 = gy << 8;
    const int gw = min(256, job.width - px0), gh = min(256, job.height - py0);
    const int gbw = (gw + 7) >> 3, gbh = (gh + 7) >> 3;

    for (int i = t; i < HYDK_MAX_CLUSTERS * kHistW; i += kThreads)
        s_hist[i] = 0;
    /* The 8-bit transfer table.  QD's 8-bit instance (AYUV) keeps it in no array of its own: a block of s_rowpass is kS0Block = 64 + 8
     * floats, and words 64 ... 71 of a block are padding that no row pass, column pass or token walk touches — 32 bytes, sixteen
     * entries; the table's 256 sit in the padding of channel 0's blocks 0 ... 15, entry v at 16-bit index 128 + v + ((v & 0xF0) << 3)
     * (byte (v >> 4) * 4 * kS0Block + 256 + 2 * (v & 15)).  That keeps the instance at the static LDS of the 16-bit class. */
    static_assert(kS0Block == 72, "lut8's index is spelled for blocks of 64 + 8 floats");
    auto lut8_at = [](uint32_t v) -> uint32_t { return 128u + v + ((v & 0xF0u) << 3); };
    auto lut8 = [&](uint32_t v) -> uint32_t { return QD ? (uint32_t)((const uint16_t *)s_rowpass)[lut8_at(v)] : (uint32_t)s_lut8[v]; };
    if (FMT == HYDK_FMT_U8) {
        if (QD)
            ((uint16_t *)s_rowpass)[lut8_at((uint32_t)t)] = job.in_lut8[t];
        else
            s_lut8[t] = job.in_lut8[t];
    }
    if (t < 64) {
        /* t as a natural index (kv, kh): where it sits in zig-zag order; t as a zig-zag position: its contexts */
        const int j = t;
        s_nnz3[t] = kNnzCtx[t] % 3;
        /* two threads write the two bytes of an entry: kept apart as bytes here, read as one u16 */
        ((uint8_t *)s_jinfo)[2 * kZigzag[t >> 3][t & 7]] = HYDK_K1_CHANSEQ ? (uint8_t)(((t & 7) << 3) | (t >> 3)) : (uint8_t)t; /* (CHANSEQ: coefficients sit [kh][kv]) */
        ((uint8_t *)s_jinfo)[2 * t + 1] = (uint8_t)((j < 2 ? 0 : j < 16 ? j - 1 : j < 32 ? 15 + ((j - 16) >> 1) : 23 + ((j - 32) >> 2)) % 3);
    }
    if (t < 192) /* t = (c, kh, kv) */
        s_wq[t] = (float)kQuantWeight[t >> 6][kZigzag[t & 7][(t >> 3) & 7]];

    /* column / token phases: thread (block cb, horizontal frequency kh) */
    const int cb = t >> 3, kh = t & 7;
    const uint32_t nib_row = (uint32_t)kh * (uint32_t)sizeof(kNibbleMasks.m[0]); /* 256 bytes per kh */
    /* first cluster holding coefficient contexts, by scheme (encoder.c:862-901) */
    const int coef_cl_lo = job.scheme == 0 ? 3 : job.scheme == 3 ? 0 : 1;

    /* (which loader a layout gets, from here to hfast, is restated by loader() in tests/pixel_layouts.py: change them together) */
    const bool packed = !YUV && job.pixel_stride == 3 &&
                        (const char *)job.src[1] == (const char *)job.src[0] + sizeof(sample_t) &&
                        (const char *)job.src[2] == (const char *)job.src[0] + 2 * sizeof(sample_t) &&
                        (((uintptr_t)job.src[0] | (uintptr_t)(job.row_stride * (long long)sizeof(sample_t))) & 3) == 0 &&
                        FMT != HYDK_FMT_F32;

    /* phase-A role of this thread: row ar of block ab */
#if HYDK_K1_WAVELOCAL
    /* wavefront w row-transforms all eight rows of blocks 8w .. 8w+7: exactly the blocks whose columns it takes in
     * phase B (cb = t >> 3), so the transposition through LDS stays inside the wavefront */
    const int ar = lane >> 3, ab = (wave << 3) | (lane & 7);
#else
    const int ar = t >> 5, ab = t & 31;
#endif
    /* half-precision storage: a block row's 24 samples are 12 dwords too — 8 interleaved pixels in one run (hrun 1), or 4
     * dwords from each of three planes (hrun 2: what an NCHW network output is) — when every row starts on a dword: the base
     * addresses and the row stride in BYTES (an odd number of samples misaligns every other row).  Anything else — RGBA,
     * odd bases, odd strides — reads sample by sample below, as float32 storage always does (job.per_sample: the probe
     * flavour's A/B switch, profiles/half_formats.txt). */
    int hrun = 0;
    if (HALF) {
        const bool rows4 = ((job.row_stride * 2) & 3) == 0;
        if (!(job.per_sample & 1u) && job.pixel_stride == 3 && rows4 && ((uintptr_t)job.src[0] & 3) == 0 &&
            (const char *)job.src[1] == (const char *)job.src[0] + 2 && (const char *)job.src[2] == (const char *)job.src[0] + 4)
            hrun = 1;
        else if (!(job.per_sample & 2u) && job.pixel_stride == 1 && rows4 &&
                 (((uintptr_t)job.src[0] | (uintptr_t)job.src[1] | (uintptr_t)job.src[2]) & 3) == 0)
            hrun = 2;
    }
    const bool hfast = HALF && hrun != 0 && ab < gbw && ab * 8 + 8 <= gw;
    /* unsigned floats in a dword (UF): a block row is eight dwords of the row's one plane, 32 bytes, fetched a strip ahead as two
     * 16-byte loads where every row of the picture starts on a 16-byte boundary — the base and the pitch in BYTES (a block's first
     * column is a multiple of 8 dwords) — and the block is whole.  A ragged last block, a crop at a column that is no multiple of
     * four and a pitch of the same kind read dword by dword at use, the pixels the row has and nothing else. */
    const bool ufast = UF && (((uintptr_t)job.src[0] | (uintptr_t)(job.row_stride * 4)) & 15) == 0 && ab < gbw && ab * 8 + 8 <= gw;
    /* YCbCr, every form: a block row is fetched as a WINDOW of dwords — its eight Y samples in nxt[0 ... kYW), and the chroma that
     * serves them — when planes and pitches are dword multiples (a block's first column is a multiple of 8, its chroma column
     * even); anything else reads sample by sample.  SB: bits of a sample; a dword holds kSPD samples or kPPD (U, V) pairs */
    constexpr int SB = FMT == HYDK_FMT_U8 ? 8 : 16, kSPD = 32 / SB, kPPD = kSPD / 2, kYW = 8 / kSPD;
    constexpr uint32_t kSMask = (1u << SB) - 1u;
    const HydkYuvMatrix yuv = YUV && SB == 16 ? hydk_yuv16_job_matrix(job.matrix) : hydk_yuv_matrix(YUV ? (int)job.matrix : 0);
    const int pcx = INTERP ? job.pic_cx0 + ((px0 + ab * 8) >> 1) : 0;
    /* log2 of the pixels one chroma sample spans across and down: the job's subsampling for two planes, 4:2:0 for pairs */
    const int csx = TWO_PLANES ? hydk_planar_sx((int)job.sub) : (int)YUV, csy = TWO_PLANES ? hydk_planar_sy((int)job.sub) : (int)(YUV && !PK);
    /* pairs in one plane (nvrun, prun): kYW dwords of Y and, from chroma row y >> 1, kYW dwords holding the block's four pairs */
    const bool prun = YUV && !TWO_PLANES && !PK && !DW && !QD &&
                      (((uintptr_t)job.src[0] | (uintptr_t)job.src[1] | (uintptr_t)(job.row_stride * (SB / 8))) & 3) == 0;
    /* packed 4:2:2 (pkrun): a block row is four GROUPS — 16 bytes, four dwords — from the row's one plane, when the first group (Y's
     * place in its pair of bytes before src[0]) and the pitch are dword multiples; Y and the four (U, V) pairs are picked out of the
     * registers at use, by the byte order (wave-uniform).  pk_y: 0 — Y is the first byte of a pair, 1 — the second; pk_vu: V before U.
     * 16-bit words (PK16): the four groups are 32 bytes, EIGHT DWORDS, under the same test with the pitch in bytes.  The test asks for
     * dword multiples and no more, as every other form's does: a crop at an odd group, or a pitch of an even number of words that
     * is no multiple of eight, keeps the dword and would lose 16 bytes.  The eight dword loads of one address are fused by the
     * compiler into two global_load_dwordx4, which the hardware takes at dword alignment */
    const int pk_y = PK ? hydk_yuy2_y_offset((int)job.sub) : 0, pk_vu = PK ? hydk_yuy2_v_first((int)job.sub) : 0;
    const bool pkrun = PK && ((((uintptr_t)job.src[0] - (uintptr_t)(pk_y * (SB / 8))) | (uintptr_t)(job.row_stride * (SB / 8))) & 3) == 0;
    /* two planes (ylrun): two dwords of Y and, from each chroma plane, the dword of four samples that serves its eight pixels
     * (the block's chroma column is a multiple of 4) — two dwords of eight for 4:4:4.  16-bit words (YP16): four dwords of Y and
     * two from each chroma plane — four for 4:4:4, kWords in all — where the three bases and both pitches IN BYTES are dword
     * multiples */
    const bool ylrun = TWO_PLANES && (((uintptr_t)job.src[0] | (uintptr_t)(job.row_stride * (SB / 8)) | (uintptr_t)job.src[1] |
                                       (uintptr_t)job.src[2] | (uintptr_t)(job.pixel_stride * (SB / 8))) & 3) == 0;
    /* interpolated chroma (irun, pirun, ylirun): beside the near row's four chroma samples the window holds the same four of the
     * far row — the one the filter mixes in: above for an even y, below for an odd one, clamped to the PICTURE's chroma rows;
     * 4:2:2 has no other row: far is near — and of both rows the sample behind those four and (centre-sited) the one before
     * them: six columns, p = 0 ... 5.  It comes as dwords only where all six lie inside the picture's chroma row; the picture's
     * first and last chroma columns, a ragged last block and shifted bases or pitches fill the same window sample by sample with
     * the clamps, at use (phase A below).  pcx: the picture's chroma column of the block's first pixel. */
    const bool irun = (TWO_PLANES ? ylrun : PK ? pkrun : prun) && (!INTERP || ((job.filter == HYDK_CHROMA_CENTRE ? pcx >= 1 : pcx >= 0) && pcx + 4 <= job.pic_cw - 1));
    /* (a dword a pixel, DW: a block row is eight dwords of the row's one plane, 32 bytes; src[0] is dword-aligned and the pitch counts
     * dwords — hyd_fmt_refusal lets nothing else through — so every whole block row comes that way.  A group of four a pixel, QD: the same of
     * eight dwords (AYUV) or eight qwords (Y416), src[0] on a boundary of the pixel's size and the pitch in pixels) */
    const bool fast = (DW || QD || (YUV ? irun : packed)) && ab < gbw && ab * 8 + 8 <= gw; /* whole block row comes as aligned dwords */
    uint32_t nxt[kWin];
    /* the window's columns 0 and 5, which sit in no dword of the four between them (YUVPI: of U and of V, column 0 | column 5
     * << 8 of the near row, the same << 16 of the far row; YP16: column 0 | column 5 << 16 of U near, U far, V near, V far) */
    constexpr int kFlank = YUV && !TWO_PLANES ? 4 / kPPD : YP16 ? 4 : 2;
    uint32_t flank[kFlank] = {};
#pragma unroll
    for (int k = 0; k < kWin; k++)
        nxt[k] = 0;
    /* The window accessor of the forms with pairs in one plane (NV12I, P016I; nearest: columns 1 ... 4 of the near row alone):
     * where chroma sample c (0: U, 1: V) of row r (0: near, 1: far) and column p sits — all the shared loops below know of a
     * form.  nxt[kYW ...] holds the near row's columns 1 ... 4 as loaded, nxt[2 kYW ...] the far row's; flank columns 0 and 5
     * of the near row, then of the far row, packed as pairs are. */
    auto win_word = [&](int r, int p) -> uint32_t & {
        const bool edge = p == 0 || p == 5;
        const int k = edge ? 2 * r + (p == 5) : p - 1;
        return edge ? flank[k / kPPD] : nxt[(1 + r) * kYW + k / kPPD];
    };
    auto win_shift = [](int c, int r, int p) -> int {
        const bool edge = p == 0 || p == 5;
        return 2 * SB * ((edge ? 2 * r + (p == 5) : p - 1) % kPPD) + SB * c;
    };
    auto win_get = [&](int c, int r, int p) -> uint32_t { return (win_word(r, p) >> win_shift(c, r, p)) & kSMask; };
    auto win_put = [&](int c, int r, int p, uint32_t v) { win_word(r, p) |= v << win_shift(c, r, p); };
    /* nearest chroma: sample c of pixel i's own column.  Two planes (YUVP): byte i >> 1 of nxt[2] (U) or nxt[3] (V), or (4:4:4, a
     * sample a pixel) byte i of the two dwords a plane at nxt[2 + 2 c].  YP16: word i >> 1, or (4:4:4) word i, of the dwords at
     * nxt[4 + 4 c] */
    auto near_get = [&](int c, int i) -> uint32_t {
        if (PK8) /* (unpacked at use into YUVP's 4:2:2 places: four U bytes in nxt[2], four V bytes in nxt[3]) */
            return (nxt[2 + c] >> (8 * (i >> 1))) & 0xFF;
        if (!TWO_PLANES && !PK16)
            return win_get(c, 0, 1 + (i >> 1));
        if (YP16 || PK16) { /* (PK16: unpacked at use into YP16's 4:2:2 places, csx = 1) */
            const uint32_t s2 = (nxt[4 + 4 * c + (i >> 2)] >> (16 * ((i >> 1) & 1))) & 0xFFFF, s4 = (nxt[4 + 4 * c + (i >> 1)] >> (16 * (i & 1))) & 0xFFFF;
            return csx ? s2 : s4;
        }
        const uint32_t s2 = (nxt[2 + c] >> (8 * (i >> 1))) & 0xFF, s4 = (nxt[2 + 2 * c + (i >> 2)] >> (8 * (i & 3))) & 0xFF;
        return csx ? s2 : s4;
    };
    /* the far chroma row of the LF group's row y: in picture coordinates, clamped there, and back relative to src[1] (may be -1:
     * the LF group above) */
    auto far_row = [&](long long y) -> long long {
        return (long long)hydk_chroma_vy(2 * job.pic_cy0 + (int32_t)y, job.pic_ch) - job.pic_cy0;
    };
    auto prefetch = [&](int s) {
        if (UF) {
            /* the eight pixels as stored in nxt[0 ... 7], the float instance's prefetch registers: eight dword loads of one 16-byte
             * aligned address, two global_load_dwordx4; the fields come out, and are widened, at use */
            if (ufast && s * 8 + ar < gh) {
                const long long y = py0 + s * 8 + ar, x = px0 + ab * 8;
                const char *pd = (const char *)job.src[0] + (y * job.row_stride + x) * 4;
#pragma unroll
                for (int k = 0; k < 8; k++)
                    nxt[k] = HYDK_GLOBAL(const uint32_t, pd)[k];
            }
            return;
        }
        if (QD) {
            /* the eight pixels as stored in nxt[0 ... kWin): kWin dword loads of one address, which the compiler fuses into two (AYUV) or
             * four (Y416) global_load_dwordx4 as it does DW's; the hardware takes them at dword alignment, and hyd_fmt_refusal
             * guarantees the pixel's own; the samples come out at use */
            if (fast && s * 8 + ar < gh) {
                /* (the lane's row and block pass through an empty statement, as DW's do and for its reason) */
                int lane_row = ar, lane_block = ab;
                asm volatile("" : "+v"(lane_row), "+v"(lane_block));
                const long long y = py0 + s * 8 + lane_row, x = px0 + lane_block * 8;
                const char *pq = (const char *)job.src[0] + (y * job.row_stride + x) * (kWin / 2);
#pragma unroll
                for (int k = 0; k < kWin; k++)
                    nxt[k] = HYDK_GLOBAL(const uint32_t, pq)[k];
            }
            return;
        }
        if (DW) {
            /* the eight pixels as stored in nxt[0 ... 7]: eight dword loads of one address, which the compiler fuses into two
             * global_load_dwordx4 as it does PK16's (the hardware takes them at dword alignment); the fields come out at use */
            if (fast && s * 8 + ar < gh) {
                /* (the lane's row and block pass through an empty statement, as PK16's do and for its reason) */
                int lane_row = ar, lane_block = ab;
                asm volatile("" : "+v"(lane_row), "+v"(lane_block));
                const long long y = py0 + s * 8 + lane_row, x = px0 + lane_block * 8;
                const char *pd = (const char *)job.src[0] + (y * job.row_stride + x) * 4;
#pragma unroll
                for (int k = 0; k < 8; k++)
                    nxt[k] = HYDK_GLOBAL(const uint32_t, pd)[k];
            }
            return;
        }
        if (PK16) {
            /* the four groups as stored in nxt[0 ... 7]; interpolated: the group behind them in nxt[8], nxt[9] and (centre-sited) the
             * one before them in nxt[10], nxt[11], whole dwords too: irun says that both lie inside the picture's row */
            if (fast && s * 8 + ar < gh) {
                /* (the lane's row and block pass through an empty statement, as YP16's do and for its reason: the address is made
                 * anew for every strip and not carried as a 64-bit pointer, which cost the nearest instances their last register) */
                int lane_row = ar, lane_block = ab;
                asm volatile("" : "+v"(lane_row), "+v"(lane_block));
                const long long y = py0 + s * 8 + lane_row, x = px0 + lane_block * 8;
                const char *pg = (const char *)job.src[0] + (y * job.row_stride + 2 * x - pk_y) * 2;
#pragma unroll
                for (int k = 0; k < 8; k++)
                    nxt[k] = HYDK_GLOBAL(const uint32_t, pg)[k];
                if (INTERP) {
                    const bool centre = job.filter == HYDK_CHROMA_CENTRE; /* (left-sited chroma never looks before) */
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        nxt[8 + k] = HYDK_GLOBAL(const uint32_t, pg)[8 + k];
                        nxt[10 + k] = centre ? HYDK_GLOBAL(const uint32_t, pg - 8)[k] : 0u;
                    }
                }
            }
            return;
        }
        if (PK8) {
            /* the four groups as stored in nxt[0 ... 3]; interpolated: the group behind them in flank[1] and (centre-sited) the one
             * before them in flank[0], whole dwords too: irun says that both lie inside the picture's row */
            if (fast && s * 8 + ar < gh) {
                const long long y = py0 + s * 8 + ar, x = px0 + ab * 8;
                const char *pg = (const char *)job.src[0] - pk_y + y * job.row_stride + 2 * x;
#pragma unroll
                for (int k = 0; k < 4; k++)
                    nxt[k] = HYDK_GLOBAL(const uint32_t, pg)[k];
                if (INTERP) {
                    flank[1] = HYDK_GLOBAL(const uint32_t, pg)[4];
                    flank[0] = job.filter == HYDK_CHROMA_CENTRE ? HYDK_GLOBAL(const uint32_t, pg - 4)[0] : 0u; /* (left-sited chroma never looks before) */
                }
            }
            return;
        }
        if (YUV && !TWO_PLANES) {
            if (fast && s * 8 + ar < gh) {
                typedef typename std::conditional<SB == 8, uint16_t, uint32_t>::type pair_t;
                const long long y = py0 + s * 8 + ar, x = px0 + ab * 8;
                const char *py = (const char *)job.src[0] + (y * job.row_stride + x) * (SB / 8);
                const char *pn = (const char *)job.src[1] + ((y >> 1) * job.row_stride + x) * (SB / 8);
#pragma unroll
                for (int k = 0; k < kYW; k++) {
                    nxt[k] = HYDK_GLOBAL(const uint32_t, py)[k];
                    nxt[kYW + k] = HYDK_GLOBAL(const uint32_t, pn)[k];
                }
                if (INTERP) {
                    const char *pf = (const char *)job.src[1] + (far_row(y) * job.row_stride + x) * (SB / 8);
#pragma unroll
                    for (int k = 0; k < kYW; k++)
                        nxt[2 * kYW + k] = HYDK_GLOBAL(const uint32_t, pf)[k];
                    uint32_t fl[4] = {0, HYDK_GLOBAL(const pair_t, pn)[4], 0, HYDK_GLOBAL(const pair_t, pf)[4]};
                    if (job.filter == HYDK_CHROMA_CENTRE) { /* (left-sited chroma never looks before the window) */
                        fl[0] = HYDK_GLOBAL(const pair_t, pn - sizeof(pair_t))[0];
                        fl[2] = HYDK_GLOBAL(const pair_t, pf - sizeof(pair_t))[0];
                    }
#pragma unroll
                    for (int k = 0; k < kFlank; k++)
                        flank[k] = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) /* columns 0, 5 of the near row, then of the far row: win_word's order */
                        flank[k / kPPD] |= fl[k] << (2 * SB * (k % kPPD));
                }
            }
            return;
        }
        if (YUVP) {
            if (fast && s * 8 + ar < gh) {
                const long long y = py0 + s * 8 + ar, x = px0 + ab * 8;
                const char *py = (const char *)job.src[0] + y * job.row_stride + x;
                const long long co = (y >> csy) * job.pixel_stride + (x >> csx);
                const char *pu = (const char *)job.src[1] + co, *pv = (const char *)job.src[2] + co;
                nxt[0] = HYDK_GLOBAL(const uint32_t, py)[0];
                nxt[1] = HYDK_GLOBAL(const uint32_t, py)[1];
                if (csx) {
                    nxt[2] = HYDK_GLOBAL(const uint32_t, pu)[0];
                    nxt[3] = HYDK_GLOBAL(const uint32_t, pv)[0];
                } else {
                    nxt[2] = HYDK_GLOBAL(const uint32_t, pu)[0];
                    nxt[3] = HYDK_GLOBAL(const uint32_t, pu)[1];
                    nxt[4] = HYDK_GLOBAL(const uint32_t, pv)[0];
                    nxt[5] = HYDK_GLOBAL(const uint32_t, pv)[1];
                }
            }
            return;
        }
        if (YUVPI) {
            if (fast && s * 8 + ar < gh) {
                const long long y = py0 + s * 8 + ar, x = px0 + ab * 8;
                /* the far row in the picture's chroma rows, clamped there, and back relative to src[1] (4:2:2: the near row) */
                const long long ny = y >> csy;
                const long long fy = csy ? (long long)hydk_chroma_vy(2 * job.pic_cy0 + (int32_t)y, job.pic_ch) - job.pic_cy0 : ny;
                const char *py = (const char *)job.src[0] + y * job.row_stride + x;
                const long long on = ny * job.pixel_stride + (x >> 1), of = fy * job.pixel_stride + (x >> 1);
                const char *un = (const char *)job.src[1] + on, *vn = (const char *)job.src[2] + on;
                nxt[0] = HYDK_GLOBAL(const uint32_t, py)[0];
                nxt[1] = HYDK_GLOBAL(const uint32_t, py)[1];
                nxt[2] = HYDK_GLOBAL(const uint32_t, un)[0];
                nxt[4] = HYDK_GLOBAL(const uint32_t, vn)[0];
                /* before | behind << 8 of the near row, the same << 16 of the far row (left-sited chroma never looks before) */
                uint32_t fu = (uint32_t)HYDK_GLOBAL(const uint8_t, un)[4] << 8, fv = (uint32_t)HYDK_GLOBAL(const uint8_t, vn)[4] << 8;
                if (job.filter == HYDK_CHROMA_CENTRE) {
                    fu |= HYDK_GLOBAL(const uint8_t, un - 1)[0];
                    fv |= HYDK_GLOBAL(const uint8_t, vn - 1)[0];
                }
                if (csy) {
                    const char *uf = (const char *)job.src[1] + of, *vf = (const char *)job.src[2] + of;
                    nxt[3] = HYDK_GLOBAL(const uint32_t, uf)[0];
                    nxt[5] = HYDK_GLOBAL(const uint32_t, vf)[0];
                    uint32_t gu = (uint32_t)HYDK_GLOBAL(const uint8_t, uf)[4] << 8, gv = (uint32_t)HYDK_GLOBAL(const uint8_t, vf)[4] << 8;
                    if (job.filter == HYDK_CHROMA_CENTRE) {
                        gu |= HYDK_GLOBAL(const uint8_t, uf - 1)[0];
                        gv |= HYDK_GLOBAL(const uint8_t, vf - 1)[0];
                    }
                    flank[0] = fu | gu << 16;
                    flank[1] = fv | gv << 16;
                } else {
                    nxt[3] = nxt[2];
                    nxt[5] = nxt[4];
                    flank[0] = fu | fu << 16;
                    flank[1] = fv | fv << 16;
                }
            }
            return;
        }
        if (YP16) {
            /* the words as stored: the depth shift waits until they are used (phase A), so that nothing here waits for a load */
            if (fast && s * 8 + ar < gh) {
                /* (the lane's row and block pass through an empty statement the compiler cannot see through, so the five addresses
                 * are made anew for every strip: carried from strip to strip as 64-bit pointers they cost the registers that left
                 * some builds of tests/kernel_variants.py with scratch) */
                int lane_row = ar, lane_block = ab;
                asm volatile("" : "+v"(lane_row), "+v"(lane_block));
                const long long y = py0 + s * 8 + lane_row, x = px0 + lane_block * 8;
                const long long ny = y >> csy, on = (ny * job.pixel_stride + (x >> csx)) * 2;
                const char *py = (const char *)job.src[0] + (y * job.row_stride + x) * 2;
                const char *un = (const char *)job.src[1] + on, *vn = (const char *)job.src[2] + on;
#pragma unroll
                for (int k = 0; k < 4; k++)
                    nxt[k] = HYDK_GLOBAL(const uint32_t, py)[k];
                if (!INTERP) {
                    /* U at nxt[4], V at nxt[8]: two dwords each, and two more for 4:4:4 */
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        nxt[4 + k] = HYDK_GLOBAL(const uint32_t, un)[k];
                        nxt[8 + k] = HYDK_GLOBAL(const uint32_t, vn)[k];
                    }
                    if (!csx) {
#pragma unroll
                        for (int k = 2; k < 4; k++) {
                            nxt[4 + k] = HYDK_GLOBAL(const uint32_t, un)[k];
                            nxt[8 + k] = HYDK_GLOBAL(const uint32_t, vn)[k];
                        }
                    }
                } else {
                    /* near and far dwords of U at nxt[4], nxt[6], of V at nxt[8], nxt[10]; 4:2:2 has no far row: it is filled in at use */
                    const bool centre = job.filter == HYDK_CHROMA_CENTRE; /* (left-sited chroma never looks before the window) */
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        nxt[4 + k] = HYDK_GLOBAL(const uint32_t, un)[k];
                        nxt[8 + k] = HYDK_GLOBAL(const uint32_t, vn)[k];
                    }
                    flank[0] = (uint32_t)HYDK_GLOBAL(const uint16_t, un)[4] << 16;
                    flank[2] = (uint32_t)HYDK_GLOBAL(const uint16_t, vn)[4] << 16;
                    if (centre) {
                        flank[0] |= HYDK_GLOBAL(const uint16_t, un - 2)[0];
                        flank[2] |= HYDK_GLOBAL(const uint16_t, vn - 2)[0];
                    }
                    if (csy) {
                        const long long of = (far_row(y) * job.pixel_stride + (x >> 1)) * 2;
                        const char *uf = (const char *)job.src[1] + of, *vf = (const char *)job.src[2] + of;
#pragma unroll
                        for (int k = 0; k < 2; k++) {
                            nxt[6 + k] = HYDK_GLOBAL(const uint32_t, uf)[k];
                            nxt[10 + k] = HYDK_GLOBAL(const uint32_t, vf)[k];
                        }
                        flank[1] = (uint32_t)HYDK_GLOBAL(const uint16_t, uf)[4] << 16;
                        flank[3] = (uint32_t)HYDK_GLOBAL(const uint16_t, vf)[4] << 16;
                        if (centre) {
                            flank[1] |= HYDK_GLOBAL(const uint16_t, uf - 2)[0];
                            flank[3] |= HYDK_GLOBAL(const uint16_t, vf - 2)[0];
                        }
                    }
                }
            }
            return;
        }
        if (HALF) {
            if (hfast && s * 8 + ar < gh) {
                const long long row = (long long)(py0 + s * 8 + ar) * job.row_stride;
                if (hrun == 1) {
                    const char *p = (const char *)job.src[0] + (row + (long long)(px0 + ab * 8) * 3) * 2;
#pragma unroll
                    for (int k = 0; k < 12; k++)
                        nxt[k] = HYDK_GLOBAL(const uint32_t, p)[k];
                } else {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const char *p = (const char *)job.src[c] + (row + (long long)(px0 + ab * 8)) * 2;
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            nxt[4 * c + k] = HYDK_GLOBAL(const uint32_t, p)[k];
                    }
                }
            }
            return;
        }
        if (fast && s * 8 + ar < gh) {
            const uint32_t *p = (const uint32_t *)((const char *)job.src[0] +
                                                   ((long long)(py0 + s * 8 + ar) * job.row_stride +
                                                    (long long)(px0 + ab * 8) * 3) * (long long)sizeof(sample_t));
#pragma unroll
            for (int k = 0; k < kWords; k++)
                nxt[k] = HYDK_GLOBAL(const uint32_t, p)[k];
        }
    };
    /* this workgroup's strips [s_first, s_end) and its share of the group's token array */
    const int s_per = (gbh + (1 << plog) - 1) >> plog;
    const int s_first = (int)part * s_per, s_end = min(gbh, s_first + s_per);
    const uint32_t tok_room = job.tok_cap >> plog;
    prefetch(s_first);

    void *const tok = (char *)job.tokens + (size_t)g * job.tok_cap * job.rec_bytes + (size_t)part * tok_room * (FMT == HYDK_FMT_F32 ? 8u : 4u);
    uint32_t goff = 0;
    uint32_t rb_sum = 0;     /* residue bits of the symbols this thread emitted */
    bool overflowed = false; /* the group outgrew its token array: stop storing, report, let the host rerun the frame */
    if (t == 0)
        s_rbits = 0;
    bool bad_sample = false;
    __syncthreads();

    for (int s = s_first; s < s_end; s++) {
        /* ---------------- phase A: 8 px of one block row -> XYB -> row DCT ---------------- */
        float xv[8], yv[8], bv[8]; /* (declared out here: HYDK_K1_CHANSEQ transforms them channel by channel further down) */
        if (ab < gbw) {
            const int y = py0 + s * 8 + ar; /* row inside the LF group */
            const int x0 = px0 + ab * 8;
            const bool row_ok = s * 8 + ar < gh;
            /* one float-class pixel, whatever its storage was: the non-finite check, then XYB */
            auto float_pixel = [&](float fr, float fg, float fb, float &X, float &Y, float &B) {
                if (job.bad_slot) {
                    /* per-slot outcomes: the slot is flagged and the sample coded as 0.0, so that what follows
                     * — bias curve, DCT, conversion, tokens — sees an ordinary picture and the slot's frame can
                     * neither fail nor rerun the launch group; a finite sample passes through bit for bit */
                    const bool ir = (__float_as_uint(fr) & 0x7f800000u) == 0x7f800000u;
                    const bool ig = (__float_as_uint(fg) & 0x7f800000u) == 0x7f800000u;
                    const bool ib = (__float_as_uint(fb) & 0x7f800000u) == 0x7f800000u;
                    bad_sample = bad_sample || ir || ig || ib;
                    fr = ir ? 0.0f : fr;
                    fg = ig ? 0.0f : fg;
                    fb = ib ? 0.0f : fb;
                }
                if (!lms_mix_f32(fr, fg, fb, job.linear_light, X, Y, B))
                    bad_sample = true;
            };
            if (UF) {
                /* A dword a pixel.  Rows that came as dwords a strip ago sit in nxt[0 ... 7]; the others — a ragged last block,
                 * rows that start on no 16-byte boundary — are read here, dword by dword, the pixels the row has: nothing outside
                 * the W dwords of a row is read.  Either way three fields come out of each dword and are widened to the float32
                 * bits they stand for (hydk_ufloat.h: integer operations only), and from there a pixel is a float32 pixel — the
                 * non-finite check, the slot's flag and the XYB mix are float_pixel's.  Edge padding is XYB = 0 (format.c:182-191). */
                const int nvalid = row_ok ? min(8, gw - ab * 8) : 0;
                if (!ufast) {
                    const char *pd = (const char *)job.src[0] + ((long long)y * job.row_stride + x0) * 4;
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        nxt[i] = i < nvalid ? HYDK_GLOBAL(const uint32_t, pd)[i] : 0u;
                }
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    xv[i] = yv[i] = bv[i] = 0.0f;
                    if (i < nvalid) {
                        uint32_t f[3];
                        hydk_ufloat_to_f32(STORE - HYDK_STORE_R11G11B10F, nxt[i], f);
                        float_pixel(__uint_as_float(f[0]), __uint_as_float(f[1]), __uint_as_float(f[2]), xv[i], yv[i], bv[i]);
                    }
                }
                prefetch(s + 1);
            } else if (HALF && hfast) {
                /* this strip's samples, fetched a strip ago: sample k of the row's 24 is half k & 1 of dword k >> 1 —
                 * k = 3 * pixel + channel in an interleaved run, 8 * channel + pixel in three planes' */
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    xv[i] = yv[i] = bv[i] = 0.0f;
                    if (row_ok) {
                        float f[3];
#pragma unroll
                        for (int ch = 0; ch < 3; ch++) {
                            const int ki = i * 3 + ch, kp = ch * 8 + i;
                            const uint32_t wi = nxt[ki >> 1] >> (16 * (ki & 1)), wp = nxt[kp >> 1] >> (16 * (kp & 1));
                            f[ch] = __uint_as_float(hydk_widen_half(STORE, (hrun == 1 ? wi : wp) & 0xFFFFu));
                        }
                        float_pixel(f[0], f[1], f[2], xv[i], yv[i], bv[i]);
                    }
                }
                prefetch(s + 1);
            } else if (fast || INTERP || PK16 || DW || QD) { /* (PK16, DW, QD: nearest rows that did not come as dwords fill the window too) */
                const int nvalid = row_ok ? min(8, gw - ab * 8) : 0;
                /* Interpolated rows that did not come as dwords — the picture's first and last chroma columns, a ragged last
                 * block, shifted bases, odd pitches — fill the same window sample by sample, here, every column clamped to the
                 * picture's chroma row and the far row to its chroma rows: the picture's chroma sample (0, 0) lies pic_cy0 rows
                 * and pic_cx0 columns before src[1] (and src[2]).  Window column p is the picture's clamp(pcx - 1 + p, 0, cw - 1),
                 * which is what cx, and hx with its clamp, come to for every pixel of the block.  The rest is shared with the
                 * dword rows. */
                if (INTERP && !TWO_PLANES && !PK && !fast) {
#pragma unroll
                    for (int k = 0; k < kWords; k++)
                        nxt[k] = 0;
#pragma unroll
                    for (int k = 0; k < kFlank; k++)
                        flank[k] = 0;
                    if (row_ok) {
                        const sample_t *py = (const sample_t *)job.src[0] + (long long)y * job.row_stride + x0;
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            if (i < nvalid)
                                nxt[i / kSPD] |= (uint32_t)py[i] << (SB * (i % kSPD));
                        /* column 0 of the picture's near and far chroma row, U and V */
                        const long long rows[2] = {y >> 1, far_row(y)};
                        const sample_t *col0[2][2];
#pragma unroll
                        for (int r = 0; r < 2; r++)
#pragma unroll
                            for (int c = 0; c < 2; c++)
                                col0[r][c] = (const sample_t *)job.src[1] + c + rows[r] * job.row_stride - 2ll * job.pic_cx0;
#pragma unroll
                        for (int p = 0; p < 6; p++) {
                            const int col = min(max(pcx - 1 + p, 0), job.pic_cw - 1);
#pragma unroll
                            for (int r = 0; r < 2; r++)
#pragma unroll
                                for (int c = 0; c < 2; c++)
                                    win_put(c, r, p, col0[r][c][2 * col]);
                        }
                    }
                }
                /* YUVPI rows that did not come as dwords: each plane's window of six samples filled byte by byte, the same clamps,
                 * into the registers the dword rows use.  The picture's sample (0, 0) lies pic_cy0 rows and pic_cx0 bytes before
                 * src[1] and src[2] */
                if (YUVPI && !fast) {
#pragma unroll
                    for (int k = 0; k < kWords; k++)
                        nxt[k] = 0;
                    flank[0] = flank[1] = 0;
                    if (row_ok) {
                        const uint8_t *py = (const uint8_t *)job.src[0] + (long long)y * job.row_stride + x0;
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            if (i < nvalid)
                                nxt[i >> 2] |= (uint32_t)py[i] << (8 * (i & 3));
                        const long long ny = y >> csy;
                        const long long fy = csy ? (long long)hydk_chroma_vy(2 * job.pic_cy0 + y, job.pic_ch) - job.pic_cy0 : ny;
                        const long long on = ny * job.pixel_stride - job.pic_cx0, of = fy * job.pixel_stride - job.pic_cx0;
                        const uint8_t *un = (const uint8_t *)job.src[1] + on, *uf = (const uint8_t *)job.src[1] + of;
                        const uint8_t *vn = (const uint8_t *)job.src[2] + on, *vf = (const uint8_t *)job.src[2] + of;
#pragma unroll
                        for (int p = 0; p < 6; p++) {
                            const int col = min(max(pcx - 1 + p, 0), job.pic_cw - 1);
                            const uint32_t a = un[col], b = uf[col], c = vn[col], d = vf[col];
                            if (p == 0 || p == 5) {
                                flank[0] |= (a | b << 16) << (p ? 8 : 0);
                                flank[1] |= (c | d << 16) << (p ? 8 : 0);
                            } else {
                                nxt[2] |= a << (8 * (p - 1));
                                nxt[3] |= b << (8 * (p - 1));
                                nxt[4] |= c << (8 * (p - 1));
                                nxt[5] |= d << (8 * (p - 1));
                            }
                        }
                    }
                }
                /* Packed 4:2:2.  Dword rows: the four groups become YUVP's window — eight Y bytes in nxt[0], nxt[1], four U bytes and
                 * four V bytes — by byte permutes whose selectors are the byte order's (uniform over the wavefront): out of a pair of
                 * groups {lo, hi}, bytes 0, 2, 4, 6 are the Y samples of YUYV and the chroma of UYVY, bytes 1, 3, 5, 7 the other; then
                 * the same split tells the first chroma component from the second.  Interpolated: YUVPI's window — U near and far in
                 * nxt[2], nxt[3], V in nxt[4], nxt[5], far = near as 4:2:2 has it there, columns 0 and 5 in flank[] — so that the mix
                 * below is YUVPI's.  Rows that did not come as dwords (a base or pitch off the dword, the picture's first and last
                 * chroma column, a ragged last block) fill the same window byte by byte with the clamps: group col of the picture's
                 * row lies 4 (col - pic_cx0) bytes from src[1] and src[2]. */
                if (PK8 && fast) {
                    const uint32_t even = 0x06040200u, odd = 0x07050301u;
                    const uint32_t sel_y = pk_y ? odd : even, sel_c = pk_y ? even : odd;
                    const uint32_t ca = __builtin_amdgcn_perm(nxt[1], nxt[0], sel_c), cb = __builtin_amdgcn_perm(nxt[3], nxt[2], sel_c);
                    const uint32_t y0 = __builtin_amdgcn_perm(nxt[1], nxt[0], sel_y), y1 = __builtin_amdgcn_perm(nxt[3], nxt[2], sel_y);
                    const uint32_t c0 = __builtin_amdgcn_perm(cb, ca, even), c1 = __builtin_amdgcn_perm(cb, ca, odd);
                    const uint32_t u4 = pk_vu ? c1 : c0, v4 = pk_vu ? c0 : c1;
                    nxt[0] = y0;
                    nxt[1] = y1;
                    if (!INTERP) {
                        nxt[2] = u4;
                        nxt[3] = v4;
                    } else {
                        /* (c0, c1) of the groups before and behind: bytes 0, 1 before, 2, 3 behind */
                        const uint32_t cf = __builtin_amdgcn_perm(flank[1], flank[0], sel_c);
                        const uint32_t f0 = (cf & 0xFFu) | ((cf >> 8) & 0xFF00u), f1 = ((cf >> 8) & 0xFFu) | ((cf >> 16) & 0xFF00u);
                        const uint32_t fu = pk_vu ? f1 : f0, fv = pk_vu ? f0 : f1;
                        nxt[2] = nxt[3] = u4;
                        nxt[4] = nxt[5] = v4;
                        flank[0] = fu | fu << 16;
                        flank[1] = fv | fv << 16;
                    }
                }
                if (PK8 && INTERP && !fast) {
#pragma unroll
                    for (int k = 0; k < kWords; k++)
                        nxt[k] = 0;
                    flank[0] = flank[1] = 0;
                    if (row_ok) {
                        const uint8_t *py = (const uint8_t *)job.src[0] + (long long)y * job.row_stride + 2ll * x0;
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            if (i < nvalid)
                                nxt[i >> 2] |= (uint32_t)py[2 * i] << (8 * (i & 3));
                        const long long on = (long long)y * job.row_stride - 4ll * job.pic_cx0;
                        const uint8_t *un = (const uint8_t *)job.src[1] + on, *vn = (const uint8_t *)job.src[2] + on;
#pragma unroll
                        for (int p = 0; p < 6; p++) {
                            const int col = min(max(pcx - 1 + p, 0), job.pic_cw - 1);
                            const uint32_t a = un[4 * col], c = vn[4 * col];
                            if (p == 0 || p == 5) {
                                flank[0] |= (a | a << 16) << (p ? 8 : 0);
                                flank[1] |= (c | c << 16) << (p ? 8 : 0);
                            } else {
                                nxt[2] |= a << (8 * (p - 1));
                                nxt[4] |= c << (8 * (p - 1));
                            }
                        }
                        nxt[3] = nxt[2];
                        nxt[5] = nxt[4];
                    }
                }
                /* Packed 4:2:2 of 16-bit words.  Dword rows: the four groups become YP16's 4:2:2 window — eight Y words in nxt[0 ... 3],
                 * four U words in nxt[4], nxt[5], four V words in nxt[8], nxt[9] — by 16-bit permutes whose selectors are the word
                 * order's (uniform over the wavefront): of a group's two dwords the low halves are the Y samples of Y210's own order
                 * and the chroma of the orders with Y second, the high halves the other; then the same split tells the first chroma
                 * component from the second.  Interpolated: columns 0 and 5 (the groups before and behind) go to flank[] as YP16I has
                 * them, column 0 | column 5 << 16 of U in flank[0], of V in flank[2].  Rows that did not come as dwords (a first
                 * group or pitch off the dword, the picture's first and last chroma column, a ragged last block) fill the same
                 * window word by word with the clamps: group col of the picture's row lies 4 (col - pic_cx0) words from src[1] and
                 * src[2].  Nearest rows take that way too (the per-sample loop at the end is never theirs: with it the nearest
                 * instances needed a 129th register).  Either way the far row is the near row, as 4:2:2 has it, and the words count as stored: no shift. */
                if (PK16 && fast) {
                    const uint32_t low = 0x05040100u, high = 0x07060302u;
                    const uint32_t sel_y = pk_y ? high : low, sel_c = pk_y ? low : high;
                    const uint32_t sel_u = pk_vu ? high : low, sel_v = pk_vu ? low : high;
                    uint32_t yd[4], cd[4]; /* per group: its two Y words; its first | second << 16 chroma word */
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        yd[k] = __builtin_amdgcn_perm(nxt[2 * k + 1], nxt[2 * k], sel_y);
                        cd[k] = __builtin_amdgcn_perm(nxt[2 * k + 1], nxt[2 * k], sel_c);
                    }
                    if (INTERP) {
                        constexpr int kB = PK16 ? 8 : 0; /* (PK16 has twelve dwords; an index every other form can hold, for its compile) */
                        const uint32_t behind = __builtin_amdgcn_perm(nxt[kB + 1], nxt[kB], sel_c), before = __builtin_amdgcn_perm(nxt[kB + 3], nxt[kB + 2], sel_c);
                        flank[0] = __builtin_amdgcn_perm(behind, before, sel_u);
                        flank[2] = __builtin_amdgcn_perm(behind, before, sel_v);
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        nxt[k] = yd[k];
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        nxt[4 + k] = __builtin_amdgcn_perm(cd[2 * k + 1], cd[2 * k], sel_u);
                        nxt[8 + k] = __builtin_amdgcn_perm(cd[2 * k + 1], cd[2 * k], sel_v);
                    }
                }
                if (PK16 && !fast) {
#pragma unroll
                    for (int k = 0; k < kWords; k++)
                        nxt[k] = 0;
#pragma unroll
                    for (int k = 0; k < kFlank; k++)
                        flank[k] = 0;
                    if (row_ok) {
                        const uint16_t *py = (const uint16_t *)job.src[0] + (long long)y * job.row_stride + 2ll * x0;
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            if (i < nvalid)
                                nxt[i >> 1] |= (uint32_t)py[2 * i] << (16 * (i & 1));
                        const long long on = (long long)y * job.row_stride;
                        const uint16_t *un = (const uint16_t *)job.src[1] + on, *vn = (const uint16_t *)job.src[2] + on;
#pragma unroll
                        for (int p = 0; p < 6; p++) {
                            /* nearest: a pixel's own group, columns 1 ... 4 as far as the row has pixels; the job carries no picture */
                            if (!INTERP && (p == 0 || p == 5 || 2 * (p - 1) >= nvalid))
                                continue;
                            const int col = INTERP ? min(max(pcx - 1 + p, 0), job.pic_cw - 1) - job.pic_cx0 : (x0 >> 1) + p - 1;
                            const uint32_t a = un[4 * col], c = vn[4 * col];
                            if (p == 0 || p == 5) {
                                flank[0] |= a << (p ? 16 : 0);
                                flank[2] |= c << (p ? 16 : 0);
                            } else {
                                nxt[4 + ((p - 1) >> 1)] |= a << (16 * ((p - 1) & 1));
                                nxt[8 + ((p - 1) >> 1)] |= c << (16 * ((p - 1) & 1));
                            }
                        }
                    }
                }
                if (PK16 && INTERP) {
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        nxt[6 + k] = nxt[4 + k];
                        nxt[10 + k] = nxt[8 + k];
                        flank[1 + 2 * k] = flank[2 * k];
                    }
                }
                /* A dword a pixel.  Rows that did not come as dwords — a ragged last block, and rows past the picture's last — fill
                 * nxt[0 ... 7] pixel by pixel with the pixels the row has, and zero elsewhere: nothing outside the W dwords of a row
                 * is read.  Either way three 10-bit fields come out of each dword (v_bfe_u32) and become an interleaved RGB16 row as
                 * hydk_rgb10.h defines it: the RGB orders widen each field, the low and the high one changing places by job.sub
                 * (uniform over the wavefront); Y410 shifts by 6 and takes the shared 16-bit conversion.  The per-sample loop at the
                 * end is never theirs. */
                if (DW && !fast) {
#pragma unroll
                    for (int k = 0; k < kWords; k++)
                        nxt[k] = 0;
                    if (row_ok) {
                        const uint32_t *pd = (const uint32_t *)job.src[0] + (long long)y * job.row_stride + x0;
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            if (i < nvalid)
                                nxt[i] = pd[i];
                    }
                }
                /* A group of four a pixel.  Rows that did not come as dwords — a ragged last block, and rows past the picture's last —
                 * fill nxt pixel by pixel, a dword or a qword each, with the pixels the row has, and zero elsewhere: nothing outside
                 * the W pixels of a row is read.  Either way Y, U and V come out of each pixel as hydk_quad.h defines it — three
                 * bytes of a dword under the 8-bit conversion, three words of two dwords under the 16-bit one — and become an
                 * interleaved RGB row of the class; the fourth sample is in the registers and in no expression. */
                if (QD && !fast) {
#pragma unroll
                    for (int k = 0; k < kWin; k++)
                        nxt[k] = 0;
                    if (row_ok) {
                        constexpr int kDPP = kWin / 8; /* dwords a pixel */
                        const uint32_t *pq = (const uint32_t *)job.src[0] + ((long long)y * job.row_stride + x0) * kDPP;
#pragma unroll
                        for (int k = 0; k < kWin; k++)
                            if (k / kDPP < nvalid)
                                nxt[k] = pq[k];
                    }
                }
                /* YP16 rows that did not come as dwords: each plane's window of six words filled word by word, the same clamps, into
                 * the registers the dword rows use, as stored */
                if (YP16 && INTERP && !fast) {
#pragma unroll
                    for (int k = 0; k < kWords; k++)
                        nxt[k] = 0;
#pragma unroll
                    for (int k = 0; k < kFlank; k++)
                        flank[k] = 0;
                    if (row_ok) {
                        const uint16_t *py = (const uint16_t *)job.src[0] + (long long)y * job.row_stride + x0;
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            if (i < nvalid)
                                nxt[i >> 1] |= (uint32_t)py[i] << (16 * (i & 1));
                        const long long ny = y >> csy, fy = csy ? far_row(y) : ny;
                        const long long on = ny * job.pixel_stride - job.pic_cx0, of = fy * job.pixel_stride - job.pic_cx0;
                        const uint16_t *un = (const uint16_t *)job.src[1] + on, *uf = (const uint16_t *)job.src[1] + of;
                        const uint16_t *vn = (const uint16_t *)job.src[2] + on, *vf = (const uint16_t *)job.src[2] + of;
#pragma unroll
                        for (int p = 0; p < 6; p++) {
                            const int col = min(max(pcx - 1 + p, 0), job.pic_cw - 1);
                            const uint32_t four[4] = {un[col], uf[col], vn[col], vf[col]};
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                if (p == 0 || p == 5)
                                    flank[q] |= four[q] << (p ? 16 : 0);
                                else
                                    nxt[4 + 2 * q + ((p - 1) >> 1)] |= four[q] << (16 * ((p - 1) & 1));
                            }
                        }
                    }
                }
                /* YP16, dword rows and filled rows alike: the stored words become samples before any tap sees them (hydk_yuvp16.h);
                 * the depth is the job's, so the shift is uniform over the wavefront.  4:2:2: the far row is the near row */
                if (YP16) {
                    const int shift = hydk_yuvp16_shift((int)(job.matrix >> 2));
                    if (INTERP && !csy) {
#pragma unroll
                        for (int k = 0; k < 2; k++) {
                            nxt[6 + k] = nxt[4 + k];
                            nxt[10 + k] = nxt[8 + k];
                            flank[1 + 2 * k] = flank[2 * k];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < kWords; k++)
                        nxt[k] = hydk_yuvp16_sample2(shift, nxt[k]);
#pragma unroll
                    for (int k = 0; k < kFlank; k++)
                        flank[k] = hydk_yuvp16_sample2(shift, flank[k]);
                }
                /* YCbCr: the eight pixels of the window, converted and packed as an interleaved RGB row of the class has them */
                uint32_t cvt[kWords];
                if (YUV || DW) {
#pragma unroll
                    for (int k = 0; k < kWords; k++)
                        cvt[k] = 0;
                    auto convert = [&](int i, uint32_t u, uint32_t v) {
                        const uint32_t luma = (nxt[i / kSPD] >> (SB * (i % kSPD))) & kSMask;
                        uint32_t rgb[3];
                        if (SB == 8)
                            hydk_yuv_to_rgb(yuv, luma, u, v, rgb);
                        else
                            hydk_yuv16_to_rgb(yuv, luma, u, v, rgb);
#pragma unroll
                        for (int ch = 0; ch < 3; ch++) {
                            const int si = i * 3 + ch;
                            cvt[si / kSPD] |= rgb[ch] << (SB * (si % kSPD));
                        }
                    };
                    if (QD) {
                        /* pixel i is dword i, or dwords 2 i and 2 i + 1: packed as convert packs */
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            uint32_t rgb[3];
                            if (SB == 8)
                                hydk_ayuv_to_rgb(yuv, nxt[i < kWin ? i : 0], rgb);
                            else
                                hydk_y416_to_rgb(yuv, nxt[2 * i < kWin ? 2 * i : 0], nxt[2 * i + 1 < kWin ? 2 * i + 1 : 0], rgb);
#pragma unroll
                            for (int ch = 0; ch < 3; ch++) {
                                const int si = i * 3 + ch;
                                cvt[si / kSPD] |= rgb[ch] << (SB * (si % kSPD));
                            }
                        }
                    } else if (DW) {
                        /* pixel i is dword i: its three fields to an RGB16 pixel, packed as convert packs */
                        const int order = (int)job.sub;
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            uint32_t rgb[3];
                            if (YUV)
                                hydk_y410_to_rgb(yuv, nxt[i < kWords ? i : 0], rgb);
                            else
                                hydk_rgb10_to_rgb(order, nxt[i < kWords ? i : 0], rgb);
#pragma unroll
                            for (int ch = 0; ch < 3; ch++) {
                                const int si = i * 3 + ch;
                                cvt[si / kSPD] |= rgb[ch] << (SB * (si % kSPD));
                            }
                        }
                    } else if ((YP16 || PK16) && INTERP) {
                        /* the same two mixes, the window's words taken plane by plane */
                        uint32_t vu[6], vv[6];
#pragma unroll
                        for (int p = 0; p < 6; p++) {
                            const int k = (p - 1) >> 1, sh = 16 * ((p - 1) & 1);
                            const uint32_t a = p == 0 ? flank[0] : p == 5 ? flank[0] >> 16 : nxt[4 + k] >> sh;
                            const uint32_t b = p == 0 ? flank[1] : p == 5 ? flank[1] >> 16 : nxt[6 + k] >> sh;
                            const uint32_t c = p == 0 ? flank[2] : p == 5 ? flank[2] >> 16 : nxt[8 + k] >> sh;
                            const uint32_t d = p == 0 ? flank[3] : p == 5 ? flank[3] >> 16 : nxt[10 + k] >> sh;
                            vu[p] = hydk_chroma_vmix(a & 0xFFFF, b & 0xFFFF);
                            vv[p] = hydk_chroma_vmix(c & 0xFFFF, d & 0xFFFF);
                        }
                        const int filter = (int)job.filter;
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            const int j = 1 + (i >> 1), hc = (i & 1) ? j + 1 : j - 1, hl = j + (i & 1);
                            convert(i, hydk_chroma_hmix(filter, i & 1, vu[j], filter == HYDK_CHROMA_CENTRE ? vu[hc] : vu[hl]),
                                    hydk_chroma_hmix(filter, i & 1, vv[j], filter == HYDK_CHROMA_CENTRE ? vv[hc] : vv[hl]));
                        }
                    } else if (YUVPI || (PK8 && INTERP)) {
                        /* NV12I's vertical mix, horizontal mix, conversion and pack, the window's samples taken plane by plane */
                        uint32_t vu[6], vv[6];
#pragma unroll
                        for (int p = 0; p < 6; p++) {
                            const int sh = 8 * (p - 1);
                            const uint32_t a = p == 0 ? flank[0] : p == 5 ? flank[0] >> 8 : nxt[2] >> sh;
                            const uint32_t b = p == 0 ? flank[0] >> 16 : p == 5 ? flank[0] >> 24 : nxt[3] >> sh;
                            const uint32_t c = p == 0 ? flank[1] : p == 5 ? flank[1] >> 8 : nxt[4] >> sh;
                            const uint32_t d = p == 0 ? flank[1] >> 16 : p == 5 ? flank[1] >> 24 : nxt[5] >> sh;
                            vu[p] = hydk_chroma_vmix(a & 0xFF, b & 0xFF);
                            vv[p] = hydk_chroma_vmix(c & 0xFF, d & 0xFF);
                        }
                        const int filter = (int)job.filter;
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            const int j = 1 + (i >> 1), hc = (i & 1) ? j + 1 : j - 1, hl = j + (i & 1);
                            const uint32_t u = hydk_chroma_hmix(filter, i & 1, vu[j], filter == HYDK_CHROMA_CENTRE ? vu[hc] : vu[hl]);
                            const uint32_t v = hydk_chroma_hmix(filter, i & 1, vv[j], filter == HYDK_CHROMA_CENTRE ? vv[hc] : vv[hl]);
                            uint32_t rgb[3];
                            hydk_yuv_to_rgb(yuv, (nxt[i >> 2] >> (8 * (i & 3))) & 0xFF, u, v, rgb);
#pragma unroll
                            for (int ch = 0; ch < 3; ch++) {
                                const int si = i * 3 + ch;
                                cvt[si >> 2] |= rgb[ch] << (8 * (si & 3));
                            }
                        }
                    } else if (INTERP) {
                        /* the vertical mix of the window's six columns, then per pixel the horizontal mix with the neighbour its
                         * filter names, the conversion, the pack */
                        uint32_t vu[6], vv[6];
#pragma unroll
                        for (int p = 0; p < 6; p++) {
                            vu[p] = hydk_chroma_vmix(win_get(0, 0, p), win_get(0, 1, p));
                            vv[p] = hydk_chroma_vmix(win_get(1, 0, p), win_get(1, 1, p));
                        }
                        const int filter = (int)job.filter;
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            const int j = 1 + (i >> 1), hc = (i & 1) ? j + 1 : j - 1, hl = j + (i & 1);
                            convert(i, hydk_chroma_hmix(filter, i & 1, vu[j], filter == HYDK_CHROMA_CENTRE ? vu[hc] : vu[hl]),
                                    hydk_chroma_hmix(filter, i & 1, vv[j], filter == HYDK_CHROMA_CENTRE ? vv[hc] : vv[hl]));
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            convert(i, near_get(0, i), near_get(1, i));
                    }
                }
                uint32_t(&w)[kWords] = YUV || DW ? cvt : reinterpret_cast<uint32_t(&)[kWords]>(nxt); /* this strip's pixels, fetched a strip ago (QD's wider window is never w) */
                /* which form of the transfer curve this wavefront's 16-bit samples need (wave-uniform) */
                int curve = kCurveBoth;
                if (FMT == HYDK_FMT_U16 && !LUTS) {
                    if (job.linear_light)
                        curve = kCurveNone;
                    else {
                        typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
                        u16x2 mn = __builtin_bit_cast(u16x2, w[0]);
#pragma unroll
                        for (int k = 1; k < kWords; k++)
                            mn = __builtin_elementwise_min(mn, __builtin_bit_cast(u16x2, w[k]));
                        const bool dark = row_ok && (uint32_t)(mn.x < mn.y ? mn.x : mn.y) <= kDarkMax;
                        curve = __builtin_amdgcn_ballot_w64(dark) ? kCurveBoth : kCurveCubic;
                    }
                }
                auto row_to_xyb = [&](auto curve_tag) {
                    constexpr int CURVE = decltype(curve_tag)::value;
#if HYDK_K1_ILP
                    if (FMT != HYDK_FMT_F32 && !LUTS) {
                        constexpr int P = HYDK_K1_ILP; /* pixels evaluated in lock step */
#pragma unroll
                        for (int i0 = 0; i0 < 8; i0 += P) {
                            uint32_t smp[3 * P], lin[3 * P], idx[3 * P];
                            float bia[3 * P];
                            if (FMT == HYDK_FMT_U8) { /* 8-bit samples: the 256-entry transfer table sits in LDS */
#pragma unroll
                                for (int k = 0; k < 3 * P; k++) {
                                    const int si = i0 * 3 + k;
                                    lin[k] = lut8((w[si >> 2] >> (8 * (si & 3))) & 0xFF);
                                }
                            } else {
#pragma unroll
                                for (int k = 0; k < 3 * P; k++) {
                                    const int si = i0 * 3 + k;
                                    smp[k] = (w[si >> 1] >> (16 * (si & 1))) & 0xFFFF;
                                }
                                input_lut16_eval_n<CURVE, 3 * P>(smp, lin);
                            }
#pragma unroll
                            for (int q = 0; q < P; q++) { /* format.c:48-56 */
                                const uint32_t r = lin[3 * q], g = lin[3 * q + 1], b = lin[3 * q + 2];
                                const uint32_t bb = __umul24(5112u, b);
                                idx[3 * q] = umad24(19661u, r, umad24(40761u, g, bb)) >> 16;
                                idx[3 * q + 1] = umad24(15073u, r, umad24(45350u, g, bb)) >> 16;
                                idx[3 * q + 2] = umad24(15953u, r, umad24(13419u, g, __umul24(36163u, b))) >> 16;
                            }
                            /* which of the 3 * P bias values come from the uploaded table through the (otherwise idle)
                             * texture path: HYDK_K1_GATHER bits 3-5 */
                            constexpr auto gathered = [](int k) constexpr { return ((xyb_gmask(XMODE) >> 3) >> (k % 3) & 1) != 0; };
                            constexpr int NG = [&]() constexpr { int n = 0; for (int k = 0; k < 3 * P; k++) n += gathered(k); return n; }();
                            if (NG == 0)
                                bias_lut_eval_n<XMODE, 3 * P>(idx, bia);
                            else {
                                const auto *gl = HYDK_GLOBAL(const float, job.bias_lut);
                                constexpr int NE = 3 * P - NG > 0 ? 3 * P - NG : 1;
                                uint32_t eidx[NE];
                                float eb[NE];
                                int n = 0;
#pragma unroll
                                for (int k = 0; k < 3 * P; k++) {
                                    if (gathered(k))
                                        bia[k] = gl[idx[k]]; /* issued first: they travel while the others are evaluated */
                                    else
                                        eidx[n++] = idx[k];
                                }
                                if (NG < 3 * P)
                                    bias_lut_eval_n<XMODE, NE>(eidx, eb);
                                n = 0;
#pragma unroll
                                for (int k = 0; k < 3 * P; k++)
                                    if (!gathered(k))
                                        bia[k] = eb[n++];
                            }
#pragma unroll
                            for (int q = 0; q < P; q++) {
                                const float Y = (bia[3 * q] + bia[3 * q + 1]) * 0.5f;
                                yv[i0 + q] = Y;
                                xv[i0 + q] = Y - bia[3 * q + 1];
                                bv[i0 + q] = bia[3 * q + 2] - Y;
                            }
                        }
                        return;
                    }
#endif
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        uint32_t rgb[3];
#pragma unroll
                        for (int ch = 0; ch < 3; ch++) {
                            const int si = i * 3 + ch;
                            if (FMT == HYDK_FMT_U8)
                                rgb[ch] = lut8((w[si >> 2] >> (8 * (si & 3))) & 0xFF);
                            else {
                                const uint32_t v = (w[si >> 1] >> (16 * (si & 1))) & 0xFFFF;
                                rgb[ch] = LUTS ? (uint32_t)job.in_lut16[v] : (xyb_gmask(XMODE) >> ch & 1) ? (uint32_t)HYDK_GLOBAL(const uint16_t, job.in_lut16)[v] : input_lut16_eval_as<CURVE>(v);
                            }
                        }
                        if (HYDK_K1_SKIP & 2) { /* timing only: no transfer or bias curves */
                            xv[i] = __uint_as_float(0x3f000000u | w[(i * 3) >> 1]);
                            yv[i] = __uint_as_float(0x3f000000u | w[(i * 3 + 1) >> 1]);
                            bv[i] = __uint_as_float(0x3f000000u | w[(i * 3 + 2) >> 1]);
                            continue;
                        }
                        lms_mix_u16<XMODE>(rgb[0], rgb[1], rgb[2], job.bias_lut, xv[i], yv[i], bv[i]);
                    }
                };
                if (row_ok) {
                    if (curve == kCurveCubic)
                        row_to_xyb(std::integral_constant<int, kCurveCubic>());
                    else if (curve == kCurveNone)
                        row_to_xyb(std::integral_constant<int, kCurveNone>());
                    else
                        row_to_xyb(std::integral_constant<int, kCurveBoth>());
                    if (INTERP || PK16 || DW || QD) { /* (a ragged last block: edge padding is XYB = 0, format.c:182-191) */
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            if (i >= nvalid)
                                xv[i] = yv[i] = bv[i] = 0.0f;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        xv[i] = yv[i] = bv[i] = 0.0f;
                }
                /* the next strip's pixels travel during the transforms and the token phase; issued only now, they
                 * take the registers this strip's pixels have just left */
                prefetch(s + 1);
            } else {
                const int nvalid = row_ok ? min(8, gw - ab * 8) : 0;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    xv[i] = yv[i] = bv[i] = 0.0f; /* edge padding is XYB = 0 (format.c:182-191) */
                    if (i < nvalid) {
                        /* (packed 4:2:2: a Y every 2 samples — the pixel stride — and a U and a V every 4, all in row y of the one plane) */
                        const long long off = (long long)y * job.row_stride + (long long)(x0 + i) * (TWO_PLANES ? 1ll : job.pixel_stride);
                        /* (pairs in one plane: the pixel's Y; its U and V sit in chroma row y >> 1 at the even sample x & ~1 and
                         * behind it.  Two planes: in row y >> sy, byte x >> sx of their own planes, whose pitch the pixel stride carries) */
                        const long long offc = TWO_PLANES ? (long long)(y >> csy) * job.pixel_stride + (long long)((x0 + i) >> csx)
                                               : PK       ? (long long)y * job.row_stride + 4ll * ((x0 + i) >> 1)
                                               : YUV      ? (long long)(y >> 1) * job.row_stride + (long long)((x0 + i) & ~1)
                                                          : off;
                        sample_t sr = ((const sample_t *)job.src[0])[off];
                        sample_t sg = ((const sample_t *)job.src[1])[offc];
                        sample_t sb = ((const sample_t *)job.src[2])[offc];
                        if (YP16) { /* the stored words become samples (hydk_yuvp16.h) */
                            const int shift = hydk_yuvp16_shift((int)(job.matrix >> 2));
                            sr = (sample_t)hydk_yuvp16_sample(shift, (uint32_t)sr);
                            sg = (sample_t)hydk_yuvp16_sample(shift, (uint32_t)sg);
                            sb = (sample_t)hydk_yuvp16_sample(shift, (uint32_t)sb);
                        }
                        if (FMT == HYDK_FMT_F32) {
                            float fr, fg, fb;
                            if (HALF) {
                                fr = __uint_as_float(hydk_widen_half(STORE, (uint32_t)sr));
                                fg = __uint_as_float(hydk_widen_half(STORE, (uint32_t)sg));
                                fb = __uint_as_float(hydk_widen_half(STORE, (uint32_t)sb));
                            } else {
                                fr = (float)sr, fg = (float)sg, fb = (float)sb;
                            }
                            float_pixel(fr, fg, fb, xv[i], yv[i], bv[i]);
                        } else {
                            uint32_t rgb[3] = {(uint32_t)sr, (uint32_t)sg, (uint32_t)sb};
                            if (YUV && SB == 8)
                                hydk_yuv_to_rgb(yuv, (uint32_t)sr, (uint32_t)sg, (uint32_t)sb, rgb);
                            if (YUV && SB == 16)
                                hydk_yuv16_to_rgb(yuv, (uint32_t)sr, (uint32_t)sg, (uint32_t)sb, rgb);
#pragma unroll
                            for (int ch = 0; ch < 3; ch++) {
                                if (FMT == HYDK_FMT_U8)
                                    rgb[ch] = lut8(rgb[ch]);
                                else
                                    rgb[ch] = LUTS ? job.in_lut16[rgb[ch]] : input_lut16_eval(rgb[ch], job.linear_light);
                            }
                            lms_mix_u16<XMODE>(rgb[0], rgb[1], rgb[2], job.bias_lut, xv[i], yv[i], bv[i]);
                        }
                    }
                }
            }
            if (job.dbg_xyb) {
                float *d = job.dbg_xyb + (size_t)y * kDbgPitch + x0;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    d[i] = xv[i];
                    d[(size_t)kDbgPitch * kDbgPitch + i] = yv[i];
                    d[(size_t)2 * kDbgPitch * kDbgPitch + i] = bv[i];
                }
            }
#if !HYDK_K1_CHANSEQ
            float o[8];
            float *dst = s_rowpass + ab * kS0Block + ar * 8;
            dct8(xv, o);
#pragma unroll
            for (int k = 0; k < 8; k++)
                dst[k] = o[k];
            dct8(yv, o);
#pragma unroll
            for (int k = 0; k < 8; k++)
                dst[kS0Chan + k] = o[k];
            dct8(bv, o);
#pragma unroll
            for (int k = 0; k < 8; k++)
                dst[2 * kS0Chan + k] = o[k];
#endif
        }
        /* LDS operations of one wavefront execute in order: its own stores are visible to its loads */
#define HYDK_K1_WAVE_SYNC()                                                                                      \
    do {                                                                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                   \
        __builtin_amdgcn_wave_barrier();                                                                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");                                                   \
    } while (0)
#if HYDK_K1_CHANSEQ
        /* (the row passes come channel by channel, inside phase B) */
#elif HYDK_K1_WAVELOCAL
        HYDK_K1_WAVE_SYNC();
#else
        __syncthreads();
#endif

        /* ---------------- phase B: column DCT, quantise (in place in LDS), LF ints, non-zero bitmaps ---------------- */
        unsigned long long msk[3] = {0, 0, 0}; /* per channel X, Y, B: non-zero coefficients by zig-zag position */
        int32_t lf_int[3] = {0, 0, 0};
        auto column_pass = [&](const int c) __attribute__((always_inline)) {
                float col[8], v[8];
                float *src = s_rowpass + (HYDK_K1_CHANSEQ ? 0 : c * kS0Chan) + cb * kS0Block + kh;
#pragma unroll
                for (int n = 0; n < 8; n++)
                    col[n] = src[n * 8];
                dct8(col, v);
                /* v[kv] = coefficient with vertical frequency kv, horizontal frequency kh; the
                 * reference leaves it at block row kh, column kv (encoder.c:660-664) */
                if (job.dbg_dct) {
                    float *d = job.dbg_dct + (size_t)c * kDbgPitch * kDbgPitch +
                               (size_t)(py0 + s * 8 + kh) * kDbgPitch + px0 + cb * 8;
#pragma unroll
                    for (int kv = 0; kv < 8; kv++)
                        d[kv] = v[kv];
                }
                uint32_t nlo = 0, nhi = 0; /* byte offsets into this kh's nibble-mask rows: bit 3 + b set if coefficient (4 * half + b, kh) is non-zero */
                int q[8];
                const float4 w03 = *(const float4 *)&s_wq[c * 64 + kh * 8], w47 = *(const float4 *)&s_wq[c * 64 + kh * 8 + 4];
                const float wq[8] = {w03.x, w03.y, w03.z, w03.w, w47.x, w47.y, w47.z, w47.w};
#pragma unroll
                for (int kv = 0; kv < 8; kv++) {
                    /* encoder.c:808-811: trunc((coef * weight) * 5); +-1 is the dead zone */
                    const float scaled = v[kv] * wq[kv] * 5.0f;
                    int qq = trunc_as_reference<FMT>(scaled);
                    /* |trunc(x)| >= 2 exactly when |x| >= 2 (NaN: neither, and converts to 0; float input: NaN converts
                     * to INT_MIN as the reference's does, and is kept) */
                    const bool nz = (FMT == HYDK_FMT_F32 ? !(__builtin_fabsf(scaled) < 2.0f) : __builtin_fabsf(scaled) >= 2.0f) &&
                                    !(kv == 0 && kh == 0); /* the DC slot is coded by the LF path */
                    qq = nz ? qq : 0;
                    q[kv] = qq;
                    if (kv < 4)
                        nlo |= nz ? 8u << kv : 0u;
                    else
                        nhi |= nz ? 8u << (kv - 4) : 0u;
#if !HYDK_K1_CHANSEQ
                    /* the thread's own column: nobody else reads or writes these eight words */
                    ((int *)src)[kv * 8] = qq;
#endif
                }
#if HYDK_K1_CHANSEQ
                {   /* the thread's eight coefficients [kh][kv = 0..7] in one piece: the wavefront's 64 stores are 1 KiB in a row */
                    coef_t *const dq = s_q + (c * 32 + cb) * kQBlock + kh * 8;
                    if (FMT == HYDK_FMT_F32) {
                        *(int4 *)dq = int4{q[0], q[1], q[2], q[3]};
                        *(int4 *)(dq + 4) = int4{q[4], q[5], q[6], q[7]};
                    } else {
                        const uint32_t k0 = 0x05040100u; /* v_perm_b32: {low half of source 1, low half of source 0} */
                        *(uint4 *)dq = uint4{__builtin_amdgcn_perm((uint32_t)q[1], (uint32_t)q[0], k0), __builtin_amdgcn_perm((uint32_t)q[3], (uint32_t)q[2], k0),
                                             __builtin_amdgcn_perm((uint32_t)q[5], (uint32_t)q[4], k0), __builtin_amdgcn_perm((uint32_t)q[7], (uint32_t)q[6], k0)};
                    }
                }
#endif
                if (job.dbg_quant) {
                    int32_t *d = job.dbg_quant + (size_t)c * kDbgPitch * kDbgPitch +
                                 (size_t)(py0 + s * 8 + kh) * kDbgPitch + px0 + cb * 8;
#pragma unroll
                    for (int kv = 0; kv < 8; kv++)
                        d[kv] = q[kv];
                }
                /* 32-bit offsets from one uniform base: the loads take an SGPR base and a VGPR offset, no 64-bit address arithmetic */
                const char *const nib = (const char *)&kNibbleMasks.m[0][0][0];
                /* the loaded masks are first used after the loop: the next channel's transform runs while they travel */
                if (!(HYDK_K1_SKIP & 4))
                msk[c] = *(const unsigned long long *)(nib + (nib_row | nlo)) | *(const unsigned long long *)(nib + (nib_row | 128u | nhi));
                lf_int[c] = trunc_as_reference<FMT>(v[0] * kLfShift[c]); /* LF int: trunc(dc * shift[c]) (encoder.c:573,582) */
        };
#if HYDK_K1_CHANSEQ
        {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (ab < gbw) { /* phase A's role: row ar of block ab */
                    float o[8];
                    float *dst = s_rowpass + ab * kS0Block + ar * 8;
                    if (c == 0)
                        dct8(xv, o);
                    else if (c == 1)
                        dct8(yv, o);
                    else
                        dct8(bv, o);
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        dst[k] = o[k];
                }
                HYDK_K1_WAVE_SYNC();
                if (!(HYDK_K1_SKIP & 8) && cb < gbw)
                    column_pass(c);
                HYDK_K1_WAVE_SYNC(); /* the next channel's rows go where this channel's columns were just read */
            }
        }
#endif
        if (!(HYDK_K1_SKIP & 8) && cb < gbw) {
#if !HYDK_K1_CHANSEQ
#pragma unroll
            for (int c = 0; c < 3; c++)
                column_pass(c);
#endif
            if (kh == 0) {
#pragma unroll
                for (int c = 0; c < 3; c++)
                    HYDK_GLOBAL(int32_t, job.dc)[(size_t)c * HYDK_DC_PITCH * HYDK_DC_PITCH + (size_t)((py0 >> 3) + s) * HYDK_DC_PITCH + (px0 >> 3) + cb] = lf_int[c];
            }
#if HYDK_K1_TRIM & 2
            /* the block's bitmap = OR over its eight threads, taken through LDS instead of three DPP steps per word (eighteen
             * vector instructions per thread and strip): the block's eight threads are eight neighbouring lanes of ONE
             * wavefront, whose LDS operations execute in order — thread kh = 0 clears the words, all eight OR into them, thread
             * kh = 0 reads the result back (only it needs it) */
            {
                typedef unsigned long long u64;
                u64 *const cell = (u64 *)&s_seg[cb * 3]; /* .x/.y of the three descriptors: visit order Y, X, B = channel 1, 0, 2 */
                if (kh == 0) {
                    cell[0] = 0;
                    cell[2] = 0;
                    cell[4] = 0;
                }
                __builtin_amdgcn_wave_barrier();
                constexpr int at[3] = {2, 0, 4}; /* channel c -> u64 index (descriptor visit * 2) */
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    __hip_atomic_fetch_or((uint32_t *)&cell[at[c]], (uint32_t)msk[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_or((uint32_t *)&cell[at[c]] + 1, (uint32_t)(msk[c] >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                __builtin_amdgcn_wave_barrier();
                if (kh == 0) {
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        msk[c] = cell[at[c]];
                }
            }
#else
#pragma unroll
            for (int c = 0; c < 3 && !(HYDK_K1_SKIP & 4); c++) { /* the block's bitmap = OR over its eight threads */
                const uint32_t lo = or_reduce8((uint32_t)msk[c]), hi = or_reduce8((uint32_t)(msk[c] >> 32));
                msk[c] = ((unsigned long long)hi << 32) | lo;
            }
#endif
        }
        /* symbols per channel: the count symbol + coefficients up to the last non-zero one; visit order
         * Y, X, B (encoder.c:712) */
        const uint32_t nY = 1u + (msk[1] ? 63u - (uint32_t)__clzll(msk[1]) : 0u);
        const uint32_t nX = 1u + (msk[0] ? 63u - (uint32_t)__clzll(msk[0]) : 0u);
        const uint32_t nB = 1u + (msk[2] ? 63u - (uint32_t)__clzll(msk[2]) : 0u);
        if (kh == 0) {
            s_blen[cb] = cb < gbw ? nY | (nX << 8) | (nB << 16) : 0u;
#if HYDK_K1_CHANSEQ
            const uint32_t base = (uint32_t)(cb * kQBlock), chan_pitch = 32u * kQBlock; /* element offsets into s_q */
#else
            const uint32_t base = (uint32_t)(cb * kS0Block), chan_pitch = (uint32_t)kS0Chan; /* word offsets into s_rowpass */
#endif
            s_seg[cb * 3 + 0] = make_uint4((uint32_t)msk[1], (uint32_t)(msk[1] >> 32), nY | ((uint32_t)__popcll(msk[1]) << 8), base + chan_pitch);
            s_seg[cb * 3 + 1] = make_uint4((uint32_t)msk[0], (uint32_t)(msk[0] >> 32), nX | ((uint32_t)__popcll(msk[0]) << 8), base);
            s_seg[cb * 3 + 2] = make_uint4((uint32_t)msk[2], (uint32_t)(msk[2] >> 32), nB | ((uint32_t)__popcll(msk[2]) << 8), base + 2 * chan_pitch);
        }
        __syncthreads();

        /* ---------------- phase C1: every wave prefix-sums the 32 block totals for itself ---------------- */
        {
            const uint32_t len3 = s_blen[lane & 31];
            const uint32_t mine = (len3 & 0xffu) + ((len3 >> 8) & 0xffu) + (len3 >> 16);
            uint32_t inc = scan16_inclusive(mine);
            inc += HYDK_DPP(inc, 0x142, 0xA); /* row_bcast:15: rows 1 and 3 add the total of the row before */
            s_boff[(lane & 31) + 1] = inc;
            if (lane == 0)
                s_boff[0] = 0;
            __builtin_amdgcn_wave_barrier();
        }
        const uint32_t strip_total = s_boff[32];

        /* ---------------- phase C2: the strip's symbol stream, cut into 256 equal runs ----------------
         * Thread t emits one of 256 consecutive runs of the strip's symbols, equal in length up to one: it finds the
         * (block, channel, zig-zag position) its run starts at by a binary search over the block offsets, then WALKS
         * — the non-zero count still to come and the "previous coefficient was non-zero" flag of the contexts
         * (encoder.c:724-738) are carried from symbol to symbol instead of being recounted from the bitmap, and the
         * work is balanced over the workgroup whatever the blocks' sizes. */
        {
            overflowed = overflowed || goff + strip_total > tok_room;
            /* runs of floor(n / 256) symbols, the first n mod 256 threads one more: the longer runs sit in the first
             * wavefronts, so the later ones leave the loop an iteration earlier */
            static_assert(kThreads == 256, "run lengths are computed with shifts");
            const uint32_t per = strip_total >> 8, extra = strip_total & 255u;
            uint32_t p = (uint32_t)t * per + min((uint32_t)t, extra);
            const uint32_t pend = overflowed ? 0u : p + per + ((uint32_t)t < extra ? 1u : 0u);
            if (!(HYDK_K1_SKIP & 1) && p < pend) {
                uint32_t b = 0;
#pragma unroll
                for (uint32_t step = 16; step; step >>= 1)
                    b += s_boff[b + step] <= p ? step : 0u;
                uint32_t j = p - s_boff[b]; /* position in the block's symbols, then in the channel's */
                const uint32_t len = s_blen[b];
                uint32_t visit = 0;
                if (j >= (len & 0xffu)) {
                    j -= len & 0xffu;
                    visit = 1;
                    if (j >= ((len >> 8) & 0xffu)) {
                        j -= (len >> 8) & 0xffu;
                        visit = 2;
                    }
                }
                uint32_t seg_at = b * 3u + visit;
                uint4 seg = s_seg[seg_at];
                uint32_t n = seg.z & 0xffu, nz_total = seg.z >> 8;
                /* non-zeros at positions >= j; whether position j - 1 holds one (encoder.c:731-738) */
                const unsigned long long m = ((unsigned long long)seg.y << 32) | seg.x;
                uint32_t remaining = nz_total - (uint32_t)__popcll(m & ((1ull << j) - 1ull));
                uint32_t prev = j <= 1u ? (uint32_t)(nz_total <= 4u) : (uint32_t)(m >> (j - 1u)) & 1u;
                /* cluster of a coefficient = coef_base + (prev & prev_mask) + (2 * ((visit + nnz ctx + freq ctx) mod 3) & ctx_mask),
                 * of a count = visit & count_mask: the four schemes of encoder.c:862-901 without a branch */
                const uint32_t coef_base = (uint32_t)coef_cl_lo;
                const uint32_t prev_mask = job.scheme <= 1 ? 1u : 0u, ctx_mask = job.scheme == 0 ? 6u : 0u;
                const uint32_t count_mask = job.scheme == 0 ? 3u : 0u;
                for (; p < pend; p++) {
                    const uint32_t ji = s_jinfo[j];
#if HYDK_K1_CHANSEQ
                    const int coef = (int)s_q[seg.w + (ji & 0xffu)];
#else
                    const int coef = ((const int *)s_rowpass)[seg.w + (ji & 0xffu)];
#endif
                    const bool is_count = j == 0u;
                    const uint32_t value = is_count ? nz_total : pack_signed(coef);
                    /* context - 111 = 458*visit + prev + 2*(nnz_ctx[remaining] + freq_ctx[j]) (encoder.c:724,731-732);
                     * scheme 0 needs it mod 6 = prev + 2*((visit + nnz_ctx + freq_ctx) mod 3), the others mod 2 = prev.
                     * u = 0..6; 2 * (u mod 3) sits at bits 2u+1, 2u+2 of 0x1248 */
                    const uint32_t u = visit + (uint32_t)s_nnz3[remaining & 63u] + (ji >> 8);
                    const uint32_t cluster = is_count ? (visit & count_mask)
                                                      : coef_base + (prev & prev_mask) + ((0x1248u >> (u + u)) & ctx_mask);
                    /* hybrid-uint split, config (4,1,0) (entropy.c:427-444) */
                    uint32_t token, rbits, residue;
                    if (FMT != HYDK_FMT_F32) {
                        /* value < 2^14 converts exactly: its float's exponent and top mantissa bit are floor(log2) and
                         * the bit below the leading one, i.e. the token's two variable parts (entropy.c:427-444) */
                        const uint32_t fb = __float_as_uint((float)value) >> 22; /* 2 * (127 + floor(log2)) + next bit */
                        const bool big = value >= 16u;
                        token = big ? fb - 246u : value;
                        rbits = big ? (fb >> 1) - 128u : 0u;
                        residue = __builtin_amdgcn_ubfe(value, 0u, rbits);
                    } else if (value < 16) {
                        token = value;
                        rbits = 0;
                        residue = 0;
                    } else {
                        const int nb = 30 - __clz((int)value); /* floor(log2) - 1 */
                        rbits = (uint32_t)nb;
                        residue = value & ((1u << nb) - 1u);
                        token = 16u + (((uint32_t)(nb - 3) << 1) | ((value >> nb) & 1u));
                    }
#if HYDK_K1_TRIM
                    const uint32_t bin = umad24(cluster, (uint32_t)kHistW, FMT == HYDK_FMT_F32 ? min(token, (uint32_t)kHistW - 1u) : token);
#else
                    const uint32_t bin = cluster * kHistW + (FMT == HYDK_FMT_F32 ? min(token, (uint32_t)kHistW - 1u) : token);
#endif
                    store_record<FMT>(tok, goff + p, token, cluster, bin, rbits, residue);
                    rb_sum += rbits;
                    /* every token straight into the LDS histogram (until round 3 zero tokens were counted in packed per-thread
                     * counters inside a divergent branch: twelve instructions to save an atomic that costs nothing) */
                    atomicAdd(&s_hist[bin], 1u);
                    /* walk on: the DC slot read for a count symbol is zero, so it leaves `remaining` alone */
                    const uint32_t here = coef != 0 ? 1u : 0u;
                    remaining -= here;
                    prev = is_count ? (uint32_t)(nz_total <= 4u) : here;
                    if (++j == n) { /* next channel of the block, or the next block (at most one step: every run has its count symbol) */
                        seg_at++;
                        visit = visit == 2u ? 0u : visit + 1u;
                        seg = s_seg[seg_at];
                        n = seg.z & 0xffu;
                        nz_total = remaining = seg.z >> 8;
                        j = 0;
                    }
                }
            }
        }
        goff += strip_total;
        /* the next strip's row pass overwrites the coefficients this strip's token phase reads */
        __syncthreads();
    }

    __syncthreads();
    uint32_t top_token = 0;
    for (int i = t; i < HYDK_MAX_CLUSTERS * kHistW; i += kThreads) {
        const uint32_t v = s_hist[i];
        if (v) {
            atomicAdd(&job.hist[(i / kHistW) * HYDK_ALPHABET + i % kHistW], v);
            top_token = max(top_token, (uint32_t)(i % kHistW) + 1u);
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1)
        top_token = max(top_token, (uint32_t)__shfl_xor((int)top_token, d));
    if (lane == 0 && top_token)
        atomicMax(job.alpha_max, top_token);
#pragma unroll
    for (int d = 32; d; d >>= 1)
        rb_sum += (uint32_t)__shfl_xor((int)rb_sum, d);
    if (lane == 0)
        atomicAdd(&s_rbits, rb_sum);
    __syncthreads();
    if (t == 0) {
        const uint32_t count = overflowed || HYDK_K1_SKIP ? 0u : goff; /* timing-only builds leave no symbols for the later stages */
        if (plog) {
            part_info[blockIdx.x] = uint2{count, s_rbits};
        } else {
            job.sym_count[g] = count;
            job.rbits_total[g] = s_rbits;
        }
        if (overflowed)
            atomicOr(status, HYDK_STATUS_TOKENS);
    }
    if (FMT == HYDK_FMT_F32 && bad_sample) {
        if (job.bad_slot)
            atomicOr(job.bad_slot, 1u); /* the slot's own word: the launch-wide status stays clean */
        else
            atomicOr(status, HYDK_STATUS_BAD_SAMPLE);
    }
