"""Pictures that make the ANS table kernel (k_build_tables) and the rANS chains (k_rans_encode, k_rans_lanes, k_rans_emit)
run the branches no other picture of the suite reaches.  Every picture is black with a few named samples, or seeded noise
from synth.make_image_f32 times a constant; each states the claim it exists for, and tests/test_entropy_corpus.py proves
every claim on the CPU from the oracle and tests/ans_model.py.  tests/test_gpu_entropy_corpus.py then holds the kernels
to the oracle and to the compiled reference on them.

How pixels reach a histogram.  A black 8x8 block codes three symbols, the non-zero counts of Y, X and B, token 0 in
clusters 0, 1 and 2.  One grey sample in a block leaves X and B at zero and gives Y a count that grows with the sample
(8 bit, sample at (5, 3) of the block: 20 -> token 1, 23 -> 2, 24 -> 3, 29 -> 4, 30 -> 6, 31 -> 9, 35 -> 10, 36 -> 12,
37 -> 16), followed by that block's coefficient tokens in clusters 3 .. 8.  So cluster 0 of a black picture of T blocks
holds T - k at token 0 and whatever k lit blocks put above it.  A count of 1 among more than 4096 scales to 0 and is
lifted to 1: the only source of an excess over 4096, so an excess needs more than 4096 symbols in one cluster.

excess (8 bit, so the wave form 4 and the lane form 5 both code them)
  excess_at_0        2048x160, 5120 blocks, cluster 0 = [5115, 1, 1, 1, 1, 0, 1]: the scan steps past every entry (skip)
                     down to j = 0 and takes the excess of 1 from freq[0] (partial)
  excess_partial     2048x160, cluster 0 = [5110, 1, 1, 1, 1, 0, 1, 0, 0, 5]: the last entry scales to 3, larger than the
                     excess: partial at once, no other branch
  excess_skip        2048x160, cluster 0 = [5110, 1, 1, 1, 4, 0, 1, 0, 0, 1, 1]: skip past tokens 10, 9 .. 5, partial at
                     token 4, above j = 0
  excess_flatten     2048x200, 6400 blocks, cluster 0 = [6388, 1, 1, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 4]: the last entry
                     scales to 2, no larger than the excess of 2: flatten, then skip, then partial at j = 0
  excess_coef        256x88: 340 blocks with a sample of 40, one of 106, one of 255, the last 10 black.  The excess is in
                     cluster 7, a coefficient cluster ([4762, 0, 0, 0, 1021, 0, 0, 1, ...]: skip, then partial at token 4);
                     cluster 0 has 352 symbols and none
  Smaller was searched with the model: with T blocks, k lifted counts give an excess only when k - ceil(4096 k / T) >= 1,
  which at 2048x136 (4352 blocks) takes 17 distinct non-zero counts, more than one grey sample reaches (13); 2048x160
  takes 5.  The flatten branch needs an excess of 2 against a last entry of 2: 8 lifted counts at 6400 blocks.

log6 (float32)
  max_32, max_33, max_64, max_65   8x8, one sample of 80, 128, 5242880 and 7500000 at (5, 3): running maxima of exactly
                     32, 33, 64 and 65, so log_alphabet_size 5, 6, 6 and 7 - both steps of 32 - clz(mx - 1).  In max_32
                     and max_64 the cluster that holds the largest token has an alphabet as large as the table
                     (n_eq_table at 5 and at 6).  The first three hand a deficit to a token 0 that was never
                     coded (deficit_into_empty_f0), and so do the two below.
  noise_36, noise_49 synth noise 64x48 times 100 and times 1e4: running maxima 36 and 49, 9216 symbols, every
                     coefficient cluster alive with alphabets of 33 .. 49 in a 64-entry table

handover (float32, (2048 + 8) x 8: two LF groups, two presets)
  log6_then_black    noise times 100 (maximum 36), then black: the second LF group's own alphabet is 1, and it builds the
                     one-symbol (`unique`) tables with 64 entries
  black_then_log6    black, then noise times 100 (its 8x8: maximum 35): 32-entry tables, then 64-entry ones
  log7_then_log6     noise times 1e7 (maximum 69), then noise times 100: the second codes with 128-entry tables though
                     its own maximum is 35

counts (one block row; a block is black, 3 symbols, or holds one grey sample at its corner: 14 -> 7 symbols, 16 -> 11,
19 -> 15, 36 -> 35, 45 -> 42, 49 -> 43; float32: 14/256 and 16/256 give the same).  The single group's symbol count n:
  n_15 .. n_129      n = 15, 16, 17 (a round of 16 lanes, a flag word of 16 symbols, one short and one over), 63, 64, 65
                     (a chunk of k_rans_encode: the partial chunk comes first, 64 takes the unrolled path alone, 65 is
                     a partial chunk of 1 and a full one), 127, 128, 129 - 8 bit
  n_128_then_3       264x8: two groups in one LF group, 128 symbols and 3
  f32_n_64, f32_n_65 64 and 65 again in float32: 8-byte records, the self-emitting chain

Nothing listed in the issue was left unreached.
"""
import functools

import numpy as np

LF_GROUP = 2048
_DTYPE = {8: np.uint8, 16: np.uint16, 32: np.float32}

# 8-bit grey sample at (5, 3) of a block -> the block's Y non-zero-count token
NZ_SAMPLE = {1: 20, 2: 23, 3: 24, 4: 29, 6: 30, 9: 31, 10: 35, 12: 36, 16: 37}


def _black(w, h, depth):
    return np.zeros((h, w, 3), _DTYPE[depth])


def _lit_blocks(w, h, depth, blocks, at=(5, 3)):
    """black, with one grey sample `value` at (x, y) = `at` inside block number b (raster order) for (b, value) in blocks"""
    img = _black(w, h, depth)
    bw = w // 8
    for b, value in blocks:
        assert b < bw * (h // 8)
        img[(b // bw) * 8 + at[1], (b % bw) * 8 + at[0]] = value
    return img


def _spread(values, total):
    """block numbers spread evenly over `total` blocks: value i at block (2 i + 1) total / (2 n)"""
    return [((2 * i + 1) * total // (2 * len(values)), v) for i, v in enumerate(values)]


def _nz(tokens):
    return [NZ_SAMPLE[t] for t in tokens]


def _noise(w, h, scale):
    from hydrium_amd import synth

    return (synth.make_image_f32("noise", w, h) * np.float32(scale)).astype(np.float32)


def _strip(blocks, value, depth=8):
    """one block row of `blocks` blocks; the corner sample of block 1 (block 0 where there is one block) is `value`"""
    img = _black(8 * blocks, 8, depth)
    img[0, 8 if blocks > 1 else 0] = value
    return img


def _beside(first, second):
    return np.concatenate([first, second], axis=1)


_MAKE = {
    # ---- excess ------------------------------------------------------------------------------------------------------------
    "excess_at_0": lambda: _lit_blocks(2048, 160, 8, _spread(_nz([1, 2, 3, 4, 6]), 5120)),
    "excess_partial": lambda: _lit_blocks(2048, 160, 8, _spread(_nz([1, 2, 3, 4, 6] + [9] * 5), 5120)),
    "excess_skip": lambda: _lit_blocks(2048, 160, 8, _spread(_nz([1, 2, 3, 6, 9, 10] + [4] * 4), 5120)),
    "excess_flatten": lambda: _lit_blocks(2048, 200, 8, _spread(_nz([1, 2, 3, 4, 6, 9, 10, 12] + [16] * 4), 6400)),
    "excess_coef": lambda: _lit_blocks(256, 88, 8, [(b, 40) for b in range(340)] + [(340, 106), (341, 255)]),
    # ---- log6 --------------------------------------------------------------------------------------------------------------
    "max_32": lambda: _lit_blocks(8, 8, 32, [(0, 80.0)]),
    "max_33": lambda: _lit_blocks(8, 8, 32, [(0, 128.0)]),
    "max_64": lambda: _lit_blocks(8, 8, 32, [(0, 5242880.0)]),
    "max_65": lambda: _lit_blocks(8, 8, 32, [(0, 7500000.0)]),
    "noise_36": lambda: _noise(64, 48, 100),
    "noise_49": lambda: _noise(64, 48, 1e4),
    # ---- handover ----------------------------------------------------------------------------------------------------------
    "log6_then_black": lambda: _beside(_noise(LF_GROUP, 8, 100), _black(8, 8, 32)),
    "black_then_log6": lambda: _beside(_black(LF_GROUP, 8, 32), _noise(8, 8, 100)),
    "log7_then_log6": lambda: _beside(_noise(LF_GROUP, 8, 1e7), _noise(8, 8, 100)),
    # ---- counts ------------------------------------------------------------------------------------------------------------
    "n_15": lambda: _strip(1, 19),
    "n_16": lambda: _strip(4, 14),
    "n_17": lambda: _strip(3, 16),
    "n_63": lambda: _strip(17, 19),
    "n_64": lambda: _strip(20, 14),
    "n_65": lambda: _strip(19, 16),
    "n_127": lambda: _strip(29, 49),
    "n_128": lambda: _strip(32, 36),
    "n_129": lambda: _strip(30, 45),
    "n_128_then_3": lambda: _strip(33, 36),
    "f32_n_64": lambda: _strip(20, 14 / 256, 32),
    "f32_n_65": lambda: _strip(19, 16 / 256, 32),
}

EXCESS = ("excess_at_0", "excess_partial", "excess_skip", "excess_flatten", "excess_coef")
LOG6 = ("max_32", "max_33", "max_64", "max_65", "noise_36", "noise_49")
HANDOVER = ("log6_then_black", "black_then_log6", "log7_then_log6")
COUNTS = ("n_15", "n_16", "n_17", "n_63", "n_64", "n_65", "n_127", "n_128", "n_129", "n_128_then_3", "f32_n_64", "f32_n_65")
NAMES = EXCESS + LOG6 + HANDOVER + COUNTS
assert set(NAMES) == set(_MAKE)

E = frozenset  # shorthand for the tables below
# ---- the claims --------------------------------------------------------------------------------------------------------------
# name -> (cluster, the excess tags that cluster takes, exactly; no other cluster of the picture takes any)
EXCESS_CLAIMS = {
    "excess_at_0": (0, E({"excess_skip", "excess_partial", "excess_at_0"})),
    "excess_partial": (0, E({"excess_partial"})),
    "excess_skip": (0, E({"excess_skip", "excess_partial"})),
    "excess_flatten": (0, E({"excess_flatten", "excess_skip", "excess_partial", "excess_at_0"})),
    "excess_coef": (7, E({"excess_skip", "excess_partial"})),
}
# name -> per LF group in send order: (the LF group's own largest alphabet, running maximum, log_alphabet_size)
ALPHABET_CLAIMS = {
    "max_32": [(32, 32, 5)], "max_33": [(33, 33, 6)], "max_64": [(64, 64, 6)], "max_65": [(65, 65, 7)],
    "noise_36": [(36, 36, 6)], "noise_49": [(49, 49, 6)],
    "log6_then_black": [(36, 36, 6), (1, 36, 6)],
    "black_then_log6": [(1, 1, 5), (35, 35, 6)],
    "log7_then_log6": [(69, 69, 7), (35, 69, 7)],
}
N_EQ_TABLE = ("max_32", "max_64")  # some cluster's alphabet equals the table size
EMPTY_F0 = ("max_32", "max_33", "max_64", "noise_36", "noise_49")
# name -> the symbol count of every group
COUNT_CLAIMS = {
    "n_15": [15], "n_16": [16], "n_17": [17], "n_63": [63], "n_64": [64], "n_65": [65], "n_127": [127], "n_128": [128],
    "n_129": [129], "n_128_then_3": [128, 3], "f32_n_64": [64], "f32_n_65": [65],
}


@functools.lru_cache(maxsize=None)
def picture(name):
    """(h, w, 3) uint8 or float32, C-contiguous and read-only; made once"""
    img = np.ascontiguousarray(_MAKE[name]())
    assert img.ndim == 3 and img.shape[2] == 3 and img.shape[0] <= LF_GROUP
    img.setflags(write=False)
    return img


def is_float(name):
    return picture(name).dtype == np.float32


def lf_groups(name):
    return -(-picture(name).shape[1] // LF_GROUP)


@functools.lru_cache(maxsize=None)
def stage(name):
    """the oracle's result for every LF group of the picture, the running alphabet maximum handed on in send order.
    Made once; never changed."""
    from oracle import binding as orc

    img, out, mx = picture(name), [], 0
    for tx in range(lf_groups(name)):
        res, mx = orc.encode_lf_group(img, tx, 0, max_alphabet_size=mx)
        out.append(res)
    return tuple(out)
