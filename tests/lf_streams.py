"""Crafted residual streams for the LF-group coder (hydrium_amd/csrc/hip/lf_coder.hip).  TEST INFRASTRUCTURE ONLY; no GPU, no torch.

The coder decides its output at fixed positions: windows of 896 values inside a scan span of 1024, a look-ahead of 127, a
backward scan in steps of 256, run chunks of 128 with "more than 3 repeats make a run pair", threads that own four
consecutive values, bit strings of up to 59 bits ORed across three words, two words that neighbouring windows share.  A
picture puts a run head wherever its content happens to; the streams here put one at each of those positions on purpose.

A wanted residual stream v (channels Y, X, B, raster) becomes LF ints by inverting the clamped-gradient predictor serially
in 32-bit wrap-around arithmetic (lf_ints_from_residuals); tests/lf_model.py's residuals() gives v back exactly.  The
background of every stream has no equal neighbours, so only the planted runs are runs.

The positions below are written out as expressions of WINDOW, SPAN, CHUNK and STEP on purpose and are not read from the
kernel's headers: if the kernel's constants change, this corpus has to be thought through again, not follow silently.
"""
from __future__ import annotations

import functools
from typing import Callable, List, Optional, Sequence

import numpy as np

from tests import lf_model

WINDOW = 896   # values a workgroup emits
SPAN = 1024    # values it looks at
CHUNK = 128    # a run's chunk: one literal + up to 127 repeats
STEP = 256     # positions per step of the backward scan
WRAPS = 0xFFFFFFFF  # the symbol the reference cannot tell from "no symbol yet"
MIN_PAIR = 4   # repeats behind a chunk's head that make a run pair ("more than 3")


# ---- residuals -> LF ints ---------------------------------------------------------------------------------------------
def _s32(a: int) -> int:
    return ((a + 0x80000000) & 0xFFFFFFFF) - 0x80000000


def lf_ints_from_residuals(v, vbw: int, vbh: int) -> np.ndarray:
    """int32[3][vbh][vbw] (planes X, Y, B) whose residual stream is v: lf = pred(w, n, nw) + unpack_signed(v), serially."""
    blocks = vbw * vbh
    v = [int(x) for x in np.asarray(v).reshape(-1)]
    assert len(v) == 3 * blocks
    out = np.zeros((3, vbh, vbw), np.int32)
    for visit, c in enumerate((1, 0, 2)):
        d = [_s32((x >> 1) ^ -(x & 1)) for x in v[visit * blocks:(visit + 1) * blocks]]
        up: Optional[list] = None
        rows = []
        i = 0
        for y in range(vbh):
            row = [0] * vbw
            for x in range(vbw):
                w = row[x - 1] if x else (up[0] if y else 0)
                n = up[x] if y else w
                nw = up[x - 1] if (x and y) else w
                p = _s32(w + n - nw)
                lo, hi = (w, n) if w < n else (n, w)
                p = lo if p < lo else hi if p > hi else p
                row[x] = _s32(p + d[i])
                i += 1
            rows.append(row)
            up = row
        out[c] = np.array(rows, np.int64).astype(np.int32)
    return out


# ---- building blocks --------------------------------------------------------------------------------------------------
def background(n: int) -> np.ndarray:
    """n values in 1..7, no two neighbours equal"""
    return (np.arange(n) % 7 + 1).astype(np.uint64)


def _repair(v: np.ndarray, i: int):
    """give v[i] a value that neither neighbour has (and that no background or planted value is)"""
    for cand in (11, 12, 13):
        if (i == 0 or v[i - 1] != cand) and (i + 1 >= len(v) or v[i + 1] != cand):
            v[i] = cand
            return
    raise AssertionError("no repair value")


def plant(v: np.ndarray, head: int, length: int, value: int = 9) -> np.ndarray:
    """a maximal run of `length` values `value` from position `head` on"""
    assert 0 <= head and head + length <= len(v) and length >= 1
    v[head:head + length] = value
    for i in (head - 1, head + length):
        if 0 <= i < len(v) and v[i] == value:
            _repair(v, i)
    return v


class Info:
    """what the model says about a stream: per position literal flag, run length, string length and bit offset"""

    def __init__(self, v):
        self.hist, self.lengths, self.alphabet, self.lit, self.r, self.val, self.ln = lf_model.strings(v)
        self.off = np.concatenate([[0], np.cumsum(self.ln)[:-1]]).astype(np.int64)
        self.nbits = int(self.ln.sum())


class Case:
    def __init__(self, name: str, vbw: int, vbh: int, make: Callable[[int], np.ndarray], prop: Callable[[np.ndarray, Info], bool]):
        self.name, self.vbw, self.vbh, self._make, self._prop = name, vbw, vbh, make, prop
        self.family = name.split("-")[0]
        self.n = 3 * vbw * vbh

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def stream(self) -> np.ndarray:
        v = np.asarray(self._make(self.n), np.uint64)
        assert v.shape == (self.n,)
        v.setflags(write=False)
        return v

    @functools.lru_cache(maxsize=None)
    def lf_ints(self) -> np.ndarray:
        dc = lf_ints_from_residuals(self.stream(), self.vbw, self.vbh)
        dc.setflags(write=False)
        return dc

    def holds(self) -> bool:
        """the property the case exists for"""
        v = self.stream()
        return bool(self._prop(v, Info(v)))


def _pairs_only_in(r: np.ndarray, spans) -> bool:
    """run pairs are sent from inside the planted runs only"""
    ok = np.zeros(len(r), bool)
    for h, ln in spans:
        ok[h:h + ln] = True
    return not (r[~ok] > 0).any()


def _is_run(v, i: Info, head: int, length: int, value: int) -> bool:
    """maximal run of `value` at [head, head + length) that the model cuts into chunks of 128 from its head"""
    if not ((v[head:head + length] == value).all() and (head == 0 or v[head - 1] != value)
            and (head + length == len(v) or v[head + length] != value)):
        return False
    if value == WRAPS:
        return True  # its chunk rule is its own (tests/test_lf_model.py); the cases state what they need themselves
    for start in range(head, head + length, CHUNK):
        rep = min(CHUNK - 1, head + length - start - 1)
        if not i.lit[start] or i.r[start] != (rep if rep >= MIN_PAIR else 0):
            return False
        behind = i.lit[start + 1:start + 1 + rep]
        if behind.any() if rep >= MIN_PAIR else not behind.all():  # repeats: one pair, or literals when 3 or fewer
            return False
    return True


def run_case(name, vbw, vbh, head, length, value=9, also=None) -> Case:
    def make(n):
        return plant(background(n), head, length, value)

    def prop(v, i):
        return _is_run(v, i, head, length, value) and _pairs_only_in(i.r, [(head, length)]) and (also is None or also(v, i))

    return Case(name, vbw, vbh, make, prop)


CASES: List[Case] = []

# ---- a. window edges: 64 x 14, n = 2688 = three full windows -----------------------------------------------------------
A_SHAPE = (64, 14)
assert 3 * A_SHAPE[0] * A_SHAPE[1] == 3 * WINDOW
for h in (WINDOW - 5, WINDOW - 4, WINDOW - 3, WINDOW - 1, WINDOW, WINDOW + 1):
    for ln in (MIN_PAIR, MIN_PAIR + 1, CHUNK, CHUNK + 1, CHUNK + MIN_PAIR):
        CASES.append(run_case(f"a-head{h}-len{ln}", *A_SHAPE, h, ln))
for h in (2 * WINDOW - 5, 2 * WINDOW - 4, 2 * WINDOW - 3, 2 * WINDOW - 1, 2 * WINDOW, 2 * WINDOW + 1):
    for ln in (MIN_PAIR, MIN_PAIR + 1):
        CASES.append(run_case(f"a-head{h}-len{ln}", *A_SHAPE, h, ln))
# the farthest value the look-ahead reads: the last repeat of a full chunk whose head is a window's last value
CASES.append(run_case("a-lookahead-end", *A_SHAPE, WINDOW - 1, CHUNK,
                      also=lambda v, i: WINDOW - 1 + CHUNK - 1 == SPAN - 2 and i.r[WINDOW - 1] == CHUNK - 1))
# a chunk that ends with the window
CASES.append(run_case("a-chunk-ends-window", *A_SHAPE, WINDOW - CHUNK, CHUNK, also=lambda v, i: i.r[WINDOW - CHUNK] == CHUNK - 1))

# ---- b. backward scan: 30 x 40, n = 3600; the run starts `back` in front of the third window and ends 10 behind its start
B_SHAPE = (30, 40)
for back in (1, 3, 4, CHUNK - 1, CHUNK, STEP - 1, STEP, STEP + 1, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1, WINDOW - 1, WINDOW,
             WINDOW + 1, 1500):
    CASES.append(run_case(f"b-back{back}", *B_SHAPE, 2 * WINDOW - back, back + 10))


def flat_case(name, vbw, vbh, value, from_one=False, also=None) -> Case:
    def make(n):
        v = np.full(n, value, np.uint64)
        if from_one:
            v[0] = value + 3
        return v

    def prop(v, i):
        first = 1 if from_one else 0
        return _is_run(v, i, first, len(v) - first, value) and (also is None or also(v, i))

    return Case(name, vbw, vbh, make, prop)


for shape in ((64, 14), (1, 1), (256, 256)):
    tag = f"{shape[0]}x{shape[1]}"
    # (1 x 1: three equal values are three literals of one token, and a code of one token takes no bits)
    single = (lambda v, i: i.alphabet == 1 and i.nbits == 0) if shape == (1, 1) else None
    CASES.append(flat_case(f"b-flat0-{tag}", *shape, 0, also=single))
    CASES.append(flat_case(f"b-flat7-{tag}", *shape, 7, also=(lambda v, i: i.nbits == 0) if shape == (1, 1) else None))
    CASES.append(flat_case(f"b-flat-from1-{tag}", *shape, 0, from_one=True))

# ---- c. stream ends and shapes: a run that ends exactly at n - 1 ---------------------------------------------------------
C_SHAPES = ((1, 1), (1, 2), (3, 1), (2, 3), (1, 256), (256, 1), (2, 149), (13, 23), (3, 100), (7, 43), (255, 2), (255, 3),
            (256, 256))
for vbw, vbh in C_SHAPES:
    n = 3 * vbw * vbh
    for ln in (1, MIN_PAIR, MIN_PAIR + 1, CHUNK - 1, CHUNK):
        if ln <= n:
            CASES.append(run_case(f"c-{vbw}x{vbh}-tail{ln}", vbw, vbh, n - ln, ln, also=lambda v, i: v[-1] == 9))

# ---- d. plane boundaries: one thread's four values in two channel planes ---------------------------------------------------
D_SHAPES = ((13, 23), (2, 149), (7, 43), (255, 3))
for vbw, vbh in D_SHAPES:
    blocks = vbw * vbh
    CASES.append(run_case(f"d-{vbw}x{vbh}-yx", vbw, vbh, blocks - 3, 7))
    ln = 200 if 2 * blocks - 1 + 200 <= 3 * blocks else 3
    CASES.append(run_case(f"d-{vbw}x{vbh}-xb", vbw, vbh, 2 * blocks - 1, ln))

# ---- e. values -----------------------------------------------------------------------------------------------------------
E_SHAPE = (64, 14)
for val in (127, 128, 129, 255, 256, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 0xFFFFFFFE):
    CASES.append(run_case(f"e-value{val:#x}-lone", *E_SHAPE, WINDOW - 6, 1, val))
    CASES.append(run_case(f"e-value{val:#x}-run9", *E_SHAPE, WINDOW - 6, 9, val))


def wraps_case(name, head, length) -> Case:
    """`length` values 0xFFFFFFFF from `head` on.  At the head of the stream they count as repeats of a value in front of it
    (chunks from position -1); inside it up to 3 repeats behind the literal are dropped."""
    def make(n):
        return plant(background(n), head, length, WRAPS)

    def prop(v, i):
        if not _is_run(v, i, head, length, WRAPS):
            return False
        if head == 0:  # the phantom literal is never sent; position 0 sends the pair when more than 3 values follow "it"
            rep = min(CHUNK - 1, length)
            return not i.lit[0] and i.r[0] == (rep if rep >= MIN_PAIR else 0)
        rep = min(CHUNK - 1, length - 1)
        return bool(i.lit[head]) and i.r[head] == (rep if rep >= MIN_PAIR else 0) and not i.lit[head + 1:head + 1 + rep].any()

    return Case(name, *E_SHAPE, make, prop)


for first in (5, CHUNK - 1, CHUNK, CHUNK + 2, WINDOW - 1, WINDOW, WINDOW + 4, SPAN + 6):
    CASES.append(wraps_case(f"e-wraps-first{first}", 0, first))
for pos in (WINDOW - 3, WINDOW - 1, WINDOW, 1000):
    for ln in (2, 3, 4, 5, 200):
        CASES.append(wraps_case(f"e-wraps-at{pos}-len{ln}", pos, ln))

# ---- f. longest strings ------------------------------------------------------------------------------------------------------
# Sixteen symbols with Fibonacci counts make a prefix code 15 deep: the literal of 0xFFFFFFFE (29 residue bits) and the run
# token of its 5 repeats once each, fourteen small literal values 2, 3, 5, ... times.  The head of that run then sends
# 15 + 29 + 15 = 59 bits.
F_SHAPE = (27, 32)
F_BIG = 0xFFFFFFFE
F_RUN = 6


def _fib_pool(n: int) -> np.ndarray:
    """n - 6 small literal values, Fibonacci counts (the commonest takes the slack), no two neighbours equal, ends unequal"""
    counts = [2, 3]
    while len(counts) < 14:
        counts.append(counts[-1] + counts[-2])
    slack = n - F_RUN - sum(counts)
    assert 0 <= slack < 100
    counts[-1] += slack
    order = [20 + k for k in range(14) for _ in range(counts[k])][::-1]  # commonest first
    m = len(order)
    assert counts[-1] <= m // 2
    pool = np.zeros(m, np.uint64)
    pool[0::2] = order[:(m + 1) // 2]
    pool[1::2] = order[(m + 1) // 2:]
    assert (pool[1:] != pool[:-1]).all() and pool[0] != pool[-1]
    return pool


def _fib_stream(n: int, pos: int, k: int) -> np.ndarray:
    pool = np.roll(_fib_pool(n), -k)
    return np.concatenate([pool[:pos], np.full(F_RUN, F_BIG, np.uint64), pool[pos:]])


@functools.lru_cache(maxsize=None)
def _fib_rotations(pos: int):
    """bit offset mod 32 of the 59-bit string for every rotation k of the pool in front of it (one code for all: the
    histogram does not depend on k)"""
    n = 3 * F_SHAPE[0] * F_SHAPE[1]
    i = Info(_fib_stream(n, pos, 0))
    pool = _fib_pool(n)
    per_value = {int(x): int(i.lengths[int(x)]) for x in np.unique(pool)}
    ln = np.array([per_value[int(x)] for x in pool], np.int64)
    cum = np.concatenate([[0], np.cumsum(np.concatenate([ln, ln]))])
    return [int((cum[k + pos] - cum[k]) % 32) for k in range(len(pool))]


def fib_case(name, pos, want_off) -> Case:
    def k_of():
        offs = _fib_rotations(pos)
        hits = [k for k, o in enumerate(offs) if o == want_off]
        assert hits, f"no rotation puts the string at bit {want_off} of a word"
        return hits[0]

    def make(n):
        return _fib_stream(n, pos, k_of())

    def prop(v, i):
        return (int(i.lengths.max()) == 15 and int(i.ln.max()) == 59 and int(i.ln[pos]) == 59 and int(i.r[pos]) == F_RUN - 1
                and int(i.off[pos]) % 32 == want_off and (v[1:] != v[:-1]).sum() == len(v) - F_RUN)

    return Case(name, *F_SHAPE, make, prop)


# where the 59-bit string starts in its word: 0; 5, the last offset at which it fits two words; 6, the first at which it
# spills into a third; 17; 31.  As a window's last value and as the next one's first.
F_OFFSETS = (0, 5, 6, 17, 31)
for pos in (WINDOW - 1, WINDOW):
    for off in F_OFFSETS:
        CASES.append(fib_case(f"f-fib-at{pos}-bit{off}", pos, off))


def dense_case(name, vbw, vbh, seed) -> Case:
    """every third value random in [2^31, 2^32): long residue fields everywhere"""
    def make(n):
        v = background(n)
        rng = np.random.default_rng(seed)
        big = rng.integers(2 ** 31, 2 ** 32 - 1, size=len(v[::3]), dtype=np.uint64)
        v[::3] = big
        return v

    def prop(v, i):
        return (v[::3] >= 2 ** 31).all() and (v != WRAPS).all() and int(i.ln.max()) >= 29 + 1 and not (i.r > 0).any()

    return Case(name, vbw, vbh, make, prop)


CASES.append(dense_case("f-dense-20x20", 20, 20, 1))

# ---- g. several slots in one frame; h. a context used twice ----------------------------------------------------------------------
DENSE_FULL = dense_case("f-dense-256x256", 256, 256, 2)
CASES.append(DENSE_FULL)


def mult32_case() -> Case:
    """a stream whose bit count is a multiple of 32: background at 13 x 23 with `pad` trailing values of 40"""
    vbw, vbh = 13, 23

    def make_pad(n, pad):
        v = background(n)
        v[n - pad:] = 40 + np.arange(pad) % 2
        return v

    @functools.lru_cache(maxsize=None)
    def pad_of():
        n = 3 * vbw * vbh
        for pad in range(0, 400):
            if Info(make_pad(n, pad)).nbits % 32 == 0:
                return pad
        raise AssertionError("no padding count gives a bit count that is a multiple of 32")

    return Case("g-bits-multiple-of-32", vbw, vbh, lambda n: make_pad(n, pad_of()), lambda v, i: i.nbits > 0 and i.nbits % 32 == 0)


MULT32 = mult32_case()
CASES.append(MULT32)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names are unique"


class Frame:
    def __init__(self, name: str, slots: Sequence[Case]):
        self.name, self.slots = name, list(slots)

    def __repr__(self):
        return self.name


FRAMES = [
    Frame("g-three-shapes", [BY_NAME[f"a-head{WINDOW - 1}-len{CHUNK}"], BY_NAME["c-13x23-tail5"], BY_NAME["d-7x43-yx"]]),
    Frame("g-four-shapes", [BY_NAME[f"b-back{STEP}"], BY_NAME["c-1x256-tail128"], BY_NAME[f"e-wraps-first{WINDOW}"], BY_NAME["c-2x3-tail4"]]),
    Frame("g-zero-bits-in-the-middle", [BY_NAME[f"a-head{WINDOW}-len{MIN_PAIR + 1}"], BY_NAME["b-flat0-1x1"], BY_NAME["c-255x3-tail127"]]),
    Frame("g-bits-multiple-of-32", [MULT32, BY_NAME["c-3x1-tail4"], BY_NAME[f"f-fib-at{WINDOW - 1}-bit31"]]),
    Frame("g-longest-then-shortest", [DENSE_FULL, BY_NAME["c-1x2-tail1"]]),
]
# h: the longest stream, then the shortest in the same context and slot
TWICE = (DENSE_FULL, BY_NAME["c-1x2-tail1"])
# routes of tests/test_gpu_lf_streams.py; the 256 x 256 streams that run on one route less are listed there
FAMILIES_ON_SIDE = ("a", "b", "g")
