"""Frames whose buffer need is known from the CPU oracle alone (tests/test_edge_frames.py, tests/test_gpu_buffer_edges.py).

One band of 8-row strips of one 256x256 group is ``synth`` noise, everything else is black (A, B and D put photo content
into the group beside it).  An all-black 8x8 block codes as exactly three symbols, one count symbol per channel: the
helper CONFIRMS that from the oracle's ``res.nz`` for every block outside the band instead of assuming it.  With it

    n = res.group_symbols[g]                              the symbols of the banded group,
    p = n - 3 * (blocks of the group outside the part)    the symbols of the transform part that holds the band,
    B = len(res.stream)                                   the section bytes of the frame

are known without a device, and HYDAMD_TOKEN_CAP / HYDAMD_PAYLOAD_CAP can be set to exactly what the frame needs, or to
one step less.  p is computed a second way, which also serves the groups that are not black: the one-LF-group frames
here use clustering scheme 0, which keeps count clusters (0..2 of the preset) apart from coefficient clusters (3..8), so a
group's symbol stream is cut into blocks at every third count symbol.

A group of ``gbh`` strips coded by 2^plog workgroups has parts of ceil(gbh / 2^plog) strips (k_transform_tokenize); part q
owns tok_cap >> plog records of the group's token array.
"""
import functools
import os

import numpy as np

from hydrium_amd import synth
from oracle import binding as orc

TOKENS_PER_GROUP = 196608      # HYDK_TOKENS_PER_GROUP: the hard maximum a rerun enlarges the token arrays to
PLOGS = (2, 1)


def r16(x):
    return (int(x) + 15) & ~15


def r32(x):
    return (int(x) + 31) & ~31


def part_strips(gbh, plog, part):
    """[first, end) strips of `part` of a group of `gbh` strips split over 2^plog workgroups."""
    per = (gbh + (1 << plog) - 1) >> plog
    first = part * per
    return min(gbh, first), min(gbh, first + per)


def band_rows(gbh, plog, part):
    """Pixel rows [y0, y1) inside the group of the strips of `part` (the last strip may be cut by the image's edge)."""
    s0, s1 = part_strips(gbh, plog, part)
    return s0 * 8, s1 * 8


# id -> (width, height, dtype, banded group, part that holds the band (negative: from the end), kind of the other groups)
SHAPES = {
    "A": (512, 256, np.uint8, 0, 0, "photo"),
    "B": (512, 256, np.uint16, 0, -1, "photo"),
    "C": (256, 256, np.float32, 0, 1, None),
    "D": (264, 136, np.uint8, 0, -1, "photo"),
    "E": (2048, 2048, np.uint8, 63, -1, None),
}
# The band is the whole part of the child's split (plog 2 for the unsplit child), in noise of this seed.  The equality
# variants were found by walking seeds upwards from 1 with the oracle (search_seed below; one hit in 16 or 32 tries):
#   n16: n % 16 == 0 (HYDAMD_K1_SPLIT=0), p16: p % 16 == 0 under plog 2, p32: p % 32 == 0 under plog 1.
# tests/test_edge_frames.py holds every one of them to the oracle again.
SEEDS = {
    ("A", 2): 1, ("A", 1): 1, ("B", 2): 1, ("B", 1): 1, ("C", 2): 1, ("C", 1): 1, ("D", 2): 1, ("D", 1): 1,
    ("E", 2): 1, ("E", 1): 1,
    ("A_n16", 2): 22, ("A_p16", 2): 22, ("A_p32", 1): 14,      # (n - p = 3 * 768 is a multiple of 16: one seed serves both)
    ("C_n16", 2): 50, ("C_p16", 2): 50, ("C_p32", 1): 16,
}
EQUALITY = {"n16": ("n", 16), "p16": ("p", 16), "p32": ("p", 32)}


def group_geometry(width, height, g):
    """(px, py, gw, gh, gbw, gbh) of 256x256 group g of a one-LF-group frame."""
    gcols = -(-width // 256)
    px, py = (g % gcols) * 256, (g // gcols) * 256
    gw, gh = min(256, width - px), min(256, height - py)
    return px, py, gw, gh, -(-gw // 8), -(-gh // 8)


def build_image(frame, plog, seed):
    """The picture of `frame` ("A" .. "E", or an equality variant "A_n16" ...) with its band laid out for `plog`."""
    w, h, dt, g, part, other = SHAPES[frame.split("_")[0]]
    px, py, gw, gh, gbw, gbh = group_geometry(w, h, g)
    part = part % (1 << plog)
    # (E's band is the last 64 rows whatever the split: they lie in the last part of both)
    y0, y1 = band_rows(gbh, 2, 3) if frame == "E" else band_rows(gbh, plog, part)
    y1 = min(y1, gh)
    depth = 8 if dt == np.uint8 else 16
    img = np.zeros((h, w, 3), dt)
    noise = synth.make_image("noise", gw, y1 - y0, depth, seed)
    if dt == np.float32:
        # samples in [0, 16]: far outside [0, 1], so that coefficients are large and residues long (10 bits where 16-bit
        # integers stop at 6), yet nothing leaves the range of a 32-bit integer: the float -> int conversion of a value
        # that does is undefined in C, and no parity is claimed there.  Negative samples are left out for the same reason.
        noise = (noise.astype(np.float32) * np.float32(16.0 / 65535.0)).astype(np.float32)
    img[py + y0:py + y1, px:px + gw] = noise
    if other:
        gcols = -(-w // 256)
        for o in range(gcols * -(-h // 256)):
            if o != g:
                ox, oy, ow, oh, _, _ = group_geometry(w, h, o)
                img[oy:oy + oh, ox:ox + ow] = synth.make_image(other, ow, oh, depth, 77, x0=ox, y0=oy)
    return np.ascontiguousarray(img), (g, part, y0, y1)


def second_image(img):
    """A different picture of the same shape and sample type (coded between two runs of a boundary frame)."""
    h, w, _ = img.shape
    if img.dtype == np.float32:
        return synth.make_image_f32("smooth", w, h, 5)
    return synth.make_image("smooth", w, h, 8 if img.dtype == np.uint8 else 16, 5)


def block_starts(res, g):
    """Index, within group g's symbols, at which each of its blocks starts (plus the group's total at the end): the stream
    is cut at every third count symbol (scheme 0: clusters 0..2 of the preset are the count clusters)."""
    assert res.cluster_to - res.cluster_from == 9, "not clustering scheme 0: count and coefficient clusters are shared"
    first = int(res.group_symbols[:g].sum())
    n = int(res.group_symbols[g])
    counts = np.flatnonzero(res.symbols["cluster"][first:first + n] - res.cluster_from < 3)
    assert len(counts) % 3 == 0
    return np.append(counts[::3], n)


def part_counts(res, width, height, g, plog):
    """Symbols of each of the 2^plog parts of group g, from the oracle's symbol stream."""
    _, _, _, _, gbw, gbh = group_geometry(width, height, g)
    starts = block_starts(res, g)
    assert len(starts) == gbw * gbh + 1, "one count symbol per channel and block"
    out = []
    for q in range(1 << plog):
        s0, s1 = part_strips(gbh, plog, q)
        out.append(int(starts[s1 * gbw] - starts[s0 * gbw]))
    return out


class Case:
    """One frame and everything the oracle says about it."""

    def __init__(self, frame, plog, seed):
        self.frame, self.plog, self.seed = frame, plog, seed
        self.img, (self.g, self.part, self.y0, self.y1) = build_image(frame, plog, seed)
        self.img.setflags(write=False)
        self.res, _ = orc.encode_lf_group(self.img)
        h, w, _ = self.img.shape
        self.width, self.height = w, h
        res, g = self.res, self.g
        _, _, _, _, gbw, gbh = group_geometry(w, h, g)
        # every block of the banded group outside the band is black for the coder: no non-zero coefficient in any channel
        nz = res.nz[g, :gbw * gbh].reshape(gbh, gbw, 3)
        s0, s1 = self.y0 // 8, -(-self.y1 // 8)
        outside = np.ones(gbh, bool)
        outside[s0:s1] = False
        self.black_confirmed = not nz[outside].any()
        self.black_blocks = int(outside.sum()) * gbw
        self.n = int(res.group_symbols[g])
        self.B = len(res.stream)
        self.parts = {pl: [part_counts(res, w, h, k, pl) for k in range(res.num_groups)] for pl in PLOGS}
        ps0, ps1 = part_strips(gbh, plog, self.part)
        assert (ps0, ps1) == (s0, s1) or (ps0 <= s0 and s1 <= ps1)
        self.blocks_outside_part = (gbh - (ps1 - ps0)) * gbw
        self.p = self.n - 3 * self.blocks_outside_part

    def largest_part(self, plog):
        return max(max(c) for c in self.parts[plog])

    def largest_group(self):
        return int(self.res.group_symbols.max())


@functools.lru_cache(maxsize=None)
def case(frame, plog):
    seed = SEEDS[(frame, plog)]
    assert seed is not None, f"no seed recorded for {frame} under plog {plog}"
    return Case(frame, plog, seed)


def search_seed(frame, plog, start=1, tries=400):
    """First seed >= start at which the variant's equality holds (how SEEDS was filled)."""
    what, mod = EQUALITY[frame.split("_")[1]]
    for seed in range(start, start + tries):
        c = Case(frame, plog, seed)
        if getattr(c, what) % mod == 0 and c.black_confirmed:
            return seed
    raise LookupError(f"{frame}: no seed in [{start}, {start + tries})")


# ---- what each child of tests/test_gpu_buffer_edges.py visits -------------------------------------------------------------
MODES = {                       # child -> (environment, plog of the transform launches it makes)
    "plog2": ({}, 2),
    "plog1": ({"HYDAMD_K1_SPLIT_LOG": "1"}, 1),
    "unsplit": ({"HYDAMD_K1_SPLIT": "0"}, 0),
}
FRAMES = {
    "plog2": ["A", "A_p16", "B", "C", "C_p16", "D", "E"],
    "plog1": ["A", "A_p32", "B", "C", "C_p32", "D", "E"],
    "unsplit": ["A", "A_n16", "B", "C", "C_n16", "D", "E"],
}
FORMS = (4, 5)


def band_plog(mode):
    return MODES[mode][1] or 2


DEFAULT_TOKEN_CAP = 98304      # HYDK_DEFAULT_TOKEN_CAP: what a context has when only HYDAMD_PAYLOAD_CAP is set
DEFAULT_PAYLOAD_CAP = 2048 * 2048   # of a one-slot context


def plan(mode, c):
    """[(name, token cap or None, payload cap or None, expected reruns as (low, high))] for case c in child `mode`.
    Every figure comes from the oracle's numbers in c.  The payload rows leave the token arrays at their default, which
    holds these groups whole but not their parts: they run in the unsplit child."""
    plog = MODES[mode][1]
    any_number = 1 << 30
    if plog == 0:
        exact = r16(c.n)
        short = exact - 16
    else:
        unit = r16 if plog == 2 else r32
        exact = (1 << plog) * unit(c.p)
        short = exact - 64
    runs = [("tokens_exact", exact, None, (0, 0)),
            ("tokens_short", short, None, (1, any_number)),
            ("tokens_and_payload_exact", exact, c.B, (0, 0))]
    if plog == 2:
        odd = r16(c.n)
        while odd % 64 != 16:
            odd += 16
        runs.append(("tokens_16_mod_64", odd, None, (0, 0)))
    if plog == 0:
        runs += [("payload_exact", None, c.B, (0, 0)), ("payload_short", None, c.B - 1, (1, 1))]
    return runs


def fits(res, width, height, mode, tok_cap, pay_cap):
    """Whether a frame with oracle result `res` fits a context of these caps in child `mode` (None: the default)."""
    plog = MODES[mode][1]
    tok_cap = DEFAULT_TOKEN_CAP if tok_cap is None else tok_cap
    pay_cap = DEFAULT_PAYLOAD_CAP if pay_cap is None else pay_cap
    if plog and tok_cap % 64 == 0:
        need = max(max(part_counts(res, width, height, k, plog)) for k in range(res.num_groups))
        room = tok_cap >> plog
    else:
        need, room = int(res.group_symbols.max()), tok_cap
    return need <= room and len(res.stream) <= pay_cap


def preconditions(mode, c):
    """Why plan()'s expectations hold for c, each from the oracle; returns the list of those that do not."""
    plog = MODES[mode][1]
    bad = []
    if not c.black_confirmed:
        bad.append("a block outside the band has non-zero coefficients")
    for pl in PLOGS:
        for k, counts in enumerate(c.parts[pl]):
            if sum(counts) != int(c.res.group_symbols[k]):
                bad.append(f"parts of group {k} under plog {pl} do not sum to the group")
    if c.largest_group() != c.n:
        bad.append("the banded group is not the frame's largest")
    for name, tok, pay, _ in plan(mode, c):
        if tok is not None and not 16 <= tok <= TOKENS_PER_GROUP - (16 if name == "tokens_short" else 0):
            bad.append(f"{name}: token cap {tok} is outside what the context accepts")
        if tok is not None and tok % 16:
            bad.append(f"{name}: token cap {tok} would be masked")
    if plog == 0:
        if c.n > DEFAULT_TOKEN_CAP:
            bad.append("the payload rows would overflow the default token arrays")
        if c.B > DEFAULT_PAYLOAD_CAP:
            bad.append("the frame outgrows the default payload")
        return bad
    if c.parts[plog][c.g][c.part] != c.p:
        bad.append(f"p from the black-block count ({c.p}) differs from the symbol stream's ({c.parts[plog][c.g][c.part]})")
    if c.largest_part(plog) != c.p:
        bad.append("the band's part is not the frame's largest part")
    tokens = {name: tok for name, tok, _, _ in plan(mode, c)}
    room, step = tokens["tokens_exact"] >> plog, 64 >> plog   # a part's records, and what the short cap takes from them
    if not room - step < c.p <= room:
        bad.append(f"room {room} is not the exact fit of p {c.p}")
    if tokens["tokens_exact"] % 64 or tokens["tokens_short"] % 64:
        bad.append("a cap of the split cases is no multiple of 64: the launch would not be split")
    if not c.n <= (1 << plog) * (room - step) <= (1 << plog) * (room - 16):
        bad.append(f"the whole group ({c.n}) outgrows the short cap too: the overflow would not be the part's")
    others = [x for k, counts in enumerate(c.parts[plog]) for q, x in enumerate(counts) if (k, q) != (c.g, c.part)]
    if others and max(others) > room - step:
        bad.append("another part overflows the short cap as well")
    if plog == 2 and tokens["tokens_16_mod_64"] < c.n:
        bad.append("the unsplit cap inside the split process is too small")
    return bad


# ---- the two runs through the drop-in API (plog 2 child): (name, frame, which token cap of plan(), payload cap) -------------
API_RUNS = [("api_A_exact", "A", "tokens_exact", 0), ("api_C_short", "C", "tokens_short", -1)]


def api_caps(name):
    _, frame, which, dpay = next(r for r in API_RUNS if r[0] == name)
    c = case(frame, 2)
    tok = next(t for n, t, _, _ in plan("plog2", c) if n == which)
    return c, tok, c.B + dpay


# ---- the child: python tests/edge_frames.py MODE REPORT -------------------------------------------------------------------
def _torch_image(img):
    import torch

    if img.dtype == np.uint16:
        return torch.from_numpy(img.view(np.int16).copy()).cuda()
    return torch.from_numpy(np.ascontiguousarray(img)).cuda()


def _set_caps(tok, pay):
    for name, v in (("HYDAMD_TOKEN_CAP", tok), ("HYDAMD_PAYLOAD_CAP", pay)):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)


def child(mode, report_path):
    """Run every frame of FRAMES[mode] at every cap of plan() under forms 4 and 5; the process was started with MODES[mode]'s
    environment.  Writes what the device answered, and how it compares with the oracle, after every run; prints the run's
    name BEFORE its context exists, so that the output of a process that dies names the boundary."""
    import hashlib
    import json

    from hydrium_amd import api, device

    report = {"mode": mode, "runs": {}, "api": {}}

    def write():
        with open(report_path, "w") as f:
            json.dump(report, f)

    def compare(ctx, res):
        bits, _ = ctx.read_sections(0)
        payload = ctx.read_payload()
        return {"payload_ok": payload == res.stream, "payload_md5": hashlib.md5(payload).hexdigest(),
                "counts_ok": bool(np.array_equal(ctx.read_symbol_counts(0)[:res.num_groups], res.group_symbols)),
                "bits_ok": bool(np.array_equal(bits[:res.num_groups], res.group_bits)),
                "reruns": ctx.overflow_reruns(), "token_capacity": ctx.token_capacity()}

    for frame in FRAMES[mode]:
        c = case(frame, band_plog(mode))
        assert not preconditions(mode, c), preconditions(mode, c)
        other = second_image(c.img)
        other_res, _ = orc.encode_lf_group(other)
        t_first, t_other = _torch_image(c.img), _torch_image(other)
        for name, tok, pay, _ in plan(mode, c):
            for form in FORMS:
                key = f"{frame}/{name}/form{form}"
                print(f"CASE {mode}/{key}: n {c.n} p {c.p} B {c.B} HYDAMD_TOKEN_CAP {tok} HYDAMD_PAYLOAD_CAP {pay}", flush=True)
                _set_caps(tok, pay)
                with device.DeviceContext(0, 1, 0) as ctx:
                    ctx.set_rans_waves(form)
                    out = {}
                    for step, t, res in (("first", t_first, c.res), ("second", t_other, other_res), ("again", t_first, c.res)):
                        ctx.encode_image_tensor(t)
                        ctx.sync()
                        out[step] = compare(ctx, res)
                report["runs"][key] = out
                write()
    if mode == "plog2":
        lib = api.Library()
        for name, *_ in API_RUNS:
            c, tok, pay = api_caps(name)
            for form in FORMS:
                print(f"CASE {mode}/{name}/form{form}: HYDAMD_TOKEN_CAP {tok} HYDAMD_PAYLOAD_CAP {pay}", flush=True)
                _set_caps(tok, pay)
                os.environ["HYDAMD_RANS_WAVES"] = str(form)
                lib.dll.hydamd_trim_cache()   # parked contexts keep the caps they were created with
                files = [bytes(api.encode_image(lib, c.img.copy(), out_buf_size=1 << 22)) for _ in range(2)]
                report["api"][f"{name}/form{form}"] = [hashlib.md5(f).hexdigest() for f in files]
                write()
        lib.dll.hydamd_trim_cache()
    report["done"] = True
    write()
    return 0


if __name__ == "__main__":
    import sys

    sys.exit(child(sys.argv[1], sys.argv[2]))
