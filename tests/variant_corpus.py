"""The corpus every build variant and run-time A/B setting is held to the reference with (tests/test_gpu_variants.py).

Two halves:
  * edge images the synthetic kinds of hydrium_amd/synth.py never produce: 8x8 blocks that each hold the sign pattern of one
    DCT basis function at full amplitude (the integer path's largest tokens: 28 and |q| up to 544 on 16-bit grey, where the
    photo / noise / ramp kinds stop at 21 / 23 / 26), saturated primaries in alternating blocks (LF residual extremes), and
    16-bit samples at 0 / 1 / 65534 / 65535 and around the transfer curve's branch point 2650;
  * the case list and the child that runs it: ``python tests/variant_corpus.py CORPUS_DIR REPORT`` loads whatever library
    HYDAMD_LIB names, proves from /proc/self/maps that it is the one mapped, runs every case and writes a JSON report.
    The expected MD5s are computed by the parent (from the compiled reference) and read from CORPUS_DIR/spec.json.
"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

EDGE_KINDS = ("basis_grey", "basis_rg", "basis_by", "primaries", "extremes16")


def _basis_signs(width, height):
    """+1 / -1 per pixel: block (bx, by) holds the sign pattern of DCT basis (u, v) = ((bx + 3 by) % 8, by % 8): every run of
    eight blocks in a row holds the eight horizontal frequencies of one vertical one, every 8x8 blocks all 64."""
    x = np.arange(width)
    y = np.arange(height)
    bx, by = x // 8, y // 8
    u = (bx[None, :] + 3 * by[:, None]) % 8
    v = np.broadcast_to((by % 8)[:, None], u.shape)
    cx = np.cos((2 * (x % 8)[None, :] + 1) * u * np.pi / 16)
    cy = np.cos((2 * (y % 8)[:, None] + 1) * v * np.pi / 16)
    return np.where(cx * cy >= 0, 1, -1)


def edge_image(kind: str, width: int, height: int, depth: int = 16) -> np.ndarray:
    """(height, width, 3) uint8 / uint16 edge content (see the module docstring)."""
    top = 255 if depth == 8 else 65535
    dt = np.uint8 if depth == 8 else np.uint16
    if kind.startswith("basis_"):
        hi = _basis_signs(width, height) > 0
        p = np.where(hi, top, 0)
        q = top - p
        if kind == "basis_grey":
            ch = (p, p, p)
        elif kind == "basis_rg":          # red against green: the X channel's extreme
            ch = (p, q, np.zeros_like(p))
        elif kind == "basis_by":          # blue against yellow: B - Y's extreme
            ch = (q, q, p)
        else:
            raise ValueError(kind)
        return np.ascontiguousarray(np.stack(ch, axis=-1).astype(dt))
    if kind == "primaries":
        # the eight corners of the RGB cube in alternating 8x8 blocks: neighbouring LF samples as far apart as they get
        corners = np.array([[1, 0, 0], [0, 1, 1], [0, 1, 0], [1, 0, 1], [0, 0, 1], [1, 1, 0], [0, 0, 0], [1, 1, 1]])
        bx = np.arange(width)[None, :] // 8
        by = np.arange(height)[:, None] // 8
        idx = (bx + 5 * by + (bx * by) % 3) % 8
        return np.ascontiguousarray((corners[idx] * top).astype(dt))
    if kind == "extremes16":
        assert depth == 16
        vals = np.array([0, 1, 65534, 65535] + list(range(2640, 2662)), np.uint16)  # 2650.9 = 0.04045 * 65535
        rng = np.random.default_rng(2650)
        img = vals[rng.integers(0, len(vals), size=(height, width, 3))]
        img[: height // 2, : width // 2] = vals[(np.arange(width // 2)[None, :, None] + np.arange(height // 2)[:, None, None]
                                                 + np.arange(3)[None, None, :]) % len(vals)]
        return np.ascontiguousarray(img)
    raise ValueError(f"unknown edge kind {kind!r}")


def image(kind: str, width: int, height: int, depth: int = 8) -> np.ndarray:
    """A synthetic kind (hydrium_amd/synth.py), an edge kind, "dark16" (16-bit photo content shifted to the transfer curve's
    lower branch, every third row black) or "float" (make_image_f32's photo in [0, 1])."""
    from hydrium_amd import synth

    if kind in EDGE_KINDS:
        return edge_image(kind, width, height, depth)
    if kind == "dark16":
        img = (synth.make_image("photo", width, height, 16) >> 4).astype(np.uint16)
        img[::3] = 0
        return np.ascontiguousarray(img)
    if kind == "float":
        return synth.make_image_f32("photo", width, height)
    return synth.make_image(kind, width, height, depth)


# ---- the cases ---------------------------------------------------------------------------------------------------------
# whole files through hyd_send_tile: (name, kind, width, height, depth, shift); each runs under entropy-stage forms 4 and 5
FILE_IMAGES = [
    ("photo_1x1", "photo", 1, 1, 8, -1),
    ("photo_8x8", "photo", 8, 8, 8, -1),
    ("noise_257x255", "noise", 257, 255, 8, -1),
    ("photo_2049x130", "photo", 2049, 130, 8, -1),
    ("dark16_300x200", "dark16", 300, 200, 16, -1),
    ("float_300x200", "float", 300, 200, 32, -1),
    ("basis_grey16_256", "basis_grey", 256, 256, 16, -1),
    ("basis_grey8_256", "basis_grey", 256, 256, 8, -1),
    ("basis_rg16_200x136", "basis_rg", 200, 136, 16, -1),
    ("basis_by8_136x200", "basis_by", 136, 200, 8, -1),
    ("primaries16_264x200", "primaries", 264, 200, 16, -1),
    ("primaries8_264x200", "primaries", 264, 200, 8, -1),
    ("extremes16_300x260", "extremes16", 300, 260, 16, -1),
    ("tiles_photo_600x520_s0", "photo", 600, 520, 8, 0),        # tile mode: one frame per 256x256 tile, split transform launches
    ("lf2x2_smooth_2100x2060", "smooth", 2100, 2060, 8, -1),    # 2x2 LF groups: the device-side assembler
]
FORMS = (4, 5)
# stage-level cases against the CPU oracle: (name, kind, width, height, depth); each under xyb modes 0 and 2
STAGE_IMAGES = [
    ("photo_256", "photo", 256, 256, 8),
    ("basis_grey16_256", "basis_grey", 256, 256, 16),
]
XYB_MODES = (0, 2)
# the four clustering schemes (9 / 3 / 2 / 1 clusters per preset), by the frame header's preset count
CLUSTER_PRESETS = (28, 29, 86, 129)
# the overflow rerun: caps small enough that a noise frame outgrows them
OVERFLOW = ("overflow_noise_520x300", "noise", 520, 300, 8)
DEVICE_FRAME = ("device_photo_4096", "photo", 4096, 4096, 8)


def golden_entries():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return [e for e in json.load(f)["files"] if e["width"] * e["height"] <= 4096 * 4096]


def golden_name(e):
    return f"golden_{e['kind']}_{e['width']}x{e['height']}_u{e['depth']}_s{e['shift']}"


def _file_kw(shift):
    return {} if shift < 0 else dict(shift_x=shift, shift_y=shift)


def case_names():
    """Every case a child reports, in order: the parent checks the count."""
    names = []
    for n, *_ in STAGE_IMAGES:
        names += [f"stage_{n}_xyb{m}" for m in XYB_MODES]
    names += [f"clusters_{p}_form{f}" for p in CLUSTER_PRESETS for f in FORMS]
    names += [f"file_{n}_form{f}" for n, *_ in FILE_IMAGES for f in FORMS]
    names += [OVERFLOW[0], DEVICE_FRAME[0]]
    names += [golden_name(e) for e in golden_entries()]
    return names


def prepare(corpus_dir, ref_lib):
    """Parent side: write every image the children need and the expected MD5s (reference for the files, the golden
    manifest for its own entries and the 4096^2 device frame)."""
    from hydrium_amd import api, synth

    os.makedirs(corpus_dir, exist_ok=True)
    expect = {}
    paths = {}

    def save(key, img):
        p = os.path.join(corpus_dir, key + ".npy")
        np.save(p, img)
        paths[key] = p

    for n, kind, w, h, d in STAGE_IMAGES:
        save("stage_" + n, image(kind, w, h, d))
    for n, kind, w, h, d, shift in FILE_IMAGES:
        img = image(kind, w, h, d)
        save("file_" + n, img)
        md5 = hashlib.md5(bytes(api.encode_image(ref_lib, img, out_buf_size=1 << 22, **_file_kw(shift)))).hexdigest()
        for f in FORMS:
            expect[f"file_{n}_form{f}"] = md5
    n, kind, w, h, d = OVERFLOW
    img = image(kind, w, h, d)
    save(n, img)
    expect[n] = hashlib.md5(bytes(api.encode_image(ref_lib, img, out_buf_size=1 << 22))).hexdigest()
    golden = golden_entries()
    # synth's kinds are functions of the pixel position, and 8-bit samples are the 16-bit ones >> 8: every photo entry is a
    # crop of ONE 16-bit photo (generating each took a minute)
    side = max(max(e["width"], e["height"]) for e in golden if e["kind"] == "photo")
    photo = synth.make_image("photo", side, side, 16)

    def golden_image(e):
        if e["kind"] != "photo":
            return synth.make_image(e["kind"], e["width"], e["height"], e["depth"])
        crop = photo[:e["height"], :e["width"]]
        return np.ascontiguousarray(crop if e["depth"] == 16 else (crop >> 8).astype(np.uint8))

    probe = {"kind": "photo", "width": 67, "height": 45, "depth": 8}
    assert np.array_equal(golden_image(probe), synth.make_image("photo", 67, 45, 8)), "synth is no longer crop-consistent"
    for e in golden:
        save(golden_name(e), golden_image(e))
        expect[golden_name(e)] = e["md5"]
    n, kind, w, h, d = DEVICE_FRAME
    dev = [e for e in golden if (e["kind"], e["width"], e["height"], e["depth"], e["shift"]) == (kind, w, h, d, -1)]
    assert len(dev) == 1, "the golden manifest lost its 4096^2 photo"
    expect[n] = dev[0]["md5"]
    paths[n] = paths[golden_name(dev[0])]
    spec = {"expect": expect, "paths": paths, "cases": case_names()}
    with open(os.path.join(corpus_dir, "spec.json"), "w") as f:
        json.dump(spec, f)
    return spec


# ---- the child ---------------------------------------------------------------------------------------------------------
def mapped_libraries():
    """Every file named libhydrium* mapped into this process."""
    seen = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 6 and os.path.basename(parts[5]).startswith("libhydrium"):
                seen.add(os.path.realpath(parts[5]))
    return sorted(seen)


def _torch_image(img):
    import torch

    if img.dtype == np.uint16:
        return torch.from_numpy(img.view(np.int16).copy()).cuda()
    return torch.from_numpy(np.ascontiguousarray(img)).cuda()


def _tokens_of(ctx, slot, res):
    """The device's token records of one LF group against the oracle's; returns the largest token."""
    from hydrium_amd import device

    counts = ctx.read_symbol_counts(slot)
    assert np.array_equal(counts[:res.num_groups], res.group_symbols), "symbol counts"
    first, top = 0, 0
    for g in range(res.num_groups):
        n = int(res.group_symbols[g])
        tok, cl, rb, resid = device.decode_token_records(ctx.read_tokens(slot, g, n))
        ref = res.symbols[first:first + n]
        assert np.array_equal(tok, ref["token"]), f"group {g} tokens"
        assert np.array_equal(cl + res.cluster_from, ref["cluster"]), f"group {g} clusters"
        assert np.array_equal(rb, ref["residue_bits"]), f"group {g} residue bits"
        assert np.array_equal(resid, ref["residue"]), f"group {g} residues"
        top = max(top, int(tok.max()) if n else 0)
        first += n
    freq, alpha, log_alpha, run_max = ctx.read_tables(slot)
    ncl = res.cluster_to - res.cluster_from
    assert np.array_equal(alpha[:ncl], res.alphabet_size[res.cluster_from:res.cluster_to]), "alphabet sizes"
    assert np.array_equal(freq[:ncl], res.freqs[res.cluster_from:res.cluster_to]), "frequencies"
    assert (log_alpha, run_max) == (res.log_alphabet_size, res.max_alphabet_size), "alphabet maxima"
    assert np.array_equal(ctx.read_dc(slot, res.vbw, res.vbh), res.dc), "LF ints"
    return top


def _stage_case(img, xyb_mode):
    from hydrium_amd import device
    from oracle import binding as orc

    res, _ = orc.encode_lf_group(img)
    with device.DeviceContext(0, 1, 0, debug_planes=True) as ctx:
        ctx.set_xyb_mode(xyb_mode)
        ctx.encode_image_tensor(_torch_image(img))
        ctx.sync()
        rows, pitch = res.vbh * 8, res.stride
        assert np.array_equal(ctx.read_debug_plane(0, pitch, rows).view(np.uint32), res.xyb.view(np.uint32)), "XYB planes"
        assert np.array_equal(ctx.read_debug_plane(1, pitch, rows), res.dct), "DCT planes"
        assert np.array_equal(ctx.read_debug_plane(2, pitch, rows), res.quant), "quantised planes"
        top = _tokens_of(ctx, 0, res)
        bits, offs = ctx.read_sections(0)
        assert np.array_equal(bits[:res.num_groups], res.group_bits), "section bits"
        assert np.array_equal(offs[:res.num_groups], res.group_offset), "section offsets"
        payload = ctx.read_payload()
        assert payload == res.stream, "sections"
    return hashlib.md5(payload).hexdigest(), top


def _cluster_case(num_presets, form):
    """As tests/test_gpu_device_parity.py::test_every_cluster_scheme_on_the_device: three small LF groups under scattered
    preset ids of a frame header of `num_presets` presets, against the oracle with the running alphabet in send order."""
    from hydrium_amd import device, synth
    from oracle import binding as orc

    imgs = [synth.make_image("photo", 300, 200, 8, 7), synth.make_image("noise", 72, 40, 8, 8),
            synth.make_image("smooth", 520, 264, 16, 9)]
    presets = [0, num_presets // 2, num_presets - 1]
    top = 0
    with device.DeviceContext(0, 3, 0) as ctx:
        ctx.set_rans_waves(form)
        ctx.begin_frame(num_presets)
        keep = []
        for slot, (img, p) in enumerate(zip(imgs, presets)):
            t = _torch_image(img)
            keep.append(t)
            isz = t.element_size()
            h, w, _ = img.shape
            base = t.data_ptr()
            ctx.encode_lf_group(slot, [base, base + isz, base + 2 * isz], 3 * w, 3, {1: 0, 2: 1}[isz], w, h, p)
        ctx.finish_frame(3)
        ctx.sync()
        payload = ctx.read_payload()
        running, at = 0, 0
        for slot, (img, p) in enumerate(zip(imgs, presets)):
            res, running = orc.encode_lf_group(np.ascontiguousarray(img), num_presets=num_presets, preset=p,
                                               max_alphabet_size=running)
            top = max(top, _tokens_of(ctx, slot, res))
            bits, offs = ctx.read_sections(slot)
            assert np.array_equal(bits[:res.num_groups], res.group_bits), f"section bits of slot {slot}"
            assert int(offs[0]) == at and payload[at:at + len(res.stream)] == res.stream, f"sections of slot {slot}"
            at += len(res.stream)
        assert at == len(payload)
    return hashlib.md5(payload).hexdigest(), top


def _with_env(lib, env, fn):
    """Run fn() with `env` set for the contexts it creates (parked contexts keep what they were created with)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    lib.dll.hydamd_trim_cache()
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.dll.hydamd_trim_cache()


def child(corpus_dir, report_path):
    want = os.path.realpath(os.environ["HYDAMD_LIB"])
    from hydrium_amd import api, multigpu

    with open(os.path.join(corpus_dir, "spec.json")) as f:
        spec = json.load(f)
    lib = api.Library()
    maps = mapped_libraries()
    report = {"lib": want, "mapped": maps, "cases": []}

    def write():
        with open(report_path, "w") as f:
            json.dump(report, f)

    if maps != [want]:
        report["error"] = f"mapped {maps}, asked for {want}"
        write()
        return 2
    load = lambda key: np.load(spec["paths"][key], mmap_mode="r")  # noqa: E731
    jobs = []
    for n, *_ in STAGE_IMAGES:
        for m in XYB_MODES:
            jobs.append((f"stage_{n}_xyb{m}", lambda n=n, m=m: _stage_case(np.ascontiguousarray(load("stage_" + n)), m)))
    for p in CLUSTER_PRESETS:
        for fm in FORMS:
            jobs.append((f"clusters_{p}_form{fm}", lambda p=p, fm=fm: _cluster_case(p, fm)))
    for n, kind, w, h, d, shift in FILE_IMAGES:
        for fm in FORMS:
            def run(n=n, shift=shift, fm=fm):
                img = np.ascontiguousarray(load("file_" + n))
                data = _with_env(lib, {"HYDAMD_RANS_WAVES": str(fm)},
                                 lambda: bytes(api.encode_image(lib, img, out_buf_size=1 << 22, **_file_kw(shift))))
                return hashlib.md5(data).hexdigest(), None
            jobs.append((f"file_{n}_form{fm}", run))

    def overflow():
        img = np.ascontiguousarray(load(OVERFLOW[0]))
        data = _with_env(lib, {"HYDAMD_TOKEN_CAP": "4096", "HYDAMD_PAYLOAD_CAP": "65536"},
                         lambda: bytes(api.encode_image(lib, img, out_buf_size=1 << 22)))
        return hashlib.md5(data).hexdigest(), None
    jobs.append((OVERFLOW[0], overflow))

    def device_frame():
        import torch

        t = torch.from_numpy(np.ascontiguousarray(load(DEVICE_FRAME[0]))).cuda()
        return hashlib.md5(multigpu.encode_serial(t, 1)).hexdigest(), None
    jobs.append((DEVICE_FRAME[0], device_frame))
    for e in golden_entries():
        def gold(e=e):
            img = np.ascontiguousarray(load(golden_name(e)))
            return hashlib.md5(bytes(api.encode_image(lib, img, out_buf_size=1 << 23, **_file_kw(e["shift"])))).hexdigest(), None
        jobs.append((golden_name(e), gold))
    assert [n for n, _ in jobs] == spec["cases"], "child and parent disagree on the corpus"
    for name, fn in jobs:
        t0 = time.time()
        try:
            md5, top = fn()
        except Exception as ex:  # noqa: BLE001 - recorded, and nothing runs after it
            report["cases"].append({"case": name, "ok": False, "error": f"{type(ex).__name__}: {ex}"})
            write()
            return 1
        exp = spec["expect"].get(name)
        report["cases"].append({"case": name, "md5": md5, "ok": exp is None or md5 == exp, "token_max": top,
                                "ms": round(1e3 * (time.time() - t0), 1)})
    report["mapped_after"] = mapped_libraries()
    write()
    return 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.exit(child(sys.argv[1], sys.argv[2]))
