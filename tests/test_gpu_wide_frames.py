"""GPU: launch groups of up to 255 slots — the number every object of the library is built around — on every path, against
the CPU oracle stage by stage and the compiled reference file by file.  Byte equality throughout; no tolerances.

What runs here and nowhere else on a device: frames of 85 ... 255 LF groups (the cluster map's schemes around 86 and 128
presets, the second and later turns of the strided sums over the slots in front, k_rans_emit<true> with thousands of groups
and empty places in front of a wavefront, the serial running alphabet maximum over 255 words, the TOC permutation and
HFGlobal of 255 presets in k_asm_prepare), batches of 255 one-group frames (2040 pieces: the copy kernel's full piece
array), of 127 x 2 and 51 x 5 LF groups, 255 images of 255 sizes, the planner's largest mixed batch (nine strips of 28 LF
groups and one of 3), a wave-form launch group of 255 slots, and 255 tiles in one launch group.

The pictures are strips 8 pixels high (tests/wide_frames.py); tests/test_wide_frames.py shows on the CPU that they hold what
these tests rest on.  A context of 255 slots at default sizes holds about 12 GB, so every test sets HYDAMD_TOKEN_CAP to 8192
records per group (no group here has more than 6144 symbols) and asserts that nothing was rerun: a rerun could hide a
misplaced write of the first pass."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import wide_frames as wf
from conftest import has_gpu, reference_expected
from hydrium_amd import api
from test_gpu_image_status import _check_outcomes
from test_gpu_mixed_batch import _check, _check_on_device

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

OUT_BUF = 8 << 20
STRIPS = [pytest.param(n, v, id=f"{n}{'v' if v else 'h'}") for n, v in wf.ONE_FRAME_STRIPS]
_cache = {}


@pytest.fixture(autouse=True)
def small_token_arrays(monkeypatch):
    """HYDAMD_TOKEN_CAP is read when a context is created; the drop-in API parks contexts, which keep the caps they were
    created with, so its cache is emptied on both sides of a test"""
    lib = api.Library()
    lib.dll.hydamd_trim_cache()
    monkeypatch.setenv("HYDAMD_TOKEN_CAP", str(wf.TOKEN_CAP))
    yield
    lib.dll.hydamd_trim_cache()


def _cuda(img):
    import torch

    return torch.from_numpy(np.array(img)).cuda()  # (a copy: the pictures of wide_frames are read-only)


def _md5(b):
    return hashlib.md5(bytes(b)).hexdigest()


def _reference(key, img, **kw):
    """the reference's file for one picture; made once per key and never changed"""
    from oracle import refprobe

    assert reference_expected()
    if "out" not in _cache:
        _cache["out"] = (C.c_uint8 * OUT_BUF)()
    if key not in _cache:
        _cache[key] = bytes(api.encode_image(refprobe.reference_library(optimised=True), np.ascontiguousarray(img), out_buf=_cache["out"], **kw))
    return _cache[key]


def _references(key, pics):
    if key not in _cache:
        _cache[key] = [_reference((key, k), p) for k, p in enumerate(pics)]
    return _cache[key]


# ---- one frame of n LF groups, stage by stage ------------------------------------------------------------------------------
def _check_frame(ctx, n, vertical, where):
    slots = wf.strip_slots(n, vertical)
    payload, bits, offs = wf.frame_sections(slots)
    for s, want in enumerate(slots):
        _, _, log_alpha, run_max = ctx.read_tables(s)
        assert (log_alpha, run_max) == (want.log_alphabet, want.running_max), f"{where}: slot {s}: running alphabet maximum"
        got_bits, got_offs = ctx.read_sections(s)
        sl = slice(s * wf.GROUPS_PER_LFG, (s + 1) * wf.GROUPS_PER_LFG)
        assert np.array_equal(got_bits, bits[sl]), f"{where}: slot {s}: section bits (0 for the empty places)"
        assert np.array_equal(got_offs, offs[sl]), f"{where}: slot {s}: offsets[], empty places included"
    assert ctx.payload_size() == len(payload), f"{where}: total"
    got = ctx.read_payload()
    assert len(got) == len(payload) and got == payload, f"{where}: payload {_md5(got)}, the oracle's {_md5(payload)}"
    # the packed LF area: every slot starts at the 4-byte-aligned end of the slot before
    info, blob = ctx.read_lf_streams(n), ctx.read_lf_payload().copy()
    end, at = 0, {}
    for s in range(n):
        assert int(info["error"][s]) == 0, f"{where}: slot {s}: LF coder error"
        off, nbits = int(info["offset"][s]), int(info["bit_count"][s])
        assert off == end, f"{where}: slot {s} starts at {off}, the slots before it end at {end}"
        at[s] = (off, nbits)
        end = off + (nbits + 31) // 32 * 4
    assert end == ctx.lf_payload_size() == len(blob), f"{where}: the LF payload is {len(blob)} bytes, the slots end at {end}"
    for s in wf.model_slots(n):
        want_bits, want_nbits = wf.lf_stream(n, vertical, s)
        off, nbits = at[s]
        assert nbits == want_nbits, f"{where}: slot {s}: LF bit count"
        nbytes = (nbits + 7) // 8
        assert np.array_equal(blob[off:off + nbytes], want_bits), f"{where}: slot {s}: LF stream differs from the model"
        assert not blob[off + nbytes:off + (nbits + 31) // 32 * 4].any(), f"{where}: slot {s}: bytes behind the stream's end"


@pytest.mark.parametrize("n,vertical", STRIPS)
def test_one_frame_stage_by_stage(n, vertical):
    """In ONE context of 255 slots, for the lane form (six launches: self-placing emit, LF pack riding) and the wave form (scan
    kernel, late LF coder, gather): another frame of 255 LF groups first, then this strip twice — its slots, and the slots
    behind its last one, hold the other frame's words."""
    from hydrium_amd import device

    t = _cuda(wf.strip(n, vertical))
    other = _cuda(wf.strip(255, vertical if n < 255 else not vertical))
    with device.DeviceContext(0, wf.MAX_SLOTS, 0) as ctx:
        ctx.set_lf_coder(2)
        for form in (5, 4):
            ctx.set_rans_waves(form)
            ctx.encode_image_tensor(other)
            ctx.sync()
            for visit in range(2):
                ctx.encode_image_tensor(t)
                ctx.sync()
                _check_frame(ctx, n, vertical, f"form {form}, visit {visit}")
        print(f"  {n} slots, {64 * n} places, {ctx.payload_size()} section bytes, {ctx.lf_payload_size()} LF bytes")
        assert ctx.overflow_reruns() == 0


# ---- one frame of n LF groups, whole files ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,vertical", STRIPS)
def test_whole_file_by_every_route(n, vertical):
    import torch
    from hydrium_amd import device

    img = wf.strip(n, vertical)
    want = _reference(("strip", n, vertical), img)
    h, w, _ = img.shape
    md = api.HYDImageMetadata(w, h, 0, -1, -1)
    t = _cuda(img)
    with device.DeviceContext(0, n, 0) as ctx, device.Assembler(0) as asm:
        ctx.encode_image_tensor(t)
        full = torch.zeros(ctx.blob_bound(n), dtype=torch.uint8, device="cuda")
        ctx.export_frame(n, full)
        ptr, cap = ctx.export_frame_owned(n)
        out = torch.full((len(want) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        asm.plan(md, [list(range(n))])
        asm.run([ptr], [cap], out.data_ptr(), out.numel(), ctx.get_stream())
        ctx.sync()
        assert ctx.overflow_reruns() == 0
        size = asm.result()
        on_device = bytes(out[:size].cpu().numpy())
        assert bool((out[size:size + 64].cpu() == 0x5A).all()), "the assembler wrote past the frame's end"
        head = device.blob_header(full[:64].cpu().numpy().tobytes())
        assert int(head["status"]) == 0 and int(head["num_slots"]) == n
        blob = full[: int(head["total_bytes"])].cpu().numpy().tobytes()
    del full
    assert (len(on_device), _md5(on_device)) == (len(want), _md5(want)), "device.Assembler (k_asm_prepare + k_pieces_copy)"
    on_host = device.frame_from_blobs(md, [blob])
    assert (len(on_host), _md5(on_host)) == (len(want), _md5(want)), "export_frame + frame_from_blobs"
    with device.FrameBatch(w, h, 1) as fb:
        fb.encode([t])
        _check_on_device(fb, [want])
        assert fb.overflow_reruns() == 0
    got = bytes(api.encode_image(api.Library(), np.array(img), out_buf_size=OUT_BUF))
    assert (len(got), _md5(got)) == (len(want), _md5(want)), f"the drop-in API, {n} tiles sent into one frame"


# ---- batches that fill the context -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,frames", [(256, 8, 255), (33, 9, 255), (2056, 8, 127), (2048 * 4 + 8, 8, 51)],
                         ids=["255x1-single-section", "255x1-ragged", "127x2", "51x5"])
def test_frame_batches_that_fill_the_context(w, h, frames):
    """255 one-group frames: 2040 pieces, the copy kernel's full array.  127 frames of 2 LF groups: 254 slots, 1397 pieces;
    51 of 5: 255 slots.  Two batches through one object, the second with the pictures reversed."""
    from hydrium_amd import device

    pics = wf.graded(w, h, frames)
    wants = _references(("graded", w, h, frames), pics)
    assert len(set(wants)) == frames and len(set(map(len, wants))) > frames // 8, "the files of the batch differ in size"
    imgs = [_cuda(p) for p in pics]
    with device.FrameBatch(w, h, frames) as fb:
        fb.encode(imgs)
        _check_on_device(fb, wants)
        fb.encode(imgs[::-1])
        _check_on_device(fb, wants[::-1])
        assert fb.overflow_reruns() == 0
    n = wf.lf_groups_of(pics[0])
    print(f"  {frames} frames, {frames * n} slots, {frames * (3 * n + 5)} pieces, {sum(map(len, wants))} bytes")


def _mixed():
    pics = wf.mixed_pictures()
    return pics, _references("mixed", pics)


def test_a_mixed_batch_of_255_sizes():
    from hydrium_amd import device

    pics, wants = _mixed()
    assert len(pics) == wf.MAX_SLOTS and len({p.shape for p in pics}) == wf.MAX_SLOTS
    imgs = [_cuda(p) for p in pics]
    with device.MixedBatch(wf.MAX_SLOTS) as mb:
        mb.encode(imgs)
        _check_on_device(mb, wants)
        mb.encode(imgs[::-1])
        _check_on_device(mb, wants[::-1])
        assert mb.overflow_reruns() == 0


def test_the_planners_largest_mixed_batch():
    """Nine strips of 28 LF groups and one of 3 in 255 slots.  The running maximum restarts at each image's first slot: the
    RGB8 strips differ in their final maximum; of the float strips three size their tables above the kernel's floor of 2^5
    from one LF group on, and the strip behind each of them must not (its bytes would change)."""
    from hydrium_amd import device

    with device.MixedBatch(10, max_lf_groups=wf.MAX_SLOTS) as mb:
        for name, pics, pair in (("rgb8", wf.planner_strips(), (0, 8)), ("f32", wf.planner_strips_f32(), (1, 2))):
            final = [wf.oracle_slots(pics[k])[-1].running_max for k in pair]  # (all ten: tests/test_wide_frames.py)
            assert final[0] != final[1], final
            wants = _references(("planner", name), pics)
            imgs = [_cuda(p) for p in pics]
            mb.encode(imgs)
            _check_on_device(mb, wants)
            mb.encode(imgs[::-1])
            _check_on_device(mb, wants[::-1])
        assert mb.overflow_reruns() == 0


def test_a_wave_form_launch_group_of_255_slots_and_one_bad_image():
    """Picture 200 is float16, the rest RGB8: the float picture puts the whole launch group on the wave form (k_scan_sections,
    k_pack_sections, the late LF coder at 255 slots).  With one NaN in it, only image 200 fails."""
    import torch
    from hydrium_amd import device

    pics, wants = _mixed()
    wants = list(wants)
    half = (pics[200].astype(np.float32) / np.float32(255.0)).astype(np.float16)
    wants[200] = _reference("mixed-200-float16", half.astype(np.float32))  # widened exactly on load
    imgs = [_cuda(p) for p in pics]
    imgs[200] = torch.from_numpy(half).cuda()
    bad = list(imgs)
    bad[200] = imgs[200].clone()
    bad[200][0, half.shape[1] // 2, 1] = float("nan")
    torch.cuda.synchronize()
    with device.MixedBatch(wf.MAX_SLOTS, image_errors=True) as mb:
        mb.encode(bad, sample_fmts="each")
        _check_outcomes(mb, wants, {200})
        mb.encode(imgs, sample_fmts="each")
        total = _check_outcomes(mb, wants, set())
        assert mb.overflow_reruns() == 0
    print(f"  255 images, {total} bytes; image 200: {len(wants[200])} bytes from float16")


@pytest.mark.parametrize("transposed", [False, True], ids=["row-of-tiles", "column-of-tiles"])
def test_255_tiles_in_one_launch_group_and_one_behind(transposed):
    """256 tiles of 256 x 8: a launch group of 255 (255 x 8 = 2040 pieces) and one of 1, which starts at the cursor the
    first left"""
    from hydrium_amd import device

    img = wf.tile_strip()
    if transposed:
        img = np.ascontiguousarray(img.transpose(1, 0, 2))
    h, w, _ = img.shape
    want = _reference(("tiles", transposed), img, shift_x=0, shift_y=0)
    with device.TiledImage(w, h, 0, 0, tiles_per_launch=wf.MAX_SLOTS) as ti:
        ti.encode(_cuda(img))
        got = bytes(ti.read())
        assert ti.overflow_reruns() == 0
    assert len(got) == len(want) and got == want, (_md5(got), _md5(want), len(got), len(want))


# ---- one past the limit ------------------------------------------------------------------------------------------------------
def test_refusals_one_past_the_limit():
    from hydrium_amd import device

    with pytest.raises(device.DeviceError, match="must not exceed 255") as e:  # 2 LF groups x 128 frames = 256 slots
        device.FrameBatch(2056, 8, 128)
    assert e.value.code == -14
    with pytest.raises(device.DeviceError, match="tiles_per_launch must be between 0 and 255") as e:
        device.TiledImage(65288, 8, 0, 0, tiles_per_launch=256)
    assert e.value.code == -14
    pics, wants = _mixed()
    imgs = [_cuda(p) for p in pics]
    with device.MixedBatch(wf.MAX_SLOTS) as mb:
        with pytest.raises(device.DeviceError, match="frames must be between 1 and max_frames") as e:
            mb.encode(imgs + imgs[:1])
        assert e.value.code == -14
        with pytest.raises(device.DeviceError, match="no batch in flight"):  # nothing of the refused call was enqueued
            mb.result()
        mb.encode(imgs)
        _check(mb, wants)
        assert mb.overflow_reruns() == 0
    good = wf.frame_sections(wf.strip_slots(86))[0]
    with device.DeviceContext(0, wf.MAX_SLOTS) as ctx:
        for lf_groups, match in ((128, "unsupported number of LF groups"), (256, "too few LF-group slots")):
            t = _cuda(wf.strip_of_width(2048 * (lf_groups - 1) + 8))
            with pytest.raises(device.DeviceError, match=match) as e:
                ctx.encode_image_tensor(t, num_slots_check=False)
            assert e.value.code == -14
            ctx.encode_image_tensor(_cuda(wf.strip(86)))
            ctx.sync()
            assert ctx.read_payload() == good
        assert ctx.overflow_reruns() == 0
