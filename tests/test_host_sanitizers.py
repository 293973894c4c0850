"""CPU: the host glue under the address and undefined-behaviour sanitizers.

The other CPU modules reach csrc/host/ through libhydrium_probe.so, loaded into Python and fed numpy arrays: that shows
the bytes are right, not that the code stays inside its buffers or inside defined C (a read a few bytes past an array lands
in the allocator's slack; a shift by 32, -INT_MIN and a typed load from an odd address give the expected bits on x86).  Here
every hook of csrc/host/*.c is called a second time by a stand-alone program (tests/c/host_replay.c, all of csrc/host built
with -fsanitize=address,undefined -fno-sanitize-recover=undefined) on the inputs those modules use: tests/host_replay.py
records each call made through ctypes — every input buffer with exactly the bytes the hook may read, every output buffer
with exactly its capacity — and the program's return code, error text and output bytes must equal what ctypes gave, with
exit status 0 and nothing on stderr.  Byte streams (blobs, payloads, LF bit streams, ICC profiles) run a second time at an
odd address.  No expected value is new: the ctypes results are what the other modules hold to the reference.

hydt_layout_from_streams and hydt_layout_from_streams_skip have no export: they are replayed through the hooks that call
them (hydt_mixed_from_streams[_skip], hydt_batch_from_streams), and the replay's link counts those calls.

Nothing sanitized is loaded into Python, nothing runs on a GPU.  The second program (tests/c/sample_formats.cc) evaluates
the shared sample-format headers as plain C++ under the same flags and is held to the numpy models.
"""
import contextlib
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from hydrium_amd import api, build as hbuild

import content_corpus as cc
import glue
import host_replay as hr
import lf_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAYED = [h for h in hr.HOOKS if ":" not in h]  # the 25 hooks of csrc/host/*.c and hydamd_frame_from_streams


class _Program:
    pass


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    p = _Program()
    p.dir = str(tmp_path_factory.mktemp("host_sanitizers"))
    t = time.perf_counter()
    p.exe, p.log, p.stubs = hr.build_program(p.dir)
    p.compile_s = time.perf_counter() - t
    p.calls, p.records, p.run_s = {}, {}, 0.0
    yield p
    print(f"\nhost sanitizers: compile {p.compile_s:.1f} s, replay {p.run_s:.1f} s; calls in the replay program:",
          ", ".join(f"{k} {v}" for k, v in sorted(p.calls.items())))


@contextlib.contextmanager
def recording():
    """a Recorder in the place of every library handle the test helpers keep in a module global"""
    rec = hr.Recorder()
    mods = [m for name in ("glue", "lf_model", "tests.glue", "tests.lf_model") if (m := sys.modules.get(name)) is not None]
    saved = [m._d for m in mods]
    for m in mods:
        m._d = rec
    try:
        yield rec
    finally:
        for m, d in zip(mods, saved):
            m._d = d


def hold(program, rec, tag):
    """replay rec's records: exit status 0, empty stderr, every pass of every record equal to the ctypes call"""
    assert rec.records, tag
    t = time.perf_counter()
    code, stderr, results, calls = hr.replay(program.exe, rec.records, program.dir, tag)
    program.run_s += time.perf_counter() - t
    assert (code, stderr) == (0, ""), f"{tag}: exit status {code}\n{stderr[-6000:]}"
    passes = [0] * len(rec.records)
    for idx, pas, ret, err, outs in results:
        r = rec.records[idx]
        assert (ret, err) == (r.ret, r.err), (tag, idx, r.label, pas, ret, err, r.ret, r.err)
        assert len(outs) == len(r.outs), (tag, idx, r.label)
        for k, (got, want) in enumerate(zip(outs, r.outs)):
            assert got == want, (tag, idx, r.label, "pass", pas, "output", k, None if got is None else len(got), None if want is None else len(want))
        passes[idx] += 1
    assert passes == [2 if r.streams else 1 for r in rec.records], tag
    for name, n in calls.items():
        program.calls[name] = program.calls.get(name, 0) + n
    for r in rec.records:
        program.records[r.label] = program.records.get(r.label, 0) + 1
    return calls


# ---- the build -------------------------------------------------------------------------------------------------------------
def test_all_host_sources_compile_without_a_warning_under_the_sanitizers(program):
    assert program.log == "", program.log
    assert len(program.stubs) > 50 and all(s.startswith(("hydamd_", "hydk_", "hyd_")) for s in program.stubs)


def test_a_device_function_reached_from_the_host_ends_the_program(program):
    """the host files call some hundred functions that live in csrc/hip/*.hip: in this link each is a stub that reports its
    name and ends the program, so no replayed hook can have gone through one and come back with a value"""
    ran = subprocess.run([program.exe, "--device-call"], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 3 and f"reached the device function {program.stubs[0]}" in ran.stderr, (ran.returncode, ran.stderr)


# ---- frames: frame.c, prefix.c, bitio.c, hostframe.c, encoder.c ---------------------------------------------------------------
def _level10_frames(image):
    """test_host_glue.test_level10_container_prologue's frames (the container prologue of images beyond level 5)"""
    import test_host_glue as thg
    from oracle import binding as orc

    for width, height, tiles in thg.LEVEL10:
        md = api.HYDImageMetadata(width, height, 0, 0, 0)
        for k, (tx, ty) in enumerate(tiles):
            tw, th = min(256, width - tx * 256), min(256, height - ty * 256)
            r, mx = orc.encode_lf_group(np.ascontiguousarray(image("photo", tw, th, 8, seed=50 + k)), num_presets=1, preset=0)
            glue.frame_from_stages(md, k == 0, k == len(tiles) - 1, [(tx, ty)], [r], mx)


def _lf_int_frames(group, image):
    import test_host_glue as thg
    from hydrium_amd import synth

    if group == "one-frame":
        for kind, w, h, depth in thg.ONE_FRAME[:-1]:
            glue.encode_with_oracle_stages(image(kind, w, h, depth))
        glue.encode_with_oracle_stages(synth.make_image_f32("photo", 264, 136))
        glue.encode_with_oracle_stages(synth.make_image("photo", 120, 72, 16), linear_light=1)
        for profile in _ICC, _ICC[:100]:
            glue.encode_with_oracle_stages(image("photo", 72, 40, 8), icc=profile)
        for order in ([(0, 0), (0, 0)], [(1, 0), (1, 0)]):  # test_repeated_lf_group_is_rejected_not_overrun
            with pytest.raises(RuntimeError, match="-14"):
                glue.encode_with_oracle_stages(image("photo", 2100, 16, 8), order=order)
    elif group == "four-lf-groups":
        kind, w, h, depth = thg.ONE_FRAME[-1]
        assert w > 2048 and h > 2048
        glue.encode_with_oracle_stages(image(kind, w, h, depth))
    elif group == "out-of-order":
        glue.encode_with_oracle_stages(image("photo", 2048 + 200, 2048 + 100, 8), order=[(1, 0), (0, 1), (0, 0), (1, 1)])
    elif group == "tile-mode":
        for shift in (0, 1, 2, 3):
            glue.encode_with_oracle_stages(image("photo", 1000, 700, 8), shift, shift)
        glue.encode_with_oracle_stages(image("smooth", 700, 530, 16), 1, 0)
        _level10_frames(image)
    elif group == "kept-buffer":
        for a in (image("noise", 1024, 768, 8), image("photo", 300, 200, 8)):
            glue.encode_with_oracle_stages(a)


@pytest.mark.parametrize("group", ["one-frame", "four-lf-groups", "out-of-order", "tile-mode", "kept-buffer"])
def test_frames_from_lf_ints_on_the_host_glue_cases(program, image, group):
    """tests/test_host_glue.py's cases through hydt_frame_from_stages: one-frame and tile mode, every shift, tiles out of order,
    float and linear light, ICC profiles (their bytes at an odd address too), the level-10 prologue, a frame description that
    is refused, and a frame above 1 MB (the buffer the library keeps)"""
    with recording() as rec:
        _lf_int_frames(group, image)
    calls = hold(program, rec, "frames-" + group)
    assert calls["hydt_frame_from_stages"] and calls["hydt_free"] and not calls["hydamd_frame_from_streams"]


def _icc_profile():
    """test_icc_profile_stream's profile"""
    rng = np.random.default_rng(7)
    head = bytearray(rng.integers(0, 256, 128, dtype=np.uint8).tobytes())
    head[36:40], head[40:44] = b"acsp", b"APPL"
    return bytes(head) + b"".join(bytes([65 + (i * 7) % 26, 48 + i % 10, 0, 255][k % 4] for k in range(4)) for i in range(150))


_ICC = _icc_profile()


def test_frames_from_coded_lf_streams_on_the_host_glue_cases(program, image):
    """hydamd_frame_from_streams as tests/glue.py calls it, on test_host_glue.py's cases with coded LF streams, one-frame and
    tile mode, with and without an ICC profile: LF bit streams and payloads at an odd address too"""
    with recording() as rec:
        for kind, w, h, depth in [("photo", 256, 256, 8), ("photo", 8, 8, 8), ("noise", 257, 255, 8), ("black", 64, 64, 8),
                                  ("white", 40, 520, 16), ("photo", 2049, 130, 8)]:
            glue.encode_with_oracle_stages(image(kind, w, h, depth), coded_lf=True)
        glue.encode_with_oracle_stages(image("photo", 600, 520, 8), 0, 0, coded_lf=True)
        for profile in _ICC, _ICC[:100]:
            glue.encode_with_oracle_stages(image("photo", 72, 40, 8), icc=profile, coded_lf=True)
    calls = hold(program, rec, "frames-coded")
    assert calls["hydamd_frame_from_streams"] and not calls["hydt_frame_from_stages"]


def test_frames_of_the_content_corpus_both_ways(program):
    """tests/content_corpus.py: black 8x8 (an LF stream of bit_count 0), noise 520x264 (10- and 22-bit TOC entries),
    primaries, float_neg and float_wide (LF ints of INT_MIN through the host coder's predictor, a running maximum of 72) and
    the 2312x264 frames of two LF groups, one of them black, in both send orders — from LF ints and from coded streams"""
    with recording() as rec:
        for coded in (False, True):
            for p in (cc._p("black", 8, 8, 8), cc._p("noise", 520, 264, 8), cc._p("primaries", 264, 200, 8),
                      cc._p("float_neg", 264, 136, 32), cc._p("float_wide", 264, 136, 32)):
                glue.encode_with_oracle_stages(cc.picture(*p), coded_lf=coded)
            for p in cc.ASSEMBLER:
                for order in ([(0, 0), (1, 0)], [(1, 0), (0, 0)]):
                    glue.encode_with_oracle_stages(cc.picture(*p), order=order, coded_lf=coded)
    calls = hold(program, rec, "frames-corpus")
    assert calls["hydt_frame_from_stages"] == calls["hydamd_frame_from_streams"] == 2 * 9  # (payloads and LF streams: an odd pass too)
    int_min = [r for r in rec.records if r.label == "hydt_frame_from_stages" and b"\x00\x00\x00\x80" in r.blob]
    assert int_min, "no LF int of INT_MIN among the float pictures: the host predictor's wrap-around went untested"


# ---- the LF coder ------------------------------------------------------------------------------------------------------------
def test_every_crafted_lf_stream(program):
    """tests/lf_streams.py: each stream's LF ints through the host coder (hydt_lf_group), the model's stream through the
    splice (hydt_lf_group_coded, its bits at an odd address too), the code lengths the model asks for (hydt_code_lengths),
    and the stream's histogram of code lengths through both constructions of the 18-symbol code (hydt_small_code_lengths)"""
    import lf_streams as ls

    with recording() as rec:
        for case in ls.CASES:
            dc = case.lf_ints()
            _, lengths, alphabet, pairs, bits, nbits = lf_model.model(dc)
            assert lf_model.coded_lf_group(case.vbw, case.vbh, lengths, alphabet, pairs, bits, nbits) == lf_model.host_lf_group(dc)
            f = np.bincount(np.asarray(lengths, np.int64), minlength=18)[:18].astype(np.uint32)
            a, b = np.zeros(18, np.uint32), np.zeros(18, np.uint32)
            assert rec.hydt_code_lengths(f.ctypes.data, a.ctypes.data, 18, 5) == rec.hydt_small_code_lengths(f.ctypes.data, b.ctypes.data, 18, 5)
            assert (a == b).all()
    calls = hold(program, rec, "lf")
    assert min(calls[h] for h in ("hydt_lf_group", "hydt_lf_group_coded", "hydt_small_code_lengths")) >= len(ls.CASES)


# ---- ICC profiles -------------------------------------------------------------------------------------------------------------
def test_icc_profiles_of_every_platform_signature_and_every_edge_length(program):
    """the profiles of test_icc_transform_is_decodable_for_every_platform_signature; lengths around every index the header
    prediction looks at (44: the platform signature, 128: the header's end, 132: the tag count); a profile whose size
    field disagrees with its length"""
    import test_host_glue as thg

    with recording() as rec:
        for platform in (b"APPL", b"MSFT", b"SGI ", b"SUNW", b"SXYZ", b"\0\0\0\0"):
            for size in (60, 128, 400):
                thg.test_icc_transform_is_decodable_for_every_platform_signature(platform, size)
        rng = np.random.default_rng(13)
        out, n = C.c_void_p(0), C.c_size_t(0)
        for size in (1, 2, 3, 4, 43, 44, 127, 128, 129, 131, 132):
            for platform in (b"SGI ", b"SUNW", b"MSFT"):
                icc = bytearray(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
                icc[0:4] = size.to_bytes(4, "big")[:size]
                icc[36:40], icc[40:44] = b"acsp"[:max(0, size - 36)], platform[:max(0, size - 40)]
                assert len(icc) == size
                assert rec.hydt_icc_mangled(bytes(icc), size, C.byref(out), C.byref(n)) == 0
                rec.hydt_free(out)
        for size, field in ((200, 100), (200, 1 << 31), (60, 200)):  # the size field says less, far more, more than there is
            icc = bytearray(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
            icc[0:4] = field.to_bytes(4, "big")
            assert rec.hydt_icc_mangled(bytes(icc), size, C.byref(out), C.byref(n)) == 0
            rec.hydt_free(out)
    assert hold(program, rec, "icc")["hydt_icc_mangled"] == 2 * (18 + 33 + 3)


# ---- the blob reader ---------------------------------------------------------------------------------------------------------
def _blobs(image):
    """{kind: (blob, expected_slots)}: one good blob per kind the CPU tests build — the staged read-back's one-slot blob
    (test_blob_reader_classes_for_the_staged_read_back), a shard's blob of hydamd_frame_from_blobs (the second LF group of
    test_frame_from_blobs_single_process_and_malformed_input) and test_layout.py's blob of nothing but consistent sizes"""
    import torch

    import oracle_engine
    from hydrium_amd import device

    def exported(img, lfs, floor=0):
        e = oracle_engine.OracleShardEngine(img, lfs)
        e.enqueue_transform()
        e.enqueue_entropy(torch.tensor([floor], dtype=torch.int32))
        out = torch.zeros(e.blob_bound(), dtype=torch.uint8)
        e.export_blob(out)
        n = int(device.blob_header(out[:64].numpy().tobytes())["total_bytes"])
        return out[:n].numpy().tobytes()

    slot = device.BLOB_SLOT_DTYPE.itemsize
    bare = np.zeros(64 + slot + 64, np.uint8)
    head = bare[:64].view(device.BLOB_HEADER_DTYPE)
    head["magic"], head["version"], head["num_slots"], head["lf_coded"] = device.BLOB_MAGIC, 1, 1, 1
    head["total_bytes"], head["lf_bytes"], head["hf_bytes"] = bare.size, 64, 0  # the HF sections start where the blob ends
    return {"staged": (exported(image("photo", 200, 120, 8), [0]), 1),
            "shard": (exported(image("photo", 2048 + 300, 72, 8), [1]), 0),
            "sizes-only": (bare.tobytes(), 1)}


def _corruptions(blob, seed):
    """256 single-field corruptions: a field of the header or of the slot record (or, one time in four, any aligned word
    of the blob) takes an edge value, a value near the blob's own size, or random bits"""
    from hydrium_amd import device

    rng = np.random.default_rng(seed)
    fields = [(device.BLOB_HEADER_DTYPE, 0), (device.BLOB_SLOT_DTYPE, 64)]
    places = [(base + dt.fields[name][1], dt.fields[name][0].itemsize) for dt, base in fields for name in dt.names
              if dt.fields[name][0].shape == () and dt.fields[name][0].itemsize in (1, 2, 4, 8)]
    for k in range(256):
        b = bytearray(blob)
        off, size = places[int(rng.integers(len(places)))] if k % 4 else (int(rng.integers(0, len(blob) // 4)) * 4, 4)
        edge = [0, 1, 2, len(blob), len(blob) - 1, len(blob) + 1, len(blob) - off, (1 << (8 * size)) - 1, 1 << (8 * size - 1),
                (1 << (8 * size)) - len(blob), int(rng.integers(0, 1 << 62))]
        b[off:off + size] = (edge[int(rng.integers(len(edge)))] % (1 << (8 * size))).to_bytes(size, "little")
        yield bytes(b)


def test_the_blob_reader_reads_nothing_past_the_size_it_is_given(program, image):
    """DESIGN.md §5 says of hyd_read_blob "nothing read past the given size".  Each good blob, every truncation of it from 0
    bytes to all of it — each in an allocation of exactly that length, at an even and at an odd address — and 256 seeded
    corruptions of single fields: the class is the ctypes run's, and the sanitizers saw no byte outside the allocation."""
    USABLE, NOT_USABLE = 0, 1
    with recording() as rec:
        for seed, (kind, (blob, expected)) in enumerate(_blobs(image).items()):
            assert rec.hydt_blob_class(blob, len(blob), expected) == USABLE, kind
            classes = rec.blob_prefixes(blob, expected)
            assert set(classes[:-1]) == {NOT_USABLE} and classes[-1] == USABLE, kind
            seen = {rec.hydt_blob_class(bad, len(bad), expected) for bad in _corruptions(blob, 100 + seed)}
            assert len(seen) >= 3, (kind, seen)  # the corruptions reach usable, not usable and malformed at the least
    calls = hold(program, rec, "blobs")
    assert calls["hydt_blob_class"] >= 2 * 3 * (1 + 256)


# ---- planners and layout hooks: assembler.c, mixed.c, tiled.c, batch.c with the shared headers ----------------------------------
def test_every_list_of_the_layout_and_planner_modules(program, image):
    """the lists test_mixed_sections.py, test_image_status_api.py (the _skip variant), test_tiled_sections.py,
    test_batch_layout.py and test_mixed_frames_layout.py run, by running their tests on the recorder: every assertion of
    theirs holds on the way, and the list of 255 images (HYDK_COPY_MAX_PIECES = 2040 pieces) is among them"""
    import test_batch_layout as tbl
    import test_image_status_api as tis
    import test_mixed_frames_layout as tmf
    import test_mixed_sections as tms
    import test_tiled_sections as tts

    with recording() as rec:
        tms.test_six_shapes_in_one_batch_each_file_what_the_host_writes_for_it_alone(rec, image)
        tms.test_a_repeated_shape_shares_its_record_and_keeps_its_own_prefix(rec, image)
        tms.test_the_same_pictures_in_reversed_order_give_the_reversed_files(rec, image)
        tms.test_one_image_and_the_largest_side(rec, image)
        for depth in sorted(cc.MIXED):
            tms.test_the_content_corpus_forward_and_reversed(rec, depth)
        tms.test_what_the_hook_refuses(rec)
        for flagged in ({0}, {2}, {3}, {4}, {5}, {1, 2}, {0, 1, 2, 3, 4, 5}):
            tis._hold(rec, tms.SIX_SHAPES, [tms._picture(image, k, w, h) for k, (w, h) in enumerate(tms.SIX_SHAPES)], flagged)
        stages = [tms._picture(image, k, w, h) for k, (w, h) in enumerate(tms.SIX_SHAPES)]
        assert tis._skipping(rec, tms.SIX_SHAPES, stages, set())[0] == tms._mixed(rec, tms.SIX_SHAPES, stages)[0]
        for w, h in ((8, 8), (256, 256), (232, 188)):
            tts.test_single_group_frame_equals_the_host_assembler(rec, image, w, h)
        tts.test_three_frames_single_and_four_group_mixed(rec, image)
        tts.test_single_group_frames_in_sequence_off_word_boundaries(rec, image)
        for picture, sx, sy in cc.TILED:
            tts.test_the_content_corpus_in_tile_mode(rec, picture, sx, sy)
        for pictures in tbl.ONE_GROUP_BATCHES:
            tbl.test_the_content_corpus_in_same_shape_batches(rec, pictures)
        plan = tmf._describe(rec, tmf.SIZES)
        assert isinstance(plan, dict), plan
        for test in (tmf.test_slots_pieces_and_kinds, tmf.test_images_of_one_size_share_a_plan,
                     tmf.test_the_workgroup_table_deals_the_frames_of_several_lf_groups_in_order,
                     tmf.test_scratch_shares_are_disjoint_and_inside_what_creation_allocates):
            test(plan)
        for k in (0, 2, 4, 6):
            tmf.test_a_frame_of_several_lf_groups_carries_the_plan_of_that_image_alone(plan, rec, k)
        tmf.test_the_same_list_plans_the_same_bytes(rec, plan)
        tmf.test_what_the_planner_refuses(rec)
        tmf.test_the_largest_batches_fit_the_scratch_creation_allocates(rec)
    calls = hold(program, rec, "layout")
    for name in ("hydt_mixed_from_streams", "hydt_mixed_from_streams_skip", "hydt_mixed_plan_counts", "hydt_mixed_plan_describe",
                 "hydt_mixed_frame_plan_alone", "hydt_tiles_from_streams", "hydt_batch_from_streams", "hydamd_frame_from_streams"):
        assert calls[name], name
    # the two hooks without an export ran once for every pass of a caller in another file that got as far as the layout
    reached = {}
    for r in rec.records:
        reached[r.label] = reached.get(r.label, 0) + (2 if r.ret == 0 else 0)
    assert calls["hydt_layout_from_streams_skip"] == reached["hydt_mixed_from_streams_skip"] > 0
    assert calls["hydt_layout_from_streams"] == reached["hydt_mixed_from_streams"] + reached["hydt_batch_from_streams"] > 0


# ---- the piece composer ------------------------------------------------------------------------------------------------------
class _AsTheDeviceHook:
    """test_gpu_builder_content.py calls the copy kernel's hook with the composer's arguments and two buffer lengths: its
    crafted lists, through the host composer"""

    def __init__(self, rec):
        self.rec = rec

    def hydt_pieces_copy_device(self, dst, n, off, count, src, src_len, lo, nbytes, err_word, out, out_len):
        return self.rec.hydt_compose_pieces(dst, n, off, count, src, lo, nbytes, out)


def test_every_piece_list(program):
    """tests/test_pieces.py's lists and, from tests/test_gpu_builder_content.py, the list of HYDK_COPY_MAX_PIECES pieces and
    every alignment of a range.  The source is allocated up to the end of the last 32-bit word a piece's string touches
    (hydk_pieces.h: the composer reads whole words, and no word that holds none of the string's bits); the output up to the
    end of the range's last word."""
    import test_gpu_builder_content as tgb
    import test_pieces as tp

    with recording() as rec:
        for end in (31, 32, 33):
            tp.test_piece_ends_around_a_word_boundary(rec, end)
        tp.test_three_pieces_inside_one_word(rec)
        tp.test_empty_pieces(rec)
        for off in (0, 1, 2, 3, 4093):
            tp.test_source_alignment(rec, off)
        tp.test_one_bit(rec)
        tp.test_gap_reads_as_zero(rec)
        tp.test_range_edges_leave_the_neighbours_alone(rec)
        tp.test_random_lists(rec)
        tgb.test_the_copy_kernel_on_the_longest_list_it_keeps_in_lds(_AsTheDeviceHook(rec))
        tgb.test_the_copy_kernel_at_every_alignment_of_the_range(_AsTheDeviceHook(rec))
    assert hold(program, rec, "pieces")["hydt_compose_pieces"] > 300


# ---- the field writers of the shared headers, the TOC entries, the peer-read checks ----------------------------------------
def test_every_list_of_the_section_writers_and_the_shard_checks(program):
    """tests/test_sections.py's lists (LF stream heads three ways, both code-length constructions, ANS distributions both
    ways, TOC entries) and test_host_glue.py's sequence of peer-read checks, whose latch table lives in the hook: the replay
    makes the same calls in the same order"""
    import test_host_glue as thg
    import test_sections as ts

    with recording() as rec:
        for case in range(len(ts._hist_cases())):
            ts.test_lf_stream_header(rec, case)
        ts.test_lf_stream_header_random(rec)
        ts.test_small_code_lengths(rec)
        ts.test_ans_distribution(rec)
        ts.test_toc_entries(rec)
        thg.test_peer_read_checks_are_chosen_and_latched_per_ordered_pair()
    calls = hold(program, rec, "sections")
    for name in ("hydt_lf_head_host", "hydt_lf_head_sections", "hydt_lf_head_wave", "hydt_code_lengths", "hydt_small_code_lengths",
                 "hydt_ans_distribution_host", "hydt_ans_distribution_sections", "hydt_toc_entry_check", "hydt_shard_checks"):
        assert calls[name], name


# ---- the shared sample-format headers as plain C++ under the same sanitizers ------------------------------------------------------
@pytest.fixture(scope="module")
def formats_program():
    """tests/c/sample_formats.cc: hyd_sample_fmt.h, hydk_half.h, hydk_yuv.h, hydk_yuv16.h, hydk_chroma.h and hydk_store.h with g++, no HIP header"""
    import format_dump

    return format_dump.sanitized_program("sample_formats")


def test_every_half_and_bfloat16_bit_pattern(formats_program):
    import pixel_layouts as pl
    import test_half_formats as thf

    got = formats_program("half").view(np.uint32).reshape(2, 65536)
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for row, storage, name, finite in ((0, thf.STORE_F16, "f16", (bits & 0x7C00) != 0x7C00), (1, thf.STORE_BF16, "bf16", (bits & 0x7F80) != 0x7F80)):
        thf.check_widening(storage, got[row])
        assert np.array_equal(got[row][finite], pl.widen_half_bits(bits, name).view(np.uint32)[finite])


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_every_8_bit_triple_under_each_matrix(formats_program, matrix):
    import test_yuv_formats as tyf
    import yuv_model as ym

    got = formats_program("yuv8", matrix).reshape(256, 65536, 3)
    tyf.check_conversion(matrix, lambda yuv: got[int(yuv[0, 0]):int(yuv[0, 0]) + tyf.Y_CHUNK].reshape(-1, 3))
    assert ym.TABLE[matrix] == tyf._header_table()[matrix]


def test_the_seeded_16_bit_triples_under_all_twelve_table_rows(formats_program):
    """tests/test_p016_formats.py's 2^20 seeded random words (low bits set) and its 27 corners, against the model's picture of
    them (made once per row and shared with that module)"""
    import test_p016_formats as tpf

    n = (1 << 20) + 27
    t = tpf.triples()[-n:]
    got = formats_program("yuv16", data=np.ascontiguousarray(t).tobytes()).view(np.uint16).reshape(12, n, 3)
    import p016_model as pm

    for k, (depth, matrix) in enumerate(tpf.ROWS):
        shared = tpf._cache.get(("rgb", depth, matrix))  # the model's picture of all of triples(), where that module has made it
        want = shared[-n:] if shared is not None else pm.yuv_to_rgb(depth, matrix, t[:, 0], t[:, 1], t[:, 2])
        wrong = np.flatnonzero((got[k] != want).any(-1))
        assert wrong.size == 0, (depth, matrix, wrong.size, [(t[i].tolist(), got[k][i].tolist()) for i in wrong[:8]])


def test_the_chroma_taps_at_the_edges_of_the_smallest_pictures(formats_program):
    """widths 1, 2, 3 and heights 1, 2 (and the sizes of the hooks' own tests), 8- and 16-bit samples, both interpolations,
    random samples and the top of the range: every chroma plane in an allocation of exactly its samples"""
    import struct

    import chroma_model as cm
    import p016_model as pm
    import test_p016_formats as tpf

    cases, blob = [], []
    for w, h in [(w, h) for h in (1, 2) for w in (1, 2, 3)] + tpf.HOOK_SIZES:
        for bits, dtype, top, model in ((8, np.uint8, 255, cm.upsample), (16, np.uint16, 65535, pm.upsample)):
            words = tpf.random_pairs(w, h)
            for uv in ((words >> (16 - bits)).astype(dtype), np.full(words.shape, top, dtype)):
                for filt in (cm.CENTRE, cm.LEFT):
                    cases.append((bits, dtype, filt, w, h, model(filt, uv, w, h)))
                    blob.append(struct.pack("<IIII", bits, filt, w, h) + np.ascontiguousarray(uv).tobytes())
    got = formats_program("chroma", data=struct.pack("<I", len(cases)) + b"".join(blob))
    at = 0
    for bits, dtype, filt, w, h, want in cases:
        n = h * w * 2 * (bits // 8)
        assert np.array_equal(got[at:at + n].view(dtype).reshape(h, w, 2), want), (bits, cm.FILTER_NAMES[filt], w, h)
        at += n
    assert at == got.size


def test_the_predicates_and_origins_of_the_sample_formats(formats_program):
    """the whole descriptor of every number -8 ... 4100 against tests/format_model.py, which is written from the prose; what the
    decode of csrc/hip/hydk_store.h makes of it; and every (number, predicate) pair the NV12 and P016 families pinned before"""
    import chroma_model as cm
    import format_dump
    import format_model as fm
    import p016_model as pm
    import yuv_model as ym

    rows, origins = format_dump.formats()
    assert sorted(rows) == list(range(-8, 4101)) and len(rows) == 4109
    for fmt, (d, job) in rows.items():
        want = fm.describe(fmt)
        assert d == want, (fmt, d, want)
        cls, storage, variant = fm.storage_of(fmt)
        assert job == (want.device, fmt if want.device else -1, cls, storage, want.matrix + 4 * want.depth, variant), (fmt, job)
    assert [f for f, (d, _) in rows.items() if d.device] == sorted(fm.ALL) and sum(d.device for d, _ in rows.values()) == 165
    assert [f for f, (d, _) in rows.items() if d.host] == [0, 1, 2]
    # the twelve predicates of the two-plane families, as they were held for -8 ... 263, read off the descriptor
    nv12 = {cm.sample_fmt(m, f): (f, m) for f in cm.FILTERS for m in ym.MATRICES}
    for fmt in range(-8, 264):
        d = rows[fmt][0]
        p016 = fmt in pm.FAMILY
        interp = (fmt in nv12 and nv12[fmt][0] != 0) or (p016 and pm.filter_of(fmt) != 0)
        size = 1 if fmt == 0 or fmt in nv12 else 2 if fmt in (1, 3, 4) or p016 else 4 if fmt == 2 else 0
        what = pm.BITS[pm.depth_of(fmt)] * 256 + pm.filter_of(fmt) * 16 + pm.matrix_of(fmt) if p016 else \
            nv12[fmt][0] * 16 + nv12[fmt][1] if fmt in nv12 else -1
        want = [fmt in nv12 and nv12[fmt][0] == 0, fmt in nv12, fmt in nv12 and interp, p016, p016 and interp, fmt in nv12 or p016, interp,
                0 <= fmt <= 4 or fmt in nv12 or p016, 0 <= fmt <= 2, 2 <= fmt <= 4, size, what]
        pairs, deep = d.layout == fm.PAIRS, d.depth != 0
        got = [pairs and not deep and d.filter == 0, pairs and not deep, pairs and not deep and d.filter != 0, pairs and deep,
               pairs and deep and d.filter != 0, pairs, pairs and d.filter != 0, d.device, d.host, d.is_float, d.bytes,
               (d.bits * 256 if deep else 0) + d.filter * 16 + d.matrix if pairs else -1]
        assert [int(x) for x in got] == [int(x) for x in want], (fmt, d, want)
        assert not pairs or (d.sub, d.sx, d.sy) == (0, 1, 1)
    for fmt in (5, 7, 15, 20, 31, 36, 47, 52, 64, 79, 84, 128, 244, 263, -1, -8):  # the two families' own lists of numbers that name nothing
        assert rows[fmt][0] == fm.NOTHING, fmt
    x0, y0, pitch, pixel = 256, 512, 1024, 3
    want = []
    for fmt, size in ((0, 1), (1, 2), (2, 4), (3, 2), (4, 2)):
        want.append([(y0 * pitch + x0 * pixel) * size] * 3)
    for fmt, size in ((18, 1), (48, 1), (80, 2), (243, 2)):
        want.append([(y0 * pitch + x0) * size] + [(y0 // 2 * pitch + x0) * size] * 2)
    assert origins.tolist() == want


def test_the_family_models_are_the_format_models():
    """format_model's lists are the four family models' and the Python layer's tuples, 5 + 12 + 36 + 28 + 84 = 165, and each
    family model reads a number's fields as format_model.describe does"""
    import chroma_model as cm
    import format_model as fm
    import p016_model as pm
    import planar16_model as m16
    import planar_model as plm
    import yuv_model as ym
    from hydrium_amd import device

    assert sorted(fm.NV12_FAMILY) == sorted(device.NV12_FAMILY) == sorted(cm.sample_fmt(m, f) for f in cm.FILTERS for m in ym.MATRICES)
    assert sorted(fm.P016_FAMILY) == sorted(device.P016_FAMILY) == sorted(pm.FAMILY)
    assert sorted(fm.PLANAR_FAMILY) == sorted(device.PLANAR_FAMILY) == sorted(plm.FAMILY)
    assert sorted(fm.PLANAR16_FAMILY) == sorted(device.PLANAR16_FAMILY) == sorted(m16.FAMILY)
    assert fm.RGB_FORMATS == (0, 1, 2, device.FLOAT16, device.BFLOAT16)
    assert sum(len(f) for f in fm.FAMILIES) == 165
    for fmt in range(fm.LO, fm.HI):
        d = fm.describe(fmt)
        assert (fmt in pm.FAMILY, plm.is_format(fmt), m16.is_format(fmt)) == \
            (d.layout == fm.PAIRS and d.depth > 0, d.layout == fm.PLANES and d.depth == 0, d.layout == fm.PLANES and d.depth > 0), fmt
        if fmt in pm.FAMILY:
            assert (pm.matrix_of(fmt), pm.filter_of(fmt), pm.depth_of(fmt), pm.BITS[pm.depth_of(fmt)]) == (d.matrix, d.filter, d.depth, d.bits)
        if plm.is_format(fmt):
            assert (plm.matrix_of(fmt), plm.filter_of(fmt), plm.sub_of(fmt), *plm.shifts(plm.sub_of(fmt))) == (d.matrix, d.filter, d.sub, d.sx, d.sy)
            assert plm.predicate_row(fmt) == (1, d.sub, d.filter, d.matrix, int(d.filter != 0), d.bytes, d.device, d.host)
        if m16.is_format(fmt):
            assert (m16.matrix_of(fmt), m16.filter_of(fmt), m16.sub_of(fmt), m16.depth_of(fmt), m16.bits_of(fmt), *plm.shifts(m16.sub_of(fmt))) == \
                (d.matrix, d.filter, d.sub, d.depth, d.bits, d.sx, d.sy)
        if d.layout != fm.RGB:
            assert getattr(device, fm.public_name(fmt)) == fmt


def test_every_public_ycbcr_name_is_spelled_by_the_descriptor_of_its_number():
    """include/hydrium_amd.h: layout and depth give the stem, the filter the C / L infix, the matrix the suffix"""
    import re

    import format_dump
    import format_model as fm

    text = open(os.path.join(ROOT, "include", "hydrium_amd.h")).read()
    found = {n: int(v) for n, v in re.findall(r"^#define HYDAMD_((?:NV12|P01[026]|I4(?:20|22|44)|I[024]1[026])[CL]?_BT\w+) (\d+)\s*$", text, re.M)}
    assert sorted(found.values()) == sorted(fm.ALL[5:]) and len(found) == 160
    for name, fmt in found.items():
        assert fm.public_name(fmt, format_dump.described(fmt)) == name, (name, fmt)


# ---- the closing count -------------------------------------------------------------------------------------------------------
def test_no_hook_of_the_host_files_was_left_out(program):
    """reads the replay program's own reports: every hook defined in csrc/host/*.c, and hydamd_frame_from_streams, was called
    there.  (Runs last: the tests above add their reports.)"""
    import re

    defined = set()
    for path in sorted(os.listdir(os.path.join(hbuild.CSRC, "host"))):
        if path.endswith(".c"):
            text = open(os.path.join(hbuild.CSRC, "host", path)).read()
            defined |= set(re.findall(r"^(?:HYDT_EXPORT |__attribute__\(\(visibility\(\"default\"\)\)\) )?(?:int|void) (hydt_[a-z_]+)\(", text, re.M))
    defined -= {"hydt_take", "hydt_take_bits"}  # static helpers of the hooks
    assert defined | {"hydamd_frame_from_streams"} == set(REPLAYED) and len(defined) == 25, sorted(defined ^ set(REPLAYED))
    missing = [h for h in REPLAYED if not program.calls.get(h)]
    assert not missing, f"never called in the replay program: {missing}"
    print("records per hook:", ", ".join(f"{k} {v}" for k, v in sorted(program.records.items())))
