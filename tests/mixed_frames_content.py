"""Content and oracle helpers of tests/test_gpu_mixed_frames.py that need no GPU: the pictures whose LF groups differ in
their alphabet maxima, and the oracle's stage results of an image LF group by LF group."""
import functools

import numpy as np

LF = 2048


def oracle_lf_groups(host, alone=False):
    """[(oracle result, running alphabet maximum)] of an image's LF groups in raster order, the maximum carried from LF
    group to LF group as one frame's is (alone: every LF group as if it were a frame of its own)"""
    from oracle import binding as orc

    h, w, _ = host.shape
    isz, fmt = host.dtype.itemsize, orc.FMT[host.dtype]
    lfx, lfy = -(-w // LF), -(-h // LF)
    out = []
    for ty in range(lfy):
        for tx in range(lfx):
            x0, y0 = tx * LF, ty * LF
            p = host.ctypes.data + (y0 * w + x0) * 3 * isz
            preset, presets, before = (0, 1, 0) if alone else (ty * lfx + tx, lfx * lfy, out[-1][1] if out else 0)
            out.append(orc.encode_lf_group_ptrs([p, p + isz, p + 2 * isz], 3 * w, 3, fmt, 0, min(LF, w - x0), min(LF, h - y0),
                                                preset, presets, before))
    return out


def log_alphabet(mx):
    """ceil(log2(mx)), what the table kernel sizes its tables by above its floor of 5"""
    return int(mx - 1).bit_length() if mx > 1 else 0


@functools.lru_cache(maxsize=None)
def restart_pictures():
    """float32 host arrays N (one LF group of noise), S (4160 x 16, three LF groups, all smooth) and Q (4160 x 16 whose LF
    groups are smooth | noise | smooth).  The noise is synth's spread over [-0.5, 1.5] (content_corpus's float_neg): in
    [0, 1] its alphabet maximum of 27 lies, like smooth's 8, below the table kernel's floor of 2^5, and a maximum carried
    into the wrong image would change no byte.  Never changed."""
    from hydrium_amd import synth

    def noise(w, h, seed):
        return (synth.make_image_f32("noise", w, h, seed) * np.float32(2.0) + np.float32(-0.5)).astype(np.float32)

    n = noise(300, 200, 1234)
    s = synth.make_image_f32("smooth", 4160, 16, 1251)
    q = np.ascontiguousarray(np.concatenate([synth.make_image_f32("smooth", LF, 16, 1268), noise(LF, 16, 1285),
                                             synth.make_image_f32("smooth", 64, 16, 1302)], axis=1))
    assert q.shape == (16, 4160, 3) and s.shape == q.shape
    return n, s, q
