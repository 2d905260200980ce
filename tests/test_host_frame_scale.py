"""CPU tests of the scaled hand-off's rule (include/poppy_hip.h: poppy_hip_set_frame_scale): poppy_bgr_downscale against a numpy restatement written from the
rule, bit for bit, for every factor 1..8, on shapes around every block edge and on content that sits on the rounding ties; poppy_frame_scaled_size; the
refusals; and the length of every format's host frame composed behind the downscale."""

import ctypes as C

import numpy as np
import pytest

from poppy_amd import capi

E_ARG = -1
FACTORS = list(range(1, 9))


def sides(s):
    """{1, s - 1, s, s + 1, 2s + 1, 8s, 8s + 3}, what is positive of it"""
    return sorted({v for v in (1, s - 1, s, s + 1, 2 * s + 1, 8 * s, 8 * s + 3) if v > 0})


def downscale_reference(bgr, s):
    """The rule in int64: output pixel (x, y) covers source columns [s x, min(s x + s, W)) and rows [s y, min(s y + s, H)), n pixels;
    out = (sum + n // 2) // n per channel."""
    h, w = bgr.shape[:2]
    ow, oh = (w + s - 1) // s, (h + s - 1) // s
    pad = np.zeros((oh * s, ow * s, 3), np.int64)
    pad[:h, :w] = bgr
    cnt = np.zeros((oh * s, ow * s), np.int64)
    cnt[:h, :w] = 1
    total = pad.reshape(oh, s, ow, s, 3).sum(axis=(1, 3))
    n = cnt.reshape(oh, s, ow, s).sum(axis=(1, 3))[..., None]
    assert n.min() >= 1 and n.max() <= 64
    return ((total + n // 2) // n).astype(np.uint8)


def tie_frame(w, h, s):
    """Blocks whose sums sit on and beside the rounding tie: in block (bx, by) the first k pixels (row-major within the full s x s block) are base + 1 and
    the rest base, k from {n / 2 - 1, n / 2, n / 2 + 1} of n = s * s and base from {0, 254, 100}, a different one per channel: {0, 0, 1, 1} at s = 2, four
    and five ones of nine at s = 3.  Clipped edge blocks keep the part of the pattern that is inside the frame."""
    y, x = np.mgrid[0:h, 0:w]
    by, bx, inner = y // s, x // s, (y % s) * s + x % s
    n = s * s
    out = np.empty((h, w, 3), np.uint8)
    for ch in range(3):
        k = np.clip(n // 2 - 1 + (bx + 2 * by + ch) % 3, 0, n)
        base = np.array([0, 254, 100])[(bx + by + ch) % 3]
        out[..., ch] = base + (inner < k)
    return out


def frames_for(w, h, s):
    rng = np.random.default_rng(w * 1009 + h * 31 + s)
    corner = np.zeros((h, w, 3), np.uint8)
    corner[h - 1, w - 1] = 255                     # a single 255 in the (clipped) corner block
    return {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "full": np.full((h, w, 3), 255, np.uint8),
            "ties": tie_frame(w, h, s), "corner": corner}


@pytest.mark.parametrize("s", FACTORS)
def test_downscale_matches_the_rule(s):
    for w in sides(s):
        for h in sides(s):
            for name, f in frames_for(w, h, s).items():
                got = capi.bgr_downscale(f, s)
                want = downscale_reference(f, s)
                assert got.shape == want.shape == (capi.frame_scaled_size(w, h, s)[1], capi.frame_scaled_size(w, h, s)[0], 3), (w, h, name)
                assert np.array_equal(got, want), f"{w}x{h} / {s}, {name}: {np.count_nonzero(got != want)} bytes differ"


@pytest.mark.parametrize("s", FACTORS)
def test_padded_strides(s):
    w, h = 8 * s + 3, 2 * s + 1
    f = frames_for(w, h, s)["random"]
    want = downscale_reference(f, s)
    assert np.array_equal(capi.bgr_downscale(f, s, row_pad=7), want)
    assert np.array_equal(capi.bgr_downscale(f, s, dst_pad=5), want)        # (the wrapper checks that the padding of dst stays as it was)
    assert np.array_equal(capi.bgr_downscale(f, s, row_pad=13, dst_pad=2), want)


def test_the_ties_round_up_and_the_corner_counts_its_own_pixels():
    """The rule by hand, independent of the restatement above."""
    assert capi.bgr_downscale(np.array([[[0] * 3, [0] * 3], [[1] * 3, [1] * 3]], np.uint8), 2).tolist() == [[[1, 1, 1]]]          # (2 + 2) / 4
    nine = np.zeros((3, 3, 3), np.uint8)
    nine.reshape(9, 3)[:4] = 1
    assert capi.bgr_downscale(nine, 3).tolist() == [[[0, 0, 0]]]                                                              # (4 + 4) / 9
    nine.reshape(9, 3)[:5] = 1
    assert capi.bgr_downscale(nine, 3).tolist() == [[[1, 1, 1]]]                                                              # (5 + 4) / 9
    f = np.zeros((5, 5, 3), np.uint8)
    f[4, 4] = 255
    got = capi.bgr_downscale(f, 4)
    assert got.shape == (2, 2, 3) and got[1, 1].tolist() == [255] * 3 and got.sum() == 3 * 255                                 # n = 1 in the corner: not 255 / 16
    f = np.zeros((6, 5, 3), np.uint8)
    f[5, 4] = 255
    assert capi.bgr_downscale(f, 4)[1, 1].tolist() == [128] * 3                                                               # n = 2: (255 + 1) / 2


def test_factor_one_is_the_identity():
    for w, h in [(1, 1), (7, 3), (64, 5), (75, 19)]:
        f = frames_for(w, h, 1)["random"]
        assert np.array_equal(capi.bgr_downscale(f, 1), f)
        assert np.array_equal(capi.bgr_downscale(f, 1, row_pad=5, dst_pad=3), f)


def test_scaled_size():
    for s in FACTORS:
        for w, h in [(1, 1), (s, s), (s + 1, 2 * s + 1), (1920, 1080), (3840, 2160), (5, 3), (2, 70000), (2147483647, 2147483647)]:
            assert capi.frame_scaled_size(w, h, s) == ((w + s - 1) // s, (h + s - 1) // s)
    assert capi.frame_scaled_size(5, 3, 8) == (1, 1) and capi.frame_scaled_size(1920, 1080, 4) == (480, 270)
    ow, oh = C.c_int(-7), C.c_int(-7)
    L = capi.lib()
    for w, h, s in [(0, 4, 2), (4, 0, 2), (-1, 4, 2), (4, 4, 0), (4, 4, 9), (4, 4, -1)]:
        assert L.poppy_frame_scaled_size(w, h, s, C.byref(ow), C.byref(oh)) == E_ARG and (ow.value, oh.value) == (-7, -7)
    assert L.poppy_frame_scaled_size(4, 4, 2, None, C.byref(oh)) == E_ARG and L.poppy_frame_scaled_size(4, 4, 2, C.byref(ow), None) == E_ARG


def test_refusals_come_before_any_access():
    L = capi.lib()
    w, h = 9, 5
    src = np.full((h, w * 3), 9, np.uint8)
    dst = np.full(h * w * 3, 0xA5, np.uint8)
    p, q = capi._p(src), capi._p(dst)
    for s in (0, 9, -1):
        assert L.poppy_bgr_downscale(p, w * 3, w, h, s, q, w * 3) == E_ARG
        with pytest.raises(capi.PoppyError):
            capi.bgr_downscale(src.reshape(h, w, 3), s)
    assert L.poppy_bgr_downscale(None, w * 3, w, h, 2, q, 15) == E_ARG
    assert L.poppy_bgr_downscale(p, w * 3, w, h, 2, None, 15) == E_ARG
    assert L.poppy_bgr_downscale(p, w * 3 - 1, w, h, 2, q, 15) == E_ARG          # a stride below 3 * width
    assert L.poppy_bgr_downscale(p, w * 3, w, h, 2, q, 14) == E_ARG              # ... and a dst_stride below 3 * ow
    assert L.poppy_bgr_downscale(p, w * 3, 0, h, 2, q, 15) == E_ARG and L.poppy_bgr_downscale(p, w * 3, w, -3, 2, q, 15) == E_ARG
    assert (dst == 0xA5).all(), "a refused call wrote into dst"
    assert L.poppy_bgr_downscale(p, w * 3, w, h, 2, q, 15) == 0 and (dst[:3 * 15] == 9).all() and (dst[3 * 15:] == 0xA5).all()


@pytest.mark.parametrize("s", [2, 3, 8])
def test_composed_host_frames_have_the_scaled_length(s):
    """A writer's frame under scale s and format F is F's host statement of the downscaled frame: poppy_frame_bytes(F, ow, oh) is its length (the capacity
    that bounds it, for the coded formats)."""
    w, h = 8 * s + 3, 5 * s + 1
    rng = np.random.default_rng(s)
    frames = [capi.bgr_downscale(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), s) for _ in range(3)]
    ow, oh = capi.frame_scaled_size(w, h, s)
    assert frames[0].shape == (oh, ow, 3) and frames[0].size == capi.frame_bytes(capi.FRAME_BGR, ow, oh)
    assert capi.bgr_to_i420(frames[0]).size == capi.frame_bytes(capi.FRAME_I420, ow, oh)
    assert capi.bgr_to_pal8(frames[0]).size == capi.frame_bytes(capi.FRAME_PAL8, ow, oh) == ow * oh + 768
    assert capi.bgr_frames_to_pal8(frames).shape == (3, capi.frame_bytes(capi.FRAME_PAL8_SEQ, ow, oh))
    assert 776 <= capi.bgr_to_gif_frame(frames[0]).size <= capi.frame_bytes(capi.FRAME_GIF, ow, oh)
    coded = capi.bgr_frames_to_gif_frames(frames)
    assert len(coded) == 3 and all(776 <= f.size <= capi.frame_bytes(capi.FRAME_GIF_SEQ, ow, oh) for f in coded)
