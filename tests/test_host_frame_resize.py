"""CPU tests of the resized hand-off's rule (include/poppy_hip.h: poppy_hip_set_frame_size): poppy_bgr_resize_area against a numpy restatement written from
the rule (integer weight matrices contracted in int64), bit for bit, on random, 0 / 255 and 127 / 128 content; its agreement with the whole-factor rule;
a frame above 2^24 pixels; poppy_frame_fit_size; the refusals; the symbols."""

import ctypes as C

import numpy as np
import pytest

from poppy_amd import capi

E_ARG, E_UNSUPPORTED = -1, -6
# (w, h, ow, oh); REFUSED: 65 > 8 * 8
SIZES = [(17, 9, 3, 2), (9, 9, 8, 8), (53, 37, 53, 37), (64, 48, 8, 6), (7, 1, 3, 1), (1, 7, 1, 3)]
REFUSED = (65, 48, 8, 6)


def weights(n, on):
    """The on x n matrix of overlaps of [x n, (x + 1) n) with [i on, (i + 1) on), in units of 1 / on of a source pixel."""
    x = np.arange(on, dtype=np.int64)[:, None]
    i = np.arange(n, dtype=np.int64)[None, :]
    m = np.clip(np.minimum((i + 1) * on, (x + 1) * n) - np.maximum(i * on, x * n), 0, None)
    assert (m.sum(axis=1) == n).all() and (m.sum(axis=0) == on).all() and m.max() <= on
    first, last = (x[:, 0] * n) // on, ((x[:, 0] + 1) * n - 1) // on          # the rule's range of non-zero weights
    for k in range(on):
        nz = np.flatnonzero(m[k])
        assert nz[0] == first[k] and nz[-1] == last[k]
    return m


def resize_reference(bgr, ow, oh):
    h, w = bgr.shape[:2]
    total = np.einsum("yr,xi,ric->yxc", weights(h, oh), weights(w, ow), bgr.astype(np.int64))
    return ((total + (w * h) // 2) // (w * h)).astype(np.uint8)


def frames_for(w, h):
    rng = np.random.default_rng(w * 1009 + h * 31)
    return {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            "0/255": (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8),
            "127/128": (127 + rng.integers(0, 2, (h, w, 3))).astype(np.uint8),          # sums that sit on and beside the rounding ties
            "white": np.full((h, w, 3), 255, np.uint8)}


@pytest.mark.parametrize("w,h,ow,oh", SIZES)
def test_resize_matches_the_rule(w, h, ow, oh):
    for name, f in frames_for(w, h).items():
        got = capi.bgr_resize_area(f, ow, oh)
        want = resize_reference(f, ow, oh)
        assert got.shape == want.shape == (oh, ow, 3)
        assert np.array_equal(got, want), f"{w}x{h} -> {ow}x{oh}, {name}: {np.count_nonzero(got != want)} bytes differ"
        assert np.array_equal(capi.bgr_resize_area(f, ow, oh, row_pad=7, dst_pad=5), want)
    if (w, h) == (ow, oh):
        assert np.array_equal(capi.bgr_resize_area(f, ow, oh), f)               # the identity
    assert (capi.bgr_resize_area(np.full((h, w, 3), 77, np.uint8), ow, oh) == 77).all()          # a constant frame stays constant


def test_a_factor_above_eight_is_refused():
    w, h, ow, oh = REFUSED
    with pytest.raises(capi.PoppyError):
        capi.bgr_resize_area(np.zeros((h, w, 3), np.uint8), ow, oh)
    assert capi.bgr_resize_area(np.zeros((h, w - 1, 3), np.uint8), ow, oh).shape == (oh, ow, 3)


def test_by_hand():
    """Independent of the restatement: 3 -> 2 columns has weights (2, 1 | 1, 2) over 3."""
    f = np.array([[[0] * 3, [90] * 3, [255] * 3]], np.uint8)
    assert capi.bgr_resize_area(f, 2, 1).tolist() == [[[30] * 3, [200] * 3]]                    # (0 * 2 + 90 + 1) / 3, (90 + 510 + 1) / 3
    f = np.array([[[1] * 3, [0] * 3]], np.uint8)
    assert capi.bgr_resize_area(f, 1, 1).tolist() == [[[1] * 3]]                                # the tie (1 + 1) / 2 rounds up


@pytest.mark.parametrize("s", range(1, 9))
def test_agrees_with_the_whole_factor_rule(s):
    for ow, oh in [(5, 3), (4, 4), (2, 7), (1, 1)]:
        for name, f in frames_for(s * ow, s * oh).items():
            assert np.array_equal(capi.bgr_resize_area(f, ow, oh), capi.bgr_downscale(f, s)), (s, ow, oh, name)


def test_differs_from_the_whole_factor_rule_where_that_clips():
    """5 -> 3 columns: the whole-factor rule at s = 2 gives the last output the last column alone; this one stretches."""
    f = np.array([[[0] * 3, [0] * 3, [0] * 3, [0] * 3, [240] * 3]], np.uint8)
    assert capi.bgr_downscale(f, 2)[0, 2].tolist() == [240] * 3
    assert capi.bgr_resize_area(f, 3, 1)[0, 2].tolist() == [144] * 3                            # (240 * 3 + 2) / 5


def test_sums_of_a_frame_above_2_to_24_pixels_are_64_bit():
    w = h = 4100
    assert w * h > 1 << 24
    got = capi.bgr_resize_area(np.full((h, w, 3), 255, np.uint8), w - 1, h - 1)
    assert got.shape == (h - 1, w - 1, 3) and (got == 255).all()


def test_fit_size():
    assert capi.frame_fit_size(1920, 1080, 1280, 720) == (1280, 720)
    assert capi.frame_fit_size(1920, 1080, 1000, 1000) == (1000, 563)
    assert capi.frame_fit_size(1080, 1920, 1000, 1000) == (563, 1000)
    assert capi.frame_fit_size(100, 50, 200, 200) == (100, 50)
    L = capi.lib()
    ow, oh = C.c_int(-7), C.c_int(-7)
    assert L.poppy_frame_fit_size(4000, 10, 100, 100, C.byref(ow), C.byref(oh)) == E_UNSUPPORTED          # a factor of 40 horizontally
    assert (ow.value, oh.value) == (-7, -7)
    with pytest.raises(capi.PoppyError):
        capi.frame_fit_size(4000, 10, 100, 100)
    for args in [(0, 4, 2, 2), (4, 0, 2, 2), (4, 4, 0, 2), (4, 4, 2, 0), (-1, 4, 2, 2), (4, 4, 2, -2)]:
        assert L.poppy_frame_fit_size(*args, C.byref(ow), C.byref(oh)) == E_ARG and (ow.value, oh.value) == (-7, -7)
    assert L.poppy_frame_fit_size(4, 4, 2, 2, None, C.byref(oh)) == E_ARG and L.poppy_frame_fit_size(4, 4, 2, 2, C.byref(ow), None) == E_ARG
    assert (ow.value, oh.value) == (-7, -7)
    assert capi.frame_fit_size(2147483647, 2147483647, 2147483647, 1 << 30) == (1 << 30, 1 << 30)          # products in 64 bits


def test_refusals_come_before_any_access():
    L = capi.lib()
    w, h, ow, oh = 9, 5, 4, 3
    src = np.full((h, w * 3), 9, np.uint8)
    dst = np.full(h * w * 3, 0xA5, np.uint8)
    p, q = capi._p(src), capi._p(dst)
    call = L.poppy_bgr_resize_area
    assert call(None, w * 3, w, h, ow, oh, q, ow * 3) == E_ARG
    assert call(p, w * 3, w, h, ow, oh, None, ow * 3) == E_ARG
    assert call(p, w * 3, 0, h, ow, oh, q, ow * 3) == E_ARG and call(p, w * 3, w, -3, ow, oh, q, ow * 3) == E_ARG          # an empty frame
    for bad_ow, bad_oh in [(0, oh), (ow, 0), (-1, oh), (w + 1, oh), (ow, h + 1), (1, oh)]:          # (1: 9 > 8 * 1)
        assert call(p, w * 3, w, h, bad_ow, bad_oh, q, w * 3 + 3) == E_ARG, (bad_ow, bad_oh)
    assert call(p, w * 3 - 1, w, h, ow, oh, q, ow * 3) == E_ARG               # a stride below 3 * width
    assert call(p, w * 3, w, h, ow, oh, q, ow * 3 - 1) == E_ARG               # ... and a dst_stride below 3 * ow
    assert (dst == 0xA5).all(), "a refused call wrote into dst"
    assert call(p, w * 3, w, h, ow, oh, q, ow * 3) == 0 and (dst[:3 * ow * oh] == 9).all() and (dst[3 * ow * oh:] == 0xA5).all()


def test_form_predicate_is_decided_by_the_sizes():
    assert capi.bgr_resize_area_form(1920, 1080, 1280, 720) == 2 and capi.bgr_resize_area_form(5, 3, 1, 1) == 2 and capi.bgr_resize_area_form(4096, 4096, 4096, 512) == 2
    assert capi.bgr_resize_area_form(2, 70000, 2, 35000) == 1 and capi.bgr_resize_area_form(32769, 2, 32769, 1) == 1          # a side above 32768
    assert capi.bgr_resize_area_form(4100, 4100, 4099, 4099) == 0 and capi.bgr_resize_area_form(4097, 4096, 4097, 4096) == 0      # above 2^24 pixels
    with pytest.raises(capi.PoppyError):
        capi.bgr_resize_area_form(65, 48, 8, 6)


def test_symbols():
    names = ["poppy_hip_set_frame_size", "poppy_hip_pool_set_frame_size", "poppy_frame_fit_size", "poppy_bgr_resize_area", "poppy_hip_bgr_resize_area",
             "poppy_hip_bgr_resize_area_form"]
    for name in names:
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name
