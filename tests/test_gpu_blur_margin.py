"""blur_margin on the device (k_strip_h / k_strip_v behind poppy_hip_blur_margin and behind poppy_hip_morph_list's canvas) against the
oracle, byte for byte, on every geometry x content of blur_margin_util.py — which test_oracle_blur_margin.py ties to an independent
restatement without a GPU — with padded and non-contiguous rows, through the image-list path with its kept scratch, and the refusals:
sizes whose margin strips leave the canvas never reach a kernel.

Measured on an MI355X with the oracle's share: no test of this file takes longer than 0.7 s (100 x 60 in 400 x 300 on the seven
contents; every other one at most 0.25 s), the whole file 2.7 s."""
import ctypes as C

import numpy as np
import pytest

import blur_margin_util as U
import oracle_lib as O
from poppy_amd import capi

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, number_of_frames=2)
    yield c
    c.close()


@pytest.mark.parametrize("name", U.ADMITTED_IDS)
def test_equals_the_oracle(ctx, name):
    _, w, h, uw, uh = U.BY_NAME[name]
    for kind in U.CONTENTS:
        got = ctx.blur_margin(U.content(kind, w, h), uw, uh)
        want = U.oracle_padded(name, kind)
        assert np.array_equal(got, want), (name, kind, int((got != want).sum()))


STRIDED = ["same_1x1", "same_5x3", "wide_d01", "wide_d03", "wide_d16", "high_d17", "both_30x20_in_47x41", "large_100x60_in_400x300",
           "most_8x900_in_10x900", "most_900x8_in_900x10", "zero_3x3_in_4x4"]


@pytest.mark.parametrize("name", STRIDED)
def test_padded_rows(ctx, name):
    """stride and dst_stride longer than the rows: the pad bytes are neither read (0x5A would show) nor written (the wrapper checks its 0xA5)"""
    _, w, h, uw, uh = U.BY_NAME[name]
    for kind, src_pad, dst_pad in (("noise", 1, 0), ("noise", 0, 5), ("textured", 13, 64), ("impulse", 64, 1)):
        got = ctx.blur_margin(U.content(kind, w, h), uw, uh, src_pad=src_pad, dst_pad=dst_pad)
        assert np.array_equal(got, U.oracle_padded(name, kind)), (name, kind, src_pad, dst_pad)


@pytest.mark.parametrize("name", STRIDED)
def test_non_contiguous_source(ctx, name):
    """the image as a window of a larger one, read in place through its row stride"""
    _, w, h, uw, uh = U.BY_NAME[name]
    img = U.content("noise", w, h)
    big = np.full((h + 5, w + 9, 3), 0x5A, np.uint8)
    big[2:2 + h, 4:4 + w] = img
    window = big[2:2 + h, 4:4 + w]
    assert not window.flags["C_CONTIGUOUS"] or h == 1
    assert np.array_equal(ctx.blur_margin(window, uw, uh), U.oracle_padded(name, "noise")), name


# ---- the image-list path: list_pad on the context's kept scratch -------------------------------------------------------------------
def _to_device(img):
    hip = C.CDLL("libamdhip64.so")
    a = np.ascontiguousarray(img)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return hip, d


def _list_pads(c, a, b, canvas, on_device=False):
    """(image 0 padded, image 1 padded) as morph_list hands them out at phase 0 and phase 1"""
    devs = [_to_device(im) for im in (a, b)] if on_device else []
    try:
        images = [(d.value, im.shape[1], im.shape[0]) for (_, d), im in zip(devs, (a, b))] if on_device else [a, b]
        out = []
        for phase in (0.0, 1.0):
            rc, frames, _, done = c.morph_list(images, phase=phase, canvas=canvas, on_device=on_device)
            assert rc == 0 and done == 1 and len(frames[0]) == 2 and np.array_equal(frames[0][0], frames[0][1])
            out.append(frames[0][0])
        return out
    finally:
        for hip, d in devs:
            hip.hipFree(d)


@pytest.mark.parametrize("on_device", [False, True])
def test_morph_list_canvas_equals_the_oracle(on_device):
    """two images of different sizes per list; then a larger canvas on the same context (the scratch is allocated again), then a
    smaller one (it is kept)"""
    c = capi.Context(0, number_of_frames=2)
    try:
        for (wa, ha), (wb, hb), canvas in (((64, 36), (50, 30), (75, 51)), ((100, 60), (151, 300), (400, 300)), ((30, 20), (47, 3), (47, 41)),
                                            ((8, 900), (10, 1), (10, 900)), ((64, 36), (50, 30), (75, 51))):
            a, b = U.content("noise", wa, ha), U.content("textured", wb, hb)
            got = _list_pads(c, a, b, canvas, on_device)
            assert np.array_equal(got[0], O.blur_margin(a, *canvas)), (wa, ha, canvas)
            assert np.array_equal(got[1], O.blur_margin(b, *canvas)), (wb, hb, canvas)
    finally:
        c.close()


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def _raw(c, src, stride, w, h, uw, uh, dst, dst_stride):
    return capi.lib().poppy_hip_blur_margin(c.h, None if src is None else src.ctypes.data, stride, w, h, uw, uh, None if dst is None else dst.ctypes.data, dst_stride)


def _pads_after(c):
    """the context still pads: 64 x 36 in 75 x 51, on both paths"""
    img = U.content("noise", 64, 36)
    want = U.oracle_padded("both_64x36_in_75x51", "noise")
    assert np.array_equal(c.blur_margin(img, 75, 51), want)
    assert np.array_equal(_list_pads(c, img, U.content("textured", 50, 30), (75, 51))[0], want)


@pytest.mark.parametrize("name", U.REFUSED_IDS)
def test_strips_off_the_canvas_are_refused(name):
    _, w, h, uw, uh = U.BY_NAME[name]
    assert capi.blur_margin_rects(w, h, uw, uh)[0] == E_UNSUPPORTED
    bad = U.content("noise", w, h)
    good = U.content("noise", uw, uh)                      # the canvas's own size: equal sizes, admitted
    assert capi.blur_margin_rects(uw, uh, uw, uh)[0] == 0
    c = capi.Context(0, number_of_frames=2)
    try:
        dst = np.full((uh, uw * 3 + 7), 0xA5, np.uint8)
        assert _raw(c, bad, w * 3, w, h, uw, uh, dst, uw * 3 + 7) == E_UNSUPPORTED
        assert (dst == 0xA5).all(), "the destination was written"
        for images in ([bad, good], [good, bad]):
            for phase in (0.0, -1.0):
                calls = []
                with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                    c.morph_list(images, phase=phase, canvas=(uw, uh), write=lambda k, j, v: calls.append(1))
                assert not calls
        _pads_after(c)
    finally:
        c.close()


def test_argument_errors_leave_the_destination_alone():
    c = capi.Context(0, number_of_frames=2)
    try:
        w, h, uw, uh = 64, 36, 75, 51
        img = np.ascontiguousarray(U.content("noise", w, h))
        dst = np.full((uh, uw * 3), 0xA5, np.uint8)
        cases = {"canvas narrower than the image": (img, w * 3, w, h, w - 1, uh, dst, uw * 3),
                 "canvas lower than the image": (img, w * 3, w, h, uw, h - 1, dst, uw * 3),
                 "short stride": (img, w * 3 - 1, w, h, uw, uh, dst, uw * 3),
                 "short dst_stride": (img, w * 3, w, h, uw, uh, dst, uw * 3 - 1),
                 "null source": (None, w * 3, w, h, uw, uh, dst, uw * 3),
                 "null destination": (img, w * 3, w, h, uw, uh, None, uw * 3),
                 "width 0": (img, w * 3, 0, h, uw, uh, dst, uw * 3),
                 "height 0": (img, w * 3, w, 0, uw, uh, dst, uw * 3),
                 "negative width": (img, w * 3, -w, h, uw, uh, dst, uw * 3)}
        for what, args in cases.items():
            assert _raw(c, *args) == E_ARG, what
            assert (dst == 0xA5).all(), what
        assert capi.lib().poppy_hip_blur_margin(None, img.ctypes.data, w * 3, w, h, uw, uh, dst.ctypes.data, uw * 3) == E_ARG
        assert (dst == 0xA5).all()
        with pytest.raises(capi.PoppyError, match=f": {E_ARG}:"):
            c.morph_list([img, img], phase=0.0, canvas=(w - 1, h))
        _pads_after(c)
    finally:
        c.close()


def test_canvas_rows_above_65535(ctx):
    """4 x 66000: launch_strip_blur puts the strip's rows into grid.y.  The device's maxGridSize[1] decides: a canvas it holds is
    padded == the oracle, one it does not hold is refused up front (POPPY_E_UNSUPPORTED, not a failed launch's POPPY_E_DEVICE)."""
    w = 4
    limit = ctx.blur_margin_max_rows()
    assert limit >= 65535
    heights = [66000] + ([limit, limit + 1] if limit < 70000 else [])         # an MI355X reports 65536: the last height taken, the first refused
    for h in heights:
        img = U.content("noise", w, h)
        if h <= limit:
            want = O.blur_margin(img, w, h)
            assert np.array_equal(ctx.blur_margin(img, w, h), want), h
            assert np.array_equal(_list_pads(ctx, img, U.content("flat3", w, h), (w, h))[0], want), h
        else:
            dst = np.full((h, w * 3), 0xA5, np.uint8)
            assert _raw(ctx, img, w * 3, w, h, w, h, dst, w * 3) == E_UNSUPPORTED and (dst == 0xA5).all(), h
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                ctx.morph_list([img, img], phase=0.0, canvas=(w, h))
    _pads_after(ctx)
