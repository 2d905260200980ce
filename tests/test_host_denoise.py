"""CPU tests of the non-local-means denoise's host statement (include/poppy_hip.h: poppy_denoise_weights, poppy_bgr_denoise; poppy_amd/csrc/denoise.cpp)
against the numpy restatement of tests/denoise_util.py: the weight table and its constants, every image family the GPU test runs, what the restatement
must have reached on the way (so that a family cannot silently stop reaching its branch), and the refusals.  Every comparison is == on bytes."""
import ctypes as C

import numpy as np
import pytest

import denoise_util as U
from poppy_amd import capi

E_ARG, E_UNSUPPORTED = -1, -6


def _table_length(hs, tw, sw):
    return capi.denoise_weights(hs, tw, sw)["L"]


BOUND_HS = U.bound_strengths(_table_length, capi.denoise_table_bound())
CASES = U.cases(capi.denoise_tile(), BOUND_HS)


@pytest.mark.parametrize("hs", [0.5, 3, 10, 20, 40, 100])
@pytest.mark.parametrize("tw,sw", [(7, 21), (5, 21), (3, 7), (7, 3)])
def test_weights_equal_the_restatement(hs, tw, sw):
    want = U.weights(float(hs), tw, sw)
    got = capi.denoise_weights(hs, tw, sw)
    assert (got["n"], got["L"], got["fpm"], got["shift"]) == (want["n"], want["L"], want["fpm"], want["shift"])
    # Where this was written the numpy side has ONE entry within 1e-6 of a half over all 24 tables (hs 100, 5 / 21, a = 26738) and both sides round it
    # the same way: nothing is excused there.  Another libm may move such an entry by 1.
    differs = np.flatnonzero(got["table"].astype(np.int64) != want["table"])
    excused = [a for a in differs if a in want["near_half"] and abs(int(got["table"][a]) - int(want["table"][a])) == 1]
    assert len(excused) == len(differs), differs[:8]
    assert len(excused) <= 2


def test_the_issue_s_constants():
    lengths = {3: 143, 10: 1585, 20: 6340, 40: 25357, 100: 149355}
    for hs, L in lengths.items():
        w = capi.denoise_weights(hs, 7, 21)
        assert (w["fpm"], w["shift"], w["n"], w["L"]) == (38192, 6, 149355, L)
        assert w["table"][0] == 38192 and (np.diff(w["table"].astype(np.int64)) <= 0).all() and (w["table"][L:] == 0).all() and w["table"][L - 1] > 0
    lo, hi = BOUND_HS
    assert _table_length(lo, 7, 21) <= capi.denoise_table_bound() < _table_length(hi, 7, 21)


def test_constants_alone_and_short_tables():
    L = capi.lib()
    n, last, shift, fpm = C.c_int(0), C.c_int(0), C.c_int(0), C.c_uint32(0)
    assert L.poppy_denoise_weights(10.0, 7, 21, None, 0, C.byref(n), C.byref(last), C.byref(fpm), C.byref(shift)) == 0
    assert (n.value, last.value, fpm.value, shift.value) == (149355, 1585, 38192, 6)
    assert L.poppy_denoise_weights(10.0, 7, 21, None, 0, None, None, None, None) == 0
    t = np.full(1000, 0xA5A5A5A5, np.uint32)
    n.value = 0
    assert L.poppy_denoise_weights(10.0, 7, 21, t.ctypes.data, len(t), C.byref(n), None, None, None) == E_ARG
    assert n.value == 149355 and (t == 0xA5A5A5A5).all()
    assert L.poppy_denoise_weights(10.0, 7, 21, None, 5, None, None, None, None) == E_ARG


@pytest.mark.parametrize("name,img,params", CASES, ids=[c[0] for c in CASES])
def test_images_equal_the_restatement(name, img, params):
    assert np.array_equal(capi.bgr_denoise(img, *params), U.denoise(img, *params))


def test_the_all_255_image_reaches_the_32_bit_limit():
    info = {}
    out = U.denoise(U.flat(30, 20, 255), *U.DEFAULT, info=info)
    assert 0 < 2 ** 32 - info["max_est"] < 10 ** 5
    assert (out == 255).all() and np.array_equal(capi.bgr_denoise(U.flat(30, 20, 255), *U.DEFAULT), out)


@pytest.mark.parametrize("params", U.PARAMS[:-1])
def test_the_cutoff_family_sits_on_both_sides_of_L(params):
    info = {}
    U.denoise(U.cutoff(96, 48, *params), *params, info=info)
    assert info["at_last"] > 0 and info["at_cut"] > 0


def test_the_half_tie_family_hits_halves_and_one_short_of_them():
    info = {}
    U.denoise(U.half_ties(80, 40), *U.DEFAULT, info=info)
    r, ws = info["residues"], info["ws"][:, :, None]
    assert (r == 0).any() and (r == ws - 1).any()


def test_saturated_noise_and_single_pixels_come_back_unchanged():
    img = U.saturated_noise(70, 40)
    for params in (U.PARAMS[0], U.DEFAULT):
        assert np.array_equal(capi.bgr_denoise(img, *params), img)
    one = np.array([[[3, 200, 77]]], np.uint8)
    for params in U.PARAMS:
        assert np.array_equal(capi.bgr_denoise(one, *params), one)


def _raw(src, stride, w, h, hs, tw, sw, dst, dst_stride):
    return capi.lib().poppy_bgr_denoise(src, stride, w, h, hs, tw, sw, dst, dst_stride)


REFUSALS = [("hs_zero", dict(hs=0.0), E_ARG), ("hs_negative", dict(hs=-3.0), E_ARG), ("hs_nan", dict(hs=float("nan")), E_ARG),
            ("hs_inf", dict(hs=float("inf")), E_ARG), ("tw_even", dict(tw=4), E_ARG), ("sw_even", dict(sw=20), E_ARG), ("tw_zero", dict(tw=0), E_ARG),
            ("sw_negative", dict(sw=-5), E_ARG), ("w_zero", dict(w=0), E_ARG), ("h_negative", dict(h=-1), E_ARG), ("short_stride", dict(stride=8 * 3 - 1), E_ARG),
            ("short_dst_stride", dict(dst_stride=8 * 3 - 1), E_ARG), ("null_src", dict(src=None), E_ARG), ("null_dst", dict(dst=None), E_ARG),
            ("tw_1", dict(tw=1), E_UNSUPPORTED), ("tw_9", dict(tw=9), E_UNSUPPORTED), ("sw_1", dict(sw=1), E_UNSUPPORTED), ("sw_23", dict(sw=23), E_UNSUPPORTED)]


def refusal_arguments(change):
    """(args of a poppy_bgr_denoise-shaped call with one argument made bad, the destination array)"""
    src = U.gaussian_noise(8, 6)
    dst = np.full((6, 8 * 3), 0xA5, np.uint8)
    a = dict(src=src.ctypes.data, stride=8 * 3, w=8, h=6, hs=10.0, tw=7, sw=21, dst=dst.ctypes.data, dst_stride=8 * 3)
    a.update(change)
    return (a["src"], a["stride"], a["w"], a["h"], a["hs"], a["tw"], a["sw"], a["dst"], a["dst_stride"]), dst, src


@pytest.mark.parametrize("name,change,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_dst_untouched(name, change, status):
    args, dst, _src = refusal_arguments(change)
    assert _raw(*args) == status
    assert (dst == 0xA5).all()
    if "hs" in change or "tw" in change or "sw" in change:
        assert capi.lib().poppy_denoise_weights(args[4], args[5], args[6], None, 0, None, None, None, None) == status


def test_row_padding_on_both_sides_stays_untouched():
    img = U.gaussian_noise(37, 19, seed=9)
    want = capi.bgr_denoise(img, *U.DEFAULT)
    assert np.array_equal(capi.bgr_denoise(img, *U.DEFAULT, row_pad=5, dst_pad=7), want)      # raises if dst's padding was written
