"""The RANSAC fundamental-matrix filter on the GPU — k_ransac_models, k_ransac_score (poppy_amd/csrc/kernels_ransac.hip), poppy_hip_ransac_fundamental and
the set-up poppy_hip_pair_begin_descriptors_ransac — against the host statement poppy_ransac_fundamental (tests/test_host_ransac.py pins that one on
the CPU).  Every comparison is `==`: the mask, the counts of all 2048 hypotheses, `best`, and the models and F as 64-bit patterns.  Sizes on both sides
of the wave (64), of the score kernel's point tile (1024) and of several tiles; the degenerate scenes; coordinates of +-1e6; distances 0, 3 and 1e9; n = 8
and 9, where nearly every hypothesis ties.  NaN and infinite coordinates are not pinned.

Measured on an MI355X with the host statement's share: no test of this file takes longer than 0.1 s, the whole file 1.0 s."""
import ctypes as C

import numpy as np
import pytest

import ransac_util as U
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_NOMATCH = -1, -4, -5
PW, PH = 256, 192


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _same(got, want, label):
    assert np.array_equal(got["counts"], want["counts"]), f"{label}: counts differ at hypotheses {np.flatnonzero(got['counts'] != want['counts'])[:8]}"
    bad = np.flatnonzero((got["models"].view(np.uint64) != want["models"].view(np.uint64)).reshape(len(want["models"]), -1).any(1))
    assert not len(bad), f"{label}: models differ at hypotheses {bad[:8]}"
    assert got["best"] == want["best"] and got["n_inliers"] == want["n_inliers"], label
    assert np.array_equal(got["inliers"], want["inliers"]), label
    assert np.array_equal(got["f"].view(np.uint64), want["f"].view(np.uint64)), label


def _parity(ctx, p1, p2, distance, label):
    want = capi.ransac_fundamental(p1, p2, distance)
    _same(ctx.ransac_fundamental(p1, p2, distance), want, label)
    return want


@pytest.mark.parametrize("n", U.sizes())
def test_parity_at_every_size(ctx, n):
    p1, p2, planted = U.quarter_outliers(n, n) if n >= 32 else U.two_view(n, 0, 0.5, n)
    want = _parity(ctx, p1, p2, 3.0, f"n = {n}")
    if n >= 32:
        assert want["best"] >= 0 and not (want["inliers"].astype(bool) & ~planted).any()


@pytest.mark.parametrize("name", sorted(U.degenerate()))
def test_parity_on_degenerate_scenes(ctx, name):
    p1, p2 = U.degenerate()[name]
    for d in (0.0, 3.0, 1e9):
        _parity(ctx, p1, p2, d, f"{name}, d = {d}")


@pytest.mark.parametrize("scale", [1e6 / U.W, -1e6 / U.W, -1.0])
def test_parity_on_large_and_negative_coordinates(ctx, scale):
    p1, p2, _ = U.quarter_outliers(300, 21)
    s = np.float32(scale)
    _parity(ctx, p1 * s, p2 * s, 3.0 * abs(scale), f"scale {scale}")


@pytest.mark.parametrize("d", [0.0, 3.0, 1e9])
@pytest.mark.parametrize("n", [8, 9, 1025])
def test_parity_at_every_distance_and_on_ties(ctx, n, d):
    p1, p2, _ = U.quarter_outliers(n, 30 + n) if n >= 32 else U.two_view(n, 0, 0.0, 30 + n)
    want = _parity(ctx, p1, p2, d, f"n = {n}, d = {d}")
    if d == 1e9:
        valid = want["counts"] >= 0
        assert (want["counts"][valid] == n).all() and want["best"] == np.flatnonzero(valid)[0]      # every valid hypothesis ties: the lowest wins


def test_parity_among_unrelated_pairs(ctx):
    """no geometry at all: low counts, many of them equal"""
    p1, p2 = U.unrelated(1000, 3)
    _parity(ctx, p1, p2, 3.0, "unrelated pairs")


def test_two_calls_give_the_same_bytes(ctx):
    p1, p2, _ = U.quarter_outliers(4097, 4)
    a, b = ctx.ransac_fundamental(p1, p2, 3.0), ctx.ransac_fundamental(p1, p2, 3.0)
    _same(b, a, "second call")
    small = U.quarter_outliers(65, 5)                                # a smaller problem in the same scratch, then the large one again
    _parity(ctx, small[0], small[1], 3.0, "n = 65 after n = 4097")
    _same(ctx.ransac_fundamental(p1, p2, 3.0), a, "third call")


def test_refusals(ctx):
    p, _, _ = U.quarter_outliers(64, 6)
    inl = np.full(70000, 7, np.uint8); f = np.full(9, 7.0); n_in, best = C.c_int(7), C.c_int(7)
    call = lambda n, d: capi.lib().poppy_hip_ransac_fundamental(ctx.h, _vp(p), _vp(p), n, d, _vp(inl), C.byref(n_in), _vp(f), C.byref(best), None, None)
    for n, d in ((7, 3.0), (65537, 3.0), (64, -1.0), (64, float("nan"))):
        assert call(n, d) == E_ARG
    assert (inl == 7).all() and (f == 7).all() and n_in.value == 7 and best.value == 7


def _pairs():
    a = synth.textured_bgr(PW, PH, 12)
    return {"textured": (a, np.ascontiguousarray(np.roll(a, (2, 3), axis=(0, 1)))), "identical": (a, a.copy()),
            "flat": (synth.flat_bgr(PW, PH, 77), synth.flat_bgr(PW, PH, 200))}


def test_a_resident_pair_is_not_disturbed(ctx):
    a, b = _pairs()["textured"]
    ctx.pair_begin(a, b)
    before = ctx.render(0.5, 0.5)
    points = ctx.pair_points()
    p1, p2, _ = U.quarter_outliers(1025, 7)
    ctx.ransac_fundamental(p1, p2, 3.0)
    after = ctx.render(0.5, 0.5)
    assert np.array_equal(before, after)
    assert all(np.array_equal(x, y) for x, y in zip(points, ctx.pair_points()))
    assert capi.lib().poppy_hip_pair_fundamental(ctx.h, None, None, None, None) == E_STATE      # an ordinary set-up has no fundamental matrix


def _begin(ctx, a, b, ratio, distance=None):
    L = capi.lib()
    if distance is None:
        return L.poppy_hip_pair_begin_descriptors(ctx.h, _vp(a), PW * 3, _vp(b), PW * 3, PW, PH, ratio)
    return L.poppy_hip_pair_begin_descriptors_ransac(ctx.h, _vp(a), PW * 3, _vp(b), PW * 3, PW, PH, ratio, distance)


@pytest.mark.parametrize("ratio", [0.7, 1.0])
def test_set_up_with_the_filter_textured_pair(ctx, ratio):
    a, b = _pairs()["textured"]
    assert _begin(ctx, a, b, ratio) == 0
    plain1, plain2 = ctx.pair_points()
    q1, q2 = plain1[:-4], plain2[:-4]                                 # without the four corners
    assert len(q1) >= 8
    want = capi.ransac_fundamental(q1, q2, 3.0)
    keep = want["inliers"].astype(bool)
    assert _begin(ctx, a, b, ratio, 3.0) == 0, capi.lib().poppy_hip_last_error(ctx.h)
    got1, got2 = ctx.pair_points()
    assert np.array_equal(got1.view(np.uint32), np.concatenate([q1[keep], plain1[-4:]]).view(np.uint32))
    assert np.array_equal(got2.view(np.uint32), np.concatenate([q2[keep], plain2[-4:]]).view(np.uint32))
    f = ctx.pair_fundamental()
    assert f["n_matches"] == len(q1) and f["n_inliers"] == want["n_inliers"] and f["best"] == want["best"]
    assert np.array_equal(f["f"].view(np.uint64), want["f"].view(np.uint64))
    # the existing mode is untouched: the same points as before, and no fundamental matrix behind it
    assert _begin(ctx, a, b, ratio) == 0
    again1, again2 = ctx.pair_points()
    assert np.array_equal(again1.view(np.uint32), plain1.view(np.uint32)) and np.array_equal(again2.view(np.uint32), plain2.view(np.uint32))
    assert capi.lib().poppy_hip_pair_fundamental(ctx.h, None, None, None, None) == E_STATE


def test_set_up_with_the_filter_identical_and_flat_pairs(ctx):
    a, b = _pairs()["identical"]
    assert _begin(ctx, a, b, 0.0) == 0
    plain = ctx.pair_points()
    assert _begin(ctx, a, b, 0.0, 3.0) == 0
    got = ctx.pair_points()
    assert np.array_equal(got[0].view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), plain[1].view(np.uint32))
    f = ctx.pair_fundamental()
    assert f["best"] == -1 and not f["f"].any() and f["n_matches"] == f["n_inliers"] == len(plain[0]) - 4       # identical images: planar-degenerate, no model
    a, b = _pairs()["flat"]
    assert _begin(ctx, a, b, 0.7, 3.0) == E_NOMATCH
    assert capi.lib().poppy_hip_pair_fundamental(ctx.h, None, None, None, None) == E_STATE
    a, b = _pairs()["textured"]
    for ratio, d in ((-1.0, 3.0), (0.7, -1.0), (0.7, float("nan"))):
        assert _begin(ctx, a, b, ratio, d) == E_ARG
