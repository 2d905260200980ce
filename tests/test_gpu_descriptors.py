"""The descriptor path — k_orb_blur, k_orb_describe, k_hamming, k_hamming_knn2 (poppy_amd/csrc/kernels_orb.hip), OrbDetector::describe /
hamming / hamming_knn2 and the opt-in set-up poppy_hip_pair_begin_descriptors — on inputs built to reach their branches
(tests/descriptor_util.py; tests/test_oracle_descriptors.py asserts on the CPU that they do): steered coordinates that are exact k + 0.5
ties, angles at which a fused product of the rotation moves a coordinate, flat and two-valued images, keypoints in and beyond the
unblurred reflect-101 ring up to both ends of the accepted range, on a 20 x 16 image whose ring is reflected many times, 0 to 65 537
keypoints, calls that rebuild only some levels; every train length around the lane count and the tile size of the Hamming kernels, ties
across every lane and tile, planted nearest neighbours in one lane, two lanes, two tiles, distances 0 and 256; the descriptor set-up on
a textured, an identical and a flat pair.  Every comparison is `==` on bytes or ints, against the oracle (describe, set-up) and the numpy
references (Hamming), which tests/test_oracle_descriptors.py ties to the oracle.  NaN and infinite angles and coordinates are not
pinned.

Measured on an MI355X with the oracle's share: no test of this file takes longer than 0.3 s (the 65 537-keypoint rows 0.2 s), the whole
file 2.3 s."""
import ctypes as C

import numpy as np
import pytest

import descriptor_util as U
import oracle_lib as O
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu
E_ARG, E_NOMATCH = -1, -5


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _check_describe(ctx, family, label, img, kps):
    want = U.oracle_describe(family)[label]
    got = ctx.orb_describe(img, kps)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(1))
    assert not len(bad), f"{label}: {len(bad)} of {len(kps)} descriptors differ, first row {bad[0]}: keypoint {kps[bad[0]].tolist()}"


@pytest.mark.parametrize("family", [f for f, _ in U.describe_cases()])
def test_describe_families_vs_oracle(ctx, family):
    for label, img, kps in dict(U.describe_cases())[family]():
        _check_describe(ctx, family, label, img, kps)


def test_describe_level_subsets_vs_oracle(ctx):
    """Image A with all octaves, then image B with octave 0 only (levels 1..7 of the atlas are still A's), then B with octave 7 only."""
    for label, img, kps in U.level_subsets():
        _check_describe(ctx, "level_subsets", label, img, kps)


def test_grown_keypoint_buffers_serve_the_detector(ctx):
    """65 537 keypoints make describe swap every keypoint buffer (a new image size would allocate them afresh, so everything here is
    97 x 80): the detector on the same context and size then runs in the swapped buffers, and so does a second, small describe."""
    w, h = 97, 80
    img = U.noise(w, h, 46)
    kps = U.random_keypoints(U.KP_CAP + 1, w, h, 11)
    assert np.array_equal(ctx.orb_describe(img, kps), O.orb_describe(img, kps))
    g = synth.textured_gray(w, h, 3)
    want = O.orb_detect(g, 50)
    got = ctx.orb_detect(g, 50)
    assert len(want) > 8 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ctx.orb_describe(g, want), O.orb_describe(g, want))
    few = U.random_keypoints(9, w, h, 12)
    assert np.array_equal(ctx.orb_describe(img, few), O.orb_describe(img, few))


def test_describe_refusals(ctx):
    """One level coordinate past either end of the accepted range on either axis, and octaves -1 and 8, are POPPY_E_ARG; the context then
    describes a valid set."""
    L = capi.lib()
    img = np.ascontiguousarray(U.noise())
    valid = U.random_keypoints(9)
    out = np.zeros((10, 32), np.uint8)
    for what, row in U.refused_rows():
        for at in (0, 9):                                            # alone at the front, and behind nine valid keypoints
            k = np.ascontiguousarray(np.concatenate([valid[:at], np.array([row], np.float32)]), np.float32)
            rc = L.poppy_hip_orb_describe(ctx.h, _vp(img), U.W, U.W, U.H, _vp(k), len(k), _vp(out))
            assert rc == E_ARG, f"{what}: {rc}"
        _check_describe(ctx, "counts9", "counts9", img, valid)


@pytest.mark.parametrize("family", sorted({f for f, _, _ in U.hamming_cases()}))
def test_hamming_families_vs_reference(ctx, family):
    for f, label, _ in U.hamming_cases():
        if f != family:
            continue
        q, t, match, knn = U.hamming_reference(f, label)
        got = ctx.hamming_match(q, t)
        assert got.shape == match.shape and np.array_equal(got, match), f"{f} {label}: match rows {np.flatnonzero((got != match).any(1))[:5]}"
        got = ctx.hamming_knn2(q, t)
        assert got.shape == knn.shape and np.array_equal(got, knn), f"{f} {label}: knn2 rows {np.flatnonzero((got != knn).any(1))[:5]}"


# ---- poppy_hip_pair_begin_descriptors at 256 x 192 --------------------------------------------------------------------------------------
PW, PH = 256, 192


def _pairs():
    a = synth.textured_bgr(PW, PH, 12)
    return {"textured": (a, np.ascontiguousarray(np.roll(a, (2, 3), axis=(0, 1)))), "identical": (a, a.copy()),
            "flat": (synth.flat_bgr(PW, PH, 77), synth.flat_bgr(PW, PH, 200))}


@pytest.fixture(scope="module")
def foregrounds():
    """The oracle's goodFeatures of every image, computed once."""
    pairs = _pairs()
    fg = {name: [O.foreground(img)["foreground"] for img in pairs[name]] for name in ("textured", "flat")}
    fg["identical"] = [fg["textured"][0], fg["textured"][0]]
    return fg


def _begin_descriptors(ctx, a, b, ratio):
    return capi.lib().poppy_hip_pair_begin_descriptors(ctx.h, _vp(a), PW * 3, _vp(b), PW * 3, PW, PH, ratio)


def _expected_points(ctx, a, b, fg, ratio):
    """As test_pair_set_up_1080p and test_pair_begin_descriptors_mode build it: the oracle's foregrounds, the library's own ORB inputs (their
    parity is pinned elsewhere), then the oracle's detector, descriptors, 2-NN both ways, ratio and symmetry rule, and the four corners."""
    g = [ctx.orb_input(f)["g"] for f in fg]
    s = O.pair_setup(a, b, foregrounds=fg, orb_inputs=g, with_gabor2=False)
    kp1, kp2 = s["kp1"], s["kp2"]
    d1, d2 = O.orb_describe(g[0], kp1), O.orb_describe(g[1], kp2)
    sym = O.ratio_symmetry(O.hamming_knn2(d1, d2), O.hamming_knn2(d2, d1), ratio)[2]
    corners = np.array([[0, 0], [PW - 1, 0], [0, PH - 1], [PW - 1, PH - 1]], np.float32)
    return s["nfeatures"], sym, np.concatenate([kp1[sym[:, 0], :2], corners]), np.concatenate([kp2[sym[:, 1], :2], corners])


@pytest.mark.parametrize("pair,ratio", [("textured", 0.7), ("textured", 1.0), ("identical", 0.0)])
def test_pair_begin_descriptors_vs_oracle(ctx, foregrounds, pair, ratio):
    a, b = _pairs()[pair]
    nf, sym, want1, want2 = _expected_points(ctx, a, b, foregrounds[pair], ratio)
    assert _begin_descriptors(ctx, a, b, ratio) == 0, capi.lib().poppy_hip_last_error(ctx.h)
    assert ctx.pair_begin_info()[0] == nf
    p1, p2 = ctx.pair_points()
    assert len(sym) > 20                                              # (identical images at ratio 0: the self-matches at distance 0 survive)
    if pair == "identical":
        assert (sym[:, 0] == sym[:, 1]).all() and (sym[:, 2] == 0).all()
    assert np.array_equal(p1.view(np.uint32), want1.view(np.uint32)) and np.array_equal(p2.view(np.uint32), want2.view(np.uint32))


def test_pair_begin_descriptors_flat_pair_then_an_ordinary_set_up(ctx, foregrounds):
    """A flat pair has no keypoints: POPPY_E_NOMATCH.  The context then sets up a textured pair the ordinary way, as the oracle does."""
    a, b = _pairs()["flat"]
    nf, sym, _, _ = _expected_points(ctx, a, b, foregrounds["flat"], 0.7)
    assert len(sym) == 0 and nf == O.INT_MIN
    assert _begin_descriptors(ctx, a, b, 0.7) == E_NOMATCH
    a, b = _pairs()["textured"]
    fg = foregrounds["textured"]
    s = O.pair_setup(a, b, foregrounds=fg, orb_inputs=[ctx.orb_input(f)["g"] for f in fg], with_gabor2=False)
    got_nf, det = ctx.pair_begin(a, b)
    assert got_nf == s["nfeatures"] and det == s["detail"]
    p1, p2 = ctx.pair_points()
    assert len(s["points1"]) > 4
    assert np.array_equal(p1.view(np.uint32), s["points1"].view(np.uint32)) and np.array_equal(p2.view(np.uint32), s["points2"].view(np.uint32))


def test_pair_begin_descriptors_refuses_bad_ratios(ctx):
    a, b = _pairs()["textured"]
    for ratio in (-1.0, float("nan")):
        assert _begin_descriptors(ctx, a, b, ratio) == E_ARG
