"""Known answers of the oracle's pair set-up on content that reaches its content-dependent branches on purpose: flat, saturated, two-tone and
tie-heavy images (poppy_amd/synth.py: flat_bgr, checker, plateau, dots, near_flat).  Each answer follows by hand from the reference lines cited:

  flat image -> constant foreground, dft_detail2 == 0      src/extractor.cpp:136-229 (every filter of a constant is a constant), src/experiments.hpp:267-318
                                                           (the spectrum of a constant is one DC term, which the detail leaves out) — at sizes that
                                                           getOptimalDFTSize keeps; other sizes are zero-padded first
  equalizeHist of one value -> that value                   OCV/imgproc/src/histogram.cpp (EqualizeHistLut_Invoker: the single-bin case)
  FAST threshold 20 is strict                              OCV/features2d/src/fast.cpp:78-79 (threshold_tab: d < -t / d > t), fast_score.cpp:115-200
  retainBest keeps every tie with the n-th response        OCV/features2d/src/keypoint.cpp:69-90 (nth_element, then partition on >= the n-th response)
  nfeatures of two featureless images                      src/extractor.cpp:40-45: int(300 * 255 / 0.0), cvttsd2si's INT_MIN on x86-64
"""
import numpy as np
import pytest

import oracle_lib as O
from poppy_amd import synth


@pytest.mark.parametrize("w,h", [(97, 61), (128, 96)])
@pytest.mark.parametrize("value", [0, 77, 255, (0, 0, 255), (255, 0, 0)])
def test_flat_image_constant_foreground_zero_detail(w, h, value):
    st = O.foreground(synth.flat_bgr(w, h, value))
    for name in ("grey", "masked", "foreground"):
        a = st[name]
        assert (a == a.flat[0]).all(), name
    d = O.dft_detail2(st["foreground"])
    if (w, h) == (128, 96) or st["foreground"].flat[0] == 0:
        assert d == 0.0                                 # the spectrum of a constant is its DC term alone, which lies outside the bytes the RMS reads
    else:
        assert d > 0.0                                  # 97 x 61 is zero-padded to getOptimalDFTSize (100 x 64): no longer a constant
    g = O.orb_input(st["foreground"])
    assert (g == g.flat[0]).all()                       # a constant ORB input: no FAST candidate at all
    assert len(O.orb_detect(g, 500)) == 0


@pytest.mark.parametrize("value", [0, 1, 77, 128, 254, 255])
def test_equalize_hist_of_one_value_is_that_value(value):
    a = np.full((23, 37), value, np.uint8)
    assert np.array_equal(O.equalize_hist(a), a)
    b = a.copy(); b[5, 7] = 255 - value if value != 127 else 0     # two values: the lower one maps to 0, the upper one to 255
    e = O.equalize_hist(b)
    lo, hi = min(value, int(b[5, 7])), max(value, int(b[5, 7]))
    assert set(np.unique(e).tolist()) == {0, 255} and (e[b == lo] == 0).all() and (e[b == hi] == 255).all()


@pytest.mark.parametrize("base,delta", [(b, d) for b in (0, 100, 255) for d in (-22, -21, -20, -19, 19, 20, 21, 22, 60) if 0 <= b + d <= 255])
def test_fast_threshold_is_strict_on_a_lone_pixel(base, delta):
    """One pixel off by delta on a flat image: all 16 ring pixels differ from it by |delta|, none of its neighbours' rings holds it (radius 3),
    so level 0's FAST list is that pixel alone, with score |delta| - 1, when |delta| > 20, and empty otherwise."""
    w, h = 96, 80
    img = synth.near_flat(w, h, base, 41, 37, delta)
    _, fast = O.orb_detect(img, 500, with_fast=True)
    if abs(delta) > 20:
        assert fast.tolist() == [[41.0, 37.0, float(abs(delta) - 1)]]
    else:
        assert len(fast) == 0


@pytest.mark.parametrize("contrast,corners", [(19, False), (20, False), (21, True), (22, True)])
def test_plateau_contrast_twenty_gives_no_corner(contrast, corners):
    g = synth.plateau(256, 192, 100, contrast)
    assert set(np.unique(g).tolist()) == {100, 100 + contrast}
    assert (len(O.orb_detect(g, 500)) > 0) == corners


@pytest.mark.parametrize("period,nf", [(3, 3), (4, 3), (4, 8), (5, 3), (6, 3), (6, 8), (8, 8)])
def test_checkerboard_keeps_ties_beyond_nfeatures(period, nf):
    """The first level's quota is 1 for nf 3 (2 for nf 8): retainBest(2 x quota) keeps every candidate whose response equals the quota-th one,
    the final retainBest(quota) every tie in Harris response; a checkerboard makes both lists long."""
    k = O.orb_detect(synth.checker(256, 192, period), nf)
    assert len(k) > nf
    if nf == 3:                                     # one level contributes (the other quotas round to 0): one response, repeated
        assert len(np.unique(k[:, 4])) == 1 and len(np.unique(k[:, 5])) == 1


def test_orb_detect_wrapper_sizes_from_the_reported_count():
    """More ties than the wrapper's first guess (2 nf + 64) holds: the count comes back with the refusal and the second call fits exactly."""
    k = O.orb_detect(synth.checker(640, 480, 4), 3)
    assert len(k) > 2 * 3 + 64
    assert len(np.unique(k[:, :2], axis=0)) == len(k)               # every keypoint once, none of the buffer's zero rows


def test_nfeatures_of_featureless_pairs_is_int_min():
    assert O.nfeatures_of(300, 0.0, 0.0) == -2 ** 31
    assert O.nfeatures_of(300, 1e-9, 0.0) == -2 ** 31                 # 7.65e13: no int either
    assert O.nfeatures_of(300, 0.0, 36.5) == int(300 * (255.0 / 36.5))
    assert O.nfeatures_of(300, 2.0, 1.0) == 38250


@pytest.mark.parametrize("v1,v2", [(0, 255), (77, 200), (77, 77)])
def test_two_flat_images_dissolve(v1, v2):
    a, b = synth.flat_bgr(64, 48, v1), synth.flat_bgr(64, 48, v2)
    s = O.pair_setup(a, b)
    assert s["nfeatures"] == -2 ** 31 and s["detail"] == (0.0, 0.0)
    assert len(s["kp1"]) == 0 and len(s["kp2"]) == 0 and len(s["points1"]) == 0
    frames = O.morph(a, b, 3, setup=s)
    want = O.dissolve(a, b, -1.0)
    assert len(frames) == 3 and all(np.array_equal(f, want) for f in frames)
