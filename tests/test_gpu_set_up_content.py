"""The pair set-up on content that reaches its content-dependent branches on purpose (poppy_amd/synth.py: flat, two-tone, tie-heavy, lone pixels
on black, saturated single channels, noise), against the oracle bit for bit:
  - every foreground stage (k_equalize_lut's single-bin branch, the spectrum normalisation with min == max, MOG2 on a constant image, both median kernels);
  - the ORB input and the Gabor banks in their FFT and direct forms (the FFT form's zero-window exemption and its doubt rule next to lone pixels and black
    regions at the border);
  - the detector at nfeatures 0 .. above the candidate count, where retainBest keeps ties (OCV/features2d/src/keypoint.cpp:69-90) and where FAST's threshold
    20 is met exactly, at 256 x 192 and 1080p (the split across three host threads; on noise the candidate lists' re-allocation);
  - whole pairs: set-up (nfeatures, details, prepared points), three chained frames and a phase-mode frame, and the dissolve fallback of featureless pairs."""
import numpy as np
import pytest

import oracle_lib as O
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu

E_NOMATCH = -5
ORDER = ["grey", "flow0", "acc0"] + [f"{s}{i}" for i in range(1, 13) for s in ("med", "flow", "acc", "blur")] + \
        ["lin", "logged", "finalMask", "masked", "foreground"]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(name, got, want):
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    neq = _bits(got) != _bits(want)
    if neq.any():
        idx = np.argwhere(neq)
        raise AssertionError(f"{name}: {len(idx)} of {got.size} elements differ, first at {idx[0]}, last at {idx[-1]}")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _black_border(w, h):
    """Texture in the middle, black bands 0 .. 16 px wide along all four borders (reflect-101 mirrors black into the windows there)."""
    g = synth.textured_gray(w, h, 9)
    g[:, :16] = 0; g[:11, :] = 0; g[:, w - 7:] = 0; g[h - 1:, :] = 0
    return g


# grey images (the foreground takes them as BGR with three equal channels)
GREY = {
    "flat0": lambda w, h: np.zeros((h, w), np.uint8),
    "flat77": lambda w, h: np.full((h, w), 77, np.uint8),
    "flat255": lambda w, h: np.full((h, w), 255, np.uint8),
    "near_flat": lambda w, h: synth.near_flat(w, h, 77),
    "checker4": lambda w, h: synth.checker(w, h, 4),
    "plateau21": lambda w, h: synth.plateau(w, h, 100, 21),
    "dots1": lambda w, h: synth.dots(w, h),
    "dots3": lambda w, h: synth.dots(w, h, size=3),
    "rings": lambda w, h: synth.rings(w, h),
    "black_border": _black_border,
    "noise": lambda w, h: synth.uniform_noise(w, h, 5),
}
BGR = {
    "stripes": lambda w, h: synth.channel_stripes(w, h),
    "noise_bgr": lambda w, h: synth.uniform_noise(w, h, 6, channels=3),
    "red": lambda w, h: synth.flat_bgr(w, h, (0, 0, 255)),
}


def _bgr(name, w, h):
    return BGR[name](w, h) if name in BGR else synth.as_bgr(GREY[name](w, h))


@pytest.mark.parametrize("w,h", [(97, 61), (256, 192)])
@pytest.mark.parametrize("name", sorted(GREY) + sorted(BGR))
def test_foreground_every_stage(ctx, name, w, h):
    img = _bgr(name, w, h)
    want = O.foreground(img)
    got = ctx.foreground(img, debug=True)
    for stage in ORDER:                                 # pipeline order: the first mismatch names the stage that broke
        _same(f"{name} {w}x{h} {stage}", got[stage], want[stage])
    _same(f"{name} {w}x{h} foreground (fused path)", ctx.foreground(img), want["foreground"])


# (name, w, h, the FFT form must have handed pixels to the direct sums)
GABOR_ROWS = [("flat0", 97, 61, False), ("flat77", 97, 61, False), ("flat255", 97, 61, False), ("near_flat", 97, 61, False),
              ("checker4", 97, 61, False), ("rings", 97, 61, False), ("dots1", 97, 61, True), ("dots3", 97, 61, True),
              ("black_border", 97, 61, True), ("dots1", 256, 192, True), ("black_border", 256, 192, True), ("stripes", 97, 61, False)]


@pytest.mark.parametrize("name,w,h,redo", GABOR_ROWS)
def test_orb_input_and_gabor_banks(ctx, name, w, h, redo):
    """ctx.orb_input (unsharp grey, 31-tap Gabor mean, ORB input, detail) and ctx.gabor_field (13-tap bank on the BGR image / 255), FFT form and direct form,
    against the oracle's direct double sums.  Lone pixels on black put a window edge 6 or 15 px (the banks' radii) from a non-zero pixel: the FFT form's
    zero-window ballot decides those windows; black at the border reaches the windows through reflect-101."""
    img = _bgr(name, w, h)
    gf = GREY[name](w, h) if name in GREY else img[..., 1].copy()
    us = O.orb_unsharp_gray(gf)
    gb = O.gabor_filter_direct(us, 31, O.gabor_bank(31, 5, 2))
    g = O.orb_input(gf)
    det = O.dft_detail2(gf)
    field = O.gabor_field(img)
    try:
        for direct in (False, True):
            ctx.set_gabor_direct(direct)
            capi.gabor_doubt()
            r, f = ctx.orb_input(gf), ctx.gabor_field(img)
            doubt = capi.gabor_doubt()
            form = "direct" if direct else "fft"
            _same(f"{name} {w}x{h} {form} us", r["us"], us)
            _same(f"{name} {w}x{h} {form} gb", r["gb"], gb)
            _same(f"{name} {w}x{h} {form} g", r["g"], g)
            assert r["detail"] == det, f"{name} {w}x{h} {form} detail {r['detail']!r} != {det!r}"
            _same(f"{name} {w}x{h} {form} gabor_field", f, field)
            if redo and not direct:
                assert doubt[2] > 0, f"{name} {w}x{h}: the doubt rule handed no pixel to the direct sums {doubt}"
    finally:
        ctx.set_gabor_direct(False)


NF = [0, 1, 2, 3, 8, 50, 500]
DETECT_SMALL = ["checker4", "checker6", "checker8", "checker12", "plateau19", "plateau20", "plateau21", "plateau22", "dots1", "dots3", "rings", "noise"]
# (image, nf) rows where retainBest must keep ties beyond nf (oracle: 40, 54, 20, 26, 16 keypoints)
TIE_ROWS = [("checker4", 3), ("checker4", 8), ("checker6", 3), ("checker6", 8), ("checker8", 8)]


def _detect_image(name, w, h):
    if name.startswith("checker"):
        return synth.checker(w, h, int(name[7:]))
    if name.startswith("plateau"):
        return synth.plateau(w, h, 100, int(name[7:]))
    return GREY[name](w, h)


def _detect_rows(ctx, name, w, h, nfs):
    img = _detect_image(name, w, h)
    out = {}
    for nf in nfs + [w * h + 1]:                       # the last: above any candidate count (no retainBest cuts)
        want = O.orb_detect(img, nf)
        got = ctx.orb_detect(img, nf)
        _same(f"{name} {w}x{h} nf={nf} keypoints", got, want)
        out[nf] = len(want)
    return img, out


@pytest.mark.parametrize("name", DETECT_SMALL)
def test_orb_detect_256x192(ctx, name):
    _, n = _detect_rows(ctx, name, 256, 192, NF)
    for img_name, nf in TIE_ROWS:
        if img_name == name:
            assert n[nf] > nf, f"{name} nf={nf}: {n[nf]} keypoints, the tie rule was not reached"
    if name in ("plateau19", "plateau20"):
        assert n[500] == 0                             # FAST's threshold is strict: contrast 20 is no corner
    if name in ("plateau21", "plateau22"):
        assert n[500] > 0


@pytest.mark.parametrize("name", ["checker4", "plateau21", "dots3", "noise"])
def test_orb_detect_1080p(ctx, name):
    """1080p.  On noise level 0's FAST list (204 837 entries) is longer than the default list of max(4096, w h / 16) = 129 600: the natural re-allocation;
    and more than 2000 level-0 candidates split the host's selection across three threads."""
    w, h = 1920, 1080
    img, n = _detect_rows(ctx, name, w, h, [0, 3, 500])
    _, fast = O.orb_detect(img, 3, with_fast=True)
    if name == "noise":
        assert len(fast) > max(4096, w * h // 16) > 2000
    if name == "checker4":
        assert n[3] > 3                                # ties (level 0's equal scores all fall to the 3 x 3 non-maximum suppression: the ties come from the other levels)


def _shifted_dots(w, h, dx, dy):
    pts = [(40, 50), (200, 40), (128, 100), (60, 150), (190, 160), (100, 70)]
    return synth.as_bgr(synth.dots(w, h, pts, 255, 3)), synth.as_bgr(synth.dots(w, h, [(x + dx, y + dy) for x, y in pts], 255, 3))


def _pairs():
    w, h = 256, 192
    a = synth.checker_bgr(w, h, 6)
    d1, d2 = _shifted_dots(w, h, 5, 3)
    return {
        "identical": (a, a.copy()),
        "checker_shift2": (synth.checker_bgr(w, h, 4), synth.checker_bgr(w, h, 4, phase=2)),
        "dots_shifted": (d1, d2),
        "rings": (synth.as_bgr(synth.rings(w, h)), synth.as_bgr(synth.rings(w, h, radii=(8, 15, 24, 34, 50)))),
        "flat_then_textured": (synth.flat_bgr(w, h, 77), synth.textured_bgr(w, h, 12)),
        "black_white": (synth.flat_bgr(w, h, 0), synth.flat_bgr(w, h, 255)),
        "flat77_flat200": (synth.flat_bgr(w, h, 77), synth.flat_bgr(w, h, 200)),
    }


@pytest.mark.parametrize("pair", list(_pairs()))
def test_pair_set_up_and_frames(pair):
    """A flat image has no keypoints, so a pair with one has no point pairs (the lists are cut to the shorter one, src/extractor.cpp:96-99): the dissolve
    fallback.  Two flat images also have both details 0: nfeatures INT_MIN (include/poppy_hip.h)."""
    a, b = _pairs()[pair]
    featureless = pair in ("black_white", "flat77_flat200")
    nomatch = featureless or pair == "flat_then_textured"
    s = O.pair_setup(a, b)
    assert (len(s["points1"]) == 0) == nomatch
    if featureless:
        assert s["nfeatures"] == O.INT_MIN and s["detail"] == (0.0, 0.0)
    c = capi.Context(0, number_of_frames=3)
    try:
        nf, det = c.pair_begin(a, b)
        p1, p2 = c.pair_points()
        _same(f"{pair} points1", p1, s["points1"])
        _same(f"{pair} points2", p2, s["points2"])
        assert nf == s["nfeatures"] and det == s["detail"], (pair, nf, det, s["nfeatures"], s["detail"])
        rc, frames, _ = c.morph(a, b)
        assert rc == (E_NOMATCH if nomatch else 0)
        assert c.pair_begin_info() == (nf, det)
        want = O.morph(a, b, 3, setup=s)
        assert len(frames) == 3
        for j in range(3):
            _same(f"{pair} chained frame {j}", frames[j], want[j])
        if nomatch:
            for j in range(3):
                _same(f"{pair} frame {j} = dissolve", frames[j], O.dissolve(a, b, -1.0))
    finally:
        c.close()
    c1 = capi.Context(0, number_of_frames=1)
    try:
        rc, fr, _ = c1.morph(a, b, phase=0.4)
        assert rc == (E_NOMATCH if nomatch else 0) and len(fr) == 1
        _same(f"{pair} phase frame", fr[0], O.morph(a, b, 1, phase=0.4, setup=s)[0])
        if nomatch:
            _same(f"{pair} phase frame = dissolve", fr[0], O.dissolve(a, b, 0.4))
    finally:
        c1.close()


@pytest.mark.parametrize("pair", ["noise", "checker"])
def test_pair_set_up_1080p(ctx, pair):
    """Set-up only at 1080p.  The foregrounds and details against the oracle; the ORB inputs are the library's own (their parity is pinned by
    tests/test_gpu_prefilter2.py: the oracle's 31-tap direct sums take minutes at this size); from there nfeatures, both keypoint lists and the
    prepared point pairs against the oracle's detector and matcher."""
    w, h = 1920, 1080
    if pair == "noise":
        a, b = synth.uniform_noise(w, h, 21, channels=3), synth.uniform_noise(w, h, 22, channels=3)
    else:
        a, b = synth.checker_bgr(w, h, 4), synth.checker_bgr(w, h, 4, phase=2)
    fg = []
    for k, img in enumerate((a, b)):
        want = O.foreground(img)["foreground"]
        _same(f"{pair} 1080p foreground {k + 1}", ctx.foreground(img), want)
        fg.append(want)
    g = [ctx.orb_input(f)["g"] for f in fg]
    s = O.pair_setup(a, b, foregrounds=fg, orb_inputs=g, with_gabor2=False)
    nf, det = ctx.pair_begin(a, b)
    assert nf == s["nfeatures"] and det == s["detail"], (pair, nf, det, s["nfeatures"], s["detail"])
    p1, p2 = ctx.pair_points()
    _same(f"{pair} 1080p points1", p1, s["points1"])
    _same(f"{pair} 1080p points2", p2, s["points2"])
    for k in range(2):
        _same(f"{pair} 1080p keypoints {k + 1}", ctx.orb_detect(g[k], nf), s[f"kp{k + 1}"])
