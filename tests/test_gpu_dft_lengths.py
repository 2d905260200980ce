"""dft_detail2 at every transform length the padding can produce up to 8640, in both forms of the transform, against the oracle with `==`.

dft_detail2 is the RMS of the raw bytes of a float spectrum (src/experiments.hpp:267-318) and its double sets nfeatures, so one wrong low bit anywhere
in the transform is a different double: there is no tolerance in this file.  The transform is reached through Context.orb_input(gray)["detail"] and
compared with oracle/detail.cpp, whose planner and butterflies are its own.  No length here except those of tests/golden/d_* has a fixture from the
reference: at all the others the kernels are pinned against the oracle only.

What the sizes are for (poppy_amd/csrc/kernels_prefilter2.hip):
  - launch_dft2d_exact runs k_dft_line_wg (a workgroup per line, the line in LDS) while both padded sides are <= 4096 and k_dft_lines (a thread per
    line, in global memory, the column pass strided) otherwise: both forms, both passes, 4096 itself and the lengths on either side of it;
  - the passes of a line follow its factor list (radix 4, at most one radix 2, the 5s, the 3s): every 2^a 3^b 5^c from 2 to 8640 as a row length and
    as a column length, with and without zero padding;
  - k_spectrum_bytes reads a partial float column where the cropped width Nc = N & -2 is no multiple of 4, and the crop itself drops a column where N
    is odd: widths of both kinds, also on the content the normalisation branches on (min == max);
  - the frames of two pixels a side, which setup_size_ok admits;
  - one context that goes from size to size (plans, spectrum buffers and the form are per size in ForegroundFilter::ensure2);
  - whole pairs with a side above 4096: the value of k_dft_lines reaches nfeatures, the points and the frames unchanged."""
import numpy as np
import pytest

import oracle_lib as O
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu

MAX_LEN = 8640
WG_LIMIT = 4096                      # kDftMaxN: the longest line of the workgroup form
OTHER = 6                            # the side that is not under test in the sweep: 2 * 3, nothing special about it


def optimal_dft_size(n):
    """cv::getOptimalDFTSize restated: the next length with no prime factor above 5."""
    m = n
    while True:
        t = m
        for f in (2, 3, 5):
            while t % f == 0:
                t //= f
        if t == 1:
            return m
        m += 1


def exponents(n):
    """(a, b, c) of n = 2^a 3^b 5^c."""
    out = []
    for f in (2, 3, 5):
        k = 0
        while n % f == 0:
            n //= f; k += 1
        out.append(k)
    assert n == 1
    return tuple(out)


S = [n for n in range(2, MAX_LEN + 1) if optimal_dft_size(n) == n]
AXES = ("width", "height")
SWEEP = [(axis, n) for axis in AXES for n in S]


def sweep_inputs(n):
    """The sides that pad to n: n itself, and n - 1 (one zero row or column) where that is a frame side and pads at all."""
    return [n] + ([n - 1] if n - 1 >= 2 and optimal_dft_size(n - 1) == n else [])


def check_sweep_coverage():
    """Conditions on the size list, not measurements: what the sweep claims to reach, asserted before anything is launched."""
    assert len(S) == 167 and S[0] == 2 and S[-1] == MAX_LEN
    for axis in AXES:
        mine = [n for a, n in SWEEP if a == axis]
        assert mine == S, f"{axis}: the sweep leaves out {sorted(set(S) - set(mine))}"                 # the share of S left out is zero
        above = [n for n in mine if n > WG_LIMIT]
        assert len(above) == 31 and above == [n for n in S if n > WG_LIMIT]                             # the thread-per-line form
        assert WG_LIMIT in mine and 4050 in mine and max(n for n in S if n < WG_LIMIT) == 4050          # the workgroup form at and just under its limit
    assert all(sweep_inputs(n)[0] == n for n in S)
    assert sum(len(sweep_inputs(n)) == 2 for n in S) >= 100                                             # the padded inputs are the rule, not the exception
    nc = [n & -2 for n in S]                                                                            # the cropped width of a padded width n
    assert any(c % 4 == 2 for c in nc) and any(c % 4 == 0 for c in nc) and any(n & 1 for n in S)
    assert {6, 10, 18, 30, 50, 54, 90, 150, 250, 270, 75, 135, 243} <= set(S)
    two = [exponents(n)[0] for n in S]
    assert {0, 1, 2, 3} <= set(two) and max(two) >= 4                                                   # power-of-two part: none, 2, 4, 8, >= 16
    assert any(a >= 3 and a & 1 for a in two) and any(a >= 2 and not a & 1 for a in two)                # with and without the radix-2 pass after radix 4
    assert any(exponents(n)[1] >= 5 for n in S) and any(exponents(n)[2] >= 4 for n in S)                # long runs of 3s, of 5s
    assert any(exponents(n)[0] == 0 and exponents(n)[1] and exponents(n)[2] for n in S)                 # 5s and 3s with no power of two
    assert {81, 243, 729, 2187, 6561, 125, 625, 3125, 250, 486, 1250, 12, 20, 36, 4096} <= set(S)
    assert [n for n in S if n < 16] == [2, 3, 4, 5, 6, 8, 9, 10, 12, 15]


@pytest.fixture(scope="module")
def ctx():
    check_sweep_coverage()
    c = capi.Context(0)
    yield c
    c.close()


def _plan(n):
    return capi.dft_plan(n)[0].tolist()


def _detail_eq(ctx, gray, what):
    h, w = gray.shape
    want = O.dft_detail2(gray)
    got = ctx.orb_input(gray)["detail"]
    N, M = optimal_dft_size(w), optimal_dft_size(h)
    rel = abs(got - want) / max(abs(want), 1e-300)
    assert got == want, f"{what}: {w}x{h} -> {N}x{M}, row plan {_plan(N)}, column plan {_plan(M)}: {got!r} != {want!r} (rel {rel:.2e})"
    return got


def test_sweep_covers_what_it_claims():
    check_sweep_coverage()


@pytest.mark.parametrize("axis,n", SWEEP, ids=[f"{a}-{n}" for a, n in SWEEP])
def test_every_length_on_both_axes(ctx, axis, n):
    """n as the padded row length (axis width) or column length (axis height), from a side of n (no padding) and of n - 1 (one zero column or row)."""
    for side in sweep_inputs(n):
        w, h = (side, OTHER) if axis == "width" else (OTHER, side)
        assert optimal_dft_size(side) == n
        gray = synth.textured_gray(w, h, 1000 + n)
        _detail_eq(ctx, gray, f"{axis} {n} {_plan(n)} from a side of {side}")


# (w, h, the form launch_dft2d_exact takes)
FULL_WIDTH = [(4100, 37, "lines"), (37, 4100, "lines"), (4097, 4097, "lines"), (8000, 270, "lines"), (270, 8000, "lines"),
              (4096, 4096, "wg"), (4050, 3888, "wg"), (4096, 4100, "lines")]


@pytest.mark.parametrize("w,h,form", FULL_WIDTH, ids=[f"{w}x{h}-{f}" for w, h, f in FULL_WIDTH])
def test_both_forms_in_both_passes_at_full_width(ctx, w, h, form):
    """Many lines per pass, so that the line index, the pitch and the column stride of both kernels matter: the thread-per-line form with the long side
    in the row pass, in the column pass and in both (4097 x 4097 -> 4320 x 4320), the workgroup form with both sides at its limit, and a side of
    exactly 4096 taken by the thread-per-line form because the other one is longer."""
    N, M = optimal_dft_size(w), optimal_dft_size(h)
    assert (form == "wg") == (N <= WG_LIMIT and M <= WG_LIMIT)
    _detail_eq(ctx, synth.textured_gray(w, h, w + h), f"{form} form")


CONTENT = {
    "flat0": lambda w, h: np.zeros((h, w), np.uint8),
    "flat255": lambda w, h: np.full((h, w), 255, np.uint8),
    "one_pixel": lambda w, h: synth.dots(w, h, positions=[(w // 2, h // 2)]),
    "noise": lambda w, h: synth.uniform_noise(w, h, 11),
}
CONTENT_SIZES = [(6, 5), (10, 10), (75, 100), (250, 54), (243, 81), (4100, 16), (16, 4100)]


@pytest.mark.parametrize("w,h", CONTENT_SIZES, ids=[f"{w}x{h}" for w, h in CONTENT_SIZES])
@pytest.mark.parametrize("name", sorted(CONTENT))
def test_normalisation_branches_at_partial_columns(ctx, name, w, h):
    """A flat image has min == max or nearly so (scale 0, or a huge one), a lone pixel a spectrum of constant magnitude, noise a full-range one — at
    widths whose cropped width is 2 mod 4 (6, 10, 250), odd (75, 243) or served by the thread-per-line form (4100 -> 4320; 16 x 4100)."""
    got = _detail_eq(ctx, CONTENT[name](w, h), name)
    if name == "flat0":
        assert got == 0.0


SMALLEST = [(2, 2), (2, 3), (3, 2), (3, 3), (5, 2), (2, 729), (243, 2)]


@pytest.mark.parametrize("w,h", SMALLEST, ids=[f"{w}x{h}" for w, h in SMALLEST])
def test_smallest_frames(ctx, w, h):
    """Sides of two and three pixels, which setup_size_ok admits.  orb_input also runs the unsharp mask (17 taps) and the Gabor bank (31 x 31) there: their
    reflect-101 index (pyramid_device.h: reflect101) folds as often as it takes, so a side of 2 is defined (period 2) — the stages are compared too."""
    for seed in (1, 2):
        gray = synth.uniform_noise(w, h, 40 + seed)
        _detail_eq(ctx, gray, f"noise {seed}")
        r = ctx.orb_input(gray)
        us = O.orb_unsharp_gray(gray)
        assert np.array_equal(r["us"].view(np.uint32), us.view(np.uint32)), f"{w}x{h}: unsharp grey"
        gb = O.gabor_filter_direct(us, 31, O.gabor_bank(31, 5, 2))
        assert np.array_equal(r["gb"].view(np.uint32), gb.view(np.uint32)), f"{w}x{h}: Gabor mean"
        assert np.array_equal(r["g"], O.orb_input(gray)), f"{w}x{h}: ORB input"
    _detail_eq(ctx, synth.textured_gray(w, h, 3), "textured")


def test_one_context_from_size_to_size(ctx):
    """Plans, spectrum buffers and the choice of form belong to a size (ForegroundFilter::ensure2): lines form -> workgroup form -> lines form with the
    sides swapped -> workgroup form -> the first size again, each equal to the oracle's value and to a fresh context's."""
    sizes = [(8000, 270), (97, 61), (270, 8000), (256, 192), (8000, 270)]
    imgs = {s: synth.textured_gray(s[0], s[1], 77) for s in set(sizes)}
    want = {s: O.dft_detail2(imgs[s]) for s in imgs}
    got = [ctx.orb_input(imgs[s])["detail"] for s in sizes]
    for s, g in zip(sizes, got):
        assert g == want[s], f"{s[0]}x{s[1]} on the travelling context: {g!r} != {want[s]!r} (rel {abs(g - want[s]) / want[s]:.2e})"
    for s in imgs:
        c = capi.Context(0)
        try:
            fresh = c.orb_input(imgs[s])["detail"]
        finally:
            c.close()
        assert fresh == want[s], f"{s[0]}x{s[1]} on a fresh context: {fresh!r} != {want[s]!r}"


def _same(name, got, want):
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    a = got.view(np.uint32) if got.dtype == np.float32 else got
    b = want.view(np.uint32) if want.dtype == np.float32 else want
    neq = a != b
    if neq.any():
        idx = np.argwhere(neq)
        raise AssertionError(f"{name}: {len(idx)} of {got.size} elements differ, first at {idx[0]}, last at {idx[-1]}")


@pytest.mark.parametrize("w,h", [(4100, 64), (64, 4100)], ids=["4100x64", "64x4100"])
def test_whole_pair_with_a_side_above_4096(w, h):
    """pair_begin on a pair whose padded side (4320) is beyond the workgroup form: nfeatures, both details and the prepared points bit for bit as the
    oracle's set-up, then three chained frames.  The pairs are no fallback: at least 20 point pairs (the oracle finds 27 and 26)."""
    a, b = synth.textured_bgr(w, h, 5), synth.textured_bgr(w, h, 6)
    s = O.pair_setup(a, b)
    assert len(s["points1"]) >= 20, f"{w}x{h}: only {len(s['points1'])} point pairs, the pair no longer tests the match"
    c = capi.Context(0, number_of_frames=3)
    try:
        nf, det = c.pair_begin(a, b)
        assert nf == s["nfeatures"] and det == s["detail"], \
            f"{w}x{h}: nfeatures {nf} != {s['nfeatures']} or details {det!r} != {s['detail']!r}; row plan {_plan(optimal_dft_size(w))}, column plan {_plan(optimal_dft_size(h))}"
        p1, p2 = c.pair_points()
        _same(f"{w}x{h} points1", p1, s["points1"])
        _same(f"{w}x{h} points2", p2, s["points2"])
        frames = c.morph_frames(-1.0)
        want = O.morph(a, b, 3, setup=s)
        assert len(frames) == 3
        for j in range(3):
            _same(f"{w}x{h} chained frame {j}", frames[j], want[j])
    finally:
        c.close()
