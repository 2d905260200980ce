"""The FFT form of the Gabor banks (k_gabor_fft<13>, k_gabor_fft<31>, k_gabor_redo; poppy_amd/csrc/kernels_gabor_fft.hip) on plane values
that lie exactly on, just beside and just outside the doubt band around a float midpoint (tests/gabor_ties_util.py; what each builder
reaches is asserted without a GPU by tests/test_oracle_gabor_ties.py): float bit patterns compared with ==, against the oracle's direct
double sums and against the library's direct form, and the doubt counters read around every FFT call.

  - exact ties (white pixel pairs on black, through mirrored windows at every border and on 20 x 12, inside saturated noise) and near-ties
    within 1e-14 of a midpoint: the rule must flag them and k_gabor_redo must re-form them — near_mid and redone count at least the
    constructed targets.  A wrong sign or exponent in the midpoint test, a lost hand-over for one plane of an orientation pair, or a redo
    kernel that mishandles its second trip (many_listed: 9 216 entries, one trip takes 8 192) shows as a differing float;
  - near-ties between 1.0 and 1.5 bands from a midpoint, which nothing flags: the two forms are equal there only while the transform stays
    within the band of the direct sums — the ruler for the band, at its tightest on saturated 0 / 255 noise;
  - the 31-tap bank on the committed two-dot rows, where the band follows the patch's largest magnitude.

Measured on an MI355X, with the oracle's share, which is most of it: the 256 x 192 noise images 0.93 s each, 120 x 70 0.16 - 0.24 s, 20 x 12
0.01 s, the first near-tie case 1.8 s (it runs the seeded search), a 31-tap row 0.23 s, many_listed 0.07 s; the whole file 9.2 s."""
import functools

import numpy as np
import pytest

import gabor_ties_util as U
import oracle_lib as O
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu

BUILDERS = {
    "ties_on_black": (U.ties_on_black, True),
    "ties_at_borders": (U.ties_at_borders, True),
    "ties_at_borders_20x12": (lambda: U.ties_at_borders(20, 12), True),
    "ties_in_noise": (U.ties_in_noise, True),
    "near_inside_black": (lambda: U.near_ties("inside", "black"), True),
    "near_inside_noise": (lambda: U.near_ties("inside", "noise"), True),
    "near_outside_black": (lambda: U.near_ties("outside", "black"), False),
    "near_outside_noise": (lambda: U.near_ties("outside", "noise"), False),
}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def built(name):
    img, targets = BUILDERS[name][0]()
    want = O.gabor_field(img)
    for a in (img, want):
        a.setflags(write=False)
    return img, targets, want


def same_bits(name, got, want, planes, band):
    """got == want on float bit patterns; else the first differing pixel, its channel and where its 16 plane values lie (planes(): the oracle's doubles)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    neq = got.view(np.uint32) != want.view(np.uint32)
    if not neq.any():
        return
    first = tuple(int(v) for v in np.argwhere(neq)[0])
    y, x = first[:2]
    ch = first[2] if len(first) > 2 else 0
    p = planes()[first]
    b = band(x, y)
    c = U.classify(p, b)
    raise AssertionError(f"{name}: {int(neq.sum())} of {got.size} floats differ, first at x {x} y {y} channel {ch}: {got[first]!r} != {want[first]!r}; band {b:.3e}; "
                         f"planes {[v.hex() for v in p]}; distance to a midpoint {[float(f'{v:.3e}') for v in c.mid]}; to zero {[float(f'{v:.3e}') for v in c.zero]}; doubt {list(c.doubt)}")


def both_forms_13(ctx, img):
    """(FFT form, its doubt counters, direct form) of ctx.gabor_field."""
    try:
        ctx.set_gabor_direct(False)
        capi.gabor_doubt()
        fft = ctx.gabor_field(img)
        doubt = capi.gabor_doubt()
        ctx.set_gabor_direct(True)
        direct = ctx.gabor_field(img)
    finally:
        ctx.set_gabor_direct(False)
    return fft, doubt, direct


@pytest.mark.parametrize("name", list(BUILDERS))
def test_13_tap_bank_on_ties_and_near_ties(ctx, name):
    img, targets, want = built(name)
    fft, (near_zero, near_mid, redone), direct = both_forms_13(ctx, img)
    planes = lambda: O.gabor_planes(O.u8_to_f32(img), U.KS13, U.bank(U.KS13))
    band = lambda x, y: U.band13()
    same_bits(f"{name}: direct form vs oracle", direct, want, planes, band)
    same_bits(f"{name}: FFT form vs oracle", fft, want, planes, band)
    same_bits(f"{name}: FFT form vs direct form", fft, direct, planes, band)
    if BUILDERS[name][1]:                                                            # every constructed target is in the band: flagged and re-formed
        assert near_mid >= len(targets) and redone >= len(targets), (name, len(targets), near_zero, near_mid, redone)


def test_many_listed_takes_the_redo_kernel_round_its_loop(ctx):
    """9 216 exact ties at 1024 x 768 (and the noise's own chance entries): more than the 8 192 entries the redo kernel's 512 workgroups take in one trip.
    Against the direct form only (the oracle needs 24 s here; ties_in_noise at 256 x 192 is the sibling compared with the oracle)."""
    img, targets = U.many_listed()
    fft, (near_zero, near_mid, redone), direct = both_forms_13(ctx, img)
    same_bits("many_listed: FFT form vs direct form", fft, direct, lambda: O.gabor_planes(O.u8_to_f32(img), U.KS13, U.bank(U.KS13)), lambda x, y: U.band13())
    assert redone > U.REDO_TRIP and redone >= len(targets) and near_mid >= len(targets), (len(targets), near_zero, near_mid, redone)


def test_the_list_starts_empty_on_every_launch(ctx):
    """One context through ties_on_black, a texture, and ties_on_black again: the list's count word is cleared per launch, so the results and the counters repeat."""
    img, targets, want = built("ties_on_black")
    tex = synth.textured_bgr(256, 192, 3)
    runs = []
    ctx.set_gabor_direct(False)
    for im in (img, tex, img):
        capi.gabor_doubt()
        out = ctx.gabor_field(im)
        runs.append((out, capi.gabor_doubt()))
    planes = lambda: O.gabor_planes(O.u8_to_f32(img), U.KS13, U.bank(U.KS13))
    for k in (0, 2):
        same_bits(f"ties_on_black, run {k}: FFT form vs oracle", runs[k][0], want, planes, lambda x, y: U.band13())
    assert runs[0][1] == runs[2][1] and runs[0][1][2] >= len(targets), [r[1] for r in runs]
    assert runs[1][0].shape == (192, 256, 3)


@pytest.mark.parametrize("n", range(len(U.GABOR31_ROWS)))
def test_31_tap_bank_on_the_committed_rows(ctx, n):
    row = U.GABOR31_ROWS[n]
    gf, t = U.dots31(row)
    us = O.orb_unsharp_gray(gf)
    want = O.gabor_filter_direct(us, U.KS31, U.bank(U.KS31))
    try:
        ctx.set_gabor_direct(False)
        capi.gabor_doubt()
        a = ctx.orb_input(gf)
        near_zero, near_mid, redone = capi.gabor_doubt()
        ctx.set_gabor_direct(True)
        b = ctx.orb_input(gf)
    finally:
        ctx.set_gabor_direct(False)
    assert np.array_equal(a["us"].view(np.uint32), us.view(np.uint32))               # the bank's input is the oracle's in every bit, so the row is what was searched
    planes = lambda: O.gabor_planes(us, U.KS31, U.bank(U.KS31))
    band = lambda x, y: U.band31(us, x, y)
    same_bits(f"31-tap row {n} {row}: direct form vs oracle", b["gb"], want, planes, band)
    same_bits(f"31-tap row {n} {row}: FFT form vs oracle", a["gb"], want, planes, band)
    same_bits(f"31-tap row {n} {row}: FFT form vs direct form", a["gb"], b["gb"], planes, band)
    assert np.array_equal(a["g"], b["g"])
    if row[0] == "inside":
        assert near_mid >= 1 and redone >= 1, (row, near_zero, near_mid, redone)
