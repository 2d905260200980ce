"""The doubt rule of the FFT form of the Gabor banks by itself (rounding_in_doubt, poppy_amd/csrc/gabor_doubt.h: the one function the
kernel k_gabor_fft and the host export poppy_gabor_rounding_in_doubt share), swept on the host against a restatement in exact rationals.

The images of tests/gabor_ties_util.py reach the rule's midpoint branch inside (0, 1) only: no two-pixel plane value lies within the
band of zero, and none lies just below a power of two, where the float below is half as far away (`h *= 0.5f`).  This sweep is the
only cover of those two branches, and of the exits below -band and above 1 + band.

The restatement: with M the set of midpoints between neighbouring floats, v is
    0  below -band or above 1 + band (the clamp decides either way),
    1  else below band (near zero),
    2  else when some m in M has |v - m| < band,
    0  otherwise.
The kernel forms 1 + band and h - band in double; the restatement forms nothing: it compares fractions.  On every swept value the two
agree (the sweep's values are at least 0.001 band away from the band's edge, a rounding of h - band moves it by 1e-16 band at the most)."""
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

from poppy_amd import capi

UNIT = capi.gabor_band_unit()
BANDS = [UNIT * 1.0, UNIT * 6.5]                               # band x amax, amax in {1, 6.5}
OFFSETS = [0.0, 0.5, 0.999, 1.001, 2.0]


def float_neighbours(v):
    """The floats below and above the double v (both v itself when v is a float)."""
    f = np.float32(v)
    if float(f) == v:
        return f, f
    return (f, np.nextafter(f, np.float32(np.inf))) if float(f) < v else (np.nextafter(f, np.float32(-np.inf)), f)


def expected(v, band):
    """The rule in exact rationals, from the floats around v: the midpoints that can be nearest to v are those of the two float intervals
    v touches (three floats when v is a float itself)."""
    x, b = Fr(v), Fr(band)
    if x < -b or x > 1 + b:
        return 0
    if x < b:
        return 1
    lo, hi = float_neighbours(v)
    fl = sorted({np.nextafter(lo, np.float32(-np.inf)), lo, hi, np.nextafter(hi, np.float32(np.inf))})
    mids = [(Fr(float(p)) + Fr(float(q))) / 2 for p, q in zip(fl, fl[1:])]
    return 2 if min(abs(x - m) for m in mids) < b else 0


def sweep_values(band):
    vals = []
    floats = [np.float32(m) * np.float32(2.0) ** e for e in range(-20, 1) for m in (1.0, 1.0 + 2.0 ** -23, 1.25, 1.5 + 2.0 ** -22, 2.0 - 2.0 ** -23)]
    floats = [f for f in floats if f <= 1.0]
    for f in floats:                                           # a spread of exponents, the floats next to every power of two 2^-20 .. 2^0 among them
        up = np.nextafter(f, np.float32(np.inf))
        m = (float(f) + float(up)) / 2                         # exact: 25 bits
        vals.append(float(f))                                  # an exact float
        for k in OFFSETS:
            vals += [m + k * band, m - k * band]
    for e in range(-20, 0):                                    # just below 2^e: the float below is 2^(e - 24) away, the midpoint 2^(e - 25)
        p = 2.0 ** e
        m = p - 2.0 ** (e - 25)
        for k in OFFSETS:
            vals += [m + k * band, m - k * band]
        vals += [p - k * band for k in OFFSETS] + [p + k * band for k in OFFSETS]
    vals += [-2 * band, -band, 0.0, band, 1 - band, 1.0, 1 + band, 1 + 2 * band]
    vals += [math.nextafter(band, 0.0), math.nextafter(band, 1.0), math.nextafter(-band, -1.0), math.nextafter(1 + band, 2.0), -0.0, 2.0, -1.0, 0.5, 1e-9]
    return vals


@pytest.mark.parametrize("band", BANDS)
def test_rule_against_exact_rationals(band):
    vals = sweep_values(band)
    got = [capi.gabor_rounding_in_doubt(v, band) for v in vals]
    want = [expected(v, band) for v in vals]
    bad = [(v.hex(), g, w) for v, g, w in zip(vals, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    assert {0, 1, 2} <= set(want)                              # every answer is reached ...
    below_pow2 = [w for v, w in zip(vals, want) if 0 < v < 1 and np.float32(v) == 2.0 ** round(math.log2(v)) and v < float(np.float32(v))]
    assert 0 in below_pow2 and 2 in below_pow2                 # ... and the half-spacing branch both ways


def test_rule_agrees_with_classify_on_random_values():
    """The util's classify (np.frexp) states the same rule: on random doubles, on doubles next to random midpoints and on subnormal-free small ones."""
    import gabor_ties_util as U
    rng = np.random.default_rng(5)
    f = rng.uniform(2.0 ** -20, 1.0, 4000).astype(np.float32)
    m = (f.astype(np.float64) + np.nextafter(f, np.float32(2)).astype(np.float64)) / 2
    v = np.concatenate([rng.uniform(-0.1, 1.1, 4000), m + rng.uniform(-3, 3, 4000) * UNIT, rng.uniform(-3, 3, 500) * UNIT, 1 + rng.uniform(-3, 3, 500) * UNIT])
    for band in BANDS:
        c = U.classify(v, band)
        got = np.array([capi.gabor_rounding_in_doubt(x, band) for x in v])
        edge = np.abs(np.abs(c.mid) - band) < 1e-3 * band      # classify forms its distance exactly and compares it with band; skip what a rounding could move
        assert np.array_equal(got[~edge], c.doubt[~edge]), np.nonzero(got != c.doubt)[0][:5]
        assert (c.doubt == 2).sum() > 500 and (c.doubt == 1).sum() > 50
        want = np.array([expected(float(x), band) for x in v[:6000:7]])
        assert np.array_equal(c.doubt[:6000:7], want)          # and classify against the fractions


def test_band_unit_leaves_room_between_the_floats():
    assert 0 < UNIT < 2.0 ** -36                               # far below the spacing of the floats the near-tie targets use (gabor_ties_util.MIN_VALUE)
