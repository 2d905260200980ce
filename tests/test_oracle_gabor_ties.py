"""Every builder of tests/gabor_ties_util.py reaches what it is built for — asserted from the oracle's double planes (O.gabor_planes:
gabor_filter_direct's sums before the cast to float) and the util's classify alone, without a GPU.  No target may be missing: a builder
that cannot satisfy a class fails here, so that tests/test_gpu_gabor_ties.py compares the kernels on content that is what its name says.

Measured here: the near-tie search 4.5 s (once per process), the oracle's planes 0.25 s at 120 x 70 x 3, 1.4 s at 256 x 192 x 3 and
0.35 s per 96 x 64 image of the 31-tap bank."""
import numpy as np
import pytest

import gabor_ties_util as U
import oracle_lib as O


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def planes13(img):
    """(planes (h, w, 3, 16), the oracle's float output), the output checked to be the planes' own."""
    src = O.u8_to_f32(img)
    p = O.gabor_planes(src, U.KS13, U.bank(U.KS13))
    out = O.gabor_field(img)
    assert np.array_equal(_bits(U.field_of(p.astype(np.float32))), _bits(out))      # gabor_filter_direct is written on top of the planes
    return p, out


def at(a, t):
    return a[t.y, t.x, t.ch] if a.ndim >= 3 and a.shape[2] == 3 else a[t.y, t.x]


def check_exact_ties(img, targets):
    p, out = planes13(img)
    c = U.classify(p, U.band13())
    seen = set()
    for t in targets:
        v = at(p, t)[t.o]
        assert at(c.mid, t)[t.o] == 0.0, (t, v.hex())                               # exactly the midpoint of two floats ...
        assert 0.0 < v < 1.0, (t, v)                                                # ... inside the clamp
        assert at(c.doubt, t)[t.o] == 2
        assert bool(U.rounds_up(v)) == t.up, t
        f = at(p, t).astype(np.float32)
        g = f.copy(); g[t.o] = U.other_float(v)
        assert abs(int(f[t.o].view(np.int32)) - int(g[t.o].view(np.int32))) == 1
        assert U.field_of(f) == at(out, t) and U.field_of(g) != at(out, t), t       # the other rounding changes the oracle's output float
        assert (t.x, t.y, t.ch) not in seen
        seen.add((t.x, t.y, t.ch))
    return p, c


def test_classify_on_known_values():
    """classify by hand: floats, exact midpoints, the half spacing below a power of two, both signs."""
    s = 2.0 ** -24                                                                   # the spacing of the floats in [0.5, 1)
    v = np.array([0.5 + s / 2, 0.5 + s / 2 + 1e-12, 0.75, 0.5 - s / 4, 0.5 - s / 4 - 1e-12, 0.5 + s / 16, -(0.5 + s / 2 - 1e-12), 1.0 - s / 2, 2.0 ** -12 * (1 + 2.0 ** -24)])
    c = U.classify(v, 1e-13)
    want = [0.0, 1e-12, -s / 2, 0.0, -1e-12, s / 16 + s / 4, 1e-12, 0.0, 0.0]
    assert np.allclose(c.mid, want, rtol=0, atol=2e-16), c.mid
    assert list(c.doubt) == [2, 0, 0, 2, 0, 0, 0, 2, 2]
    assert list(U.classify(np.array([-2e-13, -1e-13, 0.0, 0.99e-13, 1.0 + 0.5e-13, 1.0 + 2e-13]), 1e-13).doubt) == [0, 1, 1, 1, 0, 0]


def test_tie_table_counts():
    """From the oracle's bank alone: 14 196 tap pairs, 5 498 of them with an exact midpoint in (0, 1) in some orientation, and a visible subset in every
    orientation and both directions."""
    K = U.bank(U.KS13).astype(np.float64).reshape(16, -1)
    i, j = np.triu_indices(169, 1)
    s = K[:, i] + K[:, j]
    tie = (U.classify(s, 0.0).mid == 0) & (s > 0) & (s < 1)
    assert len(i) == 14196 and int(tie.any(0).sum()) == 5498
    ti, tj, to, tup = U.tie_rows()
    assert len(ti) > 500
    for o in range(16):
        assert ((to == o) & tup).sum() >= 10 and ((to == o) & ~tup).sum() >= 10, o


def test_ties_on_black_reaches_its_classes():
    img, targets = U.ties_on_black()
    assert img.shape == (70, 120, 3) and set(np.unique(img)) == {0, 255}
    check_exact_ties(img, targets)
    assert {t.up for t in targets} == {False, True}                                  # ties that round-to-even resolves upwards, and downwards
    assert {t.ch for t in targets} == {0, 1, 2}
    assert len({t.o for t in targets}) >= 12
    assert {t.o % 2 for t in targets} == {0, 1}                                      # the real and the imaginary plane of an orientation pair
    for o in range(0, 16, 2):                                                        # ... in every pair of the 8
        assert {o, o + 1} <= {t.o for t in targets}, o
    bx, by = {t.x % U.BLOCK13 for t in targets}, {t.y % U.BLOCK13 for t in targets}
    assert {0, U.BLOCK13 - 1} <= bx and {0, U.BLOCK13 - 1} <= by                     # the first and last column and row of a tile's block
    assert any((t.x % U.BLOCK13, t.y % U.BLOCK13) == (U.BLOCK13 - 1, U.BLOCK13 - 1) for t in targets)
    assert any(5 < t.x % U.BLOCK13 < 46 and 5 < t.y % U.BLOCK13 < 46 and t.x < 104 and t.y < 52 for t in targets)      # an interior one
    assert any(t.x >= 2 * U.BLOCK13 for t in targets) and any(t.y >= U.BLOCK13 for t in targets)                          # the ragged last blocks (16 wide, 18 high)
    assert any(t.x >= 2 * U.BLOCK13 and t.y >= U.BLOCK13 for t in targets)
    assert len(targets) >= 90


@pytest.mark.parametrize("w,h", [(120, 70), (20, 12)])
def test_ties_at_borders_reaches_its_classes(w, h):
    img, targets = U.ties_at_borders(w, h)
    assert img.shape == (h, w, 3)
    check_exact_ties(img, targets)
    for t in targets:                                                                # the window leaves the image, and a placed pixel is read more than once
        assert min(t.x, t.y, w - 1 - t.x, h - 1 - t.y) < 6 and t.mult >= 2, t
        ys, xs = np.nonzero(img[..., t.ch])
        IY, IX = U._window_hits(t.x, t.y, w, h)
        reads = sorted(int(((IY == y) & (IX == x)).sum()) for y, x in zip(ys, xs) if abs(x - t.x) <= 6 and abs(y - t.y) <= 6)
        assert len(reads) == 2 and reads[-1] == t.mult, (t, reads)                   # two white pixels in the window's footprint, counted from the geometry
    assert any(t.mult == 4 for t in targets)                                         # doubly mirrored: in x and in y
    if (w, h) == (120, 70):
        assert any(t.mult == 2 for t in targets)
        near = lambda t: (t.x < 6, t.x >= w - 6, t.y < 6, t.y >= h - 6)
        sides = {near(t) for t in targets}
        for k in range(4):                                                           # every border by itself ...
            assert tuple(i == k for i in range(4)) in sides, k
        for cx in (0, 1):                                                            # ... and every corner, doubly mirrored
            for cy in (2, 3):
                assert any(near(t)[cx] and near(t)[cy] and t.mult == 4 for t in targets), (cx, cy)
    assert {t.up for t in targets} == {False, True} and {t.ch for t in targets} == {0, 1, 2}


def test_ties_in_noise_reaches_its_classes():
    img, targets = U.ties_in_noise()
    assert img.shape == (192, 256, 3) and len(targets) == 16 * 12 * 3
    check_exact_ties(img, targets)
    assert {t.up for t in targets} == {False, True} and len({t.o for t in targets}) == 16
    assert len({(t.x % U.BLOCK13, t.y % U.BLOCK13) for t in targets}) > 100          # all over the tiles' blocks
    outside = np.ones(img.shape[:2], bool)
    for t in targets:
        outside[t.y - 6:t.y + 7, t.x - 6:t.x + 7] = False
    assert set(np.unique(img[outside])) == {0, 255} and 0.45 < (img[outside] == 255).mean() < 0.55     # saturated noise: close to the largest norm a byte image has


def test_many_listed_is_longer_than_a_redo_trip():
    """1024 x 768: the planes from the windows themselves (the oracle takes 24 s there): every target an exact midpoint."""
    img, targets = U.many_listed()
    assert img.shape == (768, 1024, 3) and len(targets) == 3072 * 3 > U.REDO_TRIP
    K = U.bank(U.KS13).astype(np.float64)
    t = np.array([(q.x, q.y, q.ch, q.o) for q in targets])
    win = np.stack([img[y - 6:y + 7, x - 6:x + 7, ch] for x, y, ch, _ in t]).astype(np.float64) / 255.0
    assert (win.reshape(len(t), -1).sum(1) == 2).all()                               # two white pixels on black
    v = np.einsum("nyx,nyx->n", K[t[:, 3]], win)
    assert (U.classify(v, 0.0).mid == 0).all() and (v > 0).all() and (v < 1).all()


@pytest.mark.parametrize("layout", ["black", "noise"])
@pytest.mark.parametrize("kind", ["inside", "outside"])
def test_near_ties_lie_where_their_name_says(kind, layout):
    from poppy_amd import capi
    img, targets = U.near_ties(kind, layout)
    p, _ = planes13(img)
    band = U.band13()
    c = U.classify(p, band)
    for t in targets:
        v, d = at(p, t)[t.o], at(c.mid, t)[t.o]
        assert d == t.dist and U.MIN_VALUE <= v < 1.0, (t, v, d)
        assert U.visible(at(p, t), np.int64(t.o)), t
        if kind == "inside":
            assert 0 < abs(d) <= U.INSIDE and at(c.doubt, t)[t.o] == 2, (t, d)
            assert capi.gabor_rounding_in_doubt(v, band) == 2, t
        else:
            assert band < abs(d) <= 1.5 * band, (t, d)
            assert not at(c.doubt, t).any(), t                                       # no plane of the pixel is in doubt: nothing hands it to the direct sums
            assert not any(capi.gabor_rounding_in_doubt(x, band) for x in at(p, t)), t
    assert {t.dist > 0 for t in targets} == {False, True}                            # on both sides of the midpoint
    assert len(targets) == (96 if layout == "black" else 576)
    if kind == "outside":
        assert min(abs(t.dist) for t in targets) < 1.05 * band                       # as close to the edge as the content allows


def rows31(kind):
    return [r for r in U.GABOR31_ROWS if r[0] == kind]


@pytest.mark.parametrize("n", range(len(U.GABOR31_ROWS)))
def test_every_committed_31_tap_row_verifies(n):
    row = U.GABOR31_ROWS[n]
    gf, t = U.dots31(row)
    us = O.orb_unsharp_gray(gf)
    p = O.gabor_planes(us, U.KS31, U.bank(U.KS31))
    assert np.array_equal(_bits(U.field_of(p.astype(np.float32))), _bits(O.gabor_filter_direct(us, U.KS31, U.bank(U.KS31))))
    band = U.band31(us, t.x, t.y)
    c = U.classify(p[t.y, t.x], band)
    v, d = p[t.y, t.x, t.o], c.mid[t.o]
    assert d == t.dist and U.MIN_VALUE <= v < 1.0 and U.visible(p[t.y, t.x], np.int64(t.o)), (row, v, d)
    if row[0] == "inside":
        assert abs(d) <= U.INSIDE * band / U.band_unit() and c.doubt[t.o] == 2, (row, d, band)
    else:
        assert band < abs(d) <= 1.5 * band and not c.doubt.any(), (row, d, band)


def test_31_tap_rows_cover_both_kinds_and_the_scaled_band():
    assert len(rows31("inside")) >= 1 and len(rows31("outside")) >= 1
    scaled = 0
    for row in U.GABOR31_ROWS:
        gf, t = U.dots31(row)
        scaled += U.band31(O.orb_unsharp_gray(gf), t.x, t.y) > U.band_unit()
    assert scaled >= 2                                                               # us overshoots 1 around white dots: the band follows amax
