"""blur_margin without a GPU: the oracle, the library's host statement of the geometry (poppy_blur_margin_rects) and of the taps
(poppy_blur_margin_taps) against the independent restatement of blur_margin_util.py, on every geometry x content that
test_gpu_blur_margin.py runs on the device; the sizes whose strips leave the canvas are refused by all three; the cases reach the
branches they are chosen for; and each of the restatement's three wrong variants is caught by a named case."""
import numpy as np
import pytest

import blur_margin_util as U
import golden_util as G
import oracle_lib as O
from poppy_amd import capi

E_ARG, E_UNSUPPORTED = -1, -6


def test_status_values_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "poppy_hip.h")).read()
    for name, value in (("POPPY_E_ARG", E_ARG), ("POPPY_E_UNSUPPORTED", E_UNSUPPORTED)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), hdr) or re.search(r"#define\s+%s\s+\(?%d\)?" % (name, value), hdr), name
    for name in ("poppy_blur_margin_rects", "poppy_blur_margin_taps", "poppy_hip_blur_margin_max_rows"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in capi.SYMBOLS and hasattr(capi.lib(), name)


def test_taps():
    t = U.taps()
    assert capi.blur_margin_taps().tolist() == t
    assert O.gaussian_taps_fx(127, 6.0).tolist() == t
    assert sum(t) == 256 and t == t[::-1] and min(t) >= 0
    nz = [i - 63 for i, v in enumerate(t) if v]
    assert (nz[0], nz[-1]) == (-17, 17) == U.reach(0)
    assert t[63 + 16] == 0 and t[63 + 15] == 1 and t[63 + 17] == 1, "the tail has a hole: error diffusion, not plain rounding"
    assert 255 * 256 * 256 + (1 << 15) < 1 << 32, "the sums fit 32 bits"


@pytest.mark.parametrize("name", U.ADMITTED_IDS)
def test_rects_admitted(name):
    _, w, h, uw, uh = U.BY_NAME[name]
    rects, origin, inside = U.geometry(w, h, uw, uh)
    assert inside
    rc, got, got_origin = capi.blur_margin_rects(w, h, uw, uh)
    assert rc == 0 and got.tolist() == [list(r) for r in rects] and got_origin == origin


@pytest.mark.parametrize("name", U.ADMITTED_IDS)
def test_oracle_equals_the_restatement(name):
    _, w, h, uw, uh = U.BY_NAME[name]
    for kind in U.CONTENTS:
        img = U.content(kind, w, h)
        want, peak = U.padded(img, uw, uh, with_peak=True)
        got = U.oracle_padded(name, kind)
        assert got.shape == want.shape and np.array_equal(got, want), (name, kind, int((got != want).sum()))
        assert peak <= 255, (name, kind, "a blurred value above 255 before the clamp")
        if kind == "flat255":
            rects, (x0, y0), _ = U.geometry(w, h, uw, uh)
            if uw == w and uh == h:                      # no zero margin to blur in: a tap sum of exactly 256 keeps the whole canvas at 255
                assert (got == 255).all(), name
            core = np.zeros((uh, uw), bool)              # the image area outside every strip stays 255, the margin outside every strip 0
            core[y0:y0 + h, x0:x0 + w] = True
            free = np.ones((uh, uw), bool)
            for x, y, rw, rh in rects:
                free[y:y + rh, x:x + rw] = False
            assert (got[core & free] == 255).all() and not got[~core & free].any(), name
        if kind == "flat0":
            assert not want.any(), name


def test_reference_fixtures_still_pass():
    for case in sorted(G.make_inputs.MARGIN):
        inp = G.make_inputs.margin_inputs(case)
        uw, uh = int(inp["cfg"][0]), int(inp["cfg"][1])
        G.check(case, "padded", O.blur_margin(inp["img"], uw, uh))
        G.check(case, "padded", U.padded(inp["img"], uw, uh))


@pytest.mark.parametrize("name", U.REFUSED_IDS)
def test_refused(name):
    _, w, h, uw, uh = U.BY_NAME[name]
    rects, origin, inside = U.geometry(w, h, uw, uh)
    assert not inside
    rc, got, got_origin = capi.blur_margin_rects(w, h, uw, uh)
    assert rc == E_UNSUPPORTED and got.tolist() == [list(r) for r in rects] and got_origin == origin
    assert capi.lib().poppy_blur_margin_rects(w, h, uw, uh, None, None) == E_UNSUPPORTED
    with pytest.raises(ValueError):
        O.blur_margin(np.zeros((h, w, 3), np.uint8), uw, uh)
    with pytest.raises(ValueError):
        U.padded(np.zeros((h, w, 3), np.uint8), uw, uh)


def test_the_table_of_the_out_of_canvas_sizes():
    """the rectangles worked from the formula by hand: the largest admitted sizes and the first refused ones"""
    g = lambda *s: [list(r) for r in U.geometry(*s)[0]]
    assert g(8, 900, 10, 900) == [[0, 0, 10, 900], [0, 0, 10, 900], [0, 0, 10, 1], [0, 898, 10, 1]]
    assert g(1, 200, 2, 200)[:2] == [[0, 0, 2, 200], [0, 0, 2, 200]]
    assert g(8, 1000, 10, 1000)[:2] == [[0, 0, 11, 1000], [-1, 0, 11, 1000]]
    assert g(1, 300, 2, 300)[:2] == [[0, 0, 3, 300], [-1, 0, 3, 300]]
    assert g(1000, 8, 1000, 10)[2:] == [[0, 0, 1000, 11], [0, -1, 1000, 11]]
    assert [r[2] for r in g(3, 3, 4, 4)[:2]] == [0, 0] and [r[3] for r in g(3, 3, 4, 4)[2:]] == [0, 0]
    # the library's condition, (int)dx > UW or (int)dy > UH, is the same as "a rectangle leaves the canvas": over a band of thin sizes
    for w in range(1, 7):
        for h in range(40 * w, 160 * w, 7):
            for d in (1, 2, 3):
                inside = U.geometry(w, h, w + d, h)[2]
                assert (capi.lib().poppy_blur_margin_rects(w, h, w + d, h, None, None) == 0) == inside, (w, h, d)
                assert (capi.lib().poppy_blur_margin_rects(h, w, h, w + d, None, None) == 0) == inside, (h, w, d)


def test_bad_sizes_are_argument_errors():
    f = capi.lib().poppy_blur_margin_rects
    rects = np.full(16, -7, np.int32); origin = np.full(2, -7, np.int32)
    for s in ((0, 5, 5, 5), (5, 0, 5, 5), (-1, 5, 5, 5), (5, 5, 4, 5), (5, 5, 5, 4), (5, 5, 0, 0)):
        assert f(*s, capi._p(rects), capi._p(origin)) == E_ARG, s
    assert (rects == -7).all() and (origin == -7).all()
    assert capi.lib().poppy_blur_margin_taps(None) == E_ARG
    assert capi.lib().poppy_hip_blur_margin_max_rows(None, None) == E_ARG
    with pytest.raises(ValueError):
        O.blur_margin(np.zeros((5, 5, 3), np.uint8), 4, 5)


def test_branch_reach():
    """asserted from the restatement alone"""
    geo = {n: U.geometry(*U.BY_NAME[n][1:])[0] for n in U.ADMITTED_IDS}
    sweep_w = {geo[n][0][2] for n in U.ADMITTED_IDS if n.startswith("wide_d")}
    sweep_h = {geo[n][2][3] for n in U.ADMITTED_IDS if n.startswith("high_d")}
    assert sweep_w == set(range(1, 22)) == sweep_h, "the sweeps reach every strip width and height 1 ... 21"
    folds = {U.folds_needed(k) for k in sweep_w}
    assert 1 in folds and max(folds) >= 2, folds
    assert U.folds_needed(17) == 2 and U.folds_needed(18) == 1 and U.folds_needed(2) == 17 and U.folds_needed(151) == 1
    # a right strip that stops short of the last column (odd difference: dx is fractional), and a bottom strip likewise
    short_x = [n for n in U.ADMITTED_IDS if geo[n][1][2] and geo[n][1][0] + geo[n][1][2] < U.BY_NAME[n][3]]
    short_y = [n for n in U.ADMITTED_IDS if geo[n][3][3] and geo[n][3][1] + geo[n][3][3] < U.BY_NAME[n][4]]
    assert "wide_d03" in short_x and "high_d03" in short_y and "both_64x36_in_75x51" in short_x and "both_64x36_in_75x51" in short_y
    assert "same_5x3" in short_x and "same_5x3" in short_y, "1.3: the strip is the last column but one"
    assert "wide_d02" not in short_x and "both_30x20_in_47x41" not in short_x + short_y, "whole dx: the strip ends on the last column"
    # both forms of the 1-wide strip: 1.3 on equal sizes, and dx + margin = 0.5 + 1.0
    assert geo["same_5x3"][0][2] == 1 and geo["same_5x3"][2][3] == 1
    assert geo["wide_d01"][0][2] == 1 and U.BY_NAME["wide_d01"][3] != U.BY_NAME["wide_d01"][1]
    assert geo["high_d01"][2][3] == 1
    # 0-wide strips
    assert [r[2] for r in geo["zero_3x3_in_4x4"][:2]] == [0, 0] and [r[3] for r in geo["zero_10x10_in_11x11"][2:]] == [0, 0]
    # the largest admitted: both side strips are the whole canvas
    assert geo["most_8x900_in_10x900"][0] == geo["most_8x900_in_10x900"][1] == (0, 0, 10, 900)
    assert geo["most_900x8_in_900x10"][2] == geo["most_900x8_in_900x10"][3] == (0, 0, 900, 10)
    # more than one workgroup of 256 in x from a side strip, wider than the taps reach
    assert geo["large_100x60_in_400x300"][0][2] == 151 and geo["large_100x60_in_400x300"][2][3] == 121 and 151 * 3 > 256
    # overlapping corners: a side strip and the top strip share pixels
    assert geo["both_30x20_in_47x41"][0][2] > 0 and geo["both_30x20_in_47x41"][2][3] > 0


CONTROLS = {                                           # wrong variant -> the (case, content) that must show it
    "from_output": [("both_30x20_in_47x41", "noise"), ("same_5x3", "noise"), ("both_64x36_in_75x51", "impulse")],
    "top_bottom_first": [("both_30x20_in_47x41", "noise"), ("same_5x3", "noise"), ("both_64x36_in_75x51", "textured")],
    "fold_once": [("wide_d03", "noise"), ("high_d09", "checker"), ("wide_d20", "textured"), ("most_1x200_in_2x200", "noise")],
}


@pytest.mark.parametrize("variant", sorted(CONTROLS))
def test_negative_controls(variant):
    for name, kind in CONTROLS[variant]:
        _, w, h, uw, uh = U.BY_NAME[name]
        wrong = U.padded(U.content(kind, w, h), uw, uh, variant=variant)
        right = U.oracle_padded(name, kind)
        assert not np.array_equal(wrong, right), f"the wrong variant '{variant}' changes nothing on {name} / {kind}: the case is too weak"


def test_negative_controls_where_the_variant_is_right():
    """the counterpart: where a wrong variant's fault cannot show, it agrees — the controls fail for their reason"""
    _, w, h, uw, uh = U.BY_NAME["large_100x60_in_400x300"]
    img = U.content("noise", w, h)
    assert np.array_equal(U.padded(img, uw, uh, variant="fold_once"), U.padded(img, uw, uh)), "strips wider than 17 fold once at most"
    _, w, h, uw, uh = U.BY_NAME["wide_d09"]                                # top and bottom strips 1 high, side strips: they still overlap
    flat = U.content("flat3", w, h)
    assert np.array_equal(U.padded(flat, 64, 36, variant="top_bottom_first"), U.padded(flat, 64, 36))


def test_channels_are_independent():
    """a wrong channel index in e = x * 3 + c would mix them: the three flat values give three different margins"""
    _, w, h, uw, uh = U.BY_NAME["both_64x36_in_75x51"]
    out = U.oracle_padded("both_64x36_in_75x51", "flat3")
    one = [U.padded(np.full((h, w, 3), v, np.uint8), uw, uh)[..., 0] for v in (10, 128, 250)]
    for c in range(3):
        assert np.array_equal(out[..., c], one[c])
    assert not np.array_equal(out[..., 0], out[..., 1]) and not np.array_equal(out[..., 1], out[..., 2])
