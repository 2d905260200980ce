"""What the inputs of unsharp_content_util.py are built for, asserted from the oracle alone (no GPU): test_gpu_unsharp_content.py runs the kernels on the same
inputs, and these tests are the evidence that the content-dependent branches are then reached — the double re-formation of the sharpen decision on both sides
of its bound, half-to-even ties of the 8-bit conversion, both of its clamps and the 2^31 case, and both clamps of the blend mask.  The conditions are caps on
the inputs, not measurements of the kernels."""
import numpy as np
import pytest

import oracle_lib as O
import unsharp_content_util as U


def _ids(seq):
    return ["x".join(str(v) for v in s[:2]) for s in seq]


def test_norm2_min_is_the_smallest_double_that_reaches_the_threshold():
    x = U.norm2_min()
    assert x == 0.0900000071525575
    assert np.sqrt(np.float64(x)) >= np.float64(U.THRESHOLD) > np.sqrt(np.nextafter(np.float64(x), 0.0))


@pytest.mark.parametrize("w,h,seed", U.THRESHOLD_SIZES, ids=_ids(U.THRESHOLD_SIZES))
def test_threshold_images_sit_on_the_bound(w, h, seed):
    T = U.threshold_images(w, h, seed)
    c = T["centres"]
    cx, cy = c[:, 0], c[:, 1]
    d = np.abs(c[:, None, :] - c[None, :, :]).max(axis=2)
    assert (d[~np.eye(len(c), dtype=bool)] >= U.MIN_APART).all(), "no patch in another's footprint"
    bound, t2f = U.norm2_min(), np.float32(U.norm2_min())
    counts = {}
    for side in ("below", "above"):
        out, _, med = O.unsharp(T[side], 1.0, U.THRESHOLD)
        n2, nf = U.norm2_double(med)[cy, cx], U.norm2_float(med)[cy, cx]
        sharp = n2 >= bound
        assert (sharp == (side == "above")).all(), f"{side}: every centre on its side of the bound by the oracle's double sum"
        # the oracle's own decision is that of the double sum against norm2_min: the centre pixel changes exactly when it says so
        changed = (out[cy, cx] != T[side][cy, cx]).any(axis=1)
        assert (changed == sharp).all()
        win = U.in_window(nf)
        disagree = (nf > t2f) != sharp
        # Over the whole image the two decisions differ at those centres and at nothing but pixels that share a centre's median: the neighbours of a patch
        # cut by the frame's edge, whose replicated 3 x 3 window holds the same nine values.  A kernel that decided by the float sum alone would be wrong
        # at exactly these pixels (the pull request that added this file ran that once: 11 / 64 pixels at 256 x 256, 11 / 44 at 253 x 189).
        ys, xs = np.nonzero((U.norm2_float(med) > t2f) != (U.norm2_double(med) >= bound))
        assert (np.abs(c[None, :, :] - np.stack([xs, ys], 1)[:, None, :]).max(axis=2).min(axis=1) <= 1).all()
        assert set(zip(cx[disagree].tolist(), cy[disagree].tolist())) <= set(zip(xs.tolist(), ys.tolist()))
        counts[side] = (int(win.sum()), int(disagree.sum()), len(xs))
        assert win.sum() >= 0.9 * len(c), f"{side}: {win.sum()} of {len(c)} centres inside the kernels' window"
        assert disagree.sum() >= 4, f"{side}: {disagree.sum()} centres where the float sum alone decides the other way"
        assert (win | ~disagree).all(), "a disagreeing centre outside the window would be the kernels' claim broken, not an input for it"
        assert np.abs(n2 / bound - 1).max() <= 4e-7
    print(f"{w}x{h}: {len(c)} centres; in the window / centres with the float decision opposite / pixels with it opposite: below {counts['below']}, above {counts['above']}")
    for name, vals, period, residues in (("tile columns", cx, 32, (31, 0)), ("strip columns", cx, 60, (59, 0)), ("tile rows", cy, 16, (15, 0)),
                                         ("segment rows", cy, 8, (7, 0))):
        assert set(residues) <= set((vals % period).tolist()), f"centres either side of the {name}"
    assert {0, w - 1} <= set(cx.tolist()) and {0, h - 1} <= set(cy.tolist()), "centres on the frame's first and last column and row"


def test_tie_values_are_exact_halves():
    t = U.tie_values()
    assert t.dtype == np.float32 and len(t) == 255
    assert (t * np.float32(255.0) == np.arange(255, dtype=np.float32) + np.float32(0.5)).all()


def test_tie_image_rounds_half_to_even_and_saturates():
    T = U.tie_image()
    img = T["img"]
    assert img.shape == (U.TIE_H, U.TIE_W, 3) and np.isfinite(img).all() and not np.signbit(img[img == 0]).any()
    out, _, _ = O.unsharp(img, 0.0, U.THRESHOLD)
    assert (out.view(np.uint32) == img.view(np.uint32)).all(), "amount 0: the conversion's input is the source itself"
    b = O.f32_to_u8(out)
    seen = set()
    for x, y, ch, v, kind, k in T["cells"]:
        got = b[y, x] if ch < 0 else b[y, x, ch:ch + 1]
        assert (img[y, x] == v).all() if ch < 0 else img[y, x, ch] == v
        if kind == "tie":
            want = k if k % 2 == 0 else k + 1
            seen.add(k)
        elif kind == "under":
            want = k
        elif kind == "over":
            want = k + 1
        else:
            want = 0 if v < 0 else 255
            assert v < 0 or v > 1
        assert (got == want).all(), f"{kind} {k} at ({x}, {y}) channel {ch}: {got} != {want}"
    assert seen == set(range(255))
    lo, hi = U.two31_values()
    assert np.float32(lo * np.float32(255)) == np.float32(2147483520.0) and np.float32(hi * np.float32(255)) >= np.float32(2.0 ** 31)
    assert [(n, byte) for n, _, _, byte in T["huge"]] == [("below_2_31", 255), ("at_2_31", 0), ("plus_1e8", 0), ("minus_1e8", 0)]
    for name, x, y, byte in T["huge"]:
        assert (b[y - 1:y + 2, x - 1:x + 2] == byte).all(), name
    out1, _, _ = O.unsharp(img, 1.0, U.THRESHOLD)
    assert np.isfinite(out1).all()


@pytest.mark.parametrize("w,h", U.STRUCT_SIZES, ids=_ids(U.STRUCT_SIZES))
@pytest.mark.parametrize("name", U.STRUCT_NAMES)
def test_structure_overshoots_on_both_sides(name, w, h):
    src = U.structure_f32(name, w, h)
    assert src.min() == 0 and src.max() == 1
    for amount in U.AMOUNTS:
        out, _, _ = O.unsharp(src, amount, U.THRESHOLD)
        if amount == 0:
            assert (out == src).all()
            continue
        assert (out < 0).any() and (out > 1).any(), f"amount {amount}: overshoot below 0 and above 1"
        b = O.f32_to_u8(out)
        assert (b[out < 0] == 0).all() and (b[out > 1] == 255).all()


@pytest.mark.parametrize("name", U.flat_names())
def test_flat_images_are_not_sharpened(name):
    src = U.structure_f32(name, 97, 61)
    out, _, med = O.unsharp(src, 1.0, U.THRESHOLD)
    assert (med == 0).all() and (out == src).all()


def test_one_pixel_crops_are_decided_both_ways():
    """The 1 x 40 and 40 x 1 crops (the separable kernels' sqrt(double sum) >= threshold) hold sharpened and unsharpened pixels, ties and both clamps."""
    took = {False: 0, True: 0}
    lo = hi = ties = 0
    for src, axis, at in U.ONE_PIXEL_CROPS:
        img = U.named_input(("crop", src, axis, at))
        assert img.shape == ((40, 1, 3) if axis == "col" else (1, 40, 3))
        out, _, med = O.unsharp(img, 1.0, U.THRESHOLD)
        s = np.sqrt(U.norm2_double(med)) >= float(U.THRESHOLD)
        took[True] += int(s.sum()); took[False] += int((~s).sum())
        lo += int((out < 0).sum()); hi += int((out > 1).sum())
        p = img * np.float32(255.0)
        ties += int(((p - np.floor(p) == 0.5) & (p > 0) & (p < 255)).sum())
    assert took[True] >= 40 and took[False] >= 40, took
    assert lo >= 10 and hi >= 10 and ties >= 40, (lo, hi, ties)


@pytest.mark.parametrize("w,h,lazy", U.FRAME_GEOMS, ids=_ids(U.FRAME_GEOMS))
def test_mask_fields_reach_both_clamps(w, h, lazy):
    g = U.mask_field(w, h)
    for r in U.MASK_RATIOS:
        un, m = U.mask_unclamped(g, r), O.blend_mask(g, r)
        assert (np.clip(un, 0, 1).view(np.uint32) == m.view(np.uint32)).all()
        below, above, inside = un < 0, un > 1, (m > 0) & (m < 1)
        assert (m[below] == 0).all() and (m[above] == 1).all()
        if r == 0:                     # 1 - 2 r + r * grey: exactly 1 everywhere
            assert (m == 1).all()
            continue
        assert above.sum() >= 50 and inside.sum() >= 50, f"ratio {r}: {above.sum()} clamped at 1, {inside.sum()} inside"
        if r >= 0.5:                   # under 0 where grey < 2 - 1 / r: ratio 0.3 would need grey < -1.33 (unsharp_content_util.mask_field)
            assert below.sum() >= 50, f"ratio {r}: {below.sum()} clamped at 0"


@pytest.mark.parametrize("w,h,lazy", U.FRAME_GEOMS, ids=_ids(U.FRAME_GEOMS))
def test_frame_cases_reach_the_conversion_clamps(w, h, lazy):
    """Through the warps and the pyramid the unsharp's input is no longer within [0, 1], and its output overshoots on both sides in every pair."""
    for pi in range(len(U.FRAME_PAIRS)):
        lo = hi = False
        for r in U.MASK_RATIOS:
            d = U.frame_case(w, h, pi, r)[6][2]
            lo |= bool((d["unsharp"] < 0).any()); hi |= bool((d["unsharp"] > 1).any())
            if r in (0.5, 0.75, 1.0):
                assert (d["lbmask"] == 0).any() and (d["lbmask"] == 1).any() and ((d["lbmask"] > 0) & (d["lbmask"] < 1)).any()
        assert lo and hi, U.FRAME_PAIRS[pi]
