"""The frame unsharp (unsharp_mask(lapBlend, 1, amount, 0.3) + convertTo(CV_8U, 255): k_unsharp_tile, k_unsharp_stream and the three separable kernels) and the
two forms of the blend mask on content that reaches their data-dependent branches, against the oracle, bit for bit.

The inputs are unsharp_content_util.py's; test_oracle_unsharp_content.py shows from the oracle alone that they reach what they are built for: patch centres
whose |median difference|^2 lies within 3e-7 of the bound of the sharpen decision on either side of it (inside the window in which the tile and streaming
kernels re-form their float sum in double, and with centres where the float sum alone decides the other way), products with 255 that are exact halves, values
either side of 0 and 1, products just below 2^31, at it and beyond +-2^31, structure on which the result overshoots [0, 1], and gabor2 fields that clamp the
mask at 0 and at 1.  Every comparison is == on bytes and on float bit patterns: the kernels claim the reference's expression tree.

The kernels alone run through Context.unsharp_frame (poppy_hip_unsharp_frame), in every form the geometry allows, with the amount as an argument and in device
memory, with and without the float output, from tight rows and from rows padded with a poison value.  NaN, infinities and negative zeros are not tested
(unsharp_content_util.py says why)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import unsharp_content_util as U
from poppy_amd import capi

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -1, -6
FORM_NAMES = {0: "launcher's choice", 1: "k_unsharp_tile", 2: "k_unsharp_stream", 3: "separable kernels"}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _forms(w, h):
    """The forms a w x h frame can be given to."""
    if w < 2 or h < 2:
        return (3, 0)
    return (1, 2, 3, 0) if w >= 64 and h >= 16 else (1, 3, 0)


def _padded(img):
    """The image as the first w columns of rows padded to the next multiple of 4 pixels (4 more where w is one), the padding poisoned."""
    h, w = img.shape[:2]
    pitch = (w + 3) // 4 * 4
    if pitch == w:
        pitch += 4
    buf = np.full((h, pitch, 3), U.POISON, np.float32)
    buf[:, :w] = img
    return buf[:, :w], pitch


@functools.lru_cache(maxsize=None)
def _oracle(key, amount):
    """(bytes, float image, median of the difference) of the oracle for the input `key` names; computed once, never written to."""
    out, _, med = O.unsharp(_input(key), amount, U.THRESHOLD)
    res = (O.f32_to_u8(out), out, med)
    for a in res:
        a.setflags(write=False)
    return res


def _input(key):
    return U.named_input(key)


def _report(tag, got, want, med):
    """AssertionError naming the first differing pixel with the oracle's double norm and the float sum there."""
    neq = got.view(np.uint32) != want.view(np.uint32) if got.dtype == np.float32 else got != want
    if not neq.any():
        return
    px = np.argwhere(neq.any(axis=2))
    y, x = px[0]
    n2, nf = U.norm2_double(med)[y, x], U.norm2_float(med)[y, x]
    raise AssertionError(f"{tag}: {len(px)} pixels differ, first at x={x} y={y}: got {got[y, x].tolist()} want {want[y, x].tolist()}; the oracle's double |d|^2 "
                         f"there {n2!r} (bound {U.norm2_min()!r}, sqrt {np.sqrt(n2)!r}), the float sum {float(nf)!r} (float bound {float(np.float32(U.norm2_min()))!r})")


def _run_all(ctx, key, amounts):
    img = _input(key)
    h, w = img.shape[:2]
    pad_view, pitch = _padded(img)
    for amount in amounts:
        want_u8, want_f, med = _oracle(key, float(amount))
        for form in _forms(w, h):
            for on_device in (False, True):
                for want_float in (False, True):
                    for padded in (False, True):
                        tag = (f"{key} amount={amount} form {form} ({FORM_NAMES[form]}), amount {'in device memory' if on_device else 'by argument'}, "
                               f"float output {'on' if want_float else 'off'}, pitch {pitch if padded else w}")
                        r = ctx.unsharp_frame(pad_view if padded else img, amount, form=form, pitch=pitch if padded else None,
                                              amount_on_device=on_device, want_float=want_float)
                        got_u8, got_f = r if want_float else (r, None)
                        if want_float:
                            _report(tag + " [float]", got_f, want_f, med)
                        _report(tag + " [bytes]", got_u8, want_u8, med)


# ---- the kernels alone -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("w,h,seed", U.THRESHOLD_SIZES, ids=[f"{w}x{h}" for w, h, _ in U.THRESHOLD_SIZES])
def test_sharpen_decision_on_both_sides_of_the_bound(ctx, w, h, seed, side):
    """Every patch centre is decided by the double sum: `below` sharpens none of them, `above` all of them, in every form."""
    key = ("threshold", side, w, h, seed)
    c = U.threshold_images(w, h, seed)["centres"]
    _, want_f, _ = _oracle(key, 1.0)
    changed = (want_f[c[:, 1], c[:, 0]] != _input(key)[c[:, 1], c[:, 0]]).any(axis=1)
    assert (changed == (side == "above")).all()
    _run_all(ctx, key, (1.0, U.AMOUNTS[2]))


def test_conversion_ties_clamps_and_2_31(ctx):
    """amount 0: the bytes are the conversion of the source itself (half-to-even at every k + 0.5, 0 and 255 beyond the ends, 255 / 0 / 0 / 0 about +-2^31);
    amount 1: the same values after sharpening."""
    _run_all(ctx, ("tie",), (0.0, 1.0))


@pytest.mark.parametrize("w,h", U.STRUCT_SIZES, ids=[f"{w}x{h}" for w, h in U.STRUCT_SIZES])
@pytest.mark.parametrize("name", U.STRUCT_NAMES + U.flat_names())
def test_saturating_structure(ctx, name, w, h):
    _run_all(ctx, ("struct", name, w, h), U.AMOUNTS)


@pytest.mark.parametrize("src,axis,at", U.ONE_PIXEL_CROPS, ids=[f"{'_'.join(str(v) for v in s)}_{a}{i}" for s, a, i in U.ONE_PIXEL_CROPS])
def test_one_pixel_frames(ctx, src, axis, at):
    """1 x 40 and 40 x 1 crops: the separable kernels, the only place the decision runs as sqrt(double sum) >= (double)threshold."""
    key = ("crop", src, axis, at)
    img = _input(key)
    assert img.shape == ((40, 1, 3) if axis == "col" else (1, 40, 3))
    _run_all(ctx, key, (0.0, 1.0, U.AMOUNTS[3]))
    for form in (1, 2):
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            ctx.unsharp_frame(img, 1.0, form=form)


def test_unsharp_frame_refusals(ctx):
    """The streaming kernel under 64 x 16: POPPY_E_UNSUPPORTED; bad arguments: POPPY_E_ARG; nothing written either way."""
    L = capi.lib()
    img = U.structure_f32("checker2", 97, 61)
    for crop in (img[:15, :80], img[:40, :63]):
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            ctx.unsharp_frame(np.ascontiguousarray(crop), 1.0, form=2)
    a = np.ascontiguousarray(img[:16, :64])
    out = np.full((16, 64, 3), 7, np.uint8); outf = np.full((16, 64, 3), 7, np.float32)
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)
    bad = [(p(a), 64, 16, 63, 1, 0, p(out)), (p(a), 64, 16, 64, 4, 0, p(out)), (p(a), 64, 16, 64, -1, 0, p(out)), (p(a), 64, 16, 64, 1, 2, p(out)),
           (None, 64, 16, 64, 1, 0, p(out)), (p(a), 0, 16, 64, 1, 0, p(out)), (p(a), 64, 0, 64, 1, 0, p(out)), (p(a), 64, 16, 64, 1, 0, None)]
    for src, w, h, pitch, form, on_dev, dst in bad:
        assert L.poppy_hip_unsharp_frame(ctx.h, src, w, h, pitch, 1.0, form, on_dev, dst, p(outf)) == E_ARG
    assert L.poppy_hip_unsharp_frame(None, p(a), 64, 16, 64, 1.0, 1, 0, p(out), p(outf)) == E_ARG
    assert (out == 7).all() and (outf == 7).all()
    got = ctx.unsharp_frame(a, 1.0, form=2)                         # ... and 64 x 16 itself is taken
    _report("64 x 16 on the streaming kernel", got, O.f32_to_u8(O.unsharp(a, 1.0, U.THRESHOLD)[0]), O.unsharp(a, 1.0, U.THRESHOLD)[2])


# ---- the whole frame path --------------------------------------------------------------------------------------------------------------------------------
def _same(name, got, want):
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    neq = got.view(np.uint32) != want.view(np.uint32) if got.dtype == np.float32 else got != want
    if neq.any():
        idx = np.argwhere(neq)
        raise AssertionError(f"{name}: {len(idx)} of {got.size} elements differ, first at {idx[0]}: got {got[tuple(idx[0])]!r} want {want[tuple(idx[0])]!r}")


@pytest.mark.parametrize("pair", range(len(U.FRAME_PAIRS)), ids=["_".join(p) for p in U.FRAME_PAIRS])
@pytest.mark.parametrize("w,h,lazy", U.FRAME_GEOMS, ids=[f"{w}x{h}_{'lazy' if lazy else 'materialised'}_mask" for w, h, lazy in U.FRAME_GEOMS])
def test_frames_with_clamped_masks_and_saturating_images(w, h, lazy, pair):
    """morph_images on pairs of the structure images (identity point sets and one moved set) under the mask fields at every ratio, in debug mode with every blend
    intermediate and outside it; the geometry's launch list has the lazy level-0 mask or the materialised one, as the table says."""
    for debug in (True, False):
        c = capi.Context(0)
        try:
            c.set_debug(debug)
            for r in U.MASK_RATIOS:
                c1, c2, g, p1, p2, shape, (wf, wmp, d) = U.frame_case(w, h, pair, r)
                got, gmp = c.morph_images(c1, c2, g, p1, p2, shape, r)
                tag = f"{w}x{h} {U.FRAME_PAIRS[pair]} mask ratio {r}{'' if debug else ' (not debug)'}"
                _same(f"morphed points {tag}", gmp, wmp)
                if debug:
                    for name in ("trImg1", "trImg2", "lbmask", "lapBlend", "unsharp"):
                        _same(f"{name} {tag}", c.fetch(name), d[name])
                _same(f"frame {tag}", got, wf)
            if debug:
                forms = c.last_pyramid_forms()
                level0 = [(kind, arg) for kind, lv, arg in forms if kind in ("down", "up") and lv == 0]
                if not os.environ.get("POPPY_HIP_LBMASK_RIDER"):             # (the switch that materialises the mask everywhere)
                    assert level0 == [("down", int(lazy)), ("up", int(lazy))], f"{w}x{h}: level 0 of the launch list is {level0}"
        finally:
            c.close()
