"""The oracle's pyramid primitives on the smallest and thinnest shapes, against a plain float64 restatement of OpenCV's definitions
(the reference fixtures pin them at their own sizes only), and the host half of test_gpu_pyramid_depths.py's table.

  pyrDown: 1-4-6-4-1 / 256 in both directions, reflect-101 borders, output ((w + 1) / 2, (h + 1) / 2).
  pyrUp:   the source on the even points of the doubled grid (zeros between), 1-4-6-4-1 x 4 / 256 in both directions with reflect-101
           on that grid, cropped to dsize: OpenCV's edge rows 6a + 2b, a + 7b and 8b."""
import numpy as np
import pytest

import oracle_lib as O
from poppy_amd import capi
from test_gpu_pyramid_depths import SWEEP

K = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
SHAPES = [(1, 1), (1, 5), (6, 1), (2, 2), (2, 3), (3, 2), (3, 3), (7, 4), (5, 8), (1, 2), (2, 1)]      # (w, h)


def reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.abs(p)
    p = np.where(p >= n, 2 * n - 2 - p, p)
    return np.abs(p)


def _taps(idx, n):
    return reflect101(idx[:, None] + np.arange(-2, 3)[None, :], n)


def pyr_down64(a):
    a = a.astype(np.float64)
    h, w = a.shape[:2]
    rows, cols = _taps(2 * np.arange((h + 1) // 2), h), _taps(2 * np.arange((w + 1) // 2), w)
    t = np.tensordot(K, a[rows.T], axes=(0, 0))              # [dh, w, ...]
    return np.tensordot(K, t[:, cols.T], axes=(0, 1)) / 256.0   # [dh, dw, ...] after moving the tap axis


def pyr_up64(a, dw, dh):
    a = a.astype(np.float64)
    h, w = a.shape[:2]
    z = np.zeros((2 * h, 2 * w) + a.shape[2:])
    z[::2, ::2] = a
    rows, cols = _taps(np.arange(2 * h), 2 * h), _taps(np.arange(2 * w), 2 * w)
    t = np.tensordot(K, z[rows.T], axes=(0, 0))
    return (np.tensordot(K, t[:, cols.T], axes=(0, 1)) * 4.0 / 256.0)[:dh, :dw]


def _close(got, want, what, ulps=8):
    tol = ulps * np.finfo(np.float32).eps * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert err <= tol, f"{what}: max error {err:.3g} > {tol:.3g}"


def _img(w, h, c, seed):
    rng = np.random.default_rng(seed)
    return rng.random((h, w, c) if c > 1 else (h, w)).astype(np.float32)


def test_restatement_edges():
    """The float64 pyrUp has OpenCV's edge formulas: 6a + 2b at the first even row and column, a + 7b and 8b at the last two."""
    a = np.array([[1.0, 10.0, 100.0]])
    up = pyr_up64(a, 6, 2)
    assert np.allclose(up[0], np.array([6 + 20, 4 + 40, 1 + 60 + 100, 40 + 400, 10 + 700, 800]) / 8.0)
    assert np.allclose(up[1], up[0])               # one source row: both output rows are the same
    d = pyr_down64(np.array([[1.0, 2.0, 3.0]]))
    assert np.allclose(d, [[(6 * 1 + 8 * 2 + 2 * 3) / 16.0, (2 * 1 + 8 * 2 + 6 * 3) / 16.0]])


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES)
def test_pyr_down_vs_float64(w, h, c):
    a = _img(w, h, c, w * 10 + h)
    _close(O.pyr_down(a), pyr_down64(a), f"pyrDown {w}x{h}x{c}")


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES)
def test_pyr_up_vs_float64(w, h, c):
    """Up from the level pyrDown makes of a w x h image, to w x h (odd sizes crop the doubled grid) and to the full doubled size."""
    a = _img((w + 1) // 2, (h + 1) // 2, c, w * 10 + h + 1)
    for dw, dh in {(w, h), (2 * a.shape[1], 2 * a.shape[0])}:
        _close(O.pyr_up(a, dw, dh), pyr_up64(a, dw, dh), f"pyrUp {a.shape[1]}x{a.shape[0]} -> {dw}x{dh}x{c}")


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (2, 3), (1, 40), (3, 5), (16, 9)])
@pytest.mark.parametrize("levels", [1, 2, 3, 5, 10, 256])
def test_laplacian_blend_with_constant_masks(w, h, levels):
    """An all-ones mask gives back the left image, an all-zeros mask the right one: the Laplacian levels telescope at any depth."""
    l, r = _img(w, h, 3, 1), _img(w, h, 3, 2)
    _close(O.laplacian_blend(l, r, np.ones((h, w), np.float32), levels), l.astype(np.float64), f"mask 1 {w}x{h} L={levels}", ulps=32)
    _close(O.laplacian_blend(l, r, np.zeros((h, w), np.float32), levels), r.astype(np.float64), f"mask 0 {w}x{h} L={levels}", ulps=32)


@pytest.mark.parametrize("w,h,L,forms", SWEEP, ids=[f"{w}x{h}_L{L}" for w, h, L, _ in SWEEP])
def test_tail_plan_of_every_sweep_row(w, h, L, forms):
    """The tail's plan (first level, multi-pixel steps, single-pixel reductions, usable) that each row's launch list names."""
    plan, _ = capi.pyr_tail_plan(w, h, L)
    tail = [t for t in forms.split() if t.startswith("tail:")]
    if tail:
        first, n_wide, nl = (int(x) for x in tail[0].split(":")[1:])
        assert (plan["first"], plan["wide_steps"], plan["single_pixel_reductions"], plan["ok"]) == (first, n_wide, nl, 1), plan
    else:
        assert f"mix_top:{L}" in forms.split() and plan["ok"] == 0, plan
