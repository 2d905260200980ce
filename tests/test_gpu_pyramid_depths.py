"""The Laplacian blend at every pyramid depth and on frames down to one pixel, against the oracle, bit for bit.

Which kernels build and collapse the pyramid is decided per (width, height, pyramid_levels) in alloc_pair / enqueue_body
(poppy_hip.cpp): the per-level kernels, k_pyrdown2, the one-workgroup tail k_pyr_tail (its multi-pixel steps n_wide and its
single-pixel reductions nl) or k_mix_top when the tail does not fit, k_collapse_cone<2..6>, k_collapse2, and the separable unsharp
path of frames under 2 pixels wide or high.  Every row of SWEEP names the launch list its geometry takes (include/poppy_hip.h:
poppy_hip_last_pyramid_forms, tokens below), so that a change of a threshold cannot move the sweep off a form unnoticed; the union
test checks that the whole table still reaches every form.

Under POPPY_HIP_NOCONE, POPPY_HIP_NOFUSE or POPPY_TAIL_PX (test_gpu_bstage.py: test_pyramid_launch_forms_stay_exact) every bit-exact
comparison stays; only the per-row launch lists, which are those of the default rules, are not compared."""
import functools
import os

import numpy as np
import pytest

import golden_util as G
import oracle_lib as O
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu

SWITCHES = ("POPPY_HIP_NOCONE", "POPPY_HIP_NOFUSE", "POPPY_TAIL_PX")
DEFAULT_RULES = not any(os.environ.get(k) for k in SWITCHES)
E_UNSUPPORTED = -6

# (W, H, pyramid_levels, launch list of the default rules).  Tokens: down:i (level i -> i + 1; "*": level 0 reads the mask lazily),
# down2:i (i -> i + 2), tail:first:n_wide:nl, mix_top:L, cone:k:n (k_collapse_cone<n> writes level k), up2:i (k_collapse2 writes
# level i), up:i, unsharp / unsharp1d.  first_tail (the first level of at most 600 pixels) is 5 at 640 x 480 and 6 at 1080p.
SWEEP = [
    (160, 120, 3, "down:0* down2:1 tail:3:0:-1 cone:1:2 up:0* unsharp"),
    (1920, 1080, 3, "down:0* down:1 down:2 mix_top:3 cone:1:2 up:0* unsharp"),
    (8000, 270, 7, "down:0* down:1 down2:2 down2:4 down:6 tail:7:0:-1 cone:1:6 up:0* unsharp"),
    (3000, 9, 4, "down:0 down2:1 down:3 tail:4:0:-1 up:3 up2:1 up:0 unsharp"),
    (640, 480, 1, "down:0* mix_top:1 up:0* unsharp"),
    (640, 480, 2, "down:0* down:1 mix_top:2 up:1 up:0* unsharp"),
    (640, 480, 4, "down:0* down2:1 down:3 tail:4:0:-1 cone:1:3 up:0* unsharp"),
    (640, 480, 5, "down:0* down2:1 down2:3 tail:5:0:-1 cone:1:4 up:0* unsharp"),
    (640, 480, 6, "down:0* down2:1 down2:3 tail:5:1:-1 cone:1:4 up:0* unsharp"),
    (640, 480, 65, "down:0* down2:1 down2:3 tail:5:5:55 cone:1:4 up:0* unsharp"),
    (1920, 1080, 5, "down:0* down:1 down2:2 down:4 tail:5:0:-1 cone:1:4 up:0* unsharp"),
    (1920, 1080, 6, "down:0* down:1 down2:2 down2:4 tail:6:0:-1 cone:1:5 up:0* unsharp"),
    (1920, 1080, 7, "down:0* down:1 down2:2 down2:4 tail:6:1:-1 cone:1:5 up:0* unsharp"),
    (1920, 1080, 128, "down:0* down:1 down2:2 down2:4 tail:6:5:117 cone:1:5 up:0* unsharp"),
    (1920, 1080, 256, "down:0* down:1 down2:2 down2:4 tail:6:5:245 cone:1:5 up:0* unsharp"),
    # padded rows (kernels.h: level_pitch): level 1 of 749 x 480 and 1918 x 1080 is padded too, so at depth 1 k_mix_top mixes a padded level
    (749, 480, 1, "down:0 mix_top:1 up:0 unsharp"),
    (749, 480, 3, "down:0 down2:1 mix_top:3 cone:1:2 up:0 unsharp"),
    (1918, 1080, 1, "down:0 mix_top:1 up:0 unsharp"),
    (3840, 2160, 4, "down:0* down:1 down:2 down:3 mix_top:4 cone:2:2 up:1 up:0* unsharp"),
    (320, 200, 9, "down:0* down2:1 down:3 tail:4:5:0 cone:1:3 up:0* unsharp"),
    (1, 7, 2, "down:0 tail:1:1:-1 up:0 unsharp1d"),
    (1, 1, 1, "down:0 tail:1:0:0 up:0 unsharp1d"),
    (1, 1, 64, "down:0 tail:1:0:63 up:0 unsharp1d"),
    (2, 2, 64, "down:0 tail:1:0:63 up:0 unsharp"),
    (1, 1, 256, "down:0 tail:1:0:255 up:0 unsharp1d"),
]

# tiny and thin frames, each at the default depth and at a shallow one; 1 x 150001: the smallest one-pixel-wide frame whose
# level-0 rows are padded (to 4 pixels)
TINY = [(1, 1), (2, 2), (3, 3), (5, 3), (3, 5), (7, 7), (8, 2), (9, 9), (16, 9), (31, 31),
        (1, 2), (2, 1), (1, 7), (7, 1), (1, 40), (40, 1), (200, 7), (7, 200), (3000, 9), (1, 150001)]
RATIOS = ((0.3, 0.3), (0.75, 0.4))


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(name, got, want):
    assert got.shape == want.shape, f"{name}: shape {got.shape} != {want.shape}"
    neq = _bits(got) != _bits(want)
    if neq.any():
        idx = np.argwhere(neq)
        raise AssertionError(f"{name}: {len(idx)} of {got.size} elements differ, first at {idx[0]}, last at {idx[-1]}")


def forms_text(forms):
    """The recorded launch list in SWEEP's tokens."""
    out, k = [], 0
    while k < len(forms):
        kind, lv, arg = forms[k]
        if kind == "tail":
            assert forms[k + 1][0] == "tail_nl"
            out.append(f"tail:{lv}:{arg}:{forms[k + 1][2]}"); k += 2
            continue
        if kind in ("down", "up"):
            out.append(f"{kind}:{lv}" + ("*" if arg else ""))
        elif kind == "cone":
            out.append(f"cone:{lv}:{arg}")
        elif kind == "unsharp":
            out.append("unsharp1d" if arg else "unsharp")
        else:
            out.append(f"{kind}:{lv}")
        k += 1
    return " ".join(out)


def tiny_points(w, h, seed):
    """The four corners and four quarter-pixel interior points, clipped to the frame (synth.point_pairs needs about 3 pixels)."""
    rng = np.random.default_rng(seed)
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
    inner = np.stack([rng.integers(0, 4 * (w - 1) + 1, 4), rng.integers(0, 4 * (h - 1) + 1, 4)], 1) / 4.0
    moved = np.clip(inner + rng.integers(-3, 4, inner.shape) / 4.0, 0, [w - 1, h - 1])
    return np.concatenate([corners, inner]).astype(np.float32), np.concatenate([corners, moved]).astype(np.float32)


def _points(w, h, n, seed, spread):
    if min(w, h) < 16:
        return tiny_points(w, h, seed)
    rng = np.random.default_rng(seed)
    p1 = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1).astype(np.float32)
    p2 = (p1 + rng.normal(0, spread, (n, 2))).astype(np.float32)
    p2[:, 0] = np.clip(p2[:, 0], 0, w - 1); p2[:, 1] = np.clip(p2[:, 1], 0, h - 1)
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
    return np.concatenate([p1, corners]), np.concatenate([p2, corners])


def _textured(w, h, seed):
    """synth.textured_bgr, tiled from a 960 x 540 one above a megapixel (the generator's time grows with the frame)."""
    if w * h <= 1 << 20:
        return synth.textured_bgr(w, h, seed)
    t = synth.textured_bgr(960, 540, seed)
    return np.ascontiguousarray(np.tile(t, (-(-h // 540), -(-w // 960), 1))[:h, :w])


@functools.lru_cache(maxsize=None)
def _inputs(w, h):
    """(image 1, image 2, gabor2, points 1, points 2); random bytes where the textured generator has no room (under 33 pixels)."""
    if min(w, h) < 33:
        rng = np.random.default_rng(w * 7919 + h)
        c1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8); c2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        g = (rng.integers(0, 1025, (h, w, 3)) / 1024.0).astype(np.float32)
    else:
        c1 = _textured(w, h, 41); c2 = _textured(w, h, 42); g = synth.unit_field(w, h, 7)
    p1, p2 = _points(w, h, 60, w + 3 * h, 4.0)
    return c1, c2, g, p1, p2


def _compare(w, h, L, check_forms=None):
    """Debug-mode frames with their blend intermediates, then the same frames outside debug mode; returns the recorded launch list."""
    c1, c2, g, p1, p2 = _inputs(w, h)
    want = [O.morph_images(c1, c2, g, p1, p2, s, m, L, debug=True) for s, m in RATIOS]
    c = capi.Context(0, pyramid_levels=L)
    try:
        c.set_debug(True)
        for (s, m), (wf, wmp, d) in zip(RATIOS, want):
            got, gmp = c.morph_images(c1, c2, g, p1, p2, s, m)
            tag = f"{w}x{h} L={L} s={s}"
            _same(f"morphed points {tag}", gmp, wmp)
            for name in ("trImg1", "trImg2", "lbmask", "lapBlend", "unsharp"):
                _same(f"{name} {tag}", c.fetch(name), d[name])
            _same(f"frame {tag}", got, wf)
        forms = forms_text(c.last_pyramid_forms())
    finally:
        c.close()
    c = capi.Context(0, pyramid_levels=L)
    try:
        for (s, m), (wf, _, _) in zip(RATIOS, want):
            got, _ = c.morph_images(c1, c2, g, p1, p2, s, m)
            _same(f"frame {w}x{h} L={L} s={s} (not debug)", got, wf)
            if w < 8:
                assert c.last_warp_kind() == 0, "frames under 8 pixels wide take the general warp kernel"
    finally:
        c.close()
    if check_forms is not None and DEFAULT_RULES:
        assert forms == check_forms, f"{w}x{h} L={L}: launch list {forms!r}, the table says {check_forms!r}"
    return forms


@pytest.mark.parametrize("w,h,L,forms", SWEEP, ids=[f"{w}x{h}_L{L}" for w, h, L, _ in SWEEP])
def test_depth_sweep_vs_oracle(w, h, L, forms):
    _compare(w, h, L, forms)


@pytest.mark.parametrize("L", [64, 3])
@pytest.mark.parametrize("w,h", TINY, ids=[f"{w}x{h}" for w, h in TINY])
def test_tiny_and_thin_frames_vs_oracle(w, h, L):
    forms = _compare(w, h, L)
    assert forms.endswith("unsharp1d" if w < 2 or h < 2 else "unsharp")


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 5), (1, 7), (7, 1), (1, 40), (16, 9), (200, 7)])
def test_tiny_frames_chained_and_phase_mode(w, h):
    """Three chained frames (each warps the previous frame and its morphed points), then two independent frames (the captured graph
    when the frame is at least 2 x 2) on a loaded pair."""
    c1, c2, g, p1, p2 = _inputs(w, h)
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        cur, pts = c1, p1
        for j in range(3):
            s = capi.lib().poppy_frame_ratio(j, 3, -1.0)
            want, mp = O.morph_images(cur, c2, g, pts, p2, s, s, 64)
            _same(f"chained frame {j} {w}x{h}", c.render(s, s, chain=True), want)
            cur, pts = want, mp
        c.reset()
        for s in (0.25, 0.6):
            want, _ = O.morph_images(c1, c2, g, p1, p2, s, s, 64)
            _same(f"phase frame s={s} {w}x{h}", c.render(s, s, chain=False), want)
    finally:
        c.close()


def test_launch_forms_union():
    """One debug frame of every row: together they reach every launch form (under a switch: the forms that switch leaves)."""
    seen = set()
    for w, h, L, _ in SWEEP + [(w, h, L, None) for w, h in TINY for L in (64, 3)]:
        c1, c2, g, p1, p2 = _inputs(w, h)
        c = capi.Context(0, pyramid_levels=L)
        try:
            c.set_debug(True)
            c.morph_images(c1, c2, g, p1, p2, 0.5, 0.5)
            f = c.last_pyramid_forms()
        finally:
            c.close()
        kinds = {k for k, _, _ in f}
        seen |= {(k, a) for k, _, a in f if k in ("cone", "tail", "unsharp", "down", "up")}
        seen |= {(k, None) for k in kinds}
        seen |= {("tail_nl", max(-1, min(a, 65))) for k, _, a in f if k == "tail_nl"}
        if "mix_top" in kinds and "cone" in kinds:
            seen.add(("mix_top+cone", None))
    has = lambda k, a=None: (k, a) in seen          # noqa: E731
    assert has("tail") and has("tail_nl") and has("mix_top") and has("up") and has("down")
    assert has("tail", 0) and has("tail_nl", -1) and has("tail_nl", 0) and has("tail_nl", 65), "the tail's forms: n_wide = 0, nl = -1, 0, > 64"
    assert has("unsharp", 1) and has("unsharp", 0), "the separable unsharp path of frames under 2 pixels and the 2-D kernels"
    cones = {a for k, a in seen if k == "cone" and a is not None}
    if os.environ.get("POPPY_HIP_NOFUSE"):
        assert not cones and not has("up2") and not has("down2")
    elif os.environ.get("POPPY_HIP_NOCONE"):
        assert not cones and has("up2") and has("down2")
    elif os.environ.get("POPPY_TAIL_PX"):
        assert 6 in cones and has("up2") and has("down2")
    else:
        assert cones == {2, 3, 4, 5, 6}, f"cone depths reached: {sorted(cones)}"
        assert has("up2") and has("down2") and has("mix_top+cone") and has("down", 1) and has("up", 1)


@pytest.mark.parametrize("L", [0, 257])
def test_depth_limits_refused_at_pair_load(L):
    c1, c2, g, p1, p2 = _inputs(64, 48)
    c = capi.Context(0, pyramid_levels=L)
    try:
        for _ in range(2):                   # the refusal leaves no half-built pair behind: the same answer again
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                c.pair_load(c1, c2, g, p1, p2)
        with pytest.raises(capi.PoppyError):
            c.render(0.5, 0.5)
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):        # the dissolve fallback sets the pair's geometry too
            c.dissolve(c1, c2, 0.5)
    finally:
        c.close()
    c = capi.Context(0, pyramid_levels=256)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        _same("frame at depth 256", c.render(0.5, 0.5), O.morph_images(c1, c2, g, p1, p2, 0.5, 0.5, 256)[0])
    finally:
        c.close()


@pytest.mark.parametrize("case", ["a_256x256_chain", "a_512x512_chain30"])
def test_whole_morph_at_other_depths(case):
    """poppy::morph from the raw pair at --pyramid 2, 5, 9, 128: the point pairs do not depend on the depth (the fixture's), the frames do."""
    inp = G.astage_inputs(case)
    n = int(inp["cfg"][0])
    setup = None
    for L in (2, 5, 9, 128):
        c = capi.Context(0, number_of_frames=n, pyramid_levels=L)
        try:
            rc, frames, _ = c.morph(inp["img1"], inp["img2"])
            assert rc == 0 and len(frames) == n
            p1, p2 = c.pair_points()
        finally:
            c.close()
        G.check(case, "prepared1", p1); G.check(case, "prepared2", p2)
        if setup is None:
            gabor2 = G.full(case, "gabor2")
            setup = dict(points1=p1, points2=p2, gabor2=O.gabor_field(inp["img2"]) if gabor2 is None else gabor2)
        want = O.morph(inp["img1"], inp["img2"], n, levels=L, setup=setup)
        for j, (a, b) in enumerate(zip(frames, want)):
            _same(f"{case} L={L} frame {j}", a, b)


@pytest.mark.parametrize("w,h", [(24, 17), (5, 3)])
def test_whole_morph_tiny_raw_sizes(w, h):
    """poppy::morph from raw pairs too small for a single ORB keypoint: no point pairs, the dissolve fallback (POPPY_E_NOMATCH), at any depth."""
    rng = np.random.default_rng(w * 100 + h)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8); b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = O.morph(a, b, 3, levels=9)           # the dissolve fallback does not use the pyramid: one oracle result for both depths
    for L in (2, 9):
        c = capi.Context(0, number_of_frames=3, pyramid_levels=L)
        try:
            rc, frames, dist = c.morph(a, b)
        finally:
            c.close()
        assert rc == -5 and dist is None and len(frames) == 3
        for j, (x, y) in enumerate(zip(frames, want)):
            _same(f"{w}x{h} L={L} frame {j}", x, y)


@pytest.mark.parametrize("w,h", [(1, 40), (40, 1)])
def test_whole_morph_one_pixel_raw_sizes_refused(w, h):
    """A raw pair one pixel wide or high has no dft_detail2 (0 / 0 in the reference, whose nfeatures is then undefined, and the oracle's
    set-up fails on it): every set-up entry refuses it with POPPY_E_UNSUPPORTED before any launch, and the context stays usable."""
    rng = np.random.default_rng(w * 100 + h)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8); b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        O.pair_setup(a, b)
    c = capi.Context(0, number_of_frames=3, pyramid_levels=9)
    try:
        for call in (lambda: c.morph(a, b), lambda: c.pair_begin(a, b), lambda: c.orb_input(a[..., 0])):
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                call()
        a2, b2 = _inputs(24, 17)[:2]
        rc, frames, _ = c.morph(a2, b2)
        assert rc == -5 and len(frames) == 3
        want = O.morph(a2, b2, 3, levels=9)
        for j, (x, y) in enumerate(zip(frames, want)):
            _same(f"24x17 after the refusal, frame {j}", x, y)
    finally:
        c.close()
