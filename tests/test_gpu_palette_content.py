"""GPU checks of the palette kernels (k_pal8_hist, k_pal8_build, k_pal8_remap, k_pal8_seq_pass, k_pal8_seq_build) and the I420 kernels on content chosen
to reach what rendered frames do not (palette_util.adversarial_frames, big_noise, primaries, white_4096; tests/test_host_palette_content.py asserts what each
frame is built for and pins the host statements to the numpy rule on it).  The other GPU palette tests compare on what a morph renders: smooth frames, in
which no two boxes tie across the build's four register banks and no workgroup fills its LDS table.

The t = 0 / 1 frames of render_phases are image 1 / image 2 themselves, converted on the device (the context's scratch tables; under PAL8_SEQ the sequence
pass, build and remap), so any bytes can be put in front of the kernels; chained and phase-mode frames of the same pairs run the slots' copies on the
side streams.  Every comparison is == against the host statement of the image or frame: no tolerance."""
import functools

import numpy as np
import pytest

import palette_util as P
from palette_seq_util import same_seq
from poppy_amd import capi

pytestmark = pytest.mark.gpu
SEQ = capi.FRAME_PAL8_SEQ
FORMATS = {"bgr": capi.FRAME_BGR, "pal8": capi.FRAME_PAL8, "gif": capi.FRAME_GIF, "pal8_seq": SEQ}


@functools.lru_cache(maxsize=None)
def _frames():
    return {**P.frames(), **P.adversarial_frames(), **P.big_noise()}


def _pairs():
    """name -> (image 1, image 2) of one size: the built frames pair by pair, every frame of the host tests with a partner of its size (a channel-swapped
    copy where there is none), the two large noise frames"""
    pairs = {"cube_uniform+noise_256x128": ("cube_uniform", "noise_256x128"), "line_r+line_g": ("line_r", "line_g"), "line_b+line_r": ("line_b", "line_r"),
             "lattice512+heavy_tail": ("lattice512", "heavy_tail"), "last_slab+mirror": ("last_slab", "last_slab_mirror"),
             "photo_a+photo_b": ("photo_a", "photo_b"), "cells_256+cells_257": ("cells_256", "cells_257"), "cells_257_any_colour+cells_256": ("cells_257_any_colour", "cells_256"),
             "noise_1280x1024_a+b": ("noise_1280x1024_a", "noise_1280x1024_b")}
    paired = {n for p in pairs.values() for n in p}
    for name in sorted(P.frames()):
        if name not in paired:
            pairs[name + "+swapped"] = (name, None)
    return pairs


PAIRS = _pairs()


def _pair(name):
    a, b = PAIRS[name]
    f = _frames()
    return f[a], (np.ascontiguousarray(np.roll(f[a], 1, axis=2)) if b is None else f[b])


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, number_of_frames=1)                      # (one frame: a pair load plans no default sequence ahead)
    yield c
    c.close()


def _copies(c, fmt, a, b, ts):
    """image 1 / image 2 as the context hands them to a writer at t = 0 / 1; the four corners are both point sets"""
    h, w = a.shape[:2]
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
    c.set_frame_format(fmt)
    c.pair_load(a, b, np.zeros((h, w, 3), np.float32), corners, corners)
    return P.collect(c, c.render_phases, ts)


def _same(what, want, got, pal8=False):
    """frame by frame ==, reported as the other palette tests do (pal8: the frames end with a palette)"""
    assert len(want) == len(got) and len(got) > 0, f"{what}: {len(got)} frames, {len(want)} expected"
    for k, (x, y) in enumerate(zip(want, got)):
        assert x.shape == y.shape, f"{what}: frame {k} has shape {y.shape}, the host statement gives {x.shape}"
        neq = np.flatnonzero(y.ravel() != x.ravel())
        in_palette = f" ({(neq >= x.size - 768).sum()} of them in the palette)" if pal8 else ""
        assert neq.size == 0, f"{what}: frame {k}: {neq.size} of {x.size} bytes differ{in_palette}, first at {neq[0]}"


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_copies_equal_the_host_statement(ctx, name, fmt):
    """a, b, a, b: under BGR the images themselves (the route), under PAL8 and GIF each image's own frame — very different cell sets after each other, so
    the scratch tables must be zero again after every build —, under PAL8_SEQ one sequence of four and sequences of one."""
    a, b = _pair(name)
    got = _copies(ctx, FORMATS[fmt], a, b, [0.0, 1.0, 0.0, 1.0])
    if fmt == "pal8_seq":
        same_seq(f"{name}, PAL8_SEQ", [a, b, a, b], got)
        for t, image in ((0.0, a), (1.0, b)):
            _same(f"{name}, PAL8_SEQ, a sequence of image {int(t) + 1} alone", [capi.bgr_to_pal8(image)], P.collect(ctx, ctx.render_phases, [t]), pal8=True)
        return
    host = {"bgr": lambda f: f, "pal8": capi.bgr_to_pal8, "gif": capi.bgr_to_gif_frame}[fmt]
    want_a, want_b = host(a), host(b)
    _same(f"{name}, {fmt}", [want_a, want_b, want_a, want_b], got, pal8=fmt == "pal8")


@pytest.mark.parametrize("w,h", P.PRIMARIES_SIZES + [(256, 128)], ids=[f"{w}x{h}" for w, h in P.PRIMARIES_SIZES + [(256, 128)]])
def test_i420_copies_reach_the_chroma_clamps(ctx, w, h):
    """Saturated 2 x 2 blocks (pre-clamp U = 256 in blue blocks, V = 256 in red ones) through the wide kernel, the tail kernel and both; noise beside them."""
    a, b = (_frames()["noise_256x128"], _frames()["cube_uniform"]) if (w, h) == (256, 128) else (P.primaries(w, h, 1), P.primaries(w, h, 4))
    want_a, want_b = capi.bgr_to_i420(a), capi.bgr_to_i420(b)
    if w * h > 1 and (w, h) != (256, 128):
        assert want_a[w * h:].max() == 255 and want_a[w * h:].min() == 1
    _same(f"{w}x{h}, BGR", [a, b], _copies(ctx, capi.FRAME_BGR, a, b, [0.0, 1.0]))
    _same(f"{w}x{h}, I420", [want_a, want_b, want_a, want_b], _copies(ctx, capi.FRAME_I420, a, b, [0.0, 1.0, 0.0, 1.0]))


# ---- rendered frames: the slots' tables, the side streams, the captured bodies ---------------------------------------------------------------------------
RENDERED = {"cube_uniform+noise_256x128": (256, 128), "noise_1280x1024_a+b": (1280, 1024)}
CHAINED, UNCHAINED = [0.1, 0.3, 0.5, 0.7, 0.85, 0.95], [0.3, 0.7]


def _rendered(name, fmt):
    """[the frames of each call]: six chained frames, then the same two phase-mode shapes twice (the second call replays the captured bodies)"""
    w, h = RENDERED[name]
    c = capi.Context(0)
    try:
        c.set_frame_format(fmt)
        c.pair_load(*P.inputs(w, h, 40, *_pair(name)))
        chained = P.collect(c, c.render_many, CHAINED, chain=True)
        c.reset()
        return [chained, P.collect(c, c.render_many, UNCHAINED, chain=False), P.collect(c, c.render_many, UNCHAINED, chain=False)]
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def _rendered_bgr(name):
    return _rendered(name, capi.FRAME_BGR)


@pytest.mark.parametrize("fmt", ["gif", "pal8", "pal8_seq"])
@pytest.mark.parametrize("name", sorted(RENDERED))
def test_rendered_frames_equal_the_host_statement(name, fmt):
    bgr = _rendered_bgr(name)
    w, h = RENDERED[name]
    assert [len(call) for call in bgr] == [6, 2, 2] and all(f.shape == (h, w, 3) for call in bgr for f in call)
    assert all(np.array_equal(x, y) for x, y in zip(bgr[1], bgr[2])), "the replayed bodies render other BGR frames"
    got = _rendered(name, FORMATS[fmt])
    for k, (b, g) in enumerate(zip(bgr, got)):
        what = f"{name}, {fmt}, call {k}"
        if fmt == "pal8_seq":
            same_seq(what, b, g)                                   # (every call is a sequence)
        else:
            _same(what, [(capi.bgr_to_pal8 if fmt == "pal8" else capi.bgr_to_gif_frame)(f) for f in b], g, pal8=fmt == "pal8")


# ---- the limit -------------------------------------------------------------------------------------------------------------------------------------------
def test_white_4096_fills_the_packed_sums_and_passes_them_over_a_sequence():
    """2^24 white pixels: one cell whose channel sums are 2^24 * 255 = 4 278 190 080 < 2^32, the most the packed 32-bit fields of k_pal8_hist hold; as a
    sequence of two such frames 2^25 * 255 > 2^32, the reason the sequence tables are unpacked 64-bit words.  The smallest size at which either exists, and the one slow case of this file."""
    w = h = 4096
    white = P.white_4096()
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
    want = np.zeros(w * h + 768, np.uint8)
    want[w * h:w * h + 3] = 255
    c = capi.Context(0, number_of_frames=1)
    try:
        c.set_frame_format(capi.FRAME_PAL8)
        c.pair_load(white, white, np.zeros((h, w, 3), np.float32), corners, corners)
        _same("4096 x 4096 white, PAL8", [want, want], P.collect(c, c.render_phases, [0.0, 1.0]), pal8=True)
        c.set_frame_format(SEQ)
        got = P.collect(c, c.render_phases, [0.0, 1.0])
    finally:
        c.close()
    assert np.array_equal(capi.bgr_to_pal8(white), want), "the host statement of the white frame"
    _same("4096 x 4096 white twice, PAL8_SEQ", list(capi.bgr_frames_to_pal8(np.broadcast_to(white, (2, h, w, 3)))), got, pal8=True)
