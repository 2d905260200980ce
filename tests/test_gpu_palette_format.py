"""GPU checks of the PAL8 frame hand-off (poppy_hip_set_frame_format(POPPY_FRAME_PAL8)): every case runs on a context that hands out BGR and on
one that hands out PAL8, and every PAL8 frame must equal poppy_bgr_to_pal8 of the BGR frame in every byte, indices and palette (the host function is
the format's definition; tests/test_host_palette_format.py pins it to the rule).  Chained and phase-mode frames, the phase 0 / 1 and t 0 / 1
copies, the linear-blend fallback, render_many, render_phases, morph_list, queued pool batches, odd and thin geometries, a 4K frame, a flat pair, a
context switched BGR -> PAL8 -> I420 -> BGR, timing mode 1, frames without a writer in between, and a chained 1080p pair through the GIF sink."""
import numpy as np
import pytest

import golden_util as G
from poppy_amd import capi, synth
from palette_util import collect as _collect, gif_decode, inputs as _inputs, loaded as _loaded

pytestmark = pytest.mark.gpu
E_STATE, E_NOMATCH = -4, -5


def _same_frames(what, bgr_frames, pal_frames):
    assert len(bgr_frames) == len(pal_frames) and len(bgr_frames) > 0, f"{what}: {len(bgr_frames)} BGR frames, {len(pal_frames)} PAL8 frames"
    for k, (b, p) in enumerate(zip(bgr_frames, pal_frames)):
        assert b.ndim == 3 and p.ndim == 1, f"{what}: frame {k} has the wrong format ({b.shape}, {p.shape})"
        want = capi.bgr_to_pal8(b)
        assert p.shape == want.shape, f"{what}: frame {k}: {p.size} bytes, the format has {want.size}"
        neq = np.flatnonzero(p != want)
        n_idx = want.size - 768
        assert neq.size == 0, (f"{what}: frame {k}: {neq.size} of {want.size} bytes differ ({(neq >= n_idx).sum()} of them in the palette), first at {neq[0]}")


def _both(what, run, **settings):
    """run(ctx) -> frames, on a BGR and on a PAL8 context"""
    out = []
    for fmt in (capi.FRAME_BGR, capi.FRAME_PAL8):
        c = capi.Context(0, **settings)
        try:
            if fmt == capi.FRAME_PAL8:
                c.set_frame_format(fmt)
            out.append(run(c))
        finally:
            c.close()
    _same_frames(what, *out)
    return out


def test_morph_chained_and_phase_mode_on_fixtures():
    inp = G.astage_inputs("a_256x256_chain")
    _both("chained morph", lambda c: c.morph(inp["img1"], inp["img2"])[1], number_of_frames=12)
    inp = G.astage_inputs("a_256x256_phase")
    for ph in (0.25, 0.5):
        _both(f"phase-mode morph {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], number_of_frames=1)


def test_phase_zero_and_one_copies():
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], number_of_frames=3)
        _both(f"morph phase {ph}, padded rows", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph, row_pad=(7, 12))[1], number_of_frames=2)

    def resident(c):
        c.pair_begin(inp["img1"], inp["img2"])
        return c.morph_frames(0.0) + c.morph_frames(1.0)
    _both("morph_frames phase 0 / 1 on a resident pair", resident, number_of_frames=2)


def test_linear_blend_fallback():
    inp = G.make_inputs.dissolve_inputs("x_dissolve_200x150")
    a = inp["img1"]
    b = np.full_like(a, 77)
    for ph in (-1.0, 0.3):
        def run(c):
            rc, frames, _ = c.morph(a, b, phase=ph)
            assert rc == E_NOMATCH
            return frames
        _both(f"fallback phase {ph}", run, number_of_frames=3)


def test_render_many_and_render_phases():
    run = _loaded(320, 200)
    shapes = [0.1, 0.35, 0.6, 0.8, 0.95]
    _both("render_many chained", run(lambda c: _collect(c, c.render_many, shapes, chain=True)))
    _both("render_many unchained", run(lambda c: _collect(c, c.render_many, shapes, chain=False)))
    ts = [0.0, 0.2, 0.4, 1.0, 0.6, 0.8, 0.0, 1.0]
    _both("render_phases with t = 0 / 1", run(lambda c: _collect(c, c.render_phases, ts)))
    # more chained frames than slots, several times over: every slot's tables are used again and again
    many = list(np.linspace(0.02, 0.98, 25))
    _both("25 chained frames", run(lambda c: _collect(c, c.render_many, many, chain=True)))


def test_morph_list_three_and_four_images():
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(4)]

    def run(n):
        def r(c):
            rc, frames, _, done = c.morph_list(images[:n])
            assert rc == 0 and done == n - 1
            return [f for pair in frames for f in pair]
        return r
    _both("morph_list of 3", run(3), number_of_frames=5)
    _both("morph_list of 4", run(4), number_of_frames=3)
    _both("morph_list phase 0 of 2", lambda c: [f for p in c.morph_list(images[:2], phase=0.0)[1] for f in p], number_of_frames=2)


def test_pool_batches_and_state():
    pairs = [(synth.gen(256, 192, 77, 0, 0), synth.gen(256, 192, 77, 6 + k, 3)) for k in range(4)]
    results = []
    for fmt in (capi.FRAME_BGR, capi.FRAME_PAL8):
        p = capi.Pool([0], contexts_per_device=3, number_of_frames=4)
        try:
            got = {}
            if fmt == capi.FRAME_PAL8:
                p.set_frame_format(fmt)
            for b in range(3):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            with pytest.raises(capi.PoppyError, match=str(E_STATE)):
                p.set_frame_format(capi.FRAME_BGR if fmt == capi.FRAME_PAL8 else capi.FRAME_PAL8)
            p.wait()
            results.append(got)
            p.set_frame_format(fmt)
        finally:
            p.close()
    bgr, pal = results
    assert sorted(bgr) == sorted(pal) and len(bgr) == 3 * len(pairs) * 4
    keys = sorted(bgr)
    _same_frames("pool batches", [bgr[k] for k in keys], [pal[k] for k in keys])


@pytest.mark.parametrize("w,h", [(749, 480), (1918, 1080), (1, 40), (40, 1), (1920, 1080)])
def test_odd_and_thin_geometries(w, h):
    run = _loaded(w, h)
    _both(f"{w}x{h} chained", run(lambda c: _collect(c, c.render_many, [0.3, 0.7], chain=True)))
    _both(f"{w}x{h} phase mode", run(lambda c: _collect(c, c.render_phases, [0.0, 0.25, 0.6, 1.0])))


def test_4k_phase_frame():
    _both("3840x2160 phase frame", _loaded(3840, 2160)(lambda c: _collect(c, c.render_phases, [0.5, 0.75])))


def test_flat_pair_has_one_box():
    w, h = 320, 200
    _, _, g, p1, p2 = _inputs(w, h)
    flat = np.full((h, w, 3), (31, 140, 222), np.uint8)

    def run(c):
        c.pair_load(flat, flat, g, p1, p2)
        return _collect(c, c.render_many, [0.3, 0.6], chain=True) + _collect(c, c.render_phases, [0.0, 0.5, 1.0])      # (t = 0 / 1: the flat images themselves)
    bgr, pal = _both("flat pair", run)
    assert any(len(np.unique(b.reshape(-1, 3), axis=0)) == 1 for b in bgr), "no frame of a flat pair is flat"
    for b, f in zip(bgr, pal):
        if len(np.unique(b.reshape(-1, 3), axis=0)) == 1:
            assert not f[:w * h].any() and not f[w * h + 3:].any(), "a flat frame has one box"


def test_switch_formats_and_recapture():
    """Phase-mode bodies are captured graphs that end with the wanted format's conversion: BGR -> PAL8 -> I420 -> BGR on one context gives what fresh
    contexts give, and frames rendered without a writer under PAL8 (no conversion) do not disturb the next ones with a writer."""
    w, h = 320, 200
    c1, c2, g, p1, p2 = _inputs(w, h)
    ts = [0.15, 0.3, 0.45, 0.6, 0.75, 0.9]
    plain = capi.Context(0); sw = capi.Context(0)
    try:
        plain.pair_load(c1, c2, g, p1, p2); sw.pair_load(c1, c2, g, p1, p2)
        want = _collect(plain, plain.render_phases, ts)
        assert all(np.array_equal(a, b) for a, b in zip(want, _collect(sw, sw.render_phases, ts)))
        sw.set_frame_format(capi.FRAME_PAL8)
        _same_frames("PAL8 phase frames", want, _collect(sw, sw.render_phases, ts))
        sw.set_frame_format(capi.FRAME_I420)
        yuv = _collect(sw, sw.render_phases, ts)
        assert len(yuv) == len(want) and all(np.array_equal(y, capi.bgr_to_i420(b)) for y, b in zip(yuv, want)), "I420 frames after PAL8 differ"
        sw.set_frame_format(capi.FRAME_BGR)
        back = _collect(sw, sw.render_phases, ts)
        assert len(back) == len(want) and all(np.array_equal(a, b) for a, b in zip(want, back)), "BGR frames after PAL8 and I420 differ"
        sw.set_frame_format(capi.FRAME_PAL8)
        sw.render_phases(ts)                                        # no writer: bodies without the conversion, frames stay in HBM
        sw.render_many(ts, chain=False)
        _same_frames("PAL8 after frames without a writer", want, _collect(sw, sw.render_phases, ts))
        sw.reset()
        chained_want = _collect(plain, plain.render_many, ts, chain=True)
        sw.render_many(ts, chain=True)
        sw.reset()
        _same_frames("chained PAL8 after chained frames without a writer", chained_want, _collect(sw, sw.render_many, ts, chain=True))
        assert np.array_equal(sw.render(0.4, 0.4), plain.render(0.4, 0.4)), "explicit-destination frames stay BGR"
        for bad in (2, 4, 7, 9):
            with pytest.raises(capi.PoppyError):
                sw.set_frame_format(bad)
    finally:
        plain.close(); sw.close()


def test_timing_mode_marks_the_conversion():
    c1, c2, g, p1, p2 = _inputs(256, 192)
    plain = capi.Context(0); c = capi.Context(0)
    try:
        plain.pair_load(c1, c2, g, p1, p2); c.pair_load(c1, c2, g, p1, p2)
        want = _collect(plain, plain.render_many, [0.2, 0.5, 0.8], chain=True)
        c.set_frame_format(capi.FRAME_PAL8)
        c.set_timing(1)
        frames = _collect(c, c.render_many, [0.2, 0.5, 0.8], chain=True)
        names = {n: k for n, _, k in c.timing_summary()}
        assert names.get("frame_format") == 3 and names.get("pal8_hist") == 3 and names.get("pal8_build") == 3 and names.get("unsharp") == 3
        c.set_timing(0)
        _same_frames("timing mode 1", want, frames)
    finally:
        plain.close(); c.close()


def test_chained_1080p_pair_through_the_gif_sink(tmp_path):
    w, h, n = 1920, 1080, 3
    c1, c2, g, p1, p2 = _inputs(w, h)
    plain = capi.Context(0, number_of_frames=n); c = capi.Context(0, number_of_frames=n)
    path = tmp_path / "morph.gif"
    try:
        plain.pair_load(c1, c2, g, p1, p2); c.pair_load(c1, c2, g, p1, p2)
        want = plain.morph_frames()
        c.set_frame_format(capi.FRAME_PAL8)
        L = capi.lib()
        sink = L.poppy_sink_open(str(path).encode(), capi.SINK_GIF, w, h, 25, 1)
        assert sink
        import ctypes as C
        rc = L.poppy_hip_morph_frames(c.h, C.c_double(-1.0), C.cast(L.poppy_sink_write, C.c_void_p), C.c_void_p(sink))
        assert rc == 0
        assert L.poppy_sink_close(sink) == n
    finally:
        plain.close(); c.close()
    gif = gif_decode(path.read_bytes())
    assert len(gif["frames"]) == n == len(want) and gif["loop"] == 0
    for k, (delay, fw, fh, pal, idx) in enumerate(gif["frames"]):
        ref = capi.bgr_to_pal8(want[k])
        assert (delay, fw, fh) == (4, w, h)
        assert np.array_equal(idx, ref[:w * h]) and np.array_equal(pal.ravel(), ref[w * h:]), f"GIF frame {k} is not the host's PAL8 of the BGR frame"


def test_oversize_pair_is_refused_and_stays_refused():
    """More than 2^24 pixels under PAL8: the pair load is refused before the context changes, the second attempt as the first (no half-made pair is
    found), and the context goes on with the pairs it takes.  A BGR context that holds such a pair refuses PAL8 and stays BGR."""
    w, h = 4097, 4096
    E_UNSUPPORTED = -6
    sw, sh = 320, 200
    s1, s2, sg, sp1, sp2 = _inputs(sw, sh)
    plain = capi.Context(0); c = capi.Context(0)
    try:
        plain.pair_load(s1, s2, sg, sp1, sp2)
        want = _collect(plain, plain.render_many, [0.3, 0.7], chain=True)
        c.set_frame_format(capi.FRAME_PAL8)
        c.pair_load(s1, s2, sg, sp1, sp2)
        big = np.zeros((h, w, 3), np.uint8); bg = np.zeros((h, w, 3), np.float32)          # (refused before a byte of them is read)
        corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
        for attempt in range(2):
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                c.pair_load(big, big, bg, corners, corners)
        del bg
        c.pair_load(s1, s2, sg, sp1, sp2)
        _same_frames("after the refused loads", want, _collect(c, c.render_many, [0.3, 0.7], chain=True))
        # the same pair under BGR is taken; PAL8 is then refused and the context stays BGR
        c.set_frame_format(capi.FRAME_BGR)
        b1, b2, g, p1, p2 = _inputs(w, h)
        c.pair_load(b1, b2, g, p1, p2)
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.set_frame_format(capi.FRAME_PAL8)
        assert c.frame_format == capi.FRAME_BGR
        frames = _collect(c, c.render_phases, [0.0, 0.5])
        assert len(frames) == 2 and frames[1].shape == (h, w, 3) and np.array_equal(frames[0], b1)
        c.set_frame_format(capi.FRAME_I420)                                        # (I420 has no such limit)
        assert _collect(c, c.render_phases, [0.5])[0].size == capi.frame_bytes(capi.FRAME_I420, w, h)
    finally:
        plain.close(); c.close()
