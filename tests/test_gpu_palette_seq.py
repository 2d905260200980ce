"""GPU checks of the sequence palette hand-off (poppy_hip_set_frame_format(POPPY_FRAME_PAL8_SEQ)): every case runs on a context that hands out BGR and
on one that hands out PAL8_SEQ, and the PAL8_SEQ frames of a call (of a pair, in lists and pools) must equal poppy_bgr_frames_to_pal8 of that call's
BGR frames in every byte, indices and palette (the host function is the format's definition; tests/test_host_palette_seq.py pins it).  No tolerance
anywhere."""
import ctypes as C

import numpy as np
import pytest

import golden_util as G
from poppy_amd import capi, synth
from palette_seq_util import collect as _collect, gif_decode_any, host_seq, inputs as _inputs, loaded as _loaded, same_seq

pytestmark = pytest.mark.gpu
E_STATE, E_NOMATCH, E_UNSUPPORTED = -4, -5, -6
SEQ = capi.FRAME_PAL8_SEQ


def _both(what, run, **settings):
    """run(ctx) -> the frames of ONE sequence, on a BGR and on a PAL8_SEQ context"""
    out = []
    for fmt in (capi.FRAME_BGR, SEQ):
        c = capi.Context(0, **settings)
        try:
            if fmt == SEQ:
                c.set_frame_format(fmt)
            out.append(run(c))
        finally:
            c.close()
    same_seq(what, *out)
    return out


def test_morph_chained_and_phase_mode_on_fixtures():
    inp = G.astage_inputs("a_256x256_chain")
    bgr, seq = _both("chained morph", lambda c: c.morph(inp["img1"], inp["img2"])[1], number_of_frames=12)
    assert len(seq) == 12 and any(not np.array_equal(s, capi.bgr_to_pal8(b)) for b, s in zip(bgr, seq)), "twelve frames with one palette each"
    inp = G.astage_inputs("a_256x256_phase")
    for ph in (0.25, 0.5):
        bgr, seq = _both(f"phase-mode morph {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], number_of_frames=1)
        assert np.array_equal(seq[0], capi.bgr_to_pal8(bgr[0])), "a sequence of one frame is that frame's PAL8"


def test_phase_zero_and_one_copies():
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], number_of_frames=3)
        _both(f"morph phase {ph}, padded rows", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph, row_pad=(7, 12))[1], number_of_frames=2)
    for ph in (0.0, 1.0):                                       # (each morph_frames call is a sequence)
        def resident(c):
            c.pair_begin(inp["img1"], inp["img2"])
            return c.morph_frames(ph)
        _both(f"morph_frames phase {ph} on a resident pair", resident, number_of_frames=2)


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


def test_morph_frames_render_many_and_render_phases():
    run = _loaded(320, 200)
    _both("morph_frames", run(lambda c: c.morph_frames()), number_of_frames=9)
    shapes = [0.1, 0.35, 0.6, 0.8, 0.95]
    _both("render_many chained", run(lambda c: _collect(c, c.render_many, shapes, chain=True)))
    _both("render_many unchained", run(lambda c: _collect(c, c.render_many, shapes, chain=False)))
    ts = [0.0, 0.2, 0.4, 1.0, 0.6, 0.8, 0.0, 1.0]
    _both("render_phases with t = 0 / 1", run(lambda c: _collect(c, c.render_phases, ts)))
    _both("render_phases of copies only", run(lambda c: _collect(c, c.render_phases, [0.0, 1.0, 1.0])))
    _both("render_phases, one frame", run(lambda c: _collect(c, c.render_phases, [0.5])))
    # more chained frames than slots, several times over
    many = list(np.linspace(0.02, 0.98, 25))
    _both("25 chained frames", run(lambda c: _collect(c, c.render_many, many, chain=True)))
    _both("25 phase frames", run(lambda c: _collect(c, c.render_phases, many)))


def _per_pair(what, bgr_pairs, seq_pairs):
    assert len(bgr_pairs) == len(seq_pairs)
    for k, (b, s) in enumerate(zip(bgr_pairs, seq_pairs)):
        same_seq(f"{what}, pair {k}", b, s)
    n_px = seq_pairs[0][0].size - 768
    pals = {s[0][n_px:].tobytes() for s in seq_pairs}
    assert len(pals) == len(seq_pairs), f"{what}: pairs share a palette"


def test_morph_list_three_and_four_images():
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(4)]
    for n, frames in ((3, 5), (4, 3)):
        out = []
        for fmt in (capi.FRAME_BGR, SEQ):
            c = capi.Context(0, number_of_frames=frames)
            try:
                if fmt == SEQ:
                    c.set_frame_format(fmt)
                rc, got, _, done = c.morph_list(images[:n])
                assert rc == 0 and done == n - 1 and len(got) == n - 1
                out.append(got)
            finally:
                c.close()
        _per_pair(f"morph_list of {n}", *out)
    _both("morph_list phase 0 of 2", lambda c: [f for p in c.morph_list(images[:2], phase=0.0)[1] for f in p], number_of_frames=2)


def test_pool_batches_and_state():
    pairs = [(synth.gen(256, 192, 77, 0, 0), synth.gen(256, 192, 77, 6 + k, 3)) for k in range(4)]
    results = []
    for fmt in (capi.FRAME_BGR, SEQ):
        p = capi.Pool([0], contexts_per_device=3, number_of_frames=4)
        try:
            got = {}
            if fmt == SEQ:
                p.set_frame_format(fmt)
            for b in range(3):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            with pytest.raises(capi.PoppyError, match=str(E_STATE)):
                p.set_frame_format(capi.FRAME_BGR if fmt == SEQ else SEQ)
            p.wait()
            results.append(got)
            p.set_frame_format(fmt)
        finally:
            p.close()
    bgr, seq = results
    assert sorted(bgr) == sorted(seq) and len(bgr) == 3 * len(pairs) * 4
    for b in range(3):
        _per_pair(f"pool batch {b}", [[bgr[(b, pi, j)] for j in range(4)] for pi in range(4)], [[seq[(b, pi, j)] for j in range(4)] for pi in range(4)])


def test_pool_synchronous_pairs():
    pairs = [(synth.gen(256, 192, 78, 0, 0), synth.gen(256, 192, 78, 5 + k, 2)) for k in range(3)]
    results = []
    for fmt in (capi.FRAME_BGR, SEQ):
        p = capi.Pool([0], contexts_per_device=2, number_of_frames=5)
        try:
            if fmt == SEQ:
                p.set_frame_format(fmt)
            L = capi.lib()
            got = {}
            h, w = pairs[0][0].shape[:2]

            def src(user, pi, device, pa, sa, pb, sb):
                pa[0] = pairs[pi][0].ctypes.data; sa[0] = w * 3
                pb[0] = pairs[pi][1].ctypes.data; sb[0] = w * 3
                return 0

            def wr(user, pi, j, ptr, ww, hh, stride, fmt=fmt):
                got[(pi, j)] = capi._frame_view(ptr, ww, hh, stride, fmt).copy()
            fs, fw = capi.PAIR_SOURCE_CB(src), capi.WRITE_PAIR_CB(wr)
            err = C.create_string_buffer(512)
            rc = L.poppy_hip_pool_morph_pairs(p.h, len(pairs), w, h, C.c_double(-1.0), 0, C.cast(fs, C.c_void_p), C.cast(fw, C.c_void_p), None, err, 512)
            assert rc == 0, err.value.decode()
            results.append(got)
        finally:
            p.close()
    bgr, seq = results
    assert sorted(bgr) == sorted(seq) and len(bgr) == 15
    _per_pair("pool, synchronous", [[bgr[(pi, j)] for j in range(5)] for pi in range(3)], [[seq[(pi, j)] for j in range(5)] for pi in range(3)])


@pytest.mark.parametrize("w,h", [(749, 480), (1918, 1080), (1, 40), (40, 1)])
def test_odd_and_thin_geometries(w, h):
    run = _loaded(w, h)
    _both(f"{w}x{h} chained", run(lambda c: _collect(c, c.render_many, [0.3, 0.5, 0.7], chain=True)))
    _both(f"{w}x{h} phase mode", run(lambda c: _collect(c, c.render_phases, [0.0, 0.25, 0.6, 1.0])))


def test_1080p_chained_60_frames_passes_2_24_pixels():
    """124 M pixels in the sequence: the counts and sums of the device's tables pass 2^24 * 255 (the range of PAL8's packed words)."""
    w, h, n = 1920, 1080, 60
    assert n * w * h > 1 << 24
    shapes = list(np.linspace(0.01, 0.99, n))
    _both("1080p, 60 chained frames", _loaded(w, h)(lambda c: _collect(c, c.render_many, shapes, chain=True)))


def test_4k_phase_frames():
    _both("3840x2160 phase frames", _loaded(3840, 2160)(lambda c: _collect(c, c.render_phases, [0.0, 0.5, 0.75])))


def test_writer_is_first_called_after_the_last_frame():
    """The palette is known after the last frame only: at the writer's first call every frame of the sequence has been submitted (the context's warp
    launches count them), and the frames then come in order."""
    run = _loaded(320, 200)
    for chain in (True, False):
        def r(c):
            shapes = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
            before = sum(c.warp_counts())
            seen, frames = [], []

            def write(v):
                seen.append(sum(c.warp_counts()) - before)
                frames.append(v.copy())
            c.render_many(shapes, chain=chain, write=write)
            if c.frame_format == SEQ:
                assert seen == [len(shapes)] * len(shapes), f"frames rendered at the writer's calls: {seen}"
            return frames
        _both(f"hand-over order, chain = {chain}", run(r))          # (same_seq: frame k of the writer is frame k of the sequence)

    def phases(c):
        """render_phases: copies (t = 0 / 1, no warp launch) between two runs of rendered frames — one sequence, opened and ended by the call itself"""
        ts = [0.0, 0.2, 0.4, 0.6, 1.0, 0.0, 0.3, 0.5, 0.7, 1.0]
        rendered = sum(1 for t in ts if t not in (0.0, 1.0))
        before = sum(c.warp_counts())
        seen, frames = [], []

        def write(v):
            seen.append(sum(c.warp_counts()) - before)
            frames.append(v.copy())
        c.render_phases(ts, write=write)
        if c.frame_format == SEQ:
            assert seen == [rendered] * len(ts), f"frames rendered at the writer's calls: {seen}"
        else:
            assert seen[0] == 0 and seen[-1] == rendered, "(BGR hands the first copy over before anything is rendered)"
        return frames
    _both("hand-over order, render_phases", run(phases))


def test_switch_formats_and_recapture():
    """BGR -> PAL8_SEQ -> PAL8 -> I420 -> BGR on one context gives what fresh contexts give; frames rendered without a writer in between do not disturb
    the next sequence; a sequence after a shorter and after a longer one (the store grows, the tables are zero again)."""
    w, h = 320, 200
    c1, c2, g, p1, p2 = _inputs(w, h)
    ts = [0.15, 0.3, 0.45, 0.6, 0.75, 0.9]
    plain = capi.Context(0); sw = capi.Context(0)
    try:
        plain.pair_load(c1, c2, g, p1, p2); sw.pair_load(c1, c2, g, p1, p2)
        want = _collect(plain, plain.render_phases, ts)
        assert all(np.array_equal(a, b) for a, b in zip(want, _collect(sw, sw.render_phases, ts)))
        sw.set_frame_format(SEQ)
        same_seq("PAL8_SEQ phase frames", want, _collect(sw, sw.render_phases, ts))
        sw.set_frame_format(capi.FRAME_PAL8)
        pal = _collect(sw, sw.render_phases, ts)
        assert len(pal) == len(want) and all(np.array_equal(p, capi.bgr_to_pal8(b)) for p, b in zip(pal, want)), "PAL8 frames after PAL8_SEQ differ"
        sw.set_frame_format(capi.FRAME_I420)
        yuv = _collect(sw, sw.render_phases, ts)
        assert len(yuv) == len(want) and all(np.array_equal(y, capi.bgr_to_i420(b)) for y, b in zip(yuv, want)), "I420 frames after PAL8 differ"
        sw.set_frame_format(capi.FRAME_BGR)
        back = _collect(sw, sw.render_phases, ts)
        assert len(back) == len(want) and all(np.array_equal(a, b) for a, b in zip(want, back)), "BGR frames after the other formats differ"
        sw.set_frame_format(SEQ)
        sw.render_phases(ts)                                        # no writer: no pass, frames stay in HBM
        sw.render_many(ts, chain=False)
        same_seq("PAL8_SEQ after frames without a writer", want, _collect(sw, sw.render_phases, ts))
        same_seq("a shorter sequence", want[:2], _collect(sw, sw.render_phases, ts[:2]))
        long_ts = list(np.linspace(0.05, 0.95, 17))
        same_seq("a longer sequence", _collect(plain, plain.render_phases, long_ts), _collect(sw, sw.render_phases, long_ts))
        same_seq("the first sequence again", want, _collect(sw, sw.render_phases, ts))
        sw.reset(); plain.reset()
        chained_want = _collect(plain, plain.render_many, ts, chain=True)
        sw.render_many(ts, chain=True)
        sw.reset()
        same_seq("chained PAL8_SEQ after chained frames without a writer", chained_want, _collect(sw, sw.render_many, ts, chain=True))
        assert np.array_equal(sw.render(0.4, 0.4), plain.render(0.4, 0.4)), "explicit-destination frames stay BGR"
        for bad in (2, 4, 7, 9):
            with pytest.raises(capi.PoppyError):
                sw.set_frame_format(bad)
        assert sw.frame_format == SEQ
    finally:
        plain.close(); sw.close()


def test_timing_mode_marks():
    c1, c2, g, p1, p2 = _inputs(256, 192)
    plain = capi.Context(0); c = capi.Context(0)
    try:
        plain.pair_load(c1, c2, g, p1, p2); c.pair_load(c1, c2, g, p1, p2)
        for chain in (True, False):
            plain.reset(); c.reset()
            want = _collect(plain, plain.render_many, [0.2, 0.5, 0.8], chain=chain)
            c.set_frame_format(SEQ)
            c.set_timing(1)
            frames = _collect(c, c.render_many, [0.2, 0.5, 0.8], chain=chain)
            names = {n: k for n, _, k in c.timing_summary()}
            assert (names.get("pal8_seq_hist"), names.get("pal8_seq_build"), names.get("frame_format"), names.get("unsharp")) == (3, 1, 3, 3), names
            assert "pal8_hist" not in names and "pal8_build" not in names
            c.set_timing(0)
            same_seq(f"timing mode 1, chain = {chain}", want, frames)
    finally:
        plain.close(); c.close()


def test_sequence_limit_refuses_before_anything_is_rendered():
    """render_phases with as many frames as make 2^32 pixels of a small pair: refused on the count alone, nothing rendered, and the context goes on."""
    w, h = 64, 64
    c1, c2, g, p1, p2 = _inputs(w, h)
    n = (1 << 32) // (w * h)
    ts = np.full(n, 0.5)
    plain = capi.Context(0); c = capi.Context(0)
    try:
        plain.pair_load(c1, c2, g, p1, p2); c.pair_load(c1, c2, g, p1, p2)
        c.set_frame_format(SEQ)
        before = sum(c.warp_counts())
        calls = []
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.render_phases(ts, write=lambda v: calls.append(1))
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.render_many(ts, chain=False, write=lambda v: calls.append(1))
        assert sum(c.warp_counts()) == before and not calls, "frames were rendered or written before the refusal"
        ok = [0.0, 0.3, 0.6, 1.0]
        same_seq("after the refusal", _collect(plain, plain.render_phases, ok), _collect(c, c.render_phases, ok))
    finally:
        plain.close(); c.close()


def test_oversize_pair_is_refused():
    w, h = 4097, 4096
    sw, sh = 320, 200
    s1, s2, sg, sp1, sp2 = _inputs(sw, sh)
    plain = capi.Context(0); c = capi.Context(0)
    try:
        plain.pair_load(s1, s2, sg, sp1, sp2)
        want = _collect(plain, plain.render_many, [0.3, 0.7], chain=True)
        c.set_frame_format(SEQ)
        c.pair_load(s1, s2, sg, sp1, sp2)
        big = np.zeros((h, w, 3), np.uint8); bg = np.zeros((h, w, 3), np.float32)          # (refused before a byte of them is read)
        corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
        for attempt in range(2):
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                c.pair_load(big, big, bg, corners, corners)
        same_seq("after the refused loads", want, _collect(c, c.render_many, [0.3, 0.7], chain=True))
    finally:
        plain.close(); c.close()


def test_chained_1080p_pair_through_the_global_gif_sink(tmp_path):
    w, h, n = 1920, 1080, 3
    c1, c2, g, p1, p2 = _inputs(w, h)
    plain = capi.Context(0, number_of_frames=n); c = capi.Context(0, number_of_frames=n)
    path = tmp_path / "morph.gif"
    try:
        plain.pair_load(c1, c2, g, p1, p2); c.pair_load(c1, c2, g, p1, p2)
        want = plain.morph_frames()
        c.set_frame_format(SEQ)
        L = capi.lib()
        sink = L.poppy_sink_open(str(path).encode(), capi.SINK_GIF_GLOBAL, w, h, 25, 1)
        assert sink
        rc = L.poppy_hip_morph_frames(c.h, C.c_double(-1.0), C.cast(L.poppy_sink_write, C.c_void_p), C.c_void_p(sink))
        assert rc == 0
        assert L.poppy_sink_close(sink) == n
    finally:
        plain.close(); c.close()
    gif = gif_decode_any(path.read_bytes())
    ref = host_seq(want)
    assert len(gif["frames"]) == n == len(want) and gif["loop"] == 0 and gif["screen"][2] == 0xF7
    assert np.array_equal(gif["global"].ravel(), ref[0, w * h:])
    for k, (delay, fw, fh, pal, idx, local) in enumerate(gif["frames"]):
        assert (delay, fw, fh, local) == (4, w, h, False)
        assert np.array_equal(idx, ref[k, :w * h]), f"GIF frame {k} is not the host's PAL8_SEQ of the BGR frame"
