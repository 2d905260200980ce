"""GPU checks of the GIF frame hand-off (poppy_hip_set_frame_format(POPPY_FRAME_GIF): k_gif_lzw, k_gif_pack).  Every comparison is == against the host
statement, poppy_pal8_to_gif_frame, applied to the PAL8 frame — the one a PAL8 context renders for the same pair (tests/test_gpu_palette_format.py ties those
to the host's PAL8), or the index plane handed in.  The host statement itself is pinned to a restatement of the rule in tests/test_host_gif_coded.py."""
import numpy as np
import pytest

import gif_coded_util as U
import golden_util as G
from poppy_amd import capi, synth
from palette_util import collect as _collect, inputs as _inputs, loaded as _loaded

pytestmark = pytest.mark.gpu
E_NOMATCH, E_UNSUPPORTED = -5, -6
S = U.segment_pixels()


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _same(what, pal8_frames, gif_frames, w, h):
    assert len(pal8_frames) == len(gif_frames) and len(gif_frames) > 0, f"{what}: {len(pal8_frames)} PAL8 frames, {len(gif_frames)} GIF frames"
    for k, (p, g) in enumerate(zip(pal8_frames, gif_frames)):
        assert p.ndim == 1 and p.size == w * h + 768 and g.ndim == 1, f"{what}: frame {k} has the wrong format ({p.shape}, {g.shape})"
        want = capi.pal8_to_gif_frame(p, w, h)
        assert g.size == want.size, f"{what}: frame {k}: {g.size} bytes, the host statement gives {want.size}"
        neq = np.flatnonzero(g != want)
        assert neq.size == 0, f"{what}: frame {k}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


def _both(what, run, w, h, **settings):
    """run(ctx) -> frames, on a PAL8 and on a GIF context"""
    out = []
    for fmt in (capi.FRAME_PAL8, capi.FRAME_GIF):
        c = capi.Context(0, **settings)
        try:
            c.set_frame_format(fmt)
            out.append(run(c))
        finally:
            c.close()
    _same(what, out[0], out[1], w, h)
    return out


def _direct(ctx, pal8, w, h, what):
    got = ctx.pal8_to_gif_frame(pal8, w, h)
    want = capi.pal8_to_gif_frame(pal8, w, h)
    assert got.size == want.size, f"{what}: {got.size} bytes, the host statement gives {want.size}"
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{what}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


@pytest.mark.parametrize("content", U.CONTENTS)
def test_direct_entry_on_the_host_tests_planes(ctx, content):
    for w, h in U.shapes(S) + [(61, 47), (64, 64)]:
        _direct(ctx, U.pal8_of(U.index_plane(content, w * h), seed=w), w, h, f"{content} {w}x{h}")


def test_direct_entry_full_table_and_capacity(ctx):
    """Planes that cost a code per pixel: 4096 pixels (the table fills after 3838 strings: the restart inside a segment when S = 4096) and 3 S + 5."""
    for n in (4096, 3 * S + 5):
        for idx in (U.all_distinct(n), U.index_plane("noise", n)):
            _direct(ctx, U.pal8_of(idx), n, 1, f"incompressible {n}")


def test_direct_entry_sub_block_sweep(ctx):
    seen = set()
    for n, seed in U.sweep_cases(8):
        pal8 = U.pal8_of(U.index_plane("noise", n, seed))
        _direct(ctx, pal8, n, 1, f"noise {n}")
        seen.add(len(U.split_frame(ctx.pal8_to_gif_frame(pal8, n, 1))[2]))
    assert seen >= set(U.SWEEP_LENGTHS), sorted(seen)


def test_one_frame_640x360(ctx):
    """Hundreds of segments, and k_gif_pack's sums over them."""
    w, h = 640, 360
    assert w * h // S >= 50
    _direct(ctx, capi.bgr_to_pal8(synth.textured_bgr(w, h, 3)), w, h, "textured 640x360")
    _direct(ctx, U.pal8_of(U.index_plane("zero", w * h)), w, h, "zero 640x360")


def test_textured_pair_chained_and_phase_mode_twice():
    w, h = 256, 192
    run = _loaded(w, h)
    shapes = [0.1, 0.3, 0.5, 0.7, 0.85, 0.95]

    def frames(c):
        out = _collect(c, c.render_many, shapes, chain=True)
        for _ in range(2):                                  # the second round replays the captured bodies
            out += _collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=False)
        return out
    _both("256x192 textured pair", run(frames), w, h)


def test_phase_zero_and_one_copies():
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], 256, 256, number_of_frames=2)

    def resident(c):
        c.pair_begin(inp["img1"], inp["img2"])
        return c.morph_frames(0.0) + c.morph_frames(1.0) + _collect(c, c.render_phases, [0.0, 0.5, 1.0])
    _both("phase 0 / 1 and t 0 / 1 on a resident pair", resident, 256, 256, number_of_frames=2)


def test_flat_pair_reaches_the_nomatch_frames():
    a = np.full((150, 200, 3), (9, 99, 199), np.uint8)
    b = np.full_like(a, 77)
    for ph in (-1.0, 0.3):
        def run(c):
            rc, frames, _ = c.morph(a, b, phase=ph)
            assert rc == E_NOMATCH
            return frames
        _both(f"flat pair, phase {ph}", run, 200, 150, number_of_frames=3)


def test_morph_list_of_three():
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2
        return [f for pair in frames for f in pair]
    _both("morph_list of 3", run, 256, 192, number_of_frames=4)


def test_pool_of_two_contexts_queued():
    w, h = 256, 192
    pairs = [(synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6 + k, 3)) for k in range(3)]
    results = []
    for fmt in (capi.FRAME_PAL8, capi.FRAME_GIF):
        p = capi.Pool([0], contexts_per_device=2, number_of_frames=4)
        try:
            got = {}
            p.set_frame_format(fmt)
            for b in range(2):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            p.wait()
            results.append(got)
        finally:
            p.close()
    pal, gif = results
    assert sorted(pal) == sorted(gif) and len(gif) == 2 * len(pairs) * 4
    keys = sorted(pal)
    _same("pool batches", [pal[k] for k in keys], [gif[k] for k in keys], w, h)


def test_switching_formats_on_one_context():
    w, h = 320, 200
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        out = {}
        for k, fmt in enumerate((capi.FRAME_BGR, capi.FRAME_GIF, capi.FRAME_PAL8, capi.FRAME_GIF)):
            c.set_frame_format(fmt)
            c.reset()
            out[k] = _collect(c, c.render_many, shapes, chain=True) + _collect(c, c.render_many, shapes, chain=False)
        assert all(f.shape == (h, w, 3) for f in out[0])
        for k, f in enumerate(out[2]):
            assert np.array_equal(f, capi.bgr_to_pal8(out[0][k]))
        _same("GIF after BGR", out[2], out[1], w, h)
        _same("GIF after PAL8", out[2], out[3], w, h)
    finally:
        c.close()


def test_sink_file_from_a_gpu_sequence_decodes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    w, h = 256, 192
    run = _loaded(w, h)
    shapes = [0.2, 0.5, 0.8]
    pal, gif = _both("sequence for the sink", run(lambda c: _collect(c, c.render_many, shapes, chain=True)), w, h)
    L = capi.lib()
    path = tmp_path / "gpu.gif"
    s = L.poppy_sink_open(str(path).encode(), capi.SINK_GIF_CODED, w, h, 25, 1)
    for f in gif:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(gif)
    with Image.open(path) as im:
        assert im.n_frames == len(gif) and im.size == (w, h)
        for k, p in enumerate(pal):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert("RGB"))[:, :, ::-1], capi.pal8_to_bgr(p, w, h)), f"Pillow's frame {k} differs"


def test_oversize_refusal_keeps_the_resident_pair():
    sw, sh = 320, 200
    s1, s2, sg, sp1, sp2 = _inputs(sw, sh)
    c = capi.Context(0)
    try:
        c.set_frame_format(capi.FRAME_GIF)
        c.pair_load(s1, s2, sg, sp1, sp2)
        want = _collect(c, c.render_many, [0.3, 0.7], chain=True)
        for w, h in ((4097, 4096), (65536, 2)):
            big = np.zeros((h, w, 3), np.uint8); bg = np.zeros((h, w, 3), np.float32)      # (refused before a byte of them is read)
            corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                c.pair_load(big, big, bg, corners, corners)
            del big, bg
            with pytest.raises(capi.PoppyError, match=str(E_UNSUPPORTED)):
                c.pal8_to_gif_frame(np.zeros(w * h + 768, np.uint8), w, h)
        c.reset()
        got = _collect(c, c.render_many, [0.3, 0.7], chain=True)
        assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(want, got))
    finally:
        c.close()
