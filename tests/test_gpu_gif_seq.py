"""GPU checks of the coded sequence hand-off (poppy_hip_set_frame_format(POPPY_FRAME_GIF_SEQ): k_gif_lzw_bgr, k_gif_pack from the sequence's tables).  Every
comparison is == on bytes.  The direct entry, poppy_hip_bgr_frames_to_gif_frames, is compared with the host statement, poppy_bgr_frames_to_gif_frames
(tests/test_host_gif_seq.py pins it); on the frame path every case runs on a PAL8_SEQ context and on a GIF_SEQ context, and frame k of the second must be
poppy_pal8_to_gif_frame of frame k of the first (tests/test_gpu_palette_seq.py ties PAL8_SEQ's frames to the host statement)."""
import numpy as np
import pytest

import gif_coded_util as U
import golden_util as G
import palette_seq_util as PS
from poppy_amd import capi, synth
from palette_util import collect as _collect, inputs as _inputs, loaded as _loaded

pytestmark = pytest.mark.gpu
E_NOMATCH, E_UNSUPPORTED = -5, -6
S = U.segment_pixels()
PAL_SEQ, GIF_SEQ = capi.FRAME_PAL8_SEQ, capi.FRAME_GIF_SEQ


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


# ---- content of the direct entry's cases -------------------------------------------------------------------------------------------------------------------
def _cell_colours():
    """256 BGR colours, one in each of 256 distinct cells: a sequence of them has an exact palette, and its index plane is a relabelling of the plane of colour numbers"""
    rng = np.random.default_rng(256)
    cells = rng.choice(32768, 256, replace=False)
    rgb = np.stack([(cells >> 10) & 31, (cells >> 5) & 31, cells & 31], 1) * 8 + rng.integers(0, 8, (256, 3))
    return np.ascontiguousarray(rgb[:, ::-1].astype(np.uint8))


COLOURS = _cell_colours()
TEXTURE = {seed: synth.textured_bgr(128, 96, seed).reshape(-1, 3) for seed in (31, 32, 33)}      # 12288 pixels each, cut to every shape
CONTENTS = ("flat", "alternating", "textured", "code_per_pixel")


def frames_of(content, w, h, n_frames):
    n = w * h
    out = []
    for k in range(n_frames):
        if content == "flat":
            f = np.broadcast_to(np.array([10 + 40 * k, 200, 99 - 30 * k], np.uint8), (n, 3))
        elif content == "alternating":
            f = np.array([[250, 3, 77 + k], [4, 180 - 9 * k, 90]], np.uint8)[np.arange(n) & 1]
        elif content == "textured":
            f = TEXTURE[31 + k][:n]
        else:
            f = COLOURS[(U.all_distinct(n).astype(np.int64) + 7 * k) & 255]
        out.append(np.ascontiguousarray(f).reshape(h, w, 3))
    return np.stack(out)


def _direct(ctx, frames, what):
    got = ctx.bgr_frames_to_gif_frames(frames)
    want = capi.bgr_frames_to_gif_frames(frames)
    assert len(got) == len(want) == len(frames), what
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g.size == w_.size, f"{what}: frame {k}: {g.size} bytes, the host statement gives {w_.size}"
        neq = np.flatnonzero(g != w_)
        assert neq.size == 0, f"{what}: frame {k}: {neq.size} of {w_.size} bytes differ, first at {neq[0]}"
    return got


@pytest.mark.parametrize("n_frames", (1, 3))
@pytest.mark.parametrize("content", CONTENTS)
def test_direct_entry_on_every_shape(ctx, content, n_frames):
    for w, h in U.shapes(S) + [(61, 47), (64, 64)]:
        frames = frames_of(content, w, h, n_frames)
        if content == "code_per_pixel":                     # ... on the host's PAL8_SEQ frames: an exact palette, and no pair of neighbours twice inside a segment
            for f, p in zip(frames, capi.bgr_frames_to_pal8(frames)):
                assert np.array_equal(capi.pal8_to_bgr(p, w, h), f), "the palette is not exact"
                idx = p[:w * h].astype(np.int64)
                for at in range(0, w * h, S):
                    pairs = idx[at:at + S][:-1] * 256 + idx[at:at + S][1:]
                    assert np.unique(pairs).size == pairs.size, "a pair of neighbours repeats: the content compresses"
        _direct(ctx, frames, f"{content} {w}x{h} x {n_frames}")


def test_direct_entry_with_row_and_frame_padding(ctx):
    frames = frames_of("textured", 67, S // 67 + 1, 3)
    want = capi.bgr_frames_to_gif_frames(frames)
    for row_pad, frame_pad in ((5, 0), (0, 37), (7, 11)):
        got = ctx.bgr_frames_to_gif_frames(frames, row_pad=row_pad, frame_pad=frame_pad)
        assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want)), (row_pad, frame_pad)


def test_direct_entry_sub_block_sweep(ctx):
    seen = set()
    for n, seed in U.sweep_cases(8):
        frames = COLOURS[U.index_plane("noise", n, seed)].reshape(1, 1, n, 3)
        got = _direct(ctx, frames, f"noise {n}")
        seen.add(len(U.split_frame(got[0])[2]))
    assert seen >= set(U.SWEEP_LENGTHS), sorted(seen)


def test_three_frames_640x360(ctx):
    """Hundreds of segments per frame, and k_gif_pack's sums over them with the sequence's palette."""
    w, h = 640, 360
    assert w * h // S >= 50
    got = _direct(ctx, np.stack([synth.textured_bgr(w, h, 3 + k) for k in range(3)]), "textured 640x360 x 3")
    assert all(np.array_equal(g[4:772], got[0][4:772]) for g in got)


# ---- the frame path ---------------------------------------------------------------------------------------------------------------------------------------
def _same(what, pal8_frames, gif_frames, w, h):
    assert len(pal8_frames) == len(gif_frames) and len(gif_frames) > 0, f"{what}: {len(pal8_frames)} PAL8_SEQ frames, {len(gif_frames)} GIF_SEQ frames"
    for k, (p, g) in enumerate(zip(pal8_frames, gif_frames)):
        assert p.ndim == 1 and p.size == w * h + 768 and g.ndim == 1, f"{what}: frame {k} has the wrong format ({p.shape}, {g.shape})"
        want = capi.pal8_to_gif_frame(p, w, h)
        assert g.size == want.size, f"{what}: frame {k}: {g.size} bytes, the host statement gives {want.size}"
        neq = np.flatnonzero(g != want)
        assert neq.size == 0, f"{what}: frame {k}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


def _both(what, run, w, h, **settings):
    """run(ctx) -> frames, on a PAL8_SEQ and on a GIF_SEQ context"""
    out = []
    for fmt in (PAL_SEQ, GIF_SEQ):
        c = capi.Context(0, **settings)
        try:
            c.set_frame_format(fmt)
            out.append(run(c))
        finally:
            c.close()
    _same(what, out[0], out[1], w, h)
    return out


def test_textured_pair_chained_and_phase_mode_twice():
    """Six chained frames (more than the ring has buffers), then two rounds of four phase-mode frames: the second round replays the captured bodies."""
    w, h = 256, 192
    run = _loaded(w, h)
    shapes = [0.1, 0.3, 0.5, 0.7, 0.85, 0.95]

    def frames(c):
        out = _collect(c, c.render_many, shapes, chain=True)
        assert len(out) == 6 and (c.frame_format != GIF_SEQ or all(np.array_equal(f[4:772], out[0][4:772]) for f in out))
        for _ in range(2):
            out += _collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=False)
        return out
    _both("256x192 textured pair", run(frames), w, h)


def test_phase_zero_and_one_copies():
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], 256, 256, number_of_frames=2)


def test_render_phases_with_copies_on_a_resident_pair():
    w, h = 256, 192
    run = _loaded(w, h)
    _both("t = 0, 0.5, 1 on a resident pair", run(lambda c: _collect(c, c.render_phases, [0.0, 0.5, 1.0])), w, h)


def test_flat_pair_reaches_the_nomatch_frames():
    a = np.full((150, 200, 3), (9, 99, 199), np.uint8)
    b = np.full_like(a, 77)

    def run(c):
        rc, frames, _ = c.morph(a, b, phase=-1.0)
        assert rc == E_NOMATCH
        return frames
    _both("flat pair", run, 200, 150, number_of_frames=3)


def test_morph_list_of_three():
    """Each pair is a sequence: one palette inside a pair, another in the next."""
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2
        if c.frame_format == GIF_SEQ:
            first, second = frames
            assert all(np.array_equal(f[4:772], first[0][4:772]) for f in first) and all(np.array_equal(f[4:772], second[0][4:772]) for f in second)
            assert not np.array_equal(first[0][4:772], second[0][4:772])
        return [f for pair in frames for f in pair]
    _both("morph_list of 3", run, 256, 192, number_of_frames=4)


def test_pool_of_two_contexts_queued():
    w, h = 256, 192
    pairs = [(synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6 + k, 3)) for k in range(3)]
    results = []
    for fmt in (PAL_SEQ, GIF_SEQ):
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


def test_writer_is_first_called_after_the_last_frame():
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    c = capi.Context(0)
    try:
        c.set_frame_format(GIF_SEQ)
        c.pair_load(c1, c2, g, p1, p2)
        for chain in (True, False):
            c.reset()
            shapes = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
            before = sum(c.warp_counts())
            seen = []
            c.render_many(shapes, chain=chain, write=lambda v: seen.append(sum(c.warp_counts()) - before))
            assert seen == [len(shapes)] * len(shapes), f"frames rendered at the writer's calls (chain = {chain}): {seen}"
    finally:
        c.close()


def test_timing_mode_marks():
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    plain = capi.Context(0); c = capi.Context(0)
    try:
        plain.set_frame_format(PAL_SEQ); c.set_frame_format(GIF_SEQ)
        plain.pair_load(c1, c2, g, p1, p2); c.pair_load(c1, c2, g, p1, p2)
        want = _collect(plain, plain.render_many, [0.2, 0.5, 0.8], chain=True)
        c.set_timing(1)
        frames = _collect(c, c.render_many, [0.2, 0.5, 0.8], chain=True)
        names = {n: k for n, _, k in c.timing_summary()}
        assert (names.get("pal8_seq_hist"), names.get("pal8_seq_build"), names.get("gif_lzw"), names.get("gif_pack")) == (3, 1, 3, 3), names
        assert "frame_format" not in names and "pal8_build" not in names
        c.set_timing(0)
        _same("timing mode 1", want, frames, w, h)
    finally:
        plain.close(); c.close()


def test_switching_formats_on_one_context():
    """BGR -> GIF_SEQ -> PAL8_SEQ -> GIF -> GIF_SEQ on one context with a resident pair: each format's frames are what a fresh context of that format gives."""
    w, h = 320, 200
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    order = (capi.FRAME_BGR, GIF_SEQ, PAL_SEQ, capi.FRAME_GIF, GIF_SEQ)

    def frames(c):
        c.reset()
        return _collect(c, c.render_many, shapes, chain=True) + _collect(c, c.render_many, shapes, chain=False)
    fresh = {}
    for fmt in set(order):
        f = capi.Context(0)
        try:
            f.set_frame_format(fmt)
            f.pair_load(c1, c2, g, p1, p2)
            fresh[fmt] = frames(f)
        finally:
            f.close()
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        for k, fmt in enumerate(order):
            c.set_frame_format(fmt)
            got = frames(c)
            assert len(got) == len(fresh[fmt]) == 6, (k, fmt)
            for j, (a, b) in enumerate(zip(got, fresh[fmt])):
                assert a.shape == b.shape and np.array_equal(a, b), f"step {k} (format {fmt}), frame {j} differs from a fresh context's"
    finally:
        c.close()
    # and the fresh contexts agree with the host statements: chained and phase-mode frames are a sequence each
    for half in (slice(0, 3), slice(3, 6)):
        PS.same_seq("fresh PAL8_SEQ", fresh[capi.FRAME_BGR][half], fresh[PAL_SEQ][half])
        _same("fresh GIF_SEQ", fresh[PAL_SEQ][half], fresh[GIF_SEQ][half], w, h)


def test_refusals_keep_the_resident_pair():
    sw, sh = 64, 64
    s1, s2, sg, sp1, sp2 = _inputs(sw, sh)
    c = capi.Context(0)
    try:
        c.set_frame_format(GIF_SEQ)
        c.pair_load(s1, s2, sg, sp1, sp2)
        want = _collect(c, c.render_many, [0.3, 0.7], chain=True)
        # a sequence that reaches 2^32 pixels: refused on the count alone
        before = sum(c.warp_counts())
        calls = []
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.render_phases(np.full((1 << 32) // (sw * sh), 0.5), write=lambda v: calls.append(1))
        assert sum(c.warp_counts()) == before and not calls, "frames were rendered or written before the refusal"
        for w, h in ((4097, 4096), (65536, 2)):
            big = np.zeros((h, w, 3), np.uint8); bg = np.zeros((h, w, 3), np.float32)      # (refused before a byte of them is read)
            corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                c.pair_load(big, big, bg, corners, corners)
            del bg
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                c.bgr_frames_to_gif_frames(big[None])
            del big
        # the direct entry works on buffers of its own: the resident pair and the context's sequence state are as they were
        _direct(c, frames_of("textured", 61, 47, 2), "direct entry on a context with a resident pair")
        c.reset()
        got = _collect(c, c.render_many, [0.3, 0.7], chain=True)
        assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(want, got))
    finally:
        c.close()


def _sink_file(tmp_path, gif, w, h):
    L = capi.lib()
    path = tmp_path / "gpu.gif"
    s = L.poppy_sink_open(str(path).encode(), capi.SINK_GIF_GLOBAL_CODED, w, h, 25, 1)
    for f in gif:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(gif)
    return path


@pytest.fixture(scope="module")
def gpu_sequence():
    w, h = 256, 192
    run = _loaded(w, h)
    pal, gif = _both("sequence for the sink", run(lambda c: _collect(c, c.render_many, [0.2, 0.5, 0.8], chain=True)), w, h)
    return w, h, pal, gif


def test_sink_file_from_a_gpu_sequence_decodes(tmp_path, gpu_sequence):
    w, h, pal, gif = gpu_sequence
    dec = PS.gif_decode_any(_sink_file(tmp_path, gif, w, h).read_bytes())
    assert dec["global"] is not None and np.array_equal(dec["global"].ravel(), pal[0][w * h:])
    assert len(dec["frames"]) == len(pal)
    for k, (f, p) in enumerate(zip(dec["frames"], pal)):
        assert not f[5] and f[1:3] == (w, h), f"frame {k} has a local table or another size"
        assert np.array_equal(f[4], p[:w * h]) and np.array_equal(f[3].ravel(), p[w * h:]), f"frame {k} decodes to other pixels than the PAL8_SEQ context's"


def test_sink_file_from_a_gpu_sequence_decodes_in_pillow(tmp_path, gpu_sequence):
    Image = pytest.importorskip("PIL.Image")
    w, h, pal, gif = gpu_sequence
    with Image.open(_sink_file(tmp_path, gif, w, h)) as im:
        assert im.n_frames == len(gif) and im.size == (w, h)
        for k, p in enumerate(pal):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert("RGB"))[:, :, ::-1], capi.pal8_to_bgr(p, w, h)), f"Pillow's frame {k} differs"
