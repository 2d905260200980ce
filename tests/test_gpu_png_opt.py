"""GPU checks of the PNG own-table hand-off (poppy_hip_set_frame_format(POPPY_FRAME_PNG_OPT): k_png_opt_cost and k_png_opt_pack of kernels_frame_png.hip between the
four kernels that POPPY_FRAME_PNG shares with it).  Every comparison is == on bytes against the host statement: poppy_bgr_to_png_opt_frame of the same frame for
the coder alone, poppy_png_optimal_lengths of the same counts for the length build alone, and the statement of the BGR frame that a BGR context hands out for the
same work for the frame path.  The host statements themselves are pinned to a restatement of the rule and to zlib's and Pillow's decoders in
tests/test_host_png_opt.py."""
import io

import numpy as np
import pytest

import golden_util as G
import png_opt_util as O
import png_util as P
from poppy_amd import capi, synth
from palette_util import collect as _collect, inputs as _inputs, loaded as _loaded

pytestmark = pytest.mark.gpu
E_ARG, E_UNSUPPORTED = -1, -6
W, H = 256, 192
HOST = {capi.FRAME_PNG: capi.bgr_to_png_frame, capi.FRAME_PNG_RUNS: capi.bgr_to_png_runs_frame, capi.FRAME_PNG_OPT: capi.bgr_to_png_opt_frame}
FAMILIES = [(name, limit) for name, (_, limits) in O.count_families().items() for limit in limits]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


try:
    from PIL import Image
except ImportError:                                         # the byte comparisons do not need it; only the decodes are left out
    Image = None


def _decodes_to(what, frame, bgr):
    if Image is None:
        return
    with Image.open(io.BytesIO(frame[4:].tobytes())) as im:
        im.load()
        assert im.mode == "RGB" and (np.asarray(im) == bgr[:, :, ::-1]).all(), f"{what}: the file does not decode to the frame"


def _same(what, bgr_frames, png_frames, small=lambda f: f, fmt=capi.FRAME_PNG_OPT):
    """the coded frames are the host statement of the BGR frames (small: the writer's geometry of a BGR frame), and decode to them"""
    assert len(bgr_frames) == len(png_frames) and len(png_frames) > 0, f"{what}: {len(bgr_frames)} BGR frames, {len(png_frames)} coded frames"
    for k, (b, p) in enumerate(zip(bgr_frames, png_frames)):
        assert b.ndim == 3, f"{what}: frame {k} of the BGR run has shape {b.shape}"
        P.equal(f"{what}: frame {k}", p, HOST[fmt](small(b)))
        _decodes_to(f"{what}: frame {k}", p, small(b))


def _both(what, run, small=lambda f: f, prepare=lambda c: None, **settings):
    """run(ctx) -> frames, on a BGR and on a PNG_OPT context"""
    out = []
    for fmt in (capi.FRAME_BGR, capi.FRAME_PNG_OPT):
        c = capi.Context(0, **settings)
        try:
            c.set_frame_format(fmt)
            if fmt == capi.FRAME_PNG_OPT:
                prepare(c)
            out.append(run(c))
        finally:
            c.close()
    _same(what, out[0], out[1], small)
    return out


# ---- the coder alone ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.cases()))
def test_coder_alone_on_the_content_set(ctx, name):
    bgr = O.cases()[name]
    h, w = bgr.shape[:2]
    want = capi.bgr_to_png_opt_frame(bgr)
    for pad in (range(16) if name in O.PADDED else (0,)):
        buf = ctx.bgr_to_png_opt_frame(bgr, row_pad=pad, whole=True)
        total = capi.png_frame_bytes(buf)
        assert total <= capi.frame_bytes(capi.FRAME_PNG_OPT, w, h) and (buf[total:] == capi.PNG_CANARY).all()
        P.equal(f"{name} pad {pad}", buf[:total], want)


def test_coder_alone_on_hundreds_of_segments(ctx):
    """640 x 360 textured: 85 segments.  1280 x 600 black: 282 segments, a second trip of the scan's loop over 256 segments, and every block is an own header and 33
    tokens, a few hundred bits, so that every other word of the frame is shared by two blocks.  1280 x 600 noise at capacity: a second trip of k_png_finish's loop."""
    for name, bgr, least in (("textured 640x360", synth.textured_bgr(640, 360, 3), 80),
                             ("black 1280x600", np.zeros((600, 1280, 3), np.uint8), 256),
                             ("noise 1280x600", np.random.default_rng(5).integers(0, 256, (600, 1280, 3), dtype=np.uint8), 256)):
        h, w = bgr.shape[:2]
        assert -(-h * (1 + 3 * w) // P.SEGMENT) > least
        want = capi.bgr_to_png_opt_frame(bgr)
        assert name != "noise 1280x600" or want.size > 256 * 8192
        assert name != "black 1280x600" or want.size < 282 * 64
        P.equal(name, ctx.bgr_to_png_opt_frame(bgr), want)


@pytest.mark.parametrize("name,limit", FAMILIES)
def test_length_build_alone_on_the_count_families(ctx, name, limit):
    counts = O.count_families()[name][0]
    assert ctx.png_optimal_lengths(counts, limit).tolist() == capi.png_optimal_lengths(counts, limit).tolist()


def test_refusals_keep_the_context(ctx):
    one = np.zeros(16, np.uint8)
    L = capi.lib()
    for w, h in ((26000, 26000), (1 << 30, 1)):
        assert L.poppy_hip_bgr_to_png_opt_frame(ctx.h, capi._p(one), 3 * w, w, h, capi._p(one)) == E_UNSUPPORTED
    assert L.poppy_hip_bgr_to_png_opt_frame(ctx.h, capi._p(one), 5, 2, 2, capi._p(one)) == E_ARG
    assert L.poppy_hip_bgr_to_png_opt_frame(ctx.h, None, 6, 2, 2, capi._p(one)) == E_ARG
    for fmt in (16383, 16385):
        assert L.poppy_hip_set_frame_format(ctx.h, fmt) == E_ARG
    counts, out = np.ones(286, np.uint32), np.zeros(286, np.uint8)
    g = L.poppy_hip_png_optimal_lengths
    assert g(ctx.h, None, 286, 15, capi._p(out)) == E_ARG and g(ctx.h, capi._p(counts), 286, 15, None) == E_ARG
    assert g(ctx.h, capi._p(counts), 287, 15, capi._p(out)) == E_ARG and g(ctx.h, capi._p(counts), 19, 8, capi._p(out)) == E_ARG
    assert g(ctx.h, capi._p(counts), 129, 7, capi._p(out)) == E_ARG and g(ctx.h, capi._p(np.zeros(4, np.uint32)), 4, 15, capi._p(out)) == E_ARG
    bgr = O.cases()["thread boundaries"]
    P.equal("after the refusals", ctx.bgr_to_png_opt_frame(bgr), capi.bgr_to_png_opt_frame(bgr))


# ---- the frame path -----------------------------------------------------------------------------------------------------------------------------------------
def test_chained_frames_of_the_textured_pair():
    shapes = [(k + 1) / 13 for k in range(12)]
    _both("12 chained frames", _loaded(W, H)(lambda c: _collect(c, c.render_many, shapes, chain=True)))


def test_phase_mode_twice_and_the_copies():
    def frames(c):
        out = []
        for _ in range(2):                                  # the second round replays the captured bodies
            out += _collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=False)
        return out
    _both("phase mode, twice", _loaded(W, H)(frames))
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], number_of_frames=2)

    def resident(c):
        c.pair_begin(inp["img1"], inp["img2"])
        return c.morph_frames(0.0) + c.morph_frames(1.0) + _collect(c, c.render_phases, [0.0, 0.5, 1.0])
    _both("phase 0 / 1 and t 0 / 1 on a resident pair", resident, number_of_frames=2)


def test_chained_frames_twice():
    def frames(c):
        out = []
        for _ in range(2):
            out += _collect(c, c.render_many, [0.25, 0.5, 0.75], chain=True)
        return out
    _both("chained, twice", _loaded(W, H)(frames))


def test_morph_list_of_three():
    images = [synth.gen(W, H, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2
        return [f for pair in frames for f in pair]
    _both("morph_list of 3", run, number_of_frames=4)


def test_one_pooled_pair():
    pair = (synth.gen(W, H, 77, 0, 0), synth.gen(W, H, 77, 6, 3))
    results = []
    for fmt in (capi.FRAME_BGR, capi.FRAME_PNG_OPT):
        p = capi.Pool([0], contexts_per_device=2, number_of_frames=4)
        try:
            got = {}
            p.set_frame_format(fmt)
            p.submit_pairs([pair], lambda pi, j, v: got.__setitem__((pi, j), v.copy()))
            p.wait()
            results.append(got)
        finally:
            p.close()
    bgr, png = results
    assert sorted(bgr) == sorted(png) and len(png) == 4
    keys = sorted(bgr)
    _same("one pooled pair", [bgr[k] for k in keys], [png[k] for k in keys])


def test_frame_scale_and_frame_size():
    run = _loaded(W, H)(lambda c: _collect(c, c.render_many, [0.25, 0.5, 0.75], chain=True) + _collect(c, c.render_many, [0.3, 0.6], chain=False))
    _both("scale 2", run, small=lambda f: capi.bgr_downscale(f, 2), prepare=lambda c: c.set_frame_scale(2))
    _both("size 100 x 70", run, small=lambda f: capi.bgr_resize_area(f, 100, 70), prepare=lambda c: c.set_frame_size(100, 70))


def test_format_switches_on_one_context_with_a_resident_pair():
    """PNG -> PNG_OPT -> JPEG_OPT -> PNG_RUNS -> PNG_OPT in phase mode on one resident pair (a synthetic one: its frames have runs): the frames of the three PNG
    formats are their host statements in every round, so no body captured under another format is replayed and the slot's coded buffers and scratch, which the
    formats share, are sized for the format at hand each time (PNG_OPT's scratch is the larger: the segments' own tables)."""
    c1, c2, g, p1, p2 = _inputs(W, H, c1=synth.gen(W, H, 1234, 0, 0), c2=synth.gen(W, H, 1234, 5, 2))
    shapes = [0.25, 0.5, 0.75]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        assert any(capi.bgr_to_png_runs_frame(f).size < capi.bgr_to_png_frame(f).size for f in bgr), "the pair's frames have no runs to speak of"
        assert all(capi.bgr_to_png_opt_frame(f).size <= capi.bgr_to_png_runs_frame(f).size for f in bgr)
        for fmt in (capi.FRAME_PNG, capi.FRAME_PNG_OPT, capi.FRAME_JPEG_OPT, capi.FRAME_PNG_RUNS, capi.FRAME_PNG_OPT):
            c.set_frame_format(fmt)
            for round_ in range(2):                             # the second round replays the bodies captured in the first
                got = _collect(c, c.render_many, shapes, chain=False)
                if fmt in HOST:
                    _same(f"format {fmt}, round {round_}", bgr, got, fmt=fmt)
    finally:
        c.close()


def test_png_sink_files_from_a_gpu_sequence_decode(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    shapes = [0.2, 0.5, 0.8]
    bgr, png = _both("sequence for the sink", _loaded(W, H)(lambda c: _collect(c, c.render_many, shapes, chain=True)))
    L = capi.lib()
    s = L.poppy_sink_open(str(tmp_path / "gpu_%05d.png").encode(), capi.SINK_PNG, W, H, 25, 1)
    for f in png:
        L.poppy_sink_write(s, capi._p(f), W, H, 0)
    assert L.poppy_sink_close(s) == len(png)
    for k, b in enumerate(bgr):
        with Image.open(tmp_path / f"gpu_{k:05d}.png") as im:
            assert (np.asarray(im.convert("RGB")) == b[:, :, ::-1]).all()
