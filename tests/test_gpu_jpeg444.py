"""GPU checks of the 4:4:4 JPEG frame hand-off (poppy_hip_set_frame_format(POPPY_FRAME_JPEG444): k_bgr_to_i444, k_jpeg_code's 4:4:4 instantiation, k_jpeg_pack).
Every comparison is == on bytes against the host statement: poppy_bgr_to_i444 for the conversion kernel alone, poppy_i444_to_jpeg_frame for the coder alone,
poppy_bgr_to_jpeg444_frame of the BGR frame that a BGR context hands out for the same work for the frame path.  The host statements themselves are pinned to a
restatement of the rule in tests/test_host_jpeg444.py."""
import io

import numpy as np
import pytest

import golden_util as G
import jpeg444_util as V
from poppy_amd import capi, synth
from palette_util import collect as _collect, inputs as _inputs, loaded as _loaded

pytestmark = pytest.mark.gpu
E_ARG, E_UNSUPPORTED = -1, -6
Q = capi.JPEG_QUALITY_DEFAULT
HOST = {capi.FRAME_JPEG: capi.bgr_to_jpeg_frame, capi.FRAME_JPEG444: capi.bgr_to_jpeg444_frame}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _equal(what, got, want):
    assert got.ndim == 1 and got.size == want.size, f"{what}: {got.size} bytes, the host statement gives {want.size}"
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{what}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


def _same(what, bgr_frames, jpeg_frames, quality=Q, small=lambda f: f, fmt=capi.FRAME_JPEG444):
    """the coded frames are the format's host statement of the BGR frames (small: the writer's geometry of a BGR frame)"""
    assert len(bgr_frames) == len(jpeg_frames) and len(jpeg_frames) > 0, f"{what}: {len(bgr_frames)} BGR frames, {len(jpeg_frames)} coded frames"
    for k, (b, j) in enumerate(zip(bgr_frames, jpeg_frames)):
        assert b.ndim == 3, f"{what}: frame {k} of the BGR run has shape {b.shape}"
        _equal(f"{what}: frame {k}", j, HOST[fmt](small(b), quality))


def _both(what, run, quality=Q, small=lambda f: f, prepare=lambda c: None, **settings):
    """run(ctx) -> frames, on a BGR and on a JPEG444 context"""
    out = []
    for fmt in (capi.FRAME_BGR, capi.FRAME_JPEG444):
        c = capi.Context(0, **settings)
        try:
            c.set_frame_format(fmt)
            if fmt == capi.FRAME_JPEG444:
                if quality != Q:
                    c.set_jpeg_quality(quality)
                prepare(c)
            out.append(run(c))
        finally:
            c.close()
    _same(what, out[0], out[1], quality, small)
    return out


# ---- the conversion kernel alone ----------------------------------------------------------------------------------------------------------------------------
CUBE = np.array([[[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)]], np.uint8)


@pytest.mark.parametrize("w,h", ((1, 1), (7, 3), (8, 2), (16, 5), (24, 9), (1024, 3), (1027, 3)))
def test_conversion_kernel_alone(ctx, w, h):
    """Widths that are multiples of 8 take the wide kernel when the row pad leaves the device source 8-byte aligned (pads 0 and 8) and the bytewise one at every
    other alignment; the other widths take the bytewise kernel.  1024 x 3 and 1027 x 3 are more than one workgroup of either."""
    noise = np.random.default_rng(w * 31 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    corners = np.ascontiguousarray(np.resize(CUBE.reshape(-1, 3), (h * w, 3)).reshape(h, w, 3))      # the cube's corners, cycled: both chroma clamps
    for name, bgr in (("noise", noise), ("corners", corners)):
        want = capi.bgr_to_i444(bgr)
        for pad in (range(16) if w % 8 == 0 else (0, 3)):
            _equal(f"{name} {w}x{h} pad {pad}", ctx.bgr_to_i444(bgr, row_pad=pad), want)


def test_conversion_refusals_keep_the_context(ctx):
    one = np.zeros(16, np.uint8)
    L = capi.lib()
    assert L.poppy_hip_bgr_to_i444(ctx.h, None, 6, 2, 2, capi._p(one)) == E_ARG and L.poppy_hip_bgr_to_i444(ctx.h, capi._p(one), 5, 2, 2, capi._p(one)) == E_ARG
    assert L.poppy_hip_bgr_to_i444(ctx.h, capi._p(one), 6, 0, 2, capi._p(one)) == E_ARG
    _equal("after the refusals", ctx.bgr_to_i444(CUBE), capi.bgr_to_i444(CUBE))


# ---- the coder alone ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", V.QUALITIES)
def test_coder_alone_on_the_host_tests_content(ctx, quality):
    for name in V.CONTENTS:
        for w, h in V.SIZES:
            a = V.i444_content(name, w, h)
            _equal(f"{name} {w}x{h} q{quality}", ctx.i444_to_jpeg_frame(a, w, h, quality), capi.i444_to_jpeg_frame(a, w, h, quality))


def test_coder_alone_on_hundreds_of_segments(ctx):
    """640 x 416: 4 160 MCUs, 260 segments — more than k_jpeg_pack's 256 threads, so its strided sums take a second trip; an odd size beside it whose last MCU
    column and row are clamped."""
    assert -(-(640 // 8) * (416 // 8) // 16) == 260
    for w, h, seed in ((640, 416, 3), (333, 211, 4)):
        a = capi.bgr_to_i444(synth.textured_bgr(w, h, seed))
        _equal(f"textured {w}x{h}", ctx.i444_to_jpeg_frame(a, w, h, Q), capi.i444_to_jpeg_frame(a, w, h, Q))
    a = V.i444_content("noise", 640, 416)
    _equal("noise 640x416 q100", ctx.i444_to_jpeg_frame(a, 640, 416, 100), capi.i444_to_jpeg_frame(a, 640, 416, 100))


def test_refusals_keep_the_context(ctx):
    one = np.zeros(16, np.uint8)
    L = capi.lib()
    for w, h in ((65536, 1), (65535, 65535), (16000, 16000)):
        assert L.poppy_hip_i444_to_jpeg_frame(ctx.h, capi._p(one), w, h, Q, capi._p(one)) == E_UNSUPPORTED
    assert L.poppy_hip_i444_to_jpeg_frame(ctx.h, capi._p(one), 2, 2, 0, capi._p(one)) == E_ARG
    for fmt in (511, 513):
        assert L.poppy_hip_set_frame_format(ctx.h, fmt) == E_ARG
    a = V.i444_content("gradient", 40, 40)
    _equal("after the refusals", ctx.i444_to_jpeg_frame(a, 40, 40, Q), capi.i444_to_jpeg_frame(a, 40, 40, Q))


# ---- the frame path -----------------------------------------------------------------------------------------------------------------------------------------
def test_sixty_chained_frames_of_the_textured_pair():
    w, h = 256, 192
    shapes = [(k + 1) / 61 for k in range(60)]
    _both("60 chained frames", _loaded(w, h)(lambda c: _collect(c, c.render_many, shapes, chain=True)))


def test_phase_mode_twice_and_the_copies():
    w, h = 256, 192

    def frames(c):
        out = []
        for _ in range(2):                                  # the second round replays the captured bodies
            out += _collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=False)
        return out
    _both("phase mode, twice", _loaded(w, h)(frames))
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], number_of_frames=2)

    def resident(c):
        c.pair_begin(inp["img1"], inp["img2"])
        return c.morph_frames(0.0) + c.morph_frames(1.0) + _collect(c, c.render_phases, [0.0, 0.5, 1.0])
    _both("phase 0 / 1 and t 0 / 1 on a resident pair", resident, number_of_frames=2)


def test_morph_list_of_three():
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2
        return [f for pair in frames for f in pair]
    _both("morph_list of 3", run, number_of_frames=4)


def test_pool_of_two_contexts_queued_at_another_quality():
    w, h = 256, 192
    pairs = [(synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6 + k, 3)) for k in range(3)]
    results = []
    for fmt in (capi.FRAME_BGR, capi.FRAME_JPEG444):
        p = capi.Pool([0], contexts_per_device=2, number_of_frames=4)
        try:
            got = {}
            p.set_frame_format(fmt)
            p.set_jpeg_quality(60)
            for b in range(2):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            p.wait()
            results.append(got)
        finally:
            p.close()
    bgr, jpeg = results
    assert sorted(bgr) == sorted(jpeg) and len(jpeg) == 2 * len(pairs) * 4
    keys = sorted(bgr)
    _same("pool batches", [bgr[k] for k in keys], [jpeg[k] for k in keys], 60)


def test_frame_scale_and_frame_size():
    w, h = 256, 192
    run = _loaded(w, h)(lambda c: _collect(c, c.render_many, [0.25, 0.5, 0.75], chain=True) + _collect(c, c.render_many, [0.3, 0.6], chain=False))
    _both("scale 2", run, small=lambda f: capi.bgr_downscale(f, 2), prepare=lambda c: c.set_frame_scale(2))
    _both("size 100 x 70", run, small=lambda f: capi.bgr_resize_area(f, 100, 70), prepare=lambda c: c.set_frame_size(100, 70))


def test_quality_changed_between_two_calls_on_one_context():
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        c.set_frame_format(capi.FRAME_JPEG444)
        first = _collect(c, c.render_many, shapes, chain=False)          # captures the bodies
        c.set_jpeg_quality(35)
        second = _collect(c, c.render_many, shapes, chain=False)         # ... which are replayed on the new tables
        c.reset()
        third = _collect(c, c.render_many, shapes, chain=True)
        c.reset()
        c.set_frame_format(capi.FRAME_BGR)
        bgr_chained = _collect(c, c.render_many, shapes, chain=True)
        _same("default quality", bgr, first, Q)
        _same("quality 35, captured bodies", bgr, second, 35)
        _same("quality 35, chained", bgr_chained, third, 35)
        assert V.walk_frame(second[0])["qtables"][0] == [int(x) for x in V.quant_tables(35)[0][V.ZIGZAG]]
        assert V.walk_frame(first[0])["qtables"] != V.walk_frame(second[0])["qtables"]
    finally:
        c.close()


def test_format_switches_on_one_context_with_a_resident_pair():
    """JPEG -> JPEG444 -> JPEG in phase mode on one resident pair: every run's frames are its own format's host statement, so no body captured under the other
    format is replayed, and the slot's coded buffers are sized for the format at hand each time."""
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        for fmt in (capi.FRAME_JPEG, capi.FRAME_JPEG444, capi.FRAME_JPEG):
            c.set_frame_format(fmt)
            for round_ in range(2):                             # the second round replays the bodies captured in the first
                got = _collect(c, c.render_many, shapes, chain=False)
                _same(f"format {fmt}, round {round_}", bgr, got, Q, fmt=fmt)
                assert V.walk_frame(got[0])["sampling"][0][1] == (0x11 if fmt == capi.FRAME_JPEG444 else 0x22)
    finally:
        c.close()


def test_mjpeg_sink_file_from_a_gpu_sequence_decodes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    w, h = 256, 192
    shapes = [0.2, 0.5, 0.8]
    _, jpeg = _both("sequence for the sink", _loaded(w, h)(lambda c: _collect(c, c.render_many, shapes, chain=True)))
    L = capi.lib()
    path = tmp_path / "gpu.avi"
    s = L.poppy_sink_open(str(path).encode(), capi.SINK_MJPEG, w, h, 25, 1)
    for f in jpeg:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(jpeg)
    data = path.read_bytes()
    (riff,) = V.walk_riff(data)
    movi = riff[4][1]
    assert riff[2] == len(data) - 8 and movi[3] == b"movi" and len(movi[4]) == len(jpeg)
    for k, (cc, at, n, _, _) in enumerate(movi[4]):
        assert cc == b"00dc" and data[at:at + n] == jpeg[k][4:].tobytes()
        with Image.open(io.BytesIO(data[at:at + n])) as im:
            im.load()
            assert im.size == (w, h) and im.layer == V.LAYERS
