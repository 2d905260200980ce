"""GPU checks of the JPEG hand-off on per-frame Huffman tables (POPPY_FRAME_JPEG_OPT, POPPY_FRAME_JPEG444_OPT: k_jpeg_count, k_jpeg_tables, and the OPT forms of
k_jpeg_code and k_jpeg_pack).  Every comparison is == on bytes against the host statement: poppy_jpeg_optimal_table for the build kernel alone,
poppy_i420_to_jpeg_opt_frame / poppy_i444_to_jpeg_opt_frame for the kernels alone, poppy_bgr_to_jpeg_opt_frame of the BGR frame that a BGR context hands out
for the same work for the frame path.  The host statement itself is pinned to a restatement of the rule in tests/test_host_jpeg_opt.py."""
import io

import numpy as np
import pytest

import jpeg444_util as U4
import jpeg_opt_util as O
import jpeg_util as U
from poppy_amd import capi, synth
from palette_util import collect as _collect, inputs as _inputs, loaded as _loaded

pytestmark = pytest.mark.gpu
E_ARG, E_UNSUPPORTED = -1, -6
Q = capi.JPEG_QUALITY_DEFAULT
HOST = {capi.FRAME_JPEG_OPT: capi.bgr_to_jpeg_opt_frame, capi.FRAME_JPEG444_OPT: capi.bgr_to_jpeg444_opt_frame}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _equal(what, got, want):
    assert got.ndim == 1 and got.size == want.size, f"{what}: {got.size} bytes, the host statement gives {want.size}"
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{what}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


def _same(what, bgr_frames, opt_frames, fmt=capi.FRAME_JPEG_OPT, quality=Q, small=lambda f: f):
    """the OPT frames are the host statement of the BGR frames (small: the writer's geometry of a BGR frame)"""
    assert len(bgr_frames) == len(opt_frames) and len(opt_frames) > 0, f"{what}: {len(bgr_frames)} BGR frames, {len(opt_frames)} coded frames"
    for k, (b, j) in enumerate(zip(bgr_frames, opt_frames)):
        assert b.ndim == 3, f"{what}: frame {k} of the BGR run has shape {b.shape}"
        _equal(f"{what}: frame {k}", j, HOST[fmt](small(b), quality))


def _both(what, run, fmt=capi.FRAME_JPEG_OPT, quality=Q, small=lambda f: f, prepare=lambda c: None, **settings):
    """run(ctx) -> frames, on a BGR and on an OPT context"""
    out = []
    for f in (capi.FRAME_BGR, fmt):
        c = capi.Context(0, **settings)
        try:
            c.set_frame_format(f)
            if f == fmt:
                if quality != Q:
                    c.set_jpeg_quality(quality)
                prepare(c)
            out.append(run(c))
        finally:
            c.close()
    _same(what, out[0], out[1], fmt, quality, small)
    return out


def test_build_kernel_alone_on_every_count_family(ctx):
    families = dict(O.count_families())
    st = {}
    O.jpeg_opt_frame_reference(capi.bgr_to_i420(synth.textured_bgr(160, 128)), 160, 128, 90, 420, st)
    for key, counts in st["counts"].items():
        families[f"textured_{key[0]}{key[1]}"] = counts
    for name, counts in families.items():
        want_bits, want_vals = capi.jpeg_optimal_table(counts)
        bits, vals = ctx.jpeg_optimal_table(counts)
        assert bits.tolist() == want_bits.tolist() and vals.tolist() == want_vals.tolist(), name


@pytest.mark.parametrize("quality", U.QUALITIES)
def test_kernels_alone_on_the_host_tests_content(ctx, quality):
    for name in U.CONTENTS:
        for w, h in U.SIZES:
            a = U.i420_content(name, w, h)
            _equal(f"{name} {w}x{h} q{quality}", ctx.i420_to_jpeg_opt_frame(a, w, h, quality), capi.i420_to_jpeg_opt_frame(a, w, h, quality))
        for w, h in U4.SIZES:
            a = U4.i444_content(name, w, h)
            _equal(f"4:4:4 {name} {w}x{h} q{quality}", ctx.i444_to_jpeg_opt_frame(a, w, h, quality), capi.i444_to_jpeg_opt_frame(a, w, h, quality))


@pytest.mark.parametrize("quality", (100, 90))
def test_noise_frame_of_115_segments_limits_lengths_on_the_device(ctx, quality):
    """640 x 360 noise: 29 counting workgroups add into one set of counts, and the luma AC table passes 16 bits before limiting (tests/test_host_jpeg_opt.py
    asserts that from the restatement); an odd size beside it whose last MCU column and row are clamped, in both samplings"""
    a = O.noise_i420(640, 360, 5)
    _equal(f"noise 640x360 q{quality}", ctx.i420_to_jpeg_opt_frame(a, 640, 360, quality), capi.i420_to_jpeg_opt_frame(a, 640, 360, quality))
    bgr = synth.textured_bgr(333, 211, 4)
    _equal("textured 333x211", ctx.i420_to_jpeg_opt_frame(capi.bgr_to_i420(bgr), 333, 211, quality), capi.bgr_to_jpeg_opt_frame(bgr, quality))
    _equal("textured 333x211 4:4:4", ctx.i444_to_jpeg_opt_frame(capi.bgr_to_i444(bgr), 333, 211, quality), capi.bgr_to_jpeg444_opt_frame(bgr, quality))


def test_more_segments_than_one_trip_of_the_counting_grid(ctx):
    """1280 x 832 in 4:4:4: 1040 segments, above the 1024 that the counting pass's 256 workgroups of four waves take in one trip"""
    w, h = 1280, 832
    a = capi.bgr_to_i444(np.ascontiguousarray(np.tile(synth.textured_bgr(320, 208, 9), (4, 4, 1))))
    _equal("textured 1280x832 4:4:4", ctx.i444_to_jpeg_opt_frame(a, w, h, Q), capi.i444_to_jpeg_opt_frame(a, w, h, Q))


def test_two_frames_back_to_back_and_the_first_again():
    """The counts are zero again after a frame.  A slot's coder scratch, with the frame's count tables in it, is allocated and cleared ONCE and then codes every
    frame the slot renders; a context has at most 8 slots in a ring, so 24 phase-mode frames put at least three frames through every slot's scratch.  The pair is
    a textured image against a smooth one and the shapes alternate between the two ends, so consecutive frames of a slot have different symbol counts: counts
    that k_jpeg_tables left behind would add to the next frame's and give it other tables.  (The stand-alone entries below allocate and clear a scratch per call.)"""
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h, c1=synth.textured_bgr(w, h, 41), c2=synth.gen(w, h, 77, 0, 0))
    shapes = [0.04 + 0.02 * (k % 3) if k % 2 == 0 else 0.96 - 0.02 * (k % 5) for k in range(24)]

    def run(c):
        c.pair_load(c1, c2, g, p1, p2)
        return _collect(c, c.render_many, shapes, chain=False) + _collect(c, c.render_many, shapes[::-1], chain=False)
    bgr, opt = _both("24 different frames through the slots, twice", run)
    sizes = [f.size for f in opt[:24]]
    assert max(sizes) > 1.2 * min(sizes), f"the frames of the two ends are alike: {min(sizes)} .. {max(sizes)} bytes"


def test_stand_alone_calls_are_independent(ctx):
    w, h = 160, 128
    a, b = U.i420_content("noise", w, h), U.i420_content("flat128", w, h)
    want_a, want_b = capi.i420_to_jpeg_opt_frame(a, w, h, Q), capi.i420_to_jpeg_opt_frame(b, w, h, Q)
    for k, (planes, want) in enumerate(((a, want_a), (b, want_b), (a, want_a), (b, want_b))):
        _equal(f"frame {k}", ctx.i420_to_jpeg_opt_frame(planes, w, h, Q), want)


def test_refusals_keep_the_context(ctx):
    one = np.zeros(16, np.uint8)
    L = capi.lib()
    for call in (L.poppy_hip_i420_to_jpeg_opt_frame, L.poppy_hip_i444_to_jpeg_opt_frame):
        for w, h in ((65536, 1), (65535, 65535)):
            assert call(ctx.h, capi._p(one), w, h, Q, capi._p(one)) == E_UNSUPPORTED
        assert call(ctx.h, capi._p(one), 2, 2, 0, capi._p(one)) == E_ARG
    for fmt in (4095, 4097, 8191, 8193):
        assert L.poppy_hip_set_frame_format(ctx.h, fmt) == E_ARG
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), np.zeros(1, np.int32)
    for counts in ([0] * 256, [0xffffffff] + [0] * 255, [0x80000000] * 2 + [0] * 254):
        assert L.poppy_hip_jpeg_optimal_table(ctx.h, capi._p(np.asarray(counts, np.uint32)), capi._p(bits), capi._p(vals), capi._p(n)) == E_ARG
    assert L.poppy_hip_jpeg_optimal_table(ctx.h, None, capi._p(bits), capi._p(vals), capi._p(n)) == E_ARG
    a = U.i420_content("gradient", 48, 48)
    _equal("after the refusals", ctx.i420_to_jpeg_opt_frame(a, 48, 48, Q), capi.i420_to_jpeg_opt_frame(a, 48, 48, Q))


@pytest.mark.parametrize("fmt", (capi.FRAME_JPEG_OPT, capi.FRAME_JPEG444_OPT))
def test_chained_sequence_and_phase_mode_twice(fmt):
    w, h = 256, 192

    def frames(c):
        out = _collect(c, c.render_many, [(k + 1) / 9 for k in range(8)], chain=True)
        c.reset()
        for _ in range(2):                                  # the second round replays the captured bodies
            out += _collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=False)
        return out
    _both("chained, then phase mode twice", _loaded(w, h)(frames), fmt)


def test_copies_and_phase_0_and_1():
    w, h = 128, 96
    a, b = synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6, 3)

    def resident(c):
        c.pair_begin(a, b)
        return c.morph_frames(0.0) + c.morph_frames(1.0) + _collect(c, c.render_phases, [0.0, 0.5, 1.0])
    _both("phase 0 / 1 and t 0 / 1 on a resident pair", resident, number_of_frames=2)


def test_frame_scale_then_quality_changed_between_two_calls():
    w, h = 256, 192
    run = _loaded(w, h)(lambda c: _collect(c, c.render_many, [0.25, 0.5, 0.75], chain=True) + _collect(c, c.render_many, [0.3, 0.6], chain=False))
    _both("scale 2", run, small=lambda f: capi.bgr_downscale(f, 2), prepare=lambda c: c.set_frame_scale(2))
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        c.set_frame_format(capi.FRAME_JPEG_OPT)
        first = _collect(c, c.render_many, shapes, chain=False)          # captures the bodies
        c.set_jpeg_quality(35)
        second = _collect(c, c.render_many, shapes, chain=False)         # ... which are replayed on the new quantiser
        _same("default quality", bgr, first)
        _same("quality 35, captured bodies", bgr, second, quality=35)
        assert U.walk_frame(second[0])["qtables"][0] == [int(x) for x in U.quant_tables(35)[0][U.ZIGZAG]]
    finally:
        c.close()


def test_pool_of_two_contexts_with_frames_of_two_slots_in_flight():
    w, h = 256, 192
    pairs = [(synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6 + k, 3)) for k in range(3)]
    results = []
    for fmt in (capi.FRAME_BGR, capi.FRAME_JPEG_OPT):
        p = capi.Pool([0], contexts_per_device=2, number_of_frames=4)
        try:
            got = {}
            p.set_frame_format(fmt)
            p.set_jpeg_quality(60)
            p.submit_pairs(pairs, lambda pi, j, v: got.__setitem__((pi, j), v.copy()))
            p.wait()
            results.append(got)
        finally:
            p.close()
    bgr, opt = results
    assert sorted(bgr) == sorted(opt) and len(opt) == len(pairs) * 4
    keys = sorted(bgr)
    _same("pool batch", [bgr[k] for k in keys], [opt[k] for k in keys], quality=60)


def test_mjpeg_sink_file_from_a_gpu_sequence_decodes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    w, h = 256, 192
    shapes = [0.2, 0.5, 0.8]
    _, frames = _both("sequence for the sink", _loaded(w, h)(lambda c: _collect(c, c.render_many, shapes, chain=True)))
    L = capi.lib()
    path = tmp_path / "gpu.avi"
    s = L.poppy_sink_open(str(path).encode(), capi.SINK_MJPEG, w, h, 25, 1)
    for f in frames:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(frames)
    data = path.read_bytes()
    (riff,) = U.walk_riff(data)
    movi = riff[4][1]
    assert len(movi[4]) == len(frames)
    for k, (cc, at, n, _, _) in enumerate(movi[4]):
        assert cc == b"00dc" and data[at:at + n] == frames[k][4:].tobytes()
        with Image.open(io.BytesIO(data[at:at + n])) as im:
            im.load()
            assert im.size == (w, h) and im.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
