"""GPU checks of the JPEG hand-off on one Huffman table set per sequence (POPPY_FRAME_JPEG_SEQ, POPPY_FRAME_JPEG444_SEQ: the raster kernel and k_jpeg_count per
frame into the sequence's counts, k_jpeg_tables once on the sums, the OPT forms of k_jpeg_code and k_jpeg_pack per frame on what it built).  Every comparison is ==
on bytes against the host statement, poppy_bgr_frames_to_jpeg_seq_frames / poppy_bgr_frames_to_jpeg444_seq_frames: of the same frames for the stand-alone entry,
of the BGR frames that a BGR context hands out for the same work for the frame path.  tests/test_host_jpeg_seq.py pins the host statement to a restatement."""
import io

import numpy as np
import pytest

import jpeg_seq_util as S
import jpeg_util as U
import palette_seq_util as PS
from poppy_amd import capi, synth
from palette_util import collect as _collect, inputs as _inputs, loaded as _loaded

try:
    from PIL import Image
except ImportError:                                             # the coefficient comparison alone then carries "decodes to JPEG's pixels"
    Image = None

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_UNSUPPORTED = -1, -4, -6
Q = capi.JPEG_QUALITY_DEFAULT
SEQ, SEQ444 = capi.FRAME_JPEG_SEQ, capi.FRAME_JPEG444_SEQ
STAGE_RING = 8                                                  # context.h: kStageRing, the ring buffers of the hand-over


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _equal(what, got, want):
    assert got.ndim == 1 and got.size == want.size, f"{what}: {got.size} bytes, the host statement gives {want.size}"
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{what}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


def _equal_seq(what, got, want):
    assert len(got) == len(want) and len(want) > 0, f"{what}: {len(got)} frames, the host statement gives {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        _equal(f"{what}: frame {k}", g, w)


def _direct(ctx, frames, quality, fmt, what, **pads):
    got = ctx.bgr_frames_to_jpeg_seq_frames(frames, quality, fmt, **pads)
    _equal_seq(what, got, capi.bgr_frames_to_jpeg_seq_frames(frames, quality, fmt))
    return got


def _same(what, bgr_seqs, seq_seqs, fmt=SEQ, quality=Q, small=lambda f: f):
    """every sequence of the SEQ run is the host statement of the BGR run's frames of that sequence (small: the writer's geometry of a BGR frame)"""
    assert len(bgr_seqs) == len(seq_seqs) and len(seq_seqs) > 0, f"{what}: {len(bgr_seqs)} BGR sequences, {len(seq_seqs)} coded ones"
    for k, (b, j) in enumerate(zip(bgr_seqs, seq_seqs)):
        assert len(b) == len(j) and len(j) > 0 and all(f.ndim == 3 for f in b), f"{what}: sequence {k}: {len(b)} BGR frames, {len(j)} coded frames"
        _equal_seq(f"{what}: sequence {k}", j, S.host_seq([small(f) for f in b], quality, fmt))


def _both(what, run, fmt=SEQ, quality=Q, small=lambda f: f, prepare=lambda c: None, **settings):
    """run(ctx) -> a list of sequences (each what one call handed to its writer), on a BGR and on a SEQ context"""
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


# ---- the stand-alone entry ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("quality", S.QUALITIES)
def test_stand_alone_entry_on_the_host_tests_sequences(ctx, fmt, quality):
    for w, h in S.SIZES:
        for n in S.LENGTHS:
            frames = S.sequence(n, w, h)
            got = _direct(ctx, frames, quality, fmt, f"{w}x{h} n={n} q{quality}")
            if n == 1:                                           # ... and a sequence of one frame is the context's own OPT frame of its planes
                opt = (ctx.i444_to_jpeg_opt_frame if fmt == SEQ444 else ctx.i420_to_jpeg_opt_frame)(S.PLANES_OF[fmt](frames[0]), w, h, quality)
                _equal(f"{w}x{h} q{quality}: n = 1 against the context's OPT frame", got[0], opt)
    frames = S.sequence(5, 17, 9)
    _direct(ctx, frames, quality, fmt, "17x9 padded", row_pad=5, frame_pad=11)
    _direct(ctx, S.flat_noise_gradient(), quality, fmt, "flat, noise, gradient")


def test_stand_alone_calls_are_independent(ctx):
    """the same call twice on one context with another sequence in between: a call's counts begin at zero and are not cleared between its frames"""
    a, b = S.sequence(5, 160, 128), S.flat_noise_gradient()
    for fmt in S.FORMATS:
        for k, frames in enumerate((a, b, a, b[::-1], a[:2])):
            _direct(ctx, frames, Q, fmt, f"call {k}")


@pytest.mark.parametrize("quality", (100, 90))
def test_two_noise_frames_limit_lengths_on_summed_counts(ctx, quality):
    """two 640 x 360 noise frames: 29 counting workgroups per frame add into one table twice, and at quality 100 the summed luma AC table passes 16 bits before
    limiting (tests/test_host_jpeg_seq.py asserts that from the restatement)"""
    _direct(ctx, S.two_noise_frames(), quality, SEQ, f"two noise frames q{quality}")


def test_more_segments_than_one_trip_of_the_counting_grid(ctx):
    """1280 x 832 in 4:4:4, two frames: 1040 segments each, above the 1024 that the counting pass's 256 workgroups of four waves take in one trip, summed"""
    frames = np.stack([np.ascontiguousarray(np.tile(synth.textured_bgr(320, 208, 9 + k), (4, 4, 1))) for k in range(2)])
    _direct(ctx, frames, Q, SEQ444, "textured 1280x832 4:4:4 x 2")


# ---- the frame path -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_chained_sequence_and_phase_mode_twice(fmt):
    w, h = 256, 192

    def seqs(c):
        out = [_collect(c, c.render_many, [(k + 1) / 9 for k in range(8)], chain=True)]
        c.reset()
        for _ in range(2):                                      # the second round replays the captured bodies
            out.append(_collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=False))
        return out
    bgr, seq = _both("chained, then phase mode twice", _loaded(w, h)(seqs), fmt)
    for frames in seq:                                          # one header per sequence
        at = U.walk_frame(frames[0])["data_offset"]
        assert all(np.array_equal(f[4:4 + at], frames[0][4:4 + at]) for f in frames)


def test_long_runs_reuse_every_ring_buffer_and_frames_differ_in_size():
    """The textured-against-smooth pair, shapes alternating between the two ends: 24 phase-mode frames and 17 chained ones, each more than twice the ring, so that
    every ring buffer, its coder scratch and its pinned word carry at least two frames of one sequence; the frames of the two ends differ in size by more than 1.2x.
    The same sequence again afterwards: the counts were zero in front of it."""
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h, c1=synth.textured_bgr(w, h, 41), c2=synth.gen(w, h, 77, 0, 0))
    shapes = [0.04 + 0.02 * (k % 3) if k % 2 == 0 else 0.96 - 0.02 * (k % 5) for k in range(24)]
    chained = [(k + 1) / 18 for k in range(17)]
    assert len(shapes) >= 2 * STAGE_RING + 1 and len(chained) >= 2 * STAGE_RING + 1

    def run(c):
        c.pair_load(c1, c2, g, p1, p2)
        out = [_collect(c, c.render_many, shapes, chain=False), _collect(c, c.render_many, chained, chain=True)]
        c.reset()
        return out + [_collect(c, c.render_many, shapes, chain=False)]
    bgr, seq = _both("24 phase-mode frames, 17 chained, the 24 again", run)
    sizes = [f.size for f in seq[0]]
    assert max(sizes) > 1.2 * min(sizes), f"the frames of the two ends are alike: {min(sizes)} .. {max(sizes)} bytes"
    _equal_seq("the same sequence again", seq[2], seq[0])


def test_writer_is_first_called_after_the_last_frame():
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    c = capi.Context(0)
    try:
        c.set_frame_format(SEQ)
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


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_copies_and_phase_0_and_1(fmt):
    w, h = 128, 96
    a, b = synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6, 3)

    def resident(c):
        c.pair_begin(a, b)
        return [c.morph_frames(0.0), c.morph_frames(1.0), _collect(c, c.render_phases, [0.0, 0.3, 0.5, 1.0, 0.0, 0.7, 1.0])]
    _both("phase 0 / 1 and t 0 / 1 on a resident pair", resident, fmt, number_of_frames=3)


def test_morph_list_of_three_is_one_sequence_per_pair():
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2 and len(frames) == 2
        return frames
    bgr, seq = _both("morph_list of 3", run, number_of_frames=4)
    first, second = (U.walk_frame(s[0]) for s in seq)
    assert first["dht"] != second["dht"], "the two pairs share their tables"


def test_pool_of_two_contexts_queued_and_the_format_while_work_is_queued():
    w, h = 256, 192
    pairs = [(synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6 + k, 3)) for k in range(3)]
    results = []
    for fmt in (capi.FRAME_BGR, SEQ):
        p = capi.Pool([0], contexts_per_device=2, number_of_frames=4)
        try:
            got = {}
            p.set_frame_format(fmt)
            p.set_jpeg_quality(60)
            for b in range(2):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            with pytest.raises(capi.PoppyError, match=str(E_STATE)):      # as PAL8_SEQ answers it: not while sequences are open or queued
                p.set_frame_format(capi.FRAME_BGR if fmt == SEQ else SEQ)
            p.wait()
            p.set_frame_format(fmt)                                 # waited for: allowed again
            results.append(got)
        finally:
            p.close()
    bgr, seq = results
    assert sorted(bgr) == sorted(seq) and len(seq) == 2 * len(pairs) * 4
    calls = sorted({k[:2] for k in bgr})
    _same("pool batches", [[bgr[c + (j,)] for j in range(4)] for c in calls], [[seq[c + (j,)] for j in range(4)] for c in calls], quality=60)


def test_frame_scale_frame_size_and_a_quality_changed_between_two_calls():
    w, h = 256, 192
    run = _loaded(w, h)(lambda c: [_collect(c, c.render_many, [0.25, 0.5, 0.75], chain=True), _collect(c, c.render_many, [0.3, 0.6], chain=False),
                                   _collect(c, c.render_phases, [0.0, 0.4, 1.0])])
    _both("scale 2", run, small=lambda f: capi.bgr_downscale(f, 2), prepare=lambda c: c.set_frame_scale(2))
    _both("size 100 x 70, 4:4:4", run, SEQ444, small=lambda f: capi.bgr_resize_area(f, 100, 70), prepare=lambda c: c.set_frame_size(100, 70))
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        c.set_frame_format(SEQ)
        first = _collect(c, c.render_many, shapes, chain=False)          # captures the bodies
        c.set_jpeg_quality(35)
        second = _collect(c, c.render_many, shapes, chain=False)         # ... which are replayed; the pass and the coder read the new quantiser
        _same("default quality", [bgr], [first])
        _same("quality 35", [bgr], [second], quality=35)
        assert U.walk_frame(second[0])["qtables"][0] == [int(x) for x in U.quant_tables(35)[0][U.ZIGZAG]]
    finally:
        c.close()


def test_switching_formats_on_one_context():
    """JPEG_SEQ -> JPEG_OPT -> PAL8_SEQ -> JPEG444_SEQ -> JPEG_SEQ on one context with a resident pair, each against its host statement of a BGR context's frames:
    the stores and tables of the two sequence kinds, and the slots' OPT scratch, do not disturb each other"""
    w, h = 320, 200
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]

    def seqs(c):
        c.reset()
        return [_collect(c, c.render_many, shapes, chain=True), _collect(c, c.render_many, shapes, chain=False)]
    plain = capi.Context(0)
    try:
        plain.pair_load(c1, c2, g, p1, p2)
        bgr = seqs(plain)
    finally:
        plain.close()
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        for k, fmt in enumerate((SEQ, capi.FRAME_JPEG_OPT, capi.FRAME_PAL8_SEQ, SEQ444, SEQ)):
            c.set_frame_format(fmt)
            got = seqs(c)
            if fmt in S.FORMATS:
                _same(f"step {k}", bgr, got, fmt)
            for b, j in zip(bgr, got):
                if fmt == capi.FRAME_PAL8_SEQ:
                    PS.same_seq(f"step {k}: PAL8_SEQ", b, j)
                elif fmt == capi.FRAME_JPEG_OPT:
                    _equal_seq(f"step {k}: JPEG_OPT", j, [capi.bgr_to_jpeg_opt_frame(f, Q) for f in b])
    finally:
        c.close()


def test_timing_mode_marks():
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    plain = capi.Context(0); c = capi.Context(0)
    try:
        c.set_frame_format(SEQ)
        plain.pair_load(c1, c2, g, p1, p2); c.pair_load(c1, c2, g, p1, p2)
        want = _collect(plain, plain.render_many, [0.2, 0.5, 0.8], chain=True)
        c.set_timing(1)
        frames = _collect(c, c.render_many, [0.2, 0.5, 0.8], chain=True)
        names = {n: k for n, _, k in c.timing_summary()}
        assert (names.get("frame_format"), names.get("jpeg_count"), names.get("jpeg_tables"), names.get("jpeg_code"), names.get("jpeg_pack")) == (3, 3, 1, 3, 3), names
        assert "pal8_seq_hist" not in names and "pal8_seq_build" not in names
        c.set_timing(0)
        _same("timing mode 1", [want], [frames])
    finally:
        plain.close(); c.close()


def test_refusals_keep_the_resident_pair():
    sw, sh = 64, 64
    s1, s2, sg, sp1, sp2 = _inputs(sw, sh)
    L = capi.lib()
    c = capi.Context(0)
    try:
        c.set_frame_format(SEQ)
        c.pair_load(s1, s2, sg, sp1, sp2)
        want = _collect(c, c.render_many, [0.3, 0.7], chain=True)
        # a sequence over the symbol bound: refused on the count alone, nothing rendered, nothing written
        most = S.SEQ_MAX_SYMBOLS // (S.blocks_per_frame(sw, sh) * 64)
        before = sum(c.warp_counts())
        calls = []
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.render_phases(np.full(most + 1, 0.5), write=lambda v: calls.append(1))
        assert sum(c.warp_counts()) == before and not calls, "frames were rendered or written before the refusal"
        one = np.zeros((2, 2, 3), np.uint8)
        room = np.zeros(capi.frame_bytes(SEQ, 2, 2), np.uint8)
        for call in (L.poppy_hip_bgr_frames_to_jpeg_seq_frames, L.poppy_hip_bgr_frames_to_jpeg444_seq_frames):
            assert call(c.h, capi._p(one), 6, 12, (1 << 31) - 1, 2, 2, Q, capi._p(room)) == E_UNSUPPORTED
            assert call(c.h, capi._p(one), 3 * 65536, 1 << 40, 1, 65536, 1, Q, capi._p(room)) == E_UNSUPPORTED      # (refused before a byte is read)
            assert call(c.h, capi._p(one), 6, 12, 0, 2, 2, Q, capi._p(room)) == E_ARG and call(c.h, capi._p(one), 6, 11, 1, 2, 2, Q, capi._p(room)) == E_ARG
            assert call(c.h, capi._p(one), 6, 12, 1, 2, 2, 0, capi._p(room)) == E_ARG and call(c.h, None, 6, 12, 1, 2, 2, Q, capi._p(room)) == E_ARG
        for fmt in (32767, 32769, 65535, 65537):
            assert L.poppy_hip_set_frame_format(c.h, fmt) == E_ARG
        # the stand-alone entry works on buffers and tables of its own, at its own quality: the resident pair and the context's sequence are as they were
        _direct(c, S.flat_noise_gradient(), 25, SEQ444, "stand-alone entry on a context with a resident pair")
        c.reset()
        _equal_seq("after the refusals", _collect(c, c.render_many, [0.3, 0.7], chain=True), want)
    finally:
        c.close()


def test_mjpeg_sink_file_from_a_gpu_sequence_decodes(tmp_path):
    """every chunk of the file is a frame's own bytes, and holds the quantised coefficients of that frame's POPPY_FRAME_JPEG frame (entropy-decoded through the
    restatement); where Pillow is installed it opens the chunks and gives that frame's pixels"""
    w, h = 256, 192
    shapes = [0.2, 0.5, 0.8]
    bgr, seq = _both("sequence for the sink", _loaded(w, h)(lambda c: [_collect(c, c.render_many, shapes, chain=True)]))
    frames = seq[0]
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
        chunk = np.frombuffer((n + 4).to_bytes(4, "little") + data[at:at + n], np.uint8)
        std = capi.bgr_to_jpeg_frame(bgr[0][k], Q)
        assert U.walk_frame(chunk)["size"] == (w, h) and (S.frame_coefficients(chunk) == S.frame_coefficients(std)).all(), f"frame {k} holds other coefficients than its POPPY_FRAME_JPEG frame"
        if Image is None:
            continue
        with Image.open(io.BytesIO(data[at:at + n])) as im:
            im.load()
            assert im.size == (w, h) and im.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
        with Image.open(io.BytesIO(std[4:].tobytes())) as ref, Image.open(io.BytesIO(data[at:at + n])) as im:
            assert (np.asarray(im) == np.asarray(ref)).all(), f"frame {k} decodes to other pixels than its POPPY_FRAME_JPEG frame"
