"""GPU checks of the PNG hand-off on one ninth table per sequence (POPPY_FRAME_PNG_SEQ: k_png_filter and k_png_seq_count per frame into the sequence's sums,
k_png_seq_table once on them, k_png_seq_cost, k_png_scan, k_png_seq_pack, k_png_crc and k_png_finish per frame on what it built).  Every comparison is == on bytes
against the host statement, poppy_bgr_frames_to_png_seq_frames: of the same frames for the stand-alone entry, of the BGR frames that a BGR context hands out for
the same work for the frame path; and every frame of the frame path, through zlib's decoder and the filters undone, == the BGR frame.  tests/test_host_png_seq.py
pins the host statement to a restatement."""
import numpy as np
import pytest

import png_seq_util as S
from poppy_amd import capi, synth
from palette_util import collect as _collect, inputs as _inputs, loaded as _loaded

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_NOMATCH, E_UNSUPPORTED = -1, -4, -5, -6
SEQ = capi.FRAME_PNG_SEQ
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


def _direct(ctx, frames, what, **pads):
    got = ctx.bgr_frames_to_png_seq_frames(np.stack(frames), **pads)
    _equal_seq(what, got, S.host_frames(frames))
    return got


def _same(what, bgr_seqs, seq_seqs, small=lambda f: f):
    """every sequence of the SEQ run is the host statement of the BGR run's frames of that sequence (small: the writer's geometry of a BGR frame), and decodes to them"""
    assert len(bgr_seqs) == len(seq_seqs) and len(seq_seqs) > 0, f"{what}: {len(bgr_seqs)} BGR sequences, {len(seq_seqs)} coded ones"
    for k, (b, j) in enumerate(zip(bgr_seqs, seq_seqs)):
        assert len(b) == len(j) and len(j) > 0 and all(f.ndim == 3 for f in b), f"{what}: sequence {k}: {len(b)} BGR frames, {len(j)} coded frames"
        frames = [small(f) for f in b]
        _equal_seq(f"{what}: sequence {k}", j, S.host_frames(frames))
        h, w = frames[0].shape[:2]
        for i, (coded, bgr) in enumerate(zip(j, frames)):
            assert S.decodes_to(coded, bgr), f"{what}: sequence {k}, frame {i} does not decode to the BGR frame"
        if k == 0:                                              # ... and the first frame by the decoder's own walk, byte by byte
            assert (S.decoded(j[0], w, h) == frames[0]).all(), f"{what}: sequence {k}, frame 0 does not decode to the BGR frame"


def _both(what, run, small=lambda f: f, prepare=lambda c: None, **settings):
    """run(ctx) -> a list of sequences (each what one call handed to its writer), on a BGR and on a SEQ context"""
    out = []
    for f in (capi.FRAME_BGR, SEQ):
        c = capi.Context(0, **settings)
        try:
            c.set_frame_format(f)
            if f == SEQ:
                prepare(c)
            out.append(run(c))
        finally:
            c.close()
    _same(what, out[0], out[1], small)
    return out


# ---- the stand-alone entry and the build alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.sequences()))
def test_stand_alone_entry_on_the_host_tests_sequences(ctx, name):
    """No launch of the new kernels is capped or grid-strided (a workgroup per segment; the build is one wave), so the case with the most segments per frame is the
    set's own "all 286 symbols" (three segments a frame); test_a_frame_of_many_segments goes further."""
    frames = S.sequences()[name]
    got = _direct(ctx, frames, name)
    for bgr, f in zip(frames, got):
        assert f.size <= capi.bgr_to_png_runs_frame(bgr).size
    if name == "one frame, one segment":
        _equal(name + ": against the context's PNG_OPT frame", got[0], ctx.bgr_to_png_opt_frame(frames[0]))
    if name == "21x129 a second segment of 64 bytes":
        _direct(ctx, frames, name + " padded", row_pad=5, frame_pad=11)


def test_stand_alone_calls_are_independent(ctx):
    """the same call twice on one context with other sequences in between: a call's sums begin at zero and are not cleared between its frames"""
    a, b = S.sequences()["disjoint alphabets"], S.sequences()["40x137 noise and flat"]
    for k, frames in enumerate((a, b, a, b[::-1], a[:1], [a[0]] * 3)):
        _direct(ctx, frames, f"call {k}")


def test_a_frame_of_many_segments(ctx):
    """512 x 300 textured, two frames: 57 segments each, the last one short — 114 workgroups add into the 286 sums"""
    frames = [synth.textured_bgr(512, 300, 9 + k) for k in range(2)]
    _direct(ctx, frames, "textured 512x300 x 2")


@pytest.mark.parametrize("name", list(S.table_families()))
def test_table_build_alone_on_the_count_families(ctx, name):
    """k_png_seq_table at counts no segment and no test frame can produce: sums up to 2^32 - 1, trees of depth 39"""
    counts = S.table_families()[name]
    lengths, header = ctx.png_seq_table(counts)
    want_lengths, want_header = capi.png_seq_table(counts)
    assert lengths.tolist() == want_lengths.tolist() and header.tolist() == want_header.tolist()


def test_table_build_refusals(ctx):
    L = capi.lib()
    counts, lengths = np.ones(286, np.uint32), np.zeros(286, np.uint8)
    assert L.poppy_hip_png_seq_table(ctx.h, capi._p(counts), capi._p(lengths), None, None) == 0
    assert L.poppy_hip_png_seq_table(ctx.h, None, capi._p(lengths), None, None) == E_ARG
    counts[256] = 0
    assert L.poppy_hip_png_seq_table(ctx.h, capi._p(counts), capi._p(lengths), None, None) == E_ARG
    big = np.zeros(286, np.uint32); big[0] = 1 << 31; big[256] = 1 << 31
    assert L.poppy_hip_png_seq_table(ctx.h, capi._p(big), capi._p(lengths), None, None) == E_ARG


# ---- the frame path -----------------------------------------------------------------------------------------------------------------------------------------
def test_chained_sequence_and_phase_mode_twice():
    w, h = 256, 192

    def seqs(c):
        out = [_collect(c, c.render_many, [(k + 1) / 9 for k in range(8)], chain=True)]
        c.reset()
        for _ in range(2):                                      # the second round replays the captured bodies
            out.append(_collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=False))
        return out
    bgr, seq = _both("chained, then phase mode twice", _loaded(w, h)(seqs))
    for b, j in zip(bgr, seq):
        for f, coded in zip(b, j):
            assert coded.size <= capi.bgr_to_png_runs_frame(f).size


def test_long_runs_reuse_every_ring_buffer_and_frames_differ_in_size():
    """The textured-against-smooth pair, shapes alternating between the two ends: 24 phase-mode frames and 17 chained ones, each more than twice the ring, so that
    every ring buffer and its pinned word carry at least two frames of one sequence; the frames of the two ends differ in size.  The same sequence again afterwards:
    the sums were zero in front of it."""
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
    assert max(sizes) > 1.05 * min(sizes), f"the frames of the two ends are alike: {min(sizes)} .. {max(sizes)} bytes"
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


def test_copies_and_phase_0_and_1():
    w, h = 128, 96
    a, b = synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6, 3)

    def resident(c):
        c.pair_begin(a, b)
        return [c.morph_frames(0.0), c.morph_frames(1.0), _collect(c, c.render_phases, [0.0, 0.3, 0.5, 1.0, 0.0, 0.7, 1.0])]
    _both("phase 0 / 1 and t 0 / 1 on a resident pair", resident, number_of_frames=3)


def test_flat_pair_reaches_the_nomatch_frames():
    a = np.full((150, 200, 3), (9, 99, 199), np.uint8)
    b = np.full_like(a, 77)

    def run(c):
        rc, frames, _ = c.morph(a, b, phase=-1.0)
        assert rc == E_NOMATCH
        return [frames]
    _both("flat pair", run, number_of_frames=3)


def test_morph_list_of_three_is_one_sequence_per_pair():
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2 and len(frames) == 2
        return frames
    _both("morph_list of 3", run, number_of_frames=4)


def test_pool_of_two_contexts_queued_and_the_format_while_work_is_queued():
    w, h = 256, 192
    pairs = [(synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6 + k, 3)) for k in range(3)]
    results = []
    for fmt in (capi.FRAME_BGR, SEQ):
        p = capi.Pool([0], contexts_per_device=2, number_of_frames=4)
        try:
            got = {}
            p.set_frame_format(fmt)
            for b in range(2):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            with pytest.raises(capi.PoppyError, match=str(E_STATE)):      # as JPEG_SEQ answers it: not while sequences are open or queued
                p.set_frame_format(capi.FRAME_BGR if fmt == SEQ else SEQ)
            p.wait()
            p.set_frame_format(fmt)                                 # waited for: allowed again
            results.append(got)
        finally:
            p.close()
    bgr, seq = results
    assert sorted(bgr) == sorted(seq) and len(seq) == 2 * len(pairs) * 4
    calls = sorted({k[:2] for k in bgr})
    _same("pool batches", [[bgr[c + (j,)] for j in range(4)] for c in calls], [[seq[c + (j,)] for j in range(4)] for c in calls])


def test_frame_scale_and_frame_size():
    """the table is taken over the scaled frames"""
    w, h = 256, 192
    run = _loaded(w, h)(lambda c: [_collect(c, c.render_many, [0.25, 0.5, 0.75], chain=True), _collect(c, c.render_many, [0.3, 0.6], chain=False),
                                   _collect(c, c.render_phases, [0.0, 0.4, 1.0])])
    _both("scale 2", run, small=lambda f: capi.bgr_downscale(f, 2), prepare=lambda c: c.set_frame_scale(2))
    _both("size 100 x 70", run, small=lambda f: capi.bgr_resize_area(f, 100, 70), prepare=lambda c: c.set_frame_size(100, 70))


def test_switching_formats_on_one_context():
    """PNG_SEQ -> PNG -> PNG_RUNS -> PNG_OPT -> JPEG_SEQ -> BGR -> PNG_SEQ on one context with a resident pair, each against its host statement of a BGR context's
    frames: the sequence's store, sums and table and the slots' PNG scratch do not disturb each other"""
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
    per_frame = {capi.FRAME_PNG: capi.bgr_to_png_frame, capi.FRAME_PNG_RUNS: capi.bgr_to_png_runs_frame, capi.FRAME_PNG_OPT: capi.bgr_to_png_opt_frame}
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        for k, fmt in enumerate((SEQ, capi.FRAME_PNG, capi.FRAME_PNG_RUNS, capi.FRAME_PNG_OPT, capi.FRAME_JPEG_SEQ, capi.FRAME_BGR, SEQ)):
            c.set_frame_format(fmt)
            got = seqs(c)
            if fmt == SEQ:
                _same(f"step {k}", bgr, got)
            for b, j in zip(bgr, got):
                if fmt in per_frame:
                    _equal_seq(f"step {k}", j, [per_frame[fmt](f) for f in b])
                elif fmt == capi.FRAME_JPEG_SEQ:
                    _equal_seq(f"step {k}: JPEG_SEQ", j, capi.bgr_frames_to_jpeg_seq_frames(np.stack(b), capi.JPEG_QUALITY_DEFAULT, fmt))
                elif fmt == capi.FRAME_BGR:
                    assert all((x == y).all() for x, y in zip(b, j))
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
        marks = ("png_filter", "png_seq_count", "png_seq_table", "png_seq_cost", "png_scan", "png_seq_pack", "png_crc", "png_finish")
        assert tuple(names.get(m) for m in marks) == (3, 3, 1, 3, 3, 3, 3, 3), names
        assert "png_cost" not in names and "png_pack" not in names and "jpeg_count" not in names
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
        # a sequence over the bound: refused on the count alone, nothing rendered, nothing written
        n = sh * (1 + 3 * sw)
        most = S.MAX_SYMBOLS // (n + -(-n // S.SEGMENT))
        assert S.seq_fits(most, sw, sh) and not S.seq_fits(most + 1, sw, sh)
        before = sum(c.warp_counts())
        calls = []
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.render_phases(np.full(most + 1, 0.5), write=lambda v: calls.append(1))
        assert sum(c.warp_counts()) == before and not calls, "frames were rendered or written before the refusal"
        one = np.zeros((2, 2, 3), np.uint8)
        room = np.zeros(capi.frame_bytes(SEQ, 2, 2), np.uint8)
        call = L.poppy_hip_bgr_frames_to_png_seq_frames
        assert call(c.h, capi._p(one), 6, 12, (1 << 31) - 1, 2, 2, capi._p(room)) == E_UNSUPPORTED
        assert call(c.h, capi._p(one), 3 * 26000, 3 * 26000 * 26000, 1, 26000, 26000, capi._p(room)) == E_UNSUPPORTED      # (refused before a byte is read)
        assert call(c.h, capi._p(one), 6, 12, 0, 2, 2, capi._p(room)) == E_ARG and call(c.h, capi._p(one), 6, 11, 1, 2, 2, capi._p(room)) == E_ARG
        assert call(c.h, capi._p(one), 5, 12, 1, 2, 2, capi._p(room)) == E_ARG and call(c.h, None, 6, 12, 1, 2, 2, capi._p(room)) == E_ARG
        for fmt in (131071, 131073):
            assert L.poppy_hip_set_frame_format(c.h, fmt) == E_ARG
        # the stand-alone entry works on buffers and sums of its own: the resident pair and the context's sequence are as they were
        _direct(c, S.sequences()["40x137 noise and flat"], "stand-alone entry on a context with a resident pair")
        c.reset()
        _equal_seq("after the refusals", _collect(c, c.render_many, [0.3, 0.7], chain=True), want)
    finally:
        c.close()


def test_stand_alone_call_between_two_renders_of_one_context():
    """a render, a stand-alone call, the same render again: the resident pair and the context's own sequence (store, sums, table) are left alone"""
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    c = capi.Context(0)
    try:
        c.set_frame_format(SEQ)
        c.pair_load(c1, c2, g, p1, p2)
        first = _collect(c, c.render_many, [0.25, 0.5, 0.75], chain=False)
        _direct(c, S.sequences()["disjoint alphabets"], "between two renders")
        _equal_seq("the render again", _collect(c, c.render_many, [0.25, 0.5, 0.75], chain=False), first)
    finally:
        c.close()


def test_png_sink_files_from_a_gpu_sequence_decode(tmp_path):
    w, h = 256, 192
    shapes = [0.2, 0.5, 0.8]
    bgr, seq = _both("sequence for the sink", _loaded(w, h)(lambda c: [_collect(c, c.render_many, shapes, chain=True)]))
    frames = seq[0]
    L = capi.lib()
    s = L.poppy_sink_open(str(tmp_path / "g_%03d.png").encode(), capi.SINK_PNG, w, h, 25, 1)
    assert s
    for f in frames:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(frames)
    for k, f in enumerate(frames):
        data = (tmp_path / f"g_{k:03d}.png").read_bytes()
        assert data == f[4:].tobytes()
        assert (S.decoded(np.frombuffer(len(f).to_bytes(4, "little") + data, np.uint8), w, h) == bgr[0][k]).all(), f"file {k} does not decode to its frame"
