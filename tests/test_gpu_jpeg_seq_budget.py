"""GPU checks of the JPEG sequence budget (poppy_hip_set_jpeg_sequence_budget: the raster kernel per frame into the sequence store, k_jpeg_measure over segments x
frames and k_jpeg_pick in its sequence form once per search step, then k_jpeg_code and k_jpeg_pack per frame on the one picked quality's tables).  Every comparison
is == on bytes against the host statement, poppy_bgr_frames_to_jpeg_seq_budget_frames / poppy_bgr_frames_to_jpeg444_seq_budget_frames: of the same frames for the
stand-alone entry, of the BGR frames that a context with the setting off hands out for the same work for the frame path.  tests/test_host_jpeg_seq_budget.py pins
the host statement to a restatement."""
import numpy as np
import pytest

import jpeg_budget_util as B
import jpeg_seq_budget_util as SB
import jpeg_util as U
from poppy_amd import capi, synth
from palette_util import collect as _collect, inputs as _inputs, loaded as _loaded

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_UNSUPPORTED = -1, -4, -6
Q = capi.JPEG_QUALITY_DEFAULT
JPEG, JPEG444 = capi.FRAME_JPEG, capi.FRAME_JPEG444
FORMATS = [pytest.param(fmt, id=name) for fmt, name in zip(SB.SAMPLINGS, ("420", "444"))]
BUILT_TABLE_FORMATS = (capi.FRAME_JPEG_OPT, capi.FRAME_JPEG444_OPT, capi.FRAME_JPEG_SEQ, capi.FRAME_JPEG444_SEQ)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _host(frames, quality, budget, fmt=JPEG):
    return capi.bgr_frames_to_jpeg_seq_budget_frames(frames, quality, budget, fmt)


def _size_at(frames, quality, fmt=JPEG):
    """size(quality) of a sequence of BGR frames"""
    fixed = capi.bgr_to_jpeg444_frame if fmt == JPEG444 else capi.bgr_to_jpeg_frame
    return sum(fixed(f, quality).size - 4 for f in frames)


def _same(what, bgr_seqs, seq_seqs, budget, quality=Q, fmt=JPEG, small=lambda f: f):
    """every sequence of the budget run is the host statement of the BGR run's frames of that sequence (small: the writer's geometry of a BGR frame); the qualities"""
    assert len(bgr_seqs) == len(seq_seqs) and len(seq_seqs) > 0, f"{what}: {len(bgr_seqs)} BGR sequences, {len(seq_seqs)} coded ones"
    used = []
    for k, (b, j) in enumerate(zip(bgr_seqs, seq_seqs)):
        assert len(b) == len(j) and len(j) > 0 and all(f.ndim == 3 for f in b), f"{what}: sequence {k}: {len(b)} BGR frames, {len(j)} coded frames"
        want, q = _host([small(f) for f in b], quality, budget, fmt)
        SB.equal_seq(f"{what}: sequence {k} (quality {q})", j, want)
        assert sum(f.size - 4 for f in j) <= budget or q == 1, f"{what}: sequence {k} exceeds its budget at quality {q}"
        assert {capi.jpeg_frame_quality(f) for f in j} == {q}
        used.append(q)
    return used


def _half_of_the_first(seqs, quality, fmt):
    return _size_at(seqs[0], quality, fmt) // 2


def _both(what, run, budget=_half_of_the_first, quality=Q, fmt=JPEG, small=lambda f: f, prepare=lambda c: None, **settings):
    """run(ctx) -> a list of sequences (each what one call handed to its writer), on a BGR context and on a JPEG context under the sequence budget that
    budget(the BGR sequences in the writer's geometry, quality, fmt) gives"""
    c = capi.Context(0, **settings)
    try:
        bgr = run(c)
    finally:
        c.close()
    b = budget([[small(f) for f in s] for s in bgr], quality, fmt)
    c = capi.Context(0, **settings)
    try:
        c.set_frame_format(fmt)
        if quality != Q:
            c.set_jpeg_quality(quality)
        c.set_jpeg_sequence_budget(b)
        assert c.get_jpeg_sequence_budget() == b
        prepare(c)
        seq = run(c)
    finally:
        c.close()
    return bgr, seq, b, _same(what, bgr, seq, b, quality, fmt, small)


# ---- the kernels alone ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(SB.SEQUENCES))
def test_kernels_alone_on_every_sequence_budget_and_highest_quality(ctx, name, fmt):
    frames = SB.bgr(name)
    for qmax, b, want in SB.cases(name, fmt):                   # (want: the search on the summed table; the host statement equals the fixed frames at it: test_host_jpeg_seq_budget.py)
        got, used = ctx.bgr_frames_to_jpeg_seq_budget_frames(frames, qmax, b, fmt)
        assert used == want, f"{name} qmax {qmax}, budget {b}: quality {used}, the host statement picks {want}"
        SB.equal_seq(f"{name} qmax {qmax}, budget {b}", got, SB.fixed(name, fmt, want))


@pytest.mark.parametrize("fmt", FORMATS)
def test_kernels_alone_on_padded_frames(ctx, fmt):
    name = "noise_5_136x24"
    b = int(SB.sizes(name, fmt)[37])
    want, used = _host(SB.bgr(name), 100, b, fmt)
    got, got_used = ctx.bgr_frames_to_jpeg_seq_budget_frames(SB.bgr(name), 100, b, fmt, row_pad=5, frame_pad=11)
    assert got_used == used
    SB.equal_seq("padded rows and frames", got, want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_kernels_alone_on_hundreds_of_segments_and_several_frames(ctx, fmt):
    """3 frames of 640 x 360, noise / ramp / texture: 115 segments a frame of 4:2:0 and 225 of 4:4:4, so the pick's strided sum runs over more than 256 lengths
    per quality and blockIdx.y > 0 meets blockIdx.x > 0; 333 x 211 beside it, whose last MCU column and row are clamped"""
    for w, h in ((640, 360), (333, 211)):
        frames = [B._noise(w, h, 21), B._dithered_ramp(w, h, 22), synth.textured_bgr(w, h, 23)]
        for qmax in (100, Q):
            full = _size_at(frames, qmax, fmt)
            for f in (0.75, 0.4):
                b = int(f * full)
                want, want_used = _host(frames, qmax, b, fmt)
                got, used = ctx.bgr_frames_to_jpeg_seq_budget_frames(frames, qmax, b, fmt)
                assert used == want_used and used < qmax, f"{w}x{h} qmax {qmax}, budget {b}: quality {used}, the host statement picks {want_used}"
                SB.equal_seq(f"{w}x{h} qmax {qmax}, budget {b}", got, want)
                assert sum(x.size - 4 for x in got) <= b


def test_kernels_alone_leave_the_contexts_own_settings(ctx):
    name = "flat_ramp_noise_64x48"
    b = int(SB.sizes(name, JPEG)[40])
    ctx.set_jpeg_sequence_budget((1 << 33) + 5)
    ctx.set_jpeg_quality(77)
    try:
        got, used = ctx.bgr_frames_to_jpeg_seq_budget_frames(SB.bgr(name), 100, b)
        assert used == SB.pick(SB.sizes(name, JPEG), 100, b)
        SB.equal_seq("with a sequence budget of the context's own", got, SB.fixed(name, JPEG, used))
        assert ctx.get_jpeg_sequence_budget() == (1 << 33) + 5 and ctx.get_jpeg_budget() == 0
        pl = B.planes("ramp_64x48", JPEG)
        SB.equal("the fixed-quality entry beside it", ctx.i420_to_jpeg_frame(pl, 64, 48, 55), B.frames("ramp_64x48", JPEG)[55])
    finally:
        ctx.set_jpeg_sequence_budget(0)
        ctx.set_jpeg_quality(Q)


def test_refusals_of_the_stand_alone_entry_keep_the_context(ctx):
    L = capi.lib()
    one = np.zeros((2, 2, 2, 3), np.uint8)
    room = np.full(2 * capi.frame_bytes(JPEG444, 2, 2), 0xA5, np.uint8)
    p, d = capi._p(one), capi._p(room)
    for call in (L.poppy_hip_bgr_frames_to_jpeg_seq_budget_frames, L.poppy_hip_bgr_frames_to_jpeg444_seq_budget_frames):
        assert call(ctx.h, p, 3 * 65536, 1 << 40, 1, 65536, 1, Q, 1000, d, None) == E_UNSUPPORTED      # (refused before a byte is read)
        assert call(ctx.h, p, 6, 12, 0, 2, 2, Q, 1000, d, None) == E_ARG and call(ctx.h, p, 6, 11, 2, 2, 2, Q, 1000, d, None) == E_ARG
        assert call(ctx.h, p, 5, 12, 2, 2, 2, Q, 1000, d, None) == E_ARG
        for q in (0, 101):
            assert call(ctx.h, p, 6, 12, 2, 2, 2, q, 1000, d, None) == E_ARG
        assert call(ctx.h, p, 6, 12, 2, 2, 2, Q, 0, d, None) == E_ARG
        assert call(ctx.h, None, 6, 12, 2, 2, 2, Q, 1000, d, None) == E_ARG and call(None, p, 6, 12, 2, 2, 2, Q, 1000, d, None) == E_ARG
    assert (room == 0xA5).all(), "a refusal wrote into dst"
    assert L.poppy_hip_set_jpeg_sequence_budget(None, 5) == E_ARG and L.poppy_hip_get_jpeg_sequence_budget(ctx.h, None) == E_ARG
    assert L.poppy_hip_pool_set_jpeg_sequence_budget(None, 5) == E_ARG
    assert ctx.get_jpeg_sequence_budget() == 0
    name = "noise_saturated_2"
    b = int(SB.sizes(name, JPEG)[37])
    got, used = ctx.bgr_frames_to_jpeg_seq_budget_frames(SB.bgr(name), 100, b)
    SB.equal_seq("after the refusals", got, SB.fixed(name, JPEG, SB.pick(SB.sizes(name, JPEG), 100, b)))


# ---- the frame path -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_sixty_chained_frames_at_one_quality_below_the_highest(fmt):
    """64 x 48, sixty chained frames, half the bytes they have at the highest quality: one quality below it, the frames the host statement's, their sum within the
    budget, and the writer first called after the last frame is rendered"""
    w, h = 64, 48
    shapes = [(k + 1) / 61 for k in range(60)]
    seen = []

    def run(c):
        before = sum(c.warp_counts())
        frames = []
        c.render_many(shapes, chain=True, write=lambda v: (frames.append(v.copy()), seen.append((c.frame_format, sum(c.warp_counts()) - before))))
        return [frames]
    _, seq, b, used = _both("60 chained frames", _loaded(w, h)(run), fmt=fmt)
    assert len(seq[0]) == 60 and 1 <= used[0] < Q, used
    assert sum(f.size - 4 for f in seq[0]) <= b
    assert [n for f, n in seen if f == fmt] == [60] * 60, "the writer was called before the last frame was rendered"


def test_phase_mode_twice_with_the_budget_and_then_the_quality_changed():
    w, h = 64, 48
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.2, 0.4, 0.6, 0.8]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        full = _size_at(bgr, Q)
        c.set_frame_format(JPEG)
        plain = _collect(c, c.render_many, shapes, chain=False)          # setting off: the bodies with the fixed-quality coder
        c.set_jpeg_sequence_budget(full * 3 // 4)
        first = _collect(c, c.render_many, shapes, chain=False)          # captures the bodies without a conversion
        c.set_jpeg_sequence_budget(full // 3)
        second = _collect(c, c.render_many, shapes, chain=False)         # ... which are replayed: a search that kept the old budget fails here
        c.set_jpeg_quality(35)
        third = _collect(c, c.render_many, shapes, chain=False)          # ... and one that kept the old highest quality here
        c.set_jpeg_sequence_budget(1 << 40)
        fourth = _collect(c, c.render_many, shapes, chain=False)         # everything fits: quality 35
        c.set_jpeg_sequence_budget(0)
        c.set_jpeg_quality(Q)
        off = _collect(c, c.render_many, shapes, chain=False)
        SB.equal_seq("setting off", plain, [capi.bgr_to_jpeg_frame(b, Q) for b in bgr])
        (u1,) = _same("budget 3/4", [bgr], [first], full * 3 // 4)
        (u2,) = _same("budget 1/3, captured bodies", [bgr], [second], full // 3)
        (u3,) = _same("quality 35 under the budget, captured bodies", [bgr], [third], full // 3, 35)
        (u4,) = _same("a budget above 2^32 that everything fits", [bgr], [fourth], 1 << 40, 35)
        assert u2 < u1 < Q and u3 <= 35 and u4 == 35, (u1, u2, u3, u4)
        SB.equal_seq("setting off again", off, [capi.bgr_to_jpeg_frame(b, Q) for b in bgr])
    finally:
        c.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_copies_count_among_the_sequence(fmt):
    w, h = 128, 96
    a, b = synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6, 3)

    def resident(c):
        c.pair_begin(a, b)
        return [c.morph_frames(0.0), c.morph_frames(1.0), _collect(c, c.render_phases, [0.0, 0.3, 0.5, 1.0, 0.0, 0.7, 1.0])]
    _, _, _, used = _both("phase 0 / 1 and t 0 / 1 on a resident pair", resident, fmt=fmt, number_of_frames=3)
    assert all(q < Q for q in used), used


def test_morph_list_of_three_is_one_sequence_and_pick_per_pair():
    """each pair against the host statement of its own four frames under the whole budget: a search over the list's eight frames would pick a lower quality"""
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2 and len(frames) == 2
        return frames
    budget = lambda seqs, quality, fmt: min(_size_at(s, quality, fmt) for s in seqs) * 3 // 5
    _, seq, b, used = _both("morph_list of 3", run, budget=budget, number_of_frames=4)
    assert all(1 < q < Q for q in used), used
    assert sum(f.size - 4 for s in seq for f in s) > b, "the budget is each pair's, not the list's"


def test_pool_of_two_contexts():
    w, h = 256, 192
    pairs = [(synth.gen(w, h, 77, 0, 0), synth.gen(w, h, 77, 6 + k, 3)) for k in range(3)]
    results = []
    budget = 0
    for fmt in (capi.FRAME_BGR, JPEG):
        p = capi.Pool([0], contexts_per_device=2, number_of_frames=4)
        try:
            got = {}
            p.set_frame_format(fmt)
            if fmt == JPEG:
                budget = _size_at([results[0][k] for k in sorted(results[0]) if k[:2] == (0, 0)], 60) // 2
                p.set_jpeg_quality(60)
                p.set_jpeg_sequence_budget(budget)
            for b in range(2):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            if fmt == JPEG:
                with pytest.raises(capi.PoppyError, match=str(E_STATE)):      # as the pool's other setters: not with work submitted
                    p.set_jpeg_sequence_budget(budget + 1)
            p.wait()
            results.append(got)
        finally:
            p.close()
    bgr, seq = results
    assert sorted(bgr) == sorted(seq) and len(seq) == 2 * len(pairs) * 4
    calls = sorted({k[:2] for k in bgr})
    used = _same("pool batches", [[bgr[c + (j,)] for j in range(4)] for c in calls], [[seq[c + (j,)] for j in range(4)] for c in calls], budget, 60)
    assert min(used) < 60, used


def test_frame_scale_and_frame_size():
    w, h = 128, 96
    run = _loaded(w, h)(lambda c: [_collect(c, c.render_many, [0.25, 0.5, 0.75], chain=True), _collect(c, c.render_many, [0.3, 0.6], chain=False),
                                   _collect(c, c.render_phases, [0.0, 0.4, 1.0])])
    _, _, _, used = _both("scale 2", run, small=lambda f: capi.bgr_downscale(f, 2), prepare=lambda c: c.set_frame_scale(2))
    assert used[0] < Q, "the budget holds on the scaled frames"
    _both("size 50 x 35, 4:4:4", run, small=lambda f: capi.bgr_resize_area(f, 50, 35), prepare=lambda c: c.set_frame_size(50, 35), fmt=JPEG444)


def test_mjpeg_sink_takes_the_frames_as_they_are(tmp_path):
    w, h = 64, 48
    shapes = [0.2, 0.5, 0.8]
    _, seq, b, used = _both("sequence for the sink", _loaded(w, h)(lambda c: [_collect(c, c.render_many, shapes, chain=True)]))
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
        assert U.walk_frame(chunk)["size"] == (w, h) and capi.jpeg_frame_quality(chunk) == used[0]
    assert sum(n for _, _, n, _, _ in movi[4]) <= b, "the chunks' bytes are the budget's bytes"


def test_setting_off_is_a_context_that_never_heard_of_it():
    """frames, timing marks and chain counts of a context whose setting went on and off again, and of one whose setting was set to 0, against a context that was
    never told; and the marks with the setting on"""
    w, h = 64, 48
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]

    def run(c, touch):
        c.set_frame_format(JPEG)
        touch(c)
        c.pair_load(c1, c2, g, p1, p2)
        c.set_timing(1)
        c.timing_summary()
        frames = _collect(c, c.render_many, shapes, chain=True) + _collect(c, c.render_many, shapes, chain=False)
        return frames, {name: n for name, _, n in c.timing_summary()}, c.chain_counts()
    out = []
    for touch in (lambda c: None, lambda c: c.set_jpeg_sequence_budget(0), lambda c: (c.set_jpeg_sequence_budget(5000), c.set_jpeg_sequence_budget(0))):
        c = capi.Context(0)
        try:
            out.append(run(c, touch))
        finally:
            c.close()
    for k in (1, 2):
        SB.equal_seq(f"context {k}", out[k][0], out[0][0])
        assert out[k][1] == out[0][1] and out[k][2] == out[0][2], (out[k][1:], out[0][1:])
    assert "jpeg_measure" not in out[0][1] and out[0][1].get("jpeg_code") == 2 * len(shapes)


def test_a_context_that_was_never_told_hands_out_todays_frames_and_marks():
    """no new entry point is called here: the fixed-quality frames of the BGR frames, two coding launches a frame and no search, whatever the library knows of budgets"""
    w, h = 64, 48
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=True)
        c.reset()
        c.set_frame_format(JPEG)
        c.set_timing(1)
        c.timing_summary()
        frames = _collect(c, c.render_many, shapes, chain=True)
        marks = {name: n for name, _, n in c.timing_summary()}
        SB.equal_seq("never told", frames, [capi.bgr_to_jpeg_frame(b, Q) for b in bgr])
        assert (marks.get("frame_format"), marks.get("jpeg_code"), marks.get("jpeg_pack")) == (3, 3, 3) and "jpeg_measure" not in marks and "jpeg_pick" not in marks, marks
    finally:
        c.close()


def test_the_marks_with_the_setting_on():
    w, h = 64, 48
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    c = capi.Context(0)
    try:
        c.set_frame_format(JPEG)
        c.set_jpeg_sequence_budget(5000)
        c.pair_load(c1, c2, g, p1, p2)
        c.set_timing(1)
        c.timing_summary()
        on = _collect(c, c.render_many, shapes, chain=True)
        marks = {name: n for name, _, n in c.timing_summary()}
        assert (marks.get("frame_format"), marks.get("jpeg_code"), marks.get("jpeg_pack")) == (3, 3, 3), marks
        assert marks.get("jpeg_measure", 0) > 0 and marks.get("jpeg_measure") == marks.get("jpeg_pick"), marks      # one launch per step, not per frame
        assert marks["jpeg_measure"] <= 1 + int(np.ceil(np.log2(Q))) and "jpeg_count" not in marks and "jpeg_tables" not in marks, marks
        assert len(on) == len(shapes) and len({capi.jpeg_frame_quality(f) for f in on}) == 1
    finally:
        c.close()


def test_refusals_in_both_orders_keep_the_earlier_setting():
    w, h = 64, 48
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.3, 0.7]
    L = capi.lib()
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        budget = _size_at(bgr, Q) // 2
        c.set_frame_format(JPEG)
        c.set_jpeg_sequence_budget(budget)
        for fmt in BUILT_TABLE_FORMATS:                             # the sequence budget first, the format second: the format stays JPEG, the budget stays
            assert L.poppy_hip_set_frame_format(c.h, fmt) == E_UNSUPPORTED
            assert c.get_jpeg_sequence_budget() == budget and c.frame_format == JPEG
        assert L.poppy_hip_set_jpeg_budget(c.h, 4000) == E_UNSUPPORTED      # ... and the per-frame budget second
        assert c.get_jpeg_budget() == 0 and c.get_jpeg_sequence_budget() == budget
        _same("after the refusals", [bgr], [_collect(c, c.render_many, shapes, chain=False)], budget)
        c.set_jpeg_sequence_budget(0)
        c.set_jpeg_budget(4000)                                     # the per-frame budget first, the sequence budget second
        assert L.poppy_hip_set_jpeg_sequence_budget(c.h, budget) == E_UNSUPPORTED
        assert c.get_jpeg_sequence_budget() == 0 and c.get_jpeg_budget() == 4000
        for b, j in zip(bgr, _collect(c, c.render_many, shapes, chain=False)):
            SB.equal("the per-frame budget after the refusal", j, capi.bgr_to_jpeg_budget_frame(b, Q, 4000)[0])
        c.set_jpeg_budget(0)
        for fmt in BUILT_TABLE_FORMATS:                             # the format first, the sequence budget second: the budget stays off, the format stays
            c.set_frame_format(fmt)
            assert L.poppy_hip_set_jpeg_sequence_budget(c.h, budget) == E_UNSUPPORTED
            assert c.get_jpeg_sequence_budget() == 0
            frames = _collect(c, c.render_many, shapes, chain=False)
            assert len(frames) == len(shapes) and all(capi.jpeg_frame_quality(f) == Q for f in frames)
        c.set_frame_format(capi.FRAME_BGR)
        c.set_jpeg_sequence_budget(budget)                          # a format that ignores the setting takes it
        for k, (b, j) in enumerate(zip(bgr, _collect(c, c.render_many, shapes, chain=False))):
            assert np.array_equal(b, j), f"BGR frame {k} under a sequence budget"
        c.set_frame_format(capi.FRAME_I420)
        for b, j in zip(bgr, _collect(c, c.render_many, shapes, chain=False)):
            assert np.array_equal(np.asarray(j).ravel(), np.asarray(capi.bgr_to_i420(b)).ravel()), "an I420 frame under a sequence budget"
        c.set_frame_format(JPEG444)
        _same("JPEG444 after all of it", [bgr], [_collect(c, c.render_many, shapes, chain=False)], budget, fmt=JPEG444)
    finally:
        c.close()
