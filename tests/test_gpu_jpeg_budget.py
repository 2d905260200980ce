"""GPU checks of the JPEG byte budget (poppy_hip_set_jpeg_budget: k_jpeg_measure, k_jpeg_pick, then k_jpeg_code and k_jpeg_pack on the picked quality's tables).
Every comparison is == on bytes against the host statement: poppy_i420_to_jpeg_budget_frame / poppy_i444_to_jpeg_budget_frame for the kernels alone,
poppy_bgr_to_jpeg_budget_frame / poppy_bgr_to_jpeg444_budget_frame of the BGR frame that a BGR context hands out for the same work for the frame path.  The host
statements are pinned in tests/test_host_jpeg_budget.py."""
import numpy as np
import pytest

import golden_util as G
import jpeg_budget_util as B
from poppy_amd import capi, synth
from palette_util import collect as _collect, inputs as _inputs, loaded as _loaded

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_UNSUPPORTED = -1, -4, -6
Q = capi.JPEG_QUALITY_DEFAULT
JPEG, JPEG444 = capi.FRAME_JPEG, capi.FRAME_JPEG444
FORMATS = [pytest.param(fmt, id=name) for fmt, name in zip(B.SAMPLINGS, ("420", "444"))]
BUILT_TABLE_FORMATS = (capi.FRAME_JPEG_OPT, capi.FRAME_JPEG444_OPT, capi.FRAME_JPEG_SEQ, capi.FRAME_JPEG444_SEQ)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _equal(what, got, want):
    assert got.ndim == 1 and got.size == want.size, f"{what}: {got.size} bytes, the host statement gives {want.size}"
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{what}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


def _fixed(bgr, quality, fmt):
    return (capi.bgr_to_jpeg444_frame if fmt == JPEG444 else capi.bgr_to_jpeg_frame)(bgr, quality)


def _fraction(f):
    """a budget from the BGR run's frames: that fraction of their median file size at the highest quality"""
    return lambda frames, quality, fmt: int(f * np.median([_fixed(b, quality, fmt).size - 4 for b in frames]))


def _same(what, bgr_frames, jpeg_frames, budget, quality=Q, fmt=JPEG, small=lambda f: f):
    """the JPEG frames are the host budget statement of the BGR frames (small: the writer's geometry of a BGR frame); returns the qualities"""
    assert len(bgr_frames) == len(jpeg_frames) and len(jpeg_frames) > 0, f"{what}: {len(bgr_frames)} BGR frames, {len(jpeg_frames)} JPEG frames"
    used = []
    for k, (b, j) in enumerate(zip(bgr_frames, jpeg_frames)):
        assert b.ndim == 3, f"{what}: frame {k} of the BGR run has shape {b.shape}"
        want, q = capi.bgr_to_jpeg_budget_frame(small(b), quality, budget, fmt)
        _equal(f"{what}: frame {k} (quality {q})", j, want)
        used.append(q)
    return used


def _both(what, run, budget=_fraction(0.5), quality=Q, fmt=JPEG, small=lambda f: f, prepare=lambda c: None, **settings):
    """run(ctx) -> frames, on a BGR context and on a JPEG context under the budget that budget(BGR frames in the writer's geometry, quality, fmt) gives"""
    c = capi.Context(0, **settings)
    try:
        bgr = run(c)
    finally:
        c.close()
    b = budget([small(f) for f in bgr], quality, fmt)
    c = capi.Context(0, **settings)
    try:
        c.set_frame_format(fmt)
        if quality != Q:
            c.set_jpeg_quality(quality)
        c.set_jpeg_budget(b)
        assert c.get_jpeg_budget() == b
        prepare(c)
        jpeg = run(c)
    finally:
        c.close()
    return bgr, jpeg, b, _same(what, bgr, jpeg, b, quality, fmt, small)


# ---- the kernels alone ----------------------------------------------------------------------------------------------------------------------------------------
def _alone(c, fmt):
    return (c.i444_to_jpeg_budget_frame, capi.i444_to_jpeg_budget_frame) if fmt == JPEG444 else (c.i420_to_jpeg_budget_frame, capi.i420_to_jpeg_budget_frame)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(B.CONTENTS))
def test_kernels_alone_on_every_content_budget_and_highest_quality(ctx, name, fmt):
    _, w, h, _ = B.CONTENTS[name]
    pl, fixed = B.planes(name, fmt), B.frames(name, fmt)
    device, _ = _alone(ctx, fmt)
    for qmax, b, want in B.cases(name, fmt):                    # (want: the search on the content's table; the host statement equals fixed[want]: test_host_jpeg_budget.py)
        got, used = device(pl, w, h, qmax, b)
        assert used == want, f"{name} qmax {qmax}, budget {b}: quality {used}, the host statement picks {want}"
        _equal(f"{name} qmax {qmax}, budget {b}", got, fixed[want])


@pytest.mark.parametrize("fmt", FORMATS)
def test_kernels_alone_on_hundreds_of_segments(ctx, fmt):
    """640 x 360: 115 segments of 4:2:0 and k_jpeg_pick's sums over them; 333 x 211 beside it, whose last MCU column and row are clamped"""
    device, host = _alone(ctx, fmt)
    for w, h, seed in ((640, 360, 3), (333, 211, 4)):
        bgr = synth.textured_bgr(w, h, seed)
        pl = np.ascontiguousarray((capi.bgr_to_i444 if fmt == JPEG444 else capi.bgr_to_i420)(bgr), np.uint8).ravel()
        for qmax in (100, Q):
            full = B.fixed_frame(pl, w, h, fmt, qmax).size - 4
            for f in (0.75, 0.5, 0.25):
                b = int(f * full)
                want, want_used = host(pl, w, h, qmax, b)
                got, used = device(pl, w, h, qmax, b)
                assert used == want_used and used < qmax, f"{w}x{h} qmax {qmax}, budget {b}: quality {used}, the host statement picks {want_used}"
                _equal(f"{w}x{h} qmax {qmax}, budget {b}", got, want)


def test_kernels_alone_leave_the_contexts_own_budget_and_quality(ctx):
    pl = B.planes("ramp_64x48", JPEG)
    b = int(B.sizes("ramp_64x48", JPEG)[40])
    ctx.set_jpeg_budget(123456)
    ctx.set_jpeg_quality(77)
    try:
        got, used = ctx.i420_to_jpeg_budget_frame(pl, 64, 48, 100, b)
        assert used == B.pick(B.sizes("ramp_64x48", JPEG), 100, b)
        _equal("with a budget of the context's own", got, B.frames("ramp_64x48", JPEG)[used])
        assert ctx.get_jpeg_budget() == 123456
        _equal("the fixed-quality entry beside it", ctx.i420_to_jpeg_frame(pl, 64, 48, 55), B.frames("ramp_64x48", JPEG)[55])
    finally:
        ctx.set_jpeg_budget(0)
        ctx.set_jpeg_quality(Q)


def test_refusals_keep_the_context(ctx):
    one = np.zeros(16, np.uint8)
    p = capi._p(one)
    L = capi.lib()
    for call in (L.poppy_hip_i420_to_jpeg_budget_frame, L.poppy_hip_i444_to_jpeg_budget_frame):
        for w, h in ((65536, 1), (65535, 65535)):
            assert call(ctx.h, p, w, h, Q, 1000, p, None) == E_UNSUPPORTED
        for q in (0, 101):
            assert call(ctx.h, p, 2, 2, q, 1000, p, None) == E_ARG
        for b in (0, 1 << 32):
            assert call(ctx.h, p, 2, 2, Q, b, p, None) == E_ARG
        assert call(ctx.h, None, 2, 2, Q, 1000, p, None) == E_ARG and call(None, p, 2, 2, Q, 1000, p, None) == E_ARG
    assert L.poppy_hip_set_jpeg_budget(ctx.h, 1 << 32) == E_ARG and L.poppy_hip_set_jpeg_budget(None, 5) == E_ARG
    assert L.poppy_hip_get_jpeg_budget(ctx.h, None) == E_ARG
    assert ctx.get_jpeg_budget() == 0
    pl = B.planes("noise_17x9", JPEG)
    b = int(B.sizes("noise_17x9", JPEG)[37])
    got, used = ctx.i420_to_jpeg_budget_frame(pl, 17, 9, 100, b)
    _equal("after the refusals", got, B.frames("noise_17x9", JPEG)[B.pick(B.sizes("noise_17x9", JPEG), 100, b)])


# ---- the frame path -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_sixty_chained_frames_all_below_the_highest_quality(fmt):
    """the budget is one byte less than the smallest frame at the highest quality: no frame may keep it"""
    w, h = 256, 192
    shapes = [(k + 1) / 61 for k in range(60)]
    smallest = lambda frames, quality, f: min(_fixed(b, quality, f).size - 4 for b in frames) - 1
    _, jpeg, b, used = _both("60 chained frames", _loaded(w, h)(lambda c: _collect(c, c.render_many, shapes, chain=True)), budget=smallest, fmt=fmt)
    assert all(1 <= q < Q for q in used), used
    assert all(f.size - 4 <= b for f in jpeg)
    assert [capi.jpeg_frame_quality(f) for f in jpeg] == used


def test_phase_mode_twice_with_the_budget_and_then_the_quality_changed():
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.2, 0.4, 0.6, 0.8]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        full = int(np.median([capi.bgr_to_jpeg_frame(b, Q).size - 4 for b in bgr]))
        c.set_frame_format(JPEG)
        plain = _collect(c, c.render_many, shapes, chain=False)          # budget off: the bodies of the fixed-quality coder
        c.set_jpeg_budget(full * 3 // 4)
        first = _collect(c, c.render_many, shapes, chain=False)          # captures the bodies with the search in them
        c.set_jpeg_budget(full // 3)
        second = _collect(c, c.render_many, shapes, chain=False)         # ... which are replayed: a body that kept the old budget fails here
        c.set_jpeg_quality(35)
        third = _collect(c, c.render_many, shapes, chain=False)          # ... and one that kept the old highest quality here
        c.set_jpeg_budget(1 << 30)
        fourth = _collect(c, c.render_many, shapes, chain=False)         # everything fits: quality 35
        c.set_jpeg_budget(0)
        c.set_jpeg_quality(Q)
        off = _collect(c, c.render_many, shapes, chain=False)
        for k, (b, j) in enumerate(zip(bgr, plain)):
            _equal(f"budget off, frame {k}", j, capi.bgr_to_jpeg_frame(b, Q))
        u1 = _same("budget 3/4", bgr, first, full * 3 // 4)
        u2 = _same("budget 1/3, captured bodies", bgr, second, full // 3)
        u3 = _same("quality 35 under the budget, captured bodies", bgr, third, full // 3, 35)
        u4 = _same("a budget that everything fits", bgr, fourth, 1 << 30, 35)
        assert max(u2) < min(u1) < Q and max(u3) <= 35 and u4 == [35] * len(shapes), (u1, u2, u3, u4)
        for k, (b, j) in enumerate(zip(bgr, off)):
            _equal(f"budget off again, frame {k}", j, capi.bgr_to_jpeg_frame(b, Q))
    finally:
        c.close()


def test_a_captured_body_does_not_outlive_a_budget_switched_under_another_format():
    """phase mode: the bodies are captured under JPEG, the format goes to BGR (no frame rendered, so the slots keep their bodies), the budget is switched there,
    and the format comes back to JPEG: the next frames need the other launches.  Both orders, each == the host statement."""
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.2, 0.4, 0.6, 0.8]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        budget = _fraction(0.5)(bgr, Q, JPEG)
        c.set_frame_format(JPEG)
        c.set_jpeg_budget(budget)
        used = _same("budget on", bgr, _collect(c, c.render_many, shapes, chain=False), budget)      # bodies with the search in them
        assert max(used) < Q, used
        c.set_frame_format(capi.FRAME_BGR)
        c.set_jpeg_budget(0)
        c.set_frame_format(JPEG)
        for k, (b, j) in enumerate(zip(bgr, _collect(c, c.render_many, shapes, chain=False))):      # bodies without it
            _equal(f"budget switched off under BGR, frame {k}", j, capi.bgr_to_jpeg_frame(b, Q))
        c.set_frame_format(capi.FRAME_BGR)
        c.set_jpeg_budget(budget)
        c.set_frame_format(JPEG)
        assert _same("budget switched on under BGR", bgr, _collect(c, c.render_many, shapes, chain=False), budget) == used
        c.set_frame_format(capi.FRAME_BGR)                          # ... and with BGR frames rendered in between, on some of the slots only
        got = _collect(c, c.render_many, shapes[:2], chain=False)
        assert all(np.array_equal(a, b) for a, b in zip(bgr, got))
        c.set_jpeg_budget(0)
        c.set_frame_format(JPEG)
        for k, (b, j) in enumerate(zip(bgr, _collect(c, c.render_many, shapes, chain=False))):
            _equal(f"budget switched off under BGR behind two BGR frames, frame {k}", j, capi.bgr_to_jpeg_frame(b, Q))
    finally:
        c.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_copies(fmt):
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], fmt=fmt, number_of_frames=2)

    def resident(c):
        c.pair_begin(inp["img1"], inp["img2"])
        return c.morph_frames(0.0) + c.morph_frames(1.0) + _collect(c, c.render_phases, [0.0, 0.5, 1.0])
    _, _, _, used = _both("phase 0 / 1 and t 0 / 1 on a resident pair", resident, fmt=fmt, number_of_frames=2)
    assert all(q < Q for q in used), used


def test_morph_list_of_three():
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2
        return [f for pair in frames for f in pair]
    _both("morph_list of 3", run, number_of_frames=4)


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
                budget = _fraction(0.5)(list(results[0].values()), 60, JPEG)
                p.set_jpeg_quality(60)
                p.set_jpeg_budget(budget)
                with pytest.raises(capi.PoppyError, match=str(E_ARG)):
                    p.set_jpeg_budget(1 << 32)
            for b in range(2):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            if fmt == JPEG:
                with pytest.raises(capi.PoppyError, match=str(E_STATE)):      # as the pool's other setters: not with work submitted
                    p.set_jpeg_budget(budget + 1)
            p.wait()
            results.append(got)
        finally:
            p.close()
    bgr, jpeg = results
    assert sorted(bgr) == sorted(jpeg) and len(jpeg) == 2 * len(pairs) * 4
    keys = sorted(bgr)
    used = _same("pool batches", [bgr[k] for k in keys], [jpeg[k] for k in keys], budget, 60)
    assert min(used) < 60, used


def test_frame_scale_and_frame_size():
    w, h = 256, 192
    run = _loaded(w, h)(lambda c: _collect(c, c.render_many, [0.25, 0.5, 0.75], chain=True) + _collect(c, c.render_many, [0.3, 0.6], chain=False))
    _, jpeg, b, used = _both("scale 2", run, small=lambda f: capi.bgr_downscale(f, 2), prepare=lambda c: c.set_frame_scale(2))
    assert all(q < Q for q in used) and all(f.size - 4 <= b for f in jpeg), "the budget holds on the scaled frame"
    _both("size 100 x 70", run, small=lambda f: capi.bgr_resize_area(f, 100, 70), prepare=lambda c: c.set_frame_size(100, 70), fmt=JPEG444)


def test_budget_off_is_todays_frames_and_marks():
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=True)
        c.reset()
        c.set_frame_format(JPEG)
        c.set_jpeg_budget(0)
        c.set_timing(1)
        c.timing_summary()
        off = _collect(c, c.render_many, shapes, chain=True)
        marks_off = {name: n for name, _, n in c.timing_summary()}
        c.reset()
        c.set_jpeg_budget(4000)
        on = _collect(c, c.render_many, shapes, chain=True)
        marks_on = {name: n for name, _, n in c.timing_summary()}
        for k, (b, j) in enumerate(zip(bgr, off)):
            _equal(f"budget 0, frame {k}", j, capi.bgr_to_jpeg_frame(b, Q))
        _same("budget 4000", bgr, on, 4000)
        assert marks_off.get("jpeg_code") == len(shapes) and marks_off.get("jpeg_pack") == len(shapes), marks_off
        assert "jpeg_measure" not in marks_off and "jpeg_pick" not in marks_off, marks_off
        assert marks_on.get("jpeg_code") == len(shapes) and marks_on.get("jpeg_pack") == len(shapes), marks_on
        assert marks_on.get("jpeg_measure", 0) > 0 and marks_on.get("jpeg_measure") == marks_on.get("jpeg_pick"), marks_on
    finally:
        c.close()


def test_the_formats_on_built_tables_refuse_a_budget_in_both_orders():
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.3, 0.7]
    L = capi.lib()
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        bgr = _collect(c, c.render_many, shapes, chain=False)
        budget = _fraction(0.5)(bgr, Q, JPEG)
        c.set_frame_format(JPEG)
        c.set_jpeg_budget(budget)
        for fmt in BUILT_TABLE_FORMATS:                             # the budget first, the format second: the format stays JPEG, the budget stays
            assert L.poppy_hip_set_frame_format(c.h, fmt) == E_UNSUPPORTED
            assert c.get_jpeg_budget() == budget
            _same(f"after format {fmt} was refused", bgr, _collect(c, c.render_many, shapes, chain=False), budget)
        c.set_jpeg_budget(0)
        for fmt in BUILT_TABLE_FORMATS:                             # the format first, the budget second: the budget stays off, the format stays
            c.set_frame_format(fmt)
            assert L.poppy_hip_set_jpeg_budget(c.h, budget) == E_UNSUPPORTED
            assert c.get_jpeg_budget() == 0
            frames = _collect(c, c.render_many, shapes, chain=False)
            assert len(frames) == len(shapes) and all(capi.jpeg_frame_quality(f) == Q for f in frames)
            if fmt in (capi.FRAME_JPEG_OPT, capi.FRAME_JPEG444_OPT):
                host = capi.bgr_to_jpeg_opt_frame if fmt == capi.FRAME_JPEG_OPT else capi.bgr_to_jpeg444_opt_frame
                for k, (b, j) in enumerate(zip(bgr, frames)):
                    _equal(f"format {fmt} after the budget was refused, frame {k}", j, host(b, Q))
        c.set_frame_format(capi.FRAME_BGR)
        c.set_jpeg_budget(budget)                                   # a format that ignores the budget takes it
        for k, (b, j) in enumerate(zip(bgr, _collect(c, c.render_many, shapes, chain=False))):
            assert np.array_equal(b, j), f"BGR frame {k} under a budget"
        c.set_frame_format(JPEG444)
        _same("JPEG444 after all of it", bgr, _collect(c, c.render_many, shapes, chain=False), budget, fmt=JPEG444)
    finally:
        c.close()
