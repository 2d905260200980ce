"""GPU checks of the resized hand-off (poppy_hip_set_frame_size).  The kernel alone, through poppy_hip_bgr_resize_area, against the host statement
poppy_bgr_resize_area (tests/test_host_frame_resize.py pins that to the rule) on both sides of everything its launcher tells apart, in all three widths of
its arithmetic.
The frame path: every case runs on a context that hands out full-size BGR and on contexts with a size and a format, and every frame of those must equal
the format's host statement of the resized BGR frames, bit for bit — all six formats at two sizes, odd geometries, a 4K frame, size changes with captured
bodies, the exclusion of size and scale, timing marks, limits that follow the resized geometry, a GIF file through the coded sink, and the download forms
in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
import test_gpu_frame_scale as S
import test_host_frame_resize as HR
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_NOMATCH, E_UNSUPPORTED = S.E_ARG, S.E_STATE, S.E_NOMATCH, S.E_UNSUPPORTED
ROOT = S.ROOT
BGR, I420, PAL8, PAL8_SEQ, GIF, GIF_SEQ = S.BGR, S.I420, S.PAL8, S.PAL8_SEQ, S.GIF, S.GIF_SEQ
FORMATS = S.FORMATS
_collect, _inputs, _loaded = S._collect, S._inputs, S._loaded
_REF = S._REF                                        # case -> its sequences from a plain context: shared with the scale's tests, whose cases these repeat
BLOCK = 256                                          # the kernel's workgroup: one thread per output pixel (kernels_frame_resize.hip)


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


_FORMS = set()


def _kernel_case(c, f, ow, oh, what, **pads):
    h, w = f.shape[:2]
    _FORMS.add(capi.bgr_resize_area_form(w, h, ow, oh))
    got = c.bgr_resize_area(f, ow, oh, **pads)
    want = capi.bgr_resize_area(f, ow, oh)
    assert got.shape == want.shape, f"{what}: {got.shape}, the host statement gives {want.shape}"
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{what}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"
    return got


def _src(o, ratio):
    """a source side for o outputs: "same", "one more", 1.5, the 1027 : 613 ratio and exactly 8"""
    return {"1": o, "+1": o + 1, "1.5": (3 * o + 1) // 2, "1027/613": (1027 * o) // 613, "8": 8 * o}[ratio]


@pytest.mark.parametrize("ratio", ["1", "+1", "1.5", "1027/613", "8"])
def test_kernel_matches_the_host_statement(ctx, ratio):
    """Outputs of fewer pixels than one workgroup, of exactly one (64 x 4, 16 x 16), of one pixel more and less, and of several with a last one that is partly
    filled; widths and heights that are odd, even and 1; every ratio on both axes."""
    assert 64 * 4 == 16 * 16 == BLOCK
    for ow in (15, 16, 63, 64, 65, 129):
        for oh in (1, 3, 4, 5, 16, 17):
            w, h = _src(ow, ratio), _src(oh, ratio)
            for name, f in HR.frames_for(w, h).items():
                _kernel_case(ctx, f, ow, oh, f"{w}x{h} -> {ow}x{oh}, {name}")


def test_kernel_one_axis_and_thin_frames(ctx):
    for w, h, ow, oh in [(150, 40, 150, 17), (150, 40, 67, 40), (1, 40, 1, 17), (40, 1, 17, 1), (300, 1, 200, 1), (1, 300, 1, 200), (5, 3, 1, 1),
                         (16, 128, 16, 16), (1027, 9, 613, 3)]:
        for name, f in HR.frames_for(w, h).items():
            _kernel_case(ctx, f, ow, oh, f"{w}x{h} -> {ow}x{oh}, {name}")


def test_kernel_source_alignment_and_more_than_one_workgroup(ctx):
    """A row pad of p bytes puts the device copy of the source p mod 16 bytes behind a 256-byte boundary.  1024 x 67 -> 683 x 45 is 121 workgroups; a frame cut
    to 15 output columns and a 2 x 3000 one are more than one workgroup too."""
    f = HR.frames_for(1024, 67)["random"]
    g = HR.frames_for(2, 3000)["127/128"]
    for pad in (0, 1, 4, 8, 13):
        _kernel_case(ctx, f, 683, 45, f"1024x67 -> 683x45, row pad {pad}", row_pad=pad)
        _kernel_case(ctx, f[:, :22], 15, 45, f"22x67 -> 15x45, row pad {pad}", row_pad=pad)
        _kernel_case(ctx, g, 2, 1500, f"2x3000 -> 2x1500, row pad {pad}", row_pad=pad)
    _kernel_case(ctx, HR.frames_for(100, 9)["127/128"], 64, 6, "100x9 -> 64x6, padded destination rows", dst_pad=5)
    _kernel_case(ctx, HR.frames_for(20, 9)["127/128"], 13, 6, "20x9 -> 13x6, padded destination rows", row_pad=3, dst_pad=2)


def test_kernel_every_width_of_arithmetic(ctx):
    """The launcher tells three apart (poppy_hip_bgr_resize_area_form).  0: sums of a frame above 2^24 pixels are 64-bit, white 4100 x 4100 stays white.
    2 at its limit: 4096 x 4096 = 2^24 pixels, white, the largest 32-bit numerator.  1: a side above 32768, whose index products need 64 bits."""
    _FORMS.clear()
    w = h = 4100
    got = _kernel_case(ctx, np.full((h, w, 3), 255, np.uint8), w - 1, h - 1, "white 4100x4100 -> 4099x4099")
    assert _FORMS == {0} and got.shape == (h - 1, w - 1, 3) and (got == 255).all()
    _kernel_case(ctx, np.full((4096, 4096, 3), 255, np.uint8), 2731, 2731, "white 4096x4096 -> 2731x2731")
    assert _FORMS == {0, 2}
    for name, f in HR.frames_for(3, 40000).items():
        _kernel_case(ctx, f, 2, 33000, f"3x40000 -> 2x33000, {name}")          # the long axis as rows ...
        _kernel_case(ctx, np.ascontiguousarray(f.transpose(1, 0, 2)), 33000, 2, f"40000x3 -> 33000x2, {name}")          # ... and as columns
    assert _FORMS == {0, 1, 2}


def test_kernel_refusals(ctx):
    f = np.zeros((4, 9, 3), np.uint8)
    call = capi.lib().poppy_hip_bgr_resize_area
    out = np.full(4 * 27, 0xA5, np.uint8)
    for ow, oh in [(0, 2), (5, 0), (-1, 2), (10, 2), (5, 5), (1, 2)]:
        assert call(ctx.h, capi._p(f), 27, 9, 4, ow, oh, capi._p(out), 30) == E_ARG and (out == 0xA5).all()
    assert call(ctx.h, capi._p(f), 26, 9, 4, 5, 2, capi._p(out), 15) == E_ARG
    assert call(ctx.h, capi._p(f), 27, 9, 4, 5, 2, capi._p(out), 14) == E_ARG
    assert call(ctx.h, None, 27, 9, 4, 5, 2, capi._p(out), 15) == E_ARG and (out == 0xA5).all()


# ---- the frame path -----------------------------------------------------------------------------------------------------------------------------

def host_sequence(fmt, frames, size):
    """F_host(resize_host(frames)): what a writer gets for the BGR frames of one sequence under format fmt and size (ow, oh)"""
    small = [capi.bgr_resize_area(f, *size) for f in frames]
    if fmt == BGR:
        return small
    if fmt == PAL8_SEQ:
        return list(capi.bgr_frames_to_pal8(np.stack(small)))
    if fmt == GIF_SEQ:
        return capi.bgr_frames_to_gif_frames(np.stack(small))
    one = {I420: capi.bgr_to_i420, PAL8: capi.bgr_to_pal8, GIF: capi.bgr_to_gif_frame}[fmt]
    return [one(f) for f in small]


def _same(what, fmt, size, ref_seqs, got_seqs):
    assert len(ref_seqs) == len(got_seqs) and len(ref_seqs) > 0, f"{what}: {len(ref_seqs)} sequences plain, {len(got_seqs)} resized"
    for q, (ref, got) in enumerate(zip(ref_seqs, got_seqs)):
        assert len(ref) == len(got) and len(ref) > 0, f"{what}: sequence {q}: {len(ref)} frames plain, {len(got)} resized"
        for k, (a, b) in enumerate(zip(host_sequence(fmt, ref, size), got)):
            assert a.shape == b.shape, f"{what}: sequence {q}, frame {k}: {b.shape}, the host statement gives {a.shape}"
            neq = np.flatnonzero(a.ravel() != b.ravel())
            assert neq.size == 0, f"{what}: sequence {q}, frame {k}: {neq.size} of {a.size} bytes differ, first at {neq[0]}"


def _run(run, fmt, size, **settings):
    c = capi.Context(0, **settings)
    try:
        if fmt != BGR:
            c.set_frame_format(fmt)
        if size:
            c.set_frame_size(*size)
        return run(c)
    finally:
        c.close()


def _both(what, run, fmt, sizes, **settings):
    """run(ctx) -> a list of sequences (lists of frames, one per call or pair), on a plain BGR context and on a context of format fmt per size"""
    if what not in _REF:
        _REF[what] = _run(run, BGR, None, **settings)
    for size in sizes:
        _same(f"{what}, format {fmt}, size {size}", fmt, size, _REF[what], _run(run, fmt, size, **settings))


SIZES_256 = ((171, 171), (200, 96))


@pytest.mark.parametrize("fmt", FORMATS)
def test_morph_chained_and_phase_mode_on_fixtures(fmt):
    inp = G.astage_inputs("a_256x256_chain")
    _both("chained morph", lambda c: [c.morph(inp["img1"], inp["img2"])[1]], fmt, SIZES_256, number_of_frames=6)
    inp2 = G.astage_inputs("a_256x256_phase")
    _both("phase-mode morph 0.25", lambda c: [c.morph(inp2["img1"], inp2["img2"], phase=0.25)[1]], fmt, SIZES_256, number_of_frames=1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_phase_zero_and_one_copies(fmt):
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: [c.morph(inp["img1"], inp["img2"], phase=ph)[1]], fmt, SIZES_256[:1], number_of_frames=3)
        _both(f"morph phase {ph}, padded rows", lambda c: [c.morph(inp["img1"], inp["img2"], phase=ph, row_pad=(7, 12))[1]], fmt, SIZES_256[1:], number_of_frames=2)

    def resident(c):
        c.pair_begin(inp["img1"], inp["img2"])
        return [c.morph_frames(0.0), c.morph_frames(1.0)]
    _both("morph_frames phase 0 / 1 on a resident pair", resident, fmt, SIZES_256[:1], number_of_frames=2)


@pytest.mark.parametrize("fmt", FORMATS)
def test_linear_blend_fallback(fmt):
    inp = G.make_inputs.dissolve_inputs("x_dissolve_200x150")
    a = inp["img1"]
    b = np.full_like(a, 77)
    for ph in (-1.0, 0.3):
        def run(c):
            rc, frames, _ = c.morph(a, b, phase=ph)
            assert rc == E_NOMATCH
            return [frames]
        _both(f"fallback phase {ph}", run, fmt, ((133, 100),), number_of_frames=3)


@pytest.mark.parametrize("fmt", FORMATS)
def test_render_many_and_render_phases(fmt):
    run = _loaded(320, 200)
    shapes = [0.1, 0.35, 0.6, 0.8, 0.95]
    sizes = ((213, 133),)
    _both("render_many chained", run(lambda c: [_collect(c, c.render_many, shapes, chain=True)]), fmt, sizes)
    _both("render_many unchained", run(lambda c: [_collect(c, c.render_many, shapes, chain=False)]), fmt, sizes)
    ts = [0.0, 0.2, 0.4, 1.0, 0.6, 0.8, 0.0, 1.0]
    _both("render_phases with t = 0 / 1", run(lambda c: [_collect(c, c.render_phases, ts)]), fmt, sizes)


@pytest.mark.parametrize("fmt", FORMATS)
def test_morph_list_of_three_and_a_canvas(fmt):
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2
        return frames                                               # each pair is a sequence
    _both("morph_list of 3", run, fmt, ((171, 128),), number_of_frames=4)
    small = [images[0][:150, :200], images[1], images[2][:, :230]]

    def canvas(c):
        rc, frames, _, done = c.morph_list(small, canvas=(263, 197))
        assert rc == 0 and done == 2
        return frames
    _both("morph_list of 3 on a 263 x 197 canvas", canvas, fmt, ((175, 131),), number_of_frames=3)


@pytest.mark.parametrize("fmt", FORMATS)
def test_pool_batches_and_state(fmt):
    pairs = [(synth.gen(256, 192, 77, 0, 0), synth.gen(256, 192, 77, 6 + k, 3)) for k in range(3)]
    size = (171, 128)

    def batches(f, sz):
        p = capi.Pool([0], contexts_per_device=3, number_of_frames=4)
        try:
            got = {}
            if f != BGR:
                p.set_frame_format(f)
            if sz:
                p.set_frame_size(*sz)
            for b in range(2):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            with pytest.raises(capi.PoppyError, match=str(E_STATE)):
                p.set_frame_size(128, 96)
            p.wait()
            if sz:
                p.set_frame_size(*sz)                                   # waited for: allowed again
                with pytest.raises(capi.PoppyError, match=str(E_ARG)):
                    p.set_frame_size(0, 96)
                with pytest.raises(capi.PoppyError, match=str(E_ARG)):
                    p.set_frame_size(-1, -1)
        finally:
            p.close()
        assert sorted(got) == [(b, pi, j) for b in range(2) for pi in range(len(pairs)) for j in range(4)]
        return [[got[(b, pi, j)] for j in range(4)] for b in range(2) for pi in range(len(pairs))]      # each pair is a sequence
    if "pool" not in _REF:
        _REF["pool"] = batches(BGR, None)
    _same(f"pool batches, format {fmt}, size {size}", fmt, size, _REF["pool"], batches(fmt, size))


@pytest.mark.parametrize("fmt", [BGR, PAL8])
@pytest.mark.parametrize("w,h,size", [(749, 480, (500, 320)), (1918, 1080, (960, 540)), (1920, 1080, (1280, 720)), (5, 3, (1, 1))])
def test_odd_geometries(w, h, size, fmt):
    run = _loaded(w, h)
    _both(f"{w}x{h} chained", run(lambda c: [_collect(c, c.render_many, [0.3, 0.7], chain=True)]), fmt, (size,))
    _both(f"{w}x{h} phase mode", run(lambda c: [_collect(c, c.render_phases, [0.0, 0.25, 0.6, 1.0])]), fmt, (size,))


@pytest.mark.parametrize("fmt", [BGR, PAL8])
def test_4k_phase_frame_equals_the_whole_factor_frame(fmt):
    what, run = "3840x2160 phase frame", _loaded(3840, 2160)(lambda c: [_collect(c, c.render_phases, [0.5])])
    if what not in _REF:
        _REF[what] = _run(run, BGR, None)
    got = _run(run, fmt, (1920, 1080))
    _same(f"{what}, format {fmt}", fmt, (1920, 1080), _REF[what], got)
    halved = S._run(run, fmt, 2)
    assert len(halved) == len(got) == 1 and len(halved[0]) == len(got[0]) == 1 and np.array_equal(halved[0][0], got[0][0]), "size (1920, 1080) and s = 2 differ at 4K"


def test_size_changes_recapture_the_bodies_and_exclude_the_scale():
    """Phase-mode bodies are captured graphs; with a writer and a size they end with the resize.  size -> off -> size on one context: the frames at "off" are
    those of a context that never resized; size and scale refuse each other with POPPY_E_STATE in both orders, and each is switched off to get to the other;
    an inadmissible size is POPPY_E_UNSUPPORTED with nothing changed; an explicit destination and the debug fetch stay full size."""
    w, h = 320, 200
    c1, c2, g, p1, p2 = _inputs(w, h)
    ts = [0.15, 0.3, 0.45, 0.6, 0.75, 0.9]
    a, b = (213, 133), (160, 200)
    plain = capi.Context(0); sw = capi.Context(0)
    try:
        plain.pair_load(c1, c2, g, p1, p2); sw.pair_load(c1, c2, g, p1, p2)
        want = _collect(plain, plain.render_phases, ts)
        sw.set_frame_size(*a)
        _same("size a", BGR, a, [want], [_collect(sw, sw.render_phases, ts)])
        sw.set_frame_size(0, 0)
        back = _collect(sw, sw.render_phases, ts)
        assert len(back) == len(want) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(want, back)), "frames with the size off differ"
        sw.set_frame_size(*a)
        _same("size a again", BGR, a, [want], [_collect(sw, sw.render_phases, ts)])
        sw.set_frame_size(*b)                                       # one size to another, no "off" between
        _same("size b", BGR, b, [want], [_collect(sw, sw.render_phases, ts)])
        sw.set_frame_format(I420)                                   # the format after the size
        _same("size b, then I420", I420, b, [want], [_collect(sw, sw.render_phases, ts)])
        sw.set_frame_size(*a)                                       # ... and the size after the format
        _same("I420, then size a", I420, a, [want], [_collect(sw, sw.render_phases, ts)])
        sw.set_frame_format(BGR)
        with pytest.raises(capi.PoppyError, match=f": {E_STATE}:"):
            sw.set_frame_scale(2)
        sw.set_frame_scale(1)                                       # no scale beside a size: nothing changes
        _same("size a after the refused scale", BGR, a, [want[:2]], [_collect(sw, sw.render_phases, ts[:2])])
        sw.set_frame_size(0, 0); sw.set_frame_scale(2)
        with pytest.raises(capi.PoppyError, match=f": {E_STATE}:"):
            sw.set_frame_size(*a)
        S._same("s = 2 after the refused size", BGR, 2, [want[:2]], [_collect(sw, sw.render_phases, ts[:2])])
        sw.set_frame_scale(1); sw.set_frame_size(*a)
        sw.render_phases(ts)                                        # no writer: bodies without the resize, frames stay in HBM, full size
        sw.render_many(ts, chain=False)
        _same("size a after frames without a writer", BGR, a, [want], [_collect(sw, sw.render_phases, ts)])
        full = sw.render(0.4, 0.4)
        assert full.shape == (h, w, 3) and np.array_equal(full, plain.render(0.4, 0.4)), "explicit-destination frames stay full size"
        assert np.array_equal(sw.fetch("trImg1"), plain.fetch("trImg1")), "the debug fetch stays full size"
        for bad in ((0, 5), (5, 0), (-1, 5), (-2, -2)):
            with pytest.raises(capi.PoppyError, match=f": {E_ARG}:"):
                sw.set_frame_size(*bad)
        for bad in ((39, 200), (320, 24), (321, 200), (320, 201)):          # above a factor of 8, and upscaling
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                sw.set_frame_size(*bad)
        assert sw.frame_size == a
        _same("size a after refused sizes", BGR, a, [want[:2]], [_collect(sw, sw.render_phases, ts[:2])])
    finally:
        plain.close(); sw.close()


def test_size_before_the_pair_and_a_pair_the_size_does_not_admit():
    """The size takes effect whether it is set before a pair is there or after, before or after the format.  With the 256 x 192 pair resident, (20, 192) is
    refused and nothing changes; a pair that does not admit the set size is refused by the call that would write its frames, and the context works again
    once the size is off."""
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    size = (100, 75)
    want = _run(_loaded(w, h)(lambda c: _collect(c, c.render_many, shapes, chain=True)), BGR, None)
    for first in ("size", "format"):
        c = capi.Context(0)
        try:
            if first == "size":
                c.set_frame_size(*size); c.set_frame_format(PAL8_SEQ)
            else:
                c.set_frame_format(PAL8_SEQ); c.set_frame_size(*size)
            c.pair_load(c1, c2, g, p1, p2)
            _same(f"{first} first, then the pair", PAL8_SEQ, size, [want], [_collect(c, c.render_many, shapes, chain=True)])
            with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
                c.set_frame_size(20, 192)
            assert c.frame_size == size
            c.reset()                                               # (the chain starts over)
            _same("after the refused size", PAL8_SEQ, size, [want], [_collect(c, c.render_many, shapes, chain=True)])
        finally:
            c.close()
    images = [synth.gen(w, h, 4321, 0, 0), synth.gen(w, h, 4321, 7, 3)]
    plain = _run(lambda c: c.morph(*images)[1], BGR, None, number_of_frames=3)
    c = capi.Context(0, number_of_frames=3)
    try:
        c.set_frame_size(20, 192)                                   # no pair: any size is taken
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.morph(*images)
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.morph(*images, phase=0.0)                             # the copies of a host image likewise
        c.set_frame_size(0, 0)
        got = c.morph(*images)[1]
        assert len(got) == len(plain) and all(np.array_equal(x, y) for x, y in zip(plain, got))
        c.set_frame_size(32, 24)                                    # exactly 8 on both axes
        _same("a factor of exactly 8", BGR, (32, 24), [plain], [c.morph(*images)[1]])
    finally:
        c.close()


def test_timing_mode_marks_the_resize():
    c1, c2, g, p1, p2 = _inputs(256, 192)
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        for size, fmt in ((None, BGR), ((171, 128), BGR), ((171, 128), I420), ((171, 128), GIF_SEQ)):
            c.set_frame_format(fmt); c.set_frame_size(*(size or (0, 0)))
            c.reset()
            c.set_timing(1)
            frames = _collect(c, c.render_many, [0.2, 0.5, 0.8], chain=True)
            names = {n: k for n, _, k in c.timing_summary()}
            c.set_timing(0)
            assert len(frames) == 3 and names.get("unsharp") == 3
            assert names.get("frame_resize") == (3 if size else None) and names.get("frame_scale") is None, f"size {size}, format {fmt}: {names}"
    finally:
        c.close()


def test_limits_follow_the_resized_geometry():
    """A 2 x 70000 pair under POPPY_FRAME_GIF: refused plain (a side above 65535), rendered under size (2, 35000)."""
    w, h = 2, 70000
    size = (2, 35000)
    c1, c2, g, p1, p2 = _inputs(w, h)
    what = "2 x 70000 plain"
    if what not in _REF:
        _REF[what] = [_run(lambda c: (c.pair_load(c1, c2, g, p1, p2), _collect(c, c.render_phases, [0.0, 0.4]))[1], BGR, None)]
    c = capi.Context(0)
    try:
        c.set_frame_format(GIF)
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.pair_load(c1, c2, g, p1, p2)
        c.set_frame_size(*size)
        c.pair_load(c1, c2, g, p1, p2)
        _same("2 x 70000 -> 2 x 35000", GIF, size, _REF[what], [_collect(c, c.render_phases, [0.0, 0.4])])
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):      # off with the pair resident: refused, nothing changed
            c.set_frame_size(0, 0)
        _same("2 x 70000 -> 2 x 35000, after the refusal", GIF, size, _REF[what], [_collect(c, c.render_phases, [0.0, 0.4])])
    finally:
        c.close()


def test_sink_file_from_a_resized_gpu_sequence_decodes_in_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    w, h, n = 256, 192, 6
    images = [synth.gen(w, h, 4321, 0, 0), synth.gen(w, h, 4321, 7, 3)]
    want = _run(lambda c: c.morph(*images)[1], BGR, None, number_of_frames=n)
    ow, oh = capi.frame_fit_size(w, h, 150, 150)
    assert (ow, oh) == (150, 113)
    L = capi.lib()
    path = tmp_path / "resized.gif"
    sink = L.poppy_sink_open(str(path).encode(), capi.SINK_GIF_GLOBAL_CODED, ow, oh, 25, 1)
    assert sink

    def run(c):
        rc, frames, _ = c.morph(*images)
        assert rc == 0
        return frames
    got = _run(run, GIF_SEQ, (ow, oh), number_of_frames=n)
    assert len(got) == n == len(want)
    for f in got:
        L.poppy_sink_write(sink, capi._p(f), ow, oh, 0)
    assert L.poppy_sink_close(sink) == n
    pal = capi.bgr_frames_to_pal8(np.stack([capi.bgr_resize_area(f, ow, oh) for f in want]))
    with Image.open(path) as im:
        assert im.n_frames == n and im.size == (ow, oh)
        for k, p in enumerate(pal):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert("RGB"))[:, :, ::-1], capi.pal8_to_bgr(p, ow, oh)), f"Pillow's frame {k} differs"


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
from poppy_amd import capi
import test_gpu_frame_resize as T
run = T._loaded(320, 200)
for fmt in (T.BGR, T.I420, T.GIF):
    T._both("render_many chained", run(lambda c: [T._collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=True)]), fmt, ((213, 133),))
    T._both("render_phases", run(lambda c: [T._collect(c, c.render_phases, [0.0, 0.3, 0.5, 0.7, 1.0])]), fmt, ((213, 133),))
print("child ok")
"""


def test_download_forms_in_a_child_process():
    """POPPY_HIP_DL_EVENTS=1 (one download stream + an event per copy) and POPPY_HIP_RING=1 are read once per process: a fresh child."""
    env = dict(os.environ, POPPY_HIP_DL_EVENTS="1", POPPY_HIP_RING="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
