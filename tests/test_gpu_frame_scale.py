"""GPU checks of the scaled hand-off (poppy_hip_set_frame_scale).  The kernel alone, through poppy_hip_bgr_downscale, against the host statement
poppy_bgr_downscale (tests/test_host_frame_scale.py pins that to the rule) on both sides of everything its launcher tells apart.  The frame path: every case
runs on a context that hands out full-size BGR and on contexts with a scale and a format, and every frame of those must equal the format's host statement of
the downscaled BGR frames, bit for bit — all six formats at s = 2 and 3, odd and thin geometries, a 4K frame, scale changes with captured bodies, timing
marks, limits that follow the scaled geometry, a GIF file through the coded sink, and the download forms in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
import test_gpu_frame_format as FF
import test_host_frame_scale as HS
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_NOMATCH, E_UNSUPPORTED = -1, -4, -5, -6
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BGR, I420, PAL8, PAL8_SEQ, GIF, GIF_SEQ = capi.FRAME_BGR, capi.FRAME_I420, capi.FRAME_PAL8, capi.FRAME_PAL8_SEQ, capi.FRAME_GIF, capi.FRAME_GIF_SEQ
FORMATS = [BGR, I420, PAL8, PAL8_SEQ, GIF, GIF_SEQ]
_collect, _inputs, _loaded = FF._collect, FF._inputs, FF._loaded


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _kernel_case(c, f, s, what, **pads):
    got = c.bgr_downscale(f, s, **pads)
    want = capi.bgr_downscale(f, s)
    assert got.shape == want.shape, f"{what}: {got.shape}, the host statement gives {want.shape}"
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{what}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


@pytest.mark.parametrize("s", HS.FACTORS)
def test_kernel_matches_the_host_statement(ctx, s):
    """The wide form takes widths that are multiples of 8 (s = 2, 4, 8): 8 s k and 8 s k +- 1 for k = 1, 2 sit on both sides of it, for every factor; widths
    1 and s - 1; heights 1, s, s + 1 and 2 s + 1 (no full row, no clipped row, a clipped row behind the wide rows)."""
    widths = sorted({v for k in (1, 2) for v in (8 * s * k - 1, 8 * s * k, 8 * s * k + 1)} | {1, max(1, s - 1), 8 * 3})
    for w in widths:
        for h in sorted({1, s, s + 1, 2 * s + 1}):
            for name, f in HS.frames_for(w, h, s).items():
                _kernel_case(ctx, f, s, f"{w}x{h} / {s}, {name}")


@pytest.mark.parametrize("s", [2, 4, 8, 3])
def test_kernel_source_alignment_and_more_than_one_block(ctx, s):
    """A row pad of p bytes puts the device copy of the source p mod 16 bytes behind a 256-byte boundary: 8 keeps the wide form, every other value here
    takes the bytewise one.  1024 x 67 is more than one workgroup in both forms, 1027 x 67 has a clipped right column."""
    for w in (1024, 1027):
        f = HS.frames_for(w, 67, s)["random"]
        for pad in (0, 1, 4, 8, 13):
            _kernel_case(ctx, f, s, f"{w}x67 / {s}, row pad {pad}", row_pad=pad)
    _kernel_case(ctx, HS.frames_for(64, 9, s)["ties"], s, f"64x9 / {s}, padded destination rows", dst_pad=5)


def test_kernel_refusals(ctx):
    f = np.zeros((4, 4, 3), np.uint8)
    for s in (0, 9, -1):
        out = np.full(48, 0xA5, np.uint8)
        assert capi.lib().poppy_hip_bgr_downscale(ctx.h, capi._p(f), 12, 4, 4, s, capi._p(out), 12) == E_ARG and (out == 0xA5).all()
    out = np.full(48, 0xA5, np.uint8)
    assert capi.lib().poppy_hip_bgr_downscale(ctx.h, capi._p(f), 11, 4, 4, 2, capi._p(out), 6) == E_ARG
    assert capi.lib().poppy_hip_bgr_downscale(ctx.h, capi._p(f), 12, 4, 4, 2, capi._p(out), 5) == E_ARG
    assert capi.lib().poppy_hip_bgr_downscale(ctx.h, None, 12, 4, 4, 2, capi._p(out), 6) == E_ARG and (out == 0xA5).all()


# ---- the frame path -----------------------------------------------------------------------------------------------------------------------------

def host_sequence(fmt, frames, s):
    """F_host(downscale_host(frames)): what a writer gets for the BGR frames of one sequence under format fmt and scale s"""
    small = [capi.bgr_downscale(f, s) for f in frames]
    if fmt == BGR:
        return small
    if fmt == PAL8_SEQ:
        return list(capi.bgr_frames_to_pal8(np.stack(small)))
    if fmt == GIF_SEQ:
        return capi.bgr_frames_to_gif_frames(np.stack(small))
    one = {I420: capi.bgr_to_i420, PAL8: capi.bgr_to_pal8, GIF: capi.bgr_to_gif_frame}[fmt]
    return [one(f) for f in small]


def _same(what, fmt, s, ref_seqs, got_seqs):
    assert len(ref_seqs) == len(got_seqs) and len(ref_seqs) > 0, f"{what}: {len(ref_seqs)} sequences at s = 1, {len(got_seqs)} scaled"
    for q, (ref, got) in enumerate(zip(ref_seqs, got_seqs)):
        assert len(ref) == len(got) and len(ref) > 0, f"{what}: sequence {q}: {len(ref)} frames at s = 1, {len(got)} scaled"
        for k, (a, b) in enumerate(zip(host_sequence(fmt, ref, s), got)):
            assert a.shape == b.shape, f"{what}: sequence {q}, frame {k}: {b.shape}, the host statement gives {a.shape}"
            neq = np.flatnonzero(a.ravel() != b.ravel())
            assert neq.size == 0, f"{what}: sequence {q}, frame {k}: {neq.size} of {a.size} bytes differ, first at {neq[0]}"


def _run(run, fmt, s, **settings):
    c = capi.Context(0, **settings)
    try:
        if fmt != BGR:
            c.set_frame_format(fmt)
        if s != 1:
            c.set_frame_scale(s)
        return run(c)
    finally:
        c.close()


_REF = {}                                            # case -> its sequences from a context that never scaled, computed once


def _both(what, run, fmt, scales=(2, 3), **settings):
    """run(ctx) -> a list of sequences (lists of frames, one per call or pair), on an s = 1 BGR context and on a context of format fmt per scale"""
    if what not in _REF:
        _REF[what] = _run(run, BGR, 1, **settings)
    for s in scales:
        _same(f"{what}, format {fmt}, s = {s}", fmt, s, _REF[what], _run(run, fmt, s, **settings))


@pytest.mark.parametrize("fmt", FORMATS)
def test_morph_chained_and_phase_mode_on_fixtures(fmt):
    inp = G.astage_inputs("a_256x256_chain")
    _both("chained morph", lambda c: [c.morph(inp["img1"], inp["img2"])[1]], fmt, number_of_frames=6)
    inp2 = G.astage_inputs("a_256x256_phase")
    _both("phase-mode morph 0.25", lambda c: [c.morph(inp2["img1"], inp2["img2"], phase=0.25)[1]], fmt, number_of_frames=1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_phase_zero_and_one_copies(fmt):
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: [c.morph(inp["img1"], inp["img2"], phase=ph)[1]], fmt, number_of_frames=3)
        _both(f"morph phase {ph}, padded rows", lambda c: [c.morph(inp["img1"], inp["img2"], phase=ph, row_pad=(7, 12))[1]], fmt, number_of_frames=2)

    def resident(c):
        c.pair_begin(inp["img1"], inp["img2"])
        return [c.morph_frames(0.0), c.morph_frames(1.0)]
    _both("morph_frames phase 0 / 1 on a resident pair", resident, fmt, number_of_frames=2)


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
        _both(f"fallback phase {ph}", run, fmt, number_of_frames=3)


@pytest.mark.parametrize("fmt", FORMATS)
def test_render_many_and_render_phases(fmt):
    run = _loaded(320, 200)
    shapes = [0.1, 0.35, 0.6, 0.8, 0.95]
    _both("render_many chained", run(lambda c: [_collect(c, c.render_many, shapes, chain=True)]), fmt)
    _both("render_many unchained", run(lambda c: [_collect(c, c.render_many, shapes, chain=False)]), fmt)
    ts = [0.0, 0.2, 0.4, 1.0, 0.6, 0.8, 0.0, 1.0]
    _both("render_phases with t = 0 / 1", run(lambda c: [_collect(c, c.render_phases, ts)]), fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_morph_list_of_three_and_a_canvas(fmt):
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(3)]

    def run(c):
        rc, frames, _, done = c.morph_list(images)
        assert rc == 0 and done == 2
        return frames                                               # each pair is a sequence
    _both("morph_list of 3", run, fmt, number_of_frames=4)
    small = [images[0][:150, :200], images[1], images[2][:, :230]]

    def canvas(c):
        rc, frames, _, done = c.morph_list(small, canvas=(263, 197))
        assert rc == 0 and done == 2
        return frames
    _both("morph_list of 3 on a 263 x 197 canvas", canvas, fmt, scales=(2,), number_of_frames=3)


@pytest.mark.parametrize("fmt", FORMATS)
def test_pool_batches_and_state(fmt):
    pairs = [(synth.gen(256, 192, 77, 0, 0), synth.gen(256, 192, 77, 6 + k, 3)) for k in range(3)]

    def batches(f, s):
        p = capi.Pool([0], contexts_per_device=3, number_of_frames=4)
        try:
            got = {}
            if f != BGR:
                p.set_frame_format(f)
            if s != 1:
                p.set_frame_scale(s)
            for b in range(2):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            with pytest.raises(capi.PoppyError, match=str(E_STATE)):
                p.set_frame_scale(1 if s != 1 else 2)
            p.wait()
            p.set_frame_scale(s)                                        # waited for: allowed again
            with pytest.raises(capi.PoppyError, match=str(E_ARG)):
                p.set_frame_scale(9)
        finally:
            p.close()
        assert sorted(got) == [(b, pi, j) for b in range(2) for pi in range(len(pairs)) for j in range(4)]
        return [[got[(b, pi, j)] for j in range(4)] for b in range(2) for pi in range(len(pairs))]      # each pair is a sequence
    if "pool" not in _REF:
        _REF["pool"] = batches(BGR, 1)
    for s in (2, 3):
        _same(f"pool batches, format {fmt}, s = {s}", fmt, s, _REF["pool"], batches(fmt, s))


@pytest.mark.parametrize("fmt", [BGR, PAL8])
@pytest.mark.parametrize("w,h,scales", [(749, 480, (2, 3)), (1918, 1080, (4,)), (1, 40, (2,)), (40, 1, (2,)), (5, 3, (8,)), (1920, 1080, (2,))])
def test_odd_and_thin_geometries(w, h, scales, fmt):
    run = _loaded(w, h)
    _both(f"{w}x{h} chained", run(lambda c: [_collect(c, c.render_many, [0.3, 0.7], chain=True)]), fmt, scales=scales)
    _both(f"{w}x{h} phase mode", run(lambda c: [_collect(c, c.render_phases, [0.0, 0.25, 0.6, 1.0])]), fmt, scales=scales)
    if (w, h) == (5, 3):
        assert capi.frame_scaled_size(w, h, 8) == (1, 1)


@pytest.mark.parametrize("fmt", [BGR, PAL8])
def test_4k_phase_frame(fmt):
    _both("3840x2160 phase frame", _loaded(3840, 2160)(lambda c: [_collect(c, c.render_phases, [0.5])]), fmt, scales=(2,))


def test_scale_changes_recapture_the_bodies():
    """Phase-mode bodies are captured graphs; with a writer and a scale above 1 they end with the downscale.  s = 2 -> 1 -> 2 on one context: the frames at
    s = 1 are those of a context that never scaled, the frames at s = 2 their downscaled forms both times; frames rendered without a writer (bodies without
    the downscale) and then with one are scaled; an explicit destination and the debug fetch stay full size."""
    w, h = 320, 200
    c1, c2, g, p1, p2 = _inputs(w, h)
    ts = [0.15, 0.3, 0.45, 0.6, 0.75, 0.9]
    plain = capi.Context(0); sw = capi.Context(0)
    try:
        plain.pair_load(c1, c2, g, p1, p2); sw.pair_load(c1, c2, g, p1, p2)
        want = _collect(plain, plain.render_phases, ts)
        sw.set_frame_scale(2)
        _same("s = 2", BGR, 2, [want], [_collect(sw, sw.render_phases, ts)])
        sw.set_frame_scale(1)
        back = _collect(sw, sw.render_phases, ts)
        assert len(back) == len(want) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(want, back)), "frames at s = 1 after s = 2 differ"
        sw.set_frame_scale(2)
        _same("s = 2 again", BGR, 2, [want], [_collect(sw, sw.render_phases, ts)])
        sw.set_frame_format(I420)                                   # the format after the scale
        _same("s = 2, then I420", I420, 2, [want], [_collect(sw, sw.render_phases, ts)])
        sw.set_frame_scale(3)                                       # ... and the scale after the format
        _same("I420, then s = 3", I420, 3, [want], [_collect(sw, sw.render_phases, ts)])
        sw.set_frame_format(BGR); sw.set_frame_scale(2)
        sw.render_phases(ts)                                        # no writer: bodies without the downscale, frames stay in HBM, full size
        sw.render_many(ts, chain=False)
        _same("s = 2 after frames without a writer", BGR, 2, [want], [_collect(sw, sw.render_phases, ts)])
        full = sw.render(0.4, 0.4)
        assert full.shape == (h, w, 3) and np.array_equal(full, plain.render(0.4, 0.4)), "explicit-destination frames stay full size"
        assert np.array_equal(sw.fetch("trImg1"), plain.fetch("trImg1")), "the debug fetch stays full size"
        for bad in (0, 9):
            with pytest.raises(capi.PoppyError, match=f": {E_ARG}:"):
                sw.set_frame_scale(bad)
        assert sw.frame_scale == 2
        _same("s = 2 after refused factors", BGR, 2, [want[:2]], [_collect(sw, sw.render_phases, ts[:2])])
    finally:
        plain.close(); sw.close()


def test_scale_before_the_pair_and_without_one():
    """The scale takes effect whether it is set before a pair is there or after, before or after the format."""
    w, h = 256, 192
    c1, c2, g, p1, p2 = _inputs(w, h)
    shapes = [0.25, 0.5, 0.75]
    want = _run(_loaded(w, h)(lambda c: _collect(c, c.render_many, shapes, chain=True)), BGR, 1)
    for first in ("scale", "format"):
        c = capi.Context(0)
        try:
            if first == "scale":
                c.set_frame_scale(3); c.set_frame_format(PAL8_SEQ)
            else:
                c.set_frame_format(PAL8_SEQ); c.set_frame_scale(3)
            c.pair_load(c1, c2, g, p1, p2)
            _same(f"{first} first, then the pair", PAL8_SEQ, 3, [want], [_collect(c, c.render_many, shapes, chain=True)])
        finally:
            c.close()


def test_timing_mode_marks_the_downscale():
    c1, c2, g, p1, p2 = _inputs(256, 192)
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        for s, fmt in ((1, BGR), (2, BGR), (2, I420), (2, GIF_SEQ)):
            c.set_frame_format(fmt); c.set_frame_scale(s)
            c.reset()
            c.set_timing(1)
            frames = _collect(c, c.render_many, [0.2, 0.5, 0.8], chain=True)
            names = {n: k for n, _, k in c.timing_summary()}
            c.set_timing(0)
            assert len(frames) == 3 and names.get("unsharp") == 3
            assert names.get("frame_scale") == (3 if s == 2 else None), f"s = {s}, format {fmt}: {names}"
    finally:
        c.close()


def test_limits_follow_the_scaled_geometry():
    """A 2 x 70000 pair under POPPY_FRAME_GIF: refused at s = 1 (a side above 65535), rendered at s = 2 as a 1 x 35000 frame."""
    w, h = 2, 70000
    c1, c2, g, p1, p2 = _inputs(w, h)
    want = _run(lambda c: (c.pair_load(c1, c2, g, p1, p2), _collect(c, c.render_phases, [0.0, 0.4]))[1], BGR, 1)
    c = capi.Context(0)
    try:
        c.set_frame_format(GIF)
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):
            c.pair_load(c1, c2, g, p1, p2)
        c.set_frame_scale(2)
        c.pair_load(c1, c2, g, p1, p2)
        got = _collect(c, c.render_phases, [0.0, 0.4])
        _same("2 x 70000 at s = 2", GIF, 2, [want], [got])
        with pytest.raises(capi.PoppyError, match=f": {E_UNSUPPORTED}:"):      # back to s = 1 with the pair resident: refused, nothing changed
            c.set_frame_scale(1)
        _same("2 x 70000 at s = 2, after the refusal", GIF, 2, [want], [_collect(c, c.render_phases, [0.0, 0.4])])
    finally:
        c.close()
    assert capi.frame_scaled_size(w, h, 2) == (1, 35000)


def test_sink_file_from_a_scaled_gpu_sequence_decodes_in_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    w, h, n = 256, 192, 6
    images = [synth.gen(w, h, 4321, 0, 0), synth.gen(w, h, 4321, 7, 3)]
    want = _run(lambda c: c.morph(*images)[1], BGR, 1, number_of_frames=n)
    ow, oh = capi.frame_scaled_size(w, h, 2)
    L = capi.lib()
    path = tmp_path / "scaled.gif"
    sink = L.poppy_sink_open(str(path).encode(), capi.SINK_GIF_GLOBAL_CODED, ow, oh, 25, 1)
    assert sink

    def run(c):
        rc, frames, _ = c.morph(*images)
        assert rc == 0
        return frames
    got = _run(run, GIF_SEQ, 2, number_of_frames=n)
    assert len(got) == n == len(want)
    for f in got:
        L.poppy_sink_write(sink, capi._p(f), ow, oh, 0)
    assert L.poppy_sink_close(sink) == n
    pal = capi.bgr_frames_to_pal8(np.stack([capi.bgr_downscale(f, 2) for f in want]))
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
import test_gpu_frame_scale as T
run = T._loaded(320, 200)
for fmt in (T.BGR, T.I420, T.GIF):
    T._both("render_many chained", run(lambda c: [T._collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=True)]), fmt, scales=(2,))
    T._both("render_phases", run(lambda c: [T._collect(c, c.render_phases, [0.0, 0.3, 0.5, 0.7, 1.0])]), fmt, scales=(2,))
print("child ok")
"""


def test_download_forms_in_a_child_process():
    """POPPY_HIP_DL_EVENTS=1 (one download stream + an event per copy) and POPPY_HIP_RING=1 are read once per process: a fresh child."""
    env = dict(os.environ, POPPY_HIP_DL_EVENTS="1", POPPY_HIP_RING="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
