"""GPU checks of the I420 frame hand-off (poppy_hip_set_frame_format): every case runs twice, on a context that hands out BGR and on one that
hands out I420, and every I420 frame must equal poppy_bgr_to_i420 of the BGR frame, bit for bit (the host function is the format's
definition; tests/test_host_frame_format.py pins it to the formula).  Chained and phase-mode frames, the phase 0 / 1 and t 0 / 1 copies,
the linear-blend fallback, render_many, render_phases, morph_list, queued pool batches, odd and thin geometries, a 4K frame, a context
switched back to BGR, timing mode 1, and the download forms chosen by environment variables in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu
E_STATE, E_NOMATCH = -4, -5
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _same_frames(what, bgr_frames, i420_frames):
    assert len(bgr_frames) == len(i420_frames) and len(bgr_frames) > 0, f"{what}: {len(bgr_frames)} BGR frames, {len(i420_frames)} I420 frames"
    for k, (b, y) in enumerate(zip(bgr_frames, i420_frames)):
        assert b.ndim == 3 and y.ndim == 1, f"{what}: frame {k} has the wrong format ({b.shape}, {y.shape})"
        want = capi.bgr_to_i420(b)
        assert y.shape == want.shape, f"{what}: frame {k}: {y.size} bytes, the format has {want.size}"
        neq = np.flatnonzero(y != want)
        assert neq.size == 0, f"{what}: frame {k}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


def _both(what, run, **settings):
    """run(ctx) -> frames, on a BGR and on an I420 context"""
    out = []
    for fmt in (capi.FRAME_BGR, capi.FRAME_I420):
        c = capi.Context(0, **settings)
        try:
            if fmt == capi.FRAME_I420:
                c.set_frame_format(fmt)
            out.append(run(c))
        finally:
            c.close()
    _same_frames(what, *out)
    return out


def _collect(c, call, *args, **kw):
    frames = []
    call(*args, write=lambda v: frames.append(v.copy()), **kw)
    return frames


def _textured(w, h, seed):
    if w * h <= 1 << 20:
        return synth.textured_bgr(w, h, seed)
    t = synth.textured_bgr(960, 540, seed)
    return np.ascontiguousarray(np.tile(t, (-(-h // 540), -(-w // 960), 1))[:h, :w])


def _inputs(w, h, n=40):
    """(image 1, image 2, gabor2, points 1, points 2) for pair_load; random bytes and corner points where the frame is thin"""
    rng = np.random.default_rng(w * 7919 + h)
    if min(w, h) < 33:
        c1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8); c2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        g = (rng.integers(0, 1025, (h, w, 3)) / 1024.0).astype(np.float32)
        corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
        inner = np.stack([rng.integers(0, 4 * (w - 1) + 1, 4), rng.integers(0, 4 * (h - 1) + 1, 4)], 1) / 4.0
        moved = np.clip(inner + rng.integers(-3, 4, inner.shape) / 4.0, 0, [w - 1, h - 1])
        return c1, c2, g, np.concatenate([corners, inner]).astype(np.float32), np.concatenate([corners, moved]).astype(np.float32)
    c1 = _textured(w, h, 41); c2 = _textured(w, h, 42); g = synth.unit_field(w, h, 7)
    p1 = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1).astype(np.float32)
    p2 = np.clip(p1 + rng.normal(0, 4.0, (n, 2)), 0, [w - 1, h - 1]).astype(np.float32)
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
    return c1, c2, g, np.concatenate([p1, corners]), np.concatenate([p2, corners])


def _loaded(w, h):
    def run_with(fn):
        def run(c):
            c1, c2, g, p1, p2 = _inputs(w, h)
            c.pair_load(c1, c2, g, p1, p2)
            return fn(c)
        return run
    return run_with


def test_morph_chained_and_phase_mode_on_fixtures():
    inp = G.astage_inputs("a_256x256_chain")
    _both("chained morph", lambda c: c.morph(inp["img1"], inp["img2"])[1], number_of_frames=12)
    inp = G.astage_inputs("a_256x256_phase")
    for ph in (0.25, 0.5):
        _both(f"phase-mode morph {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], number_of_frames=1)


def test_phase_zero_and_one_copies():
    inp = G.astage_inputs("a_256x256_phase01")
    for ph in (0.0, 1.0):
        _both(f"morph phase {ph}", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph)[1], number_of_frames=3)
        # row padding: the host conversion reads the stride
        _both(f"morph phase {ph}, padded rows", lambda c: c.morph(inp["img1"], inp["img2"], phase=ph, row_pad=(7, 12))[1], number_of_frames=2)

    def resident(c):
        c.pair_begin(inp["img1"], inp["img2"])
        return c.morph_frames(0.0) + c.morph_frames(1.0)
    _both("morph_frames phase 0 / 1 on a resident pair", resident, number_of_frames=2)


def test_linear_blend_fallback():
    """x_dissolve_200x150's first image against a featureless one: no point pairs, the fallback frames with POPPY_E_NOMATCH."""
    inp = G.make_inputs.dissolve_inputs("x_dissolve_200x150")
    a = inp["img1"]
    b = np.full_like(a, 77)
    for ph in (-1.0, 0.3):
        def run(c):
            rc, frames, _ = c.morph(a, b, phase=ph)
            assert rc == E_NOMATCH
            return frames
        _both(f"fallback phase {ph}", run, number_of_frames=3)


def test_render_many_and_render_phases():
    w, h = 320, 200
    run = _loaded(w, h)
    shapes = [0.1, 0.35, 0.6, 0.8, 0.95]
    _both("render_many chained", run(lambda c: _collect(c, c.render_many, shapes, chain=True)))
    _both("render_many unchained", run(lambda c: _collect(c, c.render_many, shapes, chain=False)))
    ts = [0.0, 0.2, 0.4, 1.0, 0.6, 0.8, 0.0, 1.0]
    _both("render_phases with t = 0 / 1", run(lambda c: _collect(c, c.render_phases, ts)))


def test_morph_list_three_and_four_images():
    images = [synth.gen(256, 192, 1234, k * 5, k * 2) for k in range(4)]

    def run(n):
        def r(c):
            rc, frames, _, done = c.morph_list(images[:n])
            assert rc == 0 and done == n - 1
            return [f for pair in frames for f in pair]
        return r
    _both("morph_list of 3", run(3), number_of_frames=5)
    _both("morph_list of 4", run(4), number_of_frames=3)
    _both("morph_list phase 0 of 2", lambda c: [f for p in c.morph_list(images[:2], phase=0.0)[1] for f in p], number_of_frames=2)


def test_pool_batches_and_state():
    pairs = [(synth.gen(256, 192, 77, 0, 0), synth.gen(256, 192, 77, 6 + k, 3)) for k in range(4)]
    results = []
    for fmt in (capi.FRAME_BGR, capi.FRAME_I420):
        p = capi.Pool([0], contexts_per_device=3, number_of_frames=4)
        try:
            got = {}
            if fmt == capi.FRAME_I420:
                p.set_frame_format(fmt)
            for b in range(3):
                p.submit_pairs(pairs, lambda pi, j, v, b=b: got.__setitem__((b, pi, j), v.copy()))
            with pytest.raises(capi.PoppyError, match=str(E_STATE)):
                p.set_frame_format(capi.FRAME_BGR if fmt == capi.FRAME_I420 else capi.FRAME_I420)
            p.wait()
            results.append(got)
            p.set_frame_format(fmt)                                    # waited for: allowed again
        finally:
            p.close()
    bgr, yuv = results
    assert sorted(bgr) == sorted(yuv) and len(bgr) == 3 * len(pairs) * 4
    keys = sorted(bgr)
    _same_frames("pool batches", [bgr[k] for k in keys], [yuv[k] for k in keys])


@pytest.mark.parametrize("w,h", [(749, 480), (1918, 1080), (1, 40), (40, 1), (1, 150001), (1920, 1080)])
def test_odd_and_thin_geometries(w, h):
    run = _loaded(w, h)
    _both(f"{w}x{h} chained", run(lambda c: _collect(c, c.render_many, [0.3, 0.7], chain=True)))
    _both(f"{w}x{h} phase mode", run(lambda c: _collect(c, c.render_phases, [0.0, 0.25, 0.6, 1.0])))


def test_4k_phase_frame():
    _both("3840x2160 phase frame", _loaded(3840, 2160)(lambda c: _collect(c, c.render_phases, [0.5, 0.75])))


def test_switch_back_to_bgr_and_recapture():
    """Phase-mode bodies are captured graphs: under I420 with a writer they end with the conversion.  A context that goes I420 -> BGR must give
    what a context that never switched gives, and one that renders without a writer under I420 (no conversion) and then with one must convert."""
    w, h = 320, 200
    c1, c2, g, p1, p2 = _inputs(w, h)
    ts = [0.15, 0.3, 0.45, 0.6, 0.75, 0.9]
    plain = capi.Context(0); sw = capi.Context(0)
    try:
        plain.pair_load(c1, c2, g, p1, p2); sw.pair_load(c1, c2, g, p1, p2)
        want = _collect(plain, plain.render_phases, ts)
        sw.set_frame_format(capi.FRAME_I420)
        _same_frames("I420 phase frames", want, _collect(sw, sw.render_phases, ts))
        sw.set_frame_format(capi.FRAME_BGR)
        back = _collect(sw, sw.render_phases, ts)
        assert len(back) == len(want) and all(np.array_equal(a, b) for a, b in zip(want, back)), "BGR frames after I420 differ"
        sw.set_frame_format(capi.FRAME_I420)
        sw.render_phases(ts)                                        # no writer: bodies without the conversion, frames stay in HBM
        sw.render_many(ts, chain=False)
        _same_frames("I420 after frames without a writer", want, _collect(sw, sw.render_phases, ts))
        assert np.array_equal(sw.render(0.4, 0.4), plain.render(0.4, 0.4)), "explicit-destination frames stay BGR"
        with pytest.raises(capi.PoppyError):
            sw.set_frame_format(2)
    finally:
        plain.close(); sw.close()


def test_timing_mode_marks_the_conversion():
    c1, c2, g, p1, p2 = _inputs(256, 192)
    c = capi.Context(0)
    try:
        c.pair_load(c1, c2, g, p1, p2)
        c.set_frame_format(capi.FRAME_I420)
        c.set_timing(1)
        frames = _collect(c, c.render_many, [0.2, 0.5, 0.8], chain=True)
        names = {n: k for n, _, k in c.timing_summary()}
        assert names.get("frame_format") == 3 and names.get("unsharp") == 3
        c.set_timing(0)
        assert len(frames) == 3 and frames[0].size == capi.frame_bytes(capi.FRAME_I420, 256, 192)
    finally:
        c.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
from poppy_amd import capi
import test_gpu_frame_format as T
run = T._loaded(320, 200)
T._both("render_many chained", run(lambda c: T._collect(c, c.render_many, [0.2, 0.4, 0.6, 0.8], chain=True)))
T._both("render_phases", run(lambda c: T._collect(c, c.render_phases, [0.0, 0.3, 0.5, 0.7, 1.0])))
print("child ok")
"""


def test_download_forms_in_a_child_process():
    """POPPY_HIP_DL_EVENTS=1 (one download stream + an event per copy) and POPPY_HIP_RING=1 are read once per process: a fresh child."""
    env = dict(os.environ, POPPY_HIP_DL_EVENTS="1", POPPY_HIP_RING="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
