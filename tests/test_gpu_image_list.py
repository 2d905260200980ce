"""GPU checks of the image-list path: poppy_hip_morph_list (the CLI's loop over an image list, src/poppy.cpp:266-328, in one call) and
poppy_hip_pair_begin_next (the next pair's set-up with image 1's filter chain reused).  Everything is compared bit for bit: against the real
reference's fixtures for lists of two, and against the pinned pair path — a Python loop of Context.morph with pair_corrected2 handed forward,
what the shim does — for longer lists."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import golden_util as G
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _scene(w, h, n, seed=1234):
    """n views of one synthetic scene drifting to the right and down"""
    return [synth.gen(w, h, seed, k * w // 50, k * w // 100) for k in range(n)]


def _loop(c, images, phase=-1.0):
    """the shim's loop: poppy_hip_morph(img1, img_k+1), then img1 = corrected2 -> (frame hashes per pair, distances, last pair's points, status)"""
    h, w = images[0].shape[:2]
    img1, hashes, dists, rc = images[0], [], [], 0
    for k in range(len(images) - 1):
        rc, frames, d = c.morph(img1, images[k + 1], phase=phase)
        hashes.append([_sha(f) for f in frames])
        dists.append(d)
        if rc != 0:
            break
        img1 = c.pair_corrected2(w, h)
    return hashes, dists, c.pair_points() if rc == 0 else None, rc


def _list(c, images, phase=-1.0, canvas=None):
    hashes = [[] for _ in range(len(images) - 1)]
    rc, _, dists, done = c.morph_list(images, phase=phase, canvas=canvas, write=lambda k, j, v: hashes[k].append(_sha(v)))
    return hashes, dists, c.pair_points() if rc == 0 else None, rc, done


def _same_as_loop(images, phase=-1.0, canvas=None, **settings):
    a = capi.Context(0, **settings)
    b = capi.Context(0, **settings)
    try:
        lh, ld, lp, lrc, done = _list(a, images, phase, canvas)
        ref_images = images if canvas is None else [b.blur_margin(im, *canvas) for im in images]
        rh, rd, rp, rrc = _loop(b, ref_images, phase)
        assert lrc == rrc == 0 and done == len(images) - 1
        assert lh == rh, [k for k in range(len(lh)) if lh[k] != rh[k]]
        assert ld == rd
        assert np.array_equal(lp[0], rp[0]) and np.array_equal(lp[1], rp[1])
        return a.chain_counts()
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("case,settings", [("a_256x256_chain", {}), ("a_512x512_chain30", {}), ("a_256x256_radial", {"enable_radial_mask": 1})])
def test_list_of_two_reproduces_the_reference(case, settings):
    inp = G.astage_inputs(case)
    n = int(inp["cfg"][0])
    c = capi.Context(0, number_of_frames=n, **settings)
    rc, frames, dists, done = c.morph_list([inp["img1"], inp["img2"]])
    assert rc == 0 and done == 1 and len(frames[0]) == n
    for j, f in enumerate(frames[0]):
        G.check(case, f"frame{j}", f)
    if "printedMorphDist" in G.entries(case):
        assert dists[0] == float(G.full(case, "printedMorphDist")[0])
    c.close()


def test_list_of_two_with_auto_align_hands_back_the_aligned_image():
    case = "a_256x256_align"
    inp = G.astage_inputs(case)
    n = int(inp["cfg"][0])
    c = capi.Context(0, number_of_frames=n, enable_auto_align=1)
    rc, frames, _, done = c.morph_list([inp["img1"], inp["img2"]])
    assert rc == 0 and done == 1 and len(frames[0]) == n
    for j, f in enumerate(frames[0]):
        G.check(case, f"frame{j}", f)
    h, w = inp["img1"].shape[:2]
    G.check(case, "corrected2", c.pair_corrected2(w, h))
    c.close()


def test_chained_list_256():
    run, reused = _same_as_loop(_scene(256, 256, 5), number_of_frames=6)
    assert (run, reused) == (5, 3)                   # n chains for n images, n - 2 of them reused


def test_phase_mode_list_256():
    _same_as_loop(_scene(256, 256, 4, seed=99), phase=0.37, number_of_frames=6)


def test_auto_align_list_reuses_nothing():
    run, reused = _same_as_loop(_scene(256, 256, 4, seed=7), number_of_frames=3, enable_auto_align=1)
    assert (run, reused) == (6, 0)                   # image 1 of every later pair is the ALIGNED image: its chain runs again


def test_radial_mask_list():
    _same_as_loop(_scene(256, 256, 4, seed=5), number_of_frames=3, enable_radial_mask=1)


def test_odd_widths_on_a_canvas():
    ca, cb = synth.demo_pair("cars")                 # 749 x 480
    na, nb = synth.demo_pair("numbers")              # 639 x 480
    _same_as_loop([ca, na, cb, nb], canvas=(749, 480), number_of_frames=4)


def test_1080p_list_of_four():
    run, reused = _same_as_loop(_scene(1920, 1080, 4, seed=31), number_of_frames=60)
    assert (run, reused) == (4, 2)


def _pair_state(c):
    p1, p2 = c.pair_points()
    return p1, p2, c.pair_begin_info(), c.fetch("m2"), c.fetch("gabor2")


def _assert_same_state(got, want):
    for g, w in zip(got, want):
        if isinstance(g, np.ndarray):
            assert np.array_equal(g, w)
        else:
            assert g == w


@pytest.mark.parametrize("between", ["chained", "phase_writer", "reset", "foreground"])
def test_pair_begin_next_equals_pair_begin(between):
    A, B, Cc, D = _scene(256, 256, 4, seed=4242)
    c = capi.Context(0, number_of_frames=5)
    ref = capi.Context(0, number_of_frames=5)
    try:
        c.pair_begin(A, B)
        run0, reused0 = c.chain_counts()
        if between == "chained":
            c.morph_frames(-1.0)
        elif between == "phase_writer":
            assert len(c.morph_frames(0.37)) == 1
        elif between == "reset":
            c.morph_frames(-1.0)
            c.reset()
        else:
            c.foreground(D)                          # uses a chain slot: image 1's chain must run again
        c.pair_begin_next(Cc)
        ref.pair_begin(B, Cc)
        _assert_same_state(_pair_state(c), _pair_state(ref))
        run1, reused1 = c.chain_counts()
        if between == "foreground":
            assert (run1 - run0, reused1 - reused0) == (2, 0)
        else:
            assert (run1 - run0, reused1 - reused0) == (1, 1)
        c.morph_frames(-1.0)
        c.pair_begin_next(D)                         # and once more, from the slot the last set-up left
        ref.pair_begin(Cc, D)
        _assert_same_state(_pair_state(c), _pair_state(ref))
        assert c.chain_counts()[1] == reused1 + 1
    finally:
        c.close(); ref.close()


def _to_device(img):
    hip = C.CDLL("libamdhip64.so")
    a = np.ascontiguousarray(img)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return hip, d


def test_pair_begin_next_device():
    A, B, Cc = _scene(320, 192, 3, seed=11)
    c = capi.Context(0, number_of_frames=3)
    ref = capi.Context(0, number_of_frames=3)
    hip, d = _to_device(Cc)
    try:
        c.pair_begin(A, B)
        c.pair_begin_next_device(d.value, 320, 192)
        ref.pair_begin(B, Cc)
        _assert_same_state(_pair_state(c), _pair_state(ref))
        assert c.chain_counts() == (3, 1)
    finally:
        c.close(); ref.close()
        hip.hipFree(d)


def test_device_inputs_on_a_canvas():
    """inputs_on_device with a canvas: the padding reads device memory; against host inputs on the same canvas"""
    imgs = [synth.gen(300 - 20 * k, 200 - 10 * k, 17 + k) for k in range(3)]
    devs = [_to_device(im) for im in imgs]
    c = capi.Context(0, number_of_frames=3)
    try:
        rc, got, gd, done = c.morph_list([(d.value, im.shape[1], im.shape[0]) for (_, d), im in zip(devs, imgs)], canvas=(300, 200), on_device=True)
        rc2, want, wd, done2 = c.morph_list(imgs, canvas=(300, 200))
        assert rc == rc2 == 0 and done == done2 == 2 and gd == wd
        assert all(np.array_equal(g, w) for gp, wp in zip(got, want) for g, w in zip(gp, wp))
    finally:
        c.close()
        for hip, d in devs:
            hip.hipFree(d)


def test_errors():
    imgs = _scene(256, 256, 3)
    c = capi.Context(0, number_of_frames=2)
    try:
        with pytest.raises(capi.PoppyError, match=": -6:"):
            c.morph_list(imgs, phase=0.0)
        with pytest.raises(capi.PoppyError, match=": -1:"):
            c.morph_list([imgs[0], imgs[1], synth.gen(200, 256, 3)])
        fresh = capi.Context(0, number_of_frames=2)                  # no resident pair
        with pytest.raises(capi.PoppyError, match=": -4:"):
            fresh.pair_begin_next(imgs[0])
        fresh.close()
        with pytest.raises(capi.PoppyError, match=": -1:"):
            c.pair_begin_next(synth.gen(200, 256, 3))                # the resident pair (pair 0 of the list above) is 256 x 256
        done = C.c_int(-1)
        assert capi.lib().poppy_hip_morph_list(c.h, 3, 0, 0, -1.0, 0, None, None, None, None, C.byref(done)) == -1
        rc, frames, _, done = c.morph_list(imgs[:2], phase=1.0)      # two images: poppy_hip_morph's short-circuit
        assert rc == 0 and done == 1 and len(frames[0]) == 2 and all(np.array_equal(f, imgs[1]) for f in frames[0])
    finally:
        c.close()


def test_no_match_pair_ends_the_list():
    A, B = _scene(256, 256, 2)
    grey = np.full_like(A, 77)                       # the featureless image of test_no_match_fallback
    c = capi.Context(0, number_of_frames=2)
    ref = capi.Context(0, number_of_frames=2)
    try:
        rc, frames, dists, done = c.morph_list([A, B, grey])
        assert rc == -5 and done == 1
        assert len(frames[0]) == 2 and len(frames[1]) == 2
        _, want0, d0 = ref.morph(A, B)
        rc1, want1, _ = ref.morph(ref.pair_corrected2(256, 256), grey)
        assert rc1 == -5
        assert all(np.array_equal(f, w) for f, w in zip(frames[0], want0)) and dists[0] == d0
        assert all(np.array_equal(f, w) for f, w in zip(frames[1], want1))
    finally:
        c.close(); ref.close()
