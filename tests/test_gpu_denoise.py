"""GPU tests of the non-local-means denoise (include/poppy_hip.h: poppy_hip_denoise, poppy_hip_denoise_device, poppy_hip_set_denoise): the kernel against
the host statement poppy_bgr_denoise, which defines the rule (tests/test_host_denoise.py pins that statement to a numpy restatement), on the families of
tests/denoise_util.py — sizes at which every index folds, the kernel's tile edges (read from poppy_denoise_tile, not copied), flat, saturated, noisy,
cut-off and half-tie contents, every window pair, and strengths on each side of the bound at which the weight table leaves LDS for global memory — then
the device entry point, the refusals, and poppy_hip_morph_list with the setting on against the same list denoised beforehand.  Every comparison is ==."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import denoise_util as U
from poppy_amd import capi, synth
from test_host_denoise import REFUSALS, refusal_arguments

pytestmark = pytest.mark.gpu

BOUND_HS = U.bound_strengths(lambda hs, tw, sw: capi.denoise_weights(hs, tw, sw)["L"], capi.denoise_table_bound())
CASES = U.cases(capi.denoise_tile(), BOUND_HS)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, number_of_frames=3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name,img,params", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_host_statement(ctx, name, img, params):
    assert np.array_equal(ctx.denoise(img, *params), capi.bgr_denoise(img, *params))


def test_the_table_takes_both_forms():
    bound = capi.denoise_table_bound()
    lengths = [capi.denoise_weights(*p)["L"] for _, _, p in CASES]
    assert min(lengths) <= bound < max(lengths) and capi.denoise_weights(*U.PARAMS[-1])["L"] == 149355
    lo, hi = (capi.denoise_weights(hs, 7, 21)["L"] for hs in BOUND_HS)
    assert lo <= bound < hi and hi - lo < 64


def test_rows_with_padding(ctx):
    img = U.gaussian_noise(capi.denoise_tile()[0] + 3, 19, seed=9)
    want = capi.bgr_denoise(img, *U.DEFAULT)
    assert np.array_equal(ctx.denoise(img, *U.DEFAULT, row_pad=5, dst_pad=7), want)           # raises if dst's padding was written
    assert np.array_equal(ctx.denoise(img, *U.DEFAULT, row_pad=1), want)


def _device(hip, nbytes, fill=None):
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(nbytes)) == 0
    if fill is not None:
        a = np.ascontiguousarray(fill)
        assert a.nbytes == nbytes and hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), 1) == 0
    return d


def _fetch(hip, d, shape):
    out = np.empty(shape, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d, C.c_size_t(out.nbytes), 2) == 0
    return out


@pytest.mark.parametrize("params", [U.DEFAULT, (10.0, 3, 3), U.PARAMS[-1]])
def test_device_entry_point(ctx, hip, params):
    w, h = capi.denoise_tile()[0] + 5, 37
    img = U.gaussian_noise(w, h, seed=77)
    d_src, d_dst = _device(hip, img.nbytes, img), _device(hip, img.nbytes, np.full_like(img, 0xA5))
    try:
        ctx.denoise_device(d_src.value, d_dst.value, w, h, *params)
        ctx.sync()
        assert np.array_equal(_fetch(hip, d_dst, img.shape), capi.bgr_denoise(img, *params))
        assert np.array_equal(_fetch(hip, d_src, img.shape), img)
        with pytest.raises(capi.PoppyError, match=": -1:"):
            ctx.denoise_device(d_src.value, d_src.value, w, h, *params)
    finally:
        hip.hipFree(d_src); hip.hipFree(d_dst)


@pytest.mark.parametrize("name,change,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_dst_untouched(ctx, name, change, status):
    args, dst, _src = refusal_arguments(change)
    assert capi.lib().poppy_hip_denoise(ctx.h, *args) == status
    assert (dst == 0xA5).all()
    if "hs" in change or "tw" in change or "sw" in change:
        before = ctx.get_denoise()
        assert capi.lib().poppy_hip_set_denoise(ctx.h, args[4], args[5], args[6]) == (0 if args[4] == 0.0 else status)
        assert ctx.get_denoise() == before == (0.0, 0, 0)


def test_device_refusals_launch_nothing(ctx, hip):
    img = U.gaussian_noise(8, 6)
    d_src, d_dst = _device(hip, img.nbytes, img), _device(hip, img.nbytes, np.full_like(img, 0xA5))
    try:
        L = capi.lib()
        for args, status in [((None, d_dst.value, 8, 6, 10.0, 7, 21), -1), ((d_src.value, None, 8, 6, 10.0, 7, 21), -1), ((d_src.value, d_dst.value, 0, 6, 10.0, 7, 21), -1),
                             ((d_src.value, d_dst.value, 8, 6, 0.0, 7, 21), -1), ((d_src.value, d_dst.value, 8, 6, 10.0, 4, 21), -1),
                             ((d_src.value, d_dst.value, 8, 6, 10.0, 9, 21), -6), ((d_src.value, d_dst.value, 8, 6, 10.0, 7, 23), -6)]:
            assert L.poppy_hip_denoise_device(ctx.h, *args) == status
        ctx.sync()
        assert (_fetch(hip, d_dst, img.shape) == 0xA5).all()
    finally:
        hip.hipFree(d_src); hip.hipFree(d_dst)


# ---- the list -------------------------------------------------------------------------------------------------------------------------------------------

LW, LH, LIST_PARAMS = 96, 64, (10.0, 7, 21)


def _list_images(w=LW, h=LH):
    """three views of one drifting synthetic scene under noise of sigma 6"""
    out = []
    for k in range(3):
        noise = np.rint(6.0 * np.random.RandomState(50 + k).randn(h, w, 3))
        out.append(np.clip(synth.gen(w, h, 1234, 2 * k, k).astype(np.float64) + noise, 0, 255).astype(np.uint8))
    return out


def _run_list(c, images, **kw):
    hashes = [[] for _ in range(len(images) - 1)]
    rc, _, dists, done = c.morph_list(images, write=lambda k, j, v: hashes[k].append(_sha(v)), **kw)
    return rc, done, hashes, dists, c.pair_points() if rc == 0 else None


def _same(got, want):
    assert got[:4] == want[:4]
    assert (got[4] is None) == (want[4] is None)
    if got[4] is not None:
        assert np.array_equal(got[4][0], want[4][0]) and np.array_equal(got[4][1], want[4][1])


@pytest.fixture(scope="module")
def list_pair():
    """(a context with the setting on, a context with it off, the images, the images denoised by the host statement)"""
    on, off = capi.Context(0, number_of_frames=3), capi.Context(0, number_of_frames=3)
    on.set_denoise(*LIST_PARAMS)
    images = _list_images()
    yield on, off, images, [capi.bgr_denoise(im, *LIST_PARAMS) for im in images]
    on.close(); off.close()


@pytest.mark.parametrize("canvas", [None, (LW + 24, LH + 12)], ids=["one_size", "canvas"])
def test_list_denoises_every_image(list_pair, canvas):
    on, off, images, denoised = list_pair
    before = [im.copy() for im in images]
    assert on.get_denoise() == LIST_PARAMS and off.get_denoise() == (0.0, 0, 0)
    counts_on, counts_off = on.chain_counts(), off.chain_counts()
    got = _run_list(on, images, canvas=canvas)
    want = _run_list(off, denoised, canvas=canvas)
    assert got[0] == 0 and got[1] == 2 and len(got[2][0]) == 3
    _same(got, want)
    ran_on, ran_off = [tuple(b - a for a, b in zip(c0, c.chain_counts())) for c0, c in ((counts_on, on), (counts_off, off))]
    assert ran_on == ran_off == (3, 1)                           # each image's filter chain once, with and without the setting
    assert _run_list(off, images, canvas=canvas)[2] != got[2]    # the setting is not a no-op on these images
    assert all(np.array_equal(a, b) for a, b in zip(images, before))


@pytest.mark.parametrize("canvas", [None, (LW + 24, LH + 12)], ids=["one_size", "canvas"])
def test_list_denoises_device_images(list_pair, hip, canvas):
    on, off, images, denoised = list_pair
    devs = [_device(hip, im.nbytes, im) for im in images]
    try:
        got = _run_list(on, [(d.value, LW, LH) for d in devs], on_device=True, canvas=canvas)
        _same(got, _run_list(off, denoised, canvas=canvas))
        assert got[0] == 0
        assert all(np.array_equal(_fetch(hip, d, im.shape), im) for d, im in zip(devs, images))      # the source's buffers are never written
    finally:
        for d in devs:
            hip.hipFree(d)


def test_images_of_different_sizes_are_denoised_at_their_own_size(list_pair):
    on, off, _, _ = list_pair
    images = [im[:LH - 6 * k, :LW - 10 * k].copy() for k, im in enumerate(_list_images())]
    got = _run_list(on, images, canvas=(LW + 8, LH + 8))
    _same(got, _run_list(off, [capi.bgr_denoise(im, *LIST_PARAMS) for im in images], canvas=(LW + 8, LH + 8)))
    assert got[0] == 0


def test_switching_the_setting_off_restores_the_plain_list(list_pair):
    on, off, images, _ = list_pair
    c = capi.Context(0, number_of_frames=3)
    try:
        c.set_denoise(*LIST_PARAMS)
        first = _run_list(c, images)
        with pytest.raises(capi.PoppyError, match=": -6:"):
            c.set_denoise(10.0, 9, 21)
        with pytest.raises(capi.PoppyError, match=": -1:"):
            c.set_denoise(-1.0, 7, 21)
        assert c.get_denoise() == LIST_PARAMS
        c.set_denoise(0)
        assert c.get_denoise() == (0.0, 0, 0)
        plain = _run_list(c, images)
        _same(plain, _run_list(off, images))
        assert plain[2] != first[2]
    finally:
        c.close()


def test_morph_is_not_affected_and_the_context_stays_usable(list_pair):
    """poppy_hip_morph with the setting ON, on the context every refusal above went through: exactly the plain pair's frames"""
    on, off, images, _ = list_pair
    for args, _dst, _src in (refusal_arguments(r[1]) for r in REFUSALS):
        assert capi.lib().poppy_hip_denoise(on.h, *args) < 0
    rc, frames, dist = on.morph(images[0], images[1])
    rc2, want, dist2 = off.morph(images[0], images[1])
    assert rc == rc2 == 0 and dist == dist2 and len(frames) == 3
    assert all(np.array_equal(f, w) for f, w in zip(frames, want))
