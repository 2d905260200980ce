"""The median kernels on content built for their edges (median_content_util.py; test_oracle_median_content.py shows on the CPU that the images reach
them): k_median_cols (kernels_median_cols.hip) and k_median_u8 (kernels_prefilter.hip) through poppy_hip_median_blur in every form, and the chained form
that Extractor::foreground's medians really run - presence maps handed from link to link, the next link's padded source written by the kernel - through
poppy_hip_foreground and the pair set-up, with poppy_hip_foreground_median_links saying which kernel every link took.  Everything is == the oracle."""
import ctypes as C
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np
import pytest

import median_content_util as M
from poppy_amd import capi

pytestmark = pytest.mark.gpu

ALL_FORMS = (0, 1, 2, 3, 4, 5, 6, 7)
ALL_LINKS = 0xffe                                                    # the eleven real links of the chain (bit 0: ksize 1, a copy)
ORDER = ["grey", "flow0", "acc0"] + [f"{s}{i}" for i in range(1, 13) for s in ("med", "flow", "acc", "blur")] + ["lin", "logged", "finalMask", "masked", "foreground"]
MED_ENV = ("POPPY_MED_COLS_FORCE", "POPPY_MED_COLS_MIN", "POPPY_MED_COLS_MIN_HARD", "POPPY_MED_COLS_ROWS")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


_images, _medians, _foregrounds = {}, {}, {}


def family_images(family):
    if family not in _images:
        _images[family] = M.FAMILIES[family]()
    return _images[family]


def oracle_median(name, img, ksize):
    """computed once per (image, ksize), shared by the tests of this module and left unchanged"""
    import oracle_lib as O
    if (name, ksize) not in _medians:
        _medians[name, ksize] = O.median_blur_u8(img, ksize)
        _medians[name, ksize].setflags(write=False)
    return _medians[name, ksize]


def oracle_foreground(name, bgr):
    import oracle_lib as O
    if name not in _foregrounds:
        _foregrounds[name] = O.foreground(bgr)
    return _foregrounds[name]


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)


# ---- every family, every form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,ksize", [(f, k) for f in sorted(M.FAMILIES) for k in M.family_ksizes(f)])
def test_family_in_every_form(ctx, family, ksize):
    """ties and extremes hold 2, 64, 65, 129, 130 and 256 values per footprint: form 2 takes the one-count form at 64 and the two-count form at 65 (form
    4: the two-count form at both), windows of ranks from 130 on; forms 5 to 7 send every image through the windows, 6 and 7 every pixel through the
    pass below / above"""
    for name, img in family_images(family).items():
        want = oracle_median(name, img, ksize)
        for form in ALL_FORMS:
            got = ctx.median_blur(img, ksize, form)
            assert np.array_equal(got, want), f"{name} ksize {ksize} form {form}: {np.count_nonzero(got != want)} pixels differ"


@pytest.mark.parametrize("ksize", range(3, 91, 2))
def test_every_odd_ksize(ctx, ksize):
    """both tails of k_median_u8's window row (3 bytes of the last dword for ksize 3, 7, 11, ..., 1 for the others) and every NDW / NW instantiation, on an
    image whose rows hold wave-uniform dwords beside mixed ones, and on noise"""
    for name, img in (("uniform_blocks_small", family_images("uniform_dwords")["uniform_blocks_small"]), ("noise_200x40", M.noise(200, 40, 5))):
        want = oracle_median(name, img, ksize)
        for form in (1, 2):
            got = ctx.median_blur(img, ksize, form)
            assert np.array_equal(got, want), f"{name} ksize {ksize} form {form}: {np.count_nonzero(got != want)} pixels differ"


@pytest.mark.parametrize("w,h,rows", [(3840, 540, 22), (5120, 700, 37)])
@pytest.mark.parametrize("ksize", [9, 89])
def test_rows_per_tile_of_the_default_geometry(ctx, w, h, rows, ksize):
    """rows != 16 as the default geometry gives them (1080p has 22, too): the bitmaps of the passes below and above and the sample rows, on content
    that needs all three windows in every tile"""
    if "POPPY_MED_COLS_ROWS" in os.environ:
        pytest.skip("the rows per tile are forced in this process")
    assert capi.median_cols_geom(w, h)[2:] == (rows, 128)
    img = M.three_windows_tiled(w, h)
    want = oracle_median(f"tiled_{w}x{h}", img, ksize)
    for form in (1, 2, 6, 7):
        got = ctx.median_blur(img, ksize, form)
        assert np.array_equal(got, want), f"{w}x{h} ksize {ksize} form {form}: {np.count_nonzero(got != want)} pixels differ"


# ---- the chained form ------------------------------------------------------------------------------------------------------------------------------
def check_chain(name, got, want):
    for key in [f"med{i}" for i in range(1, 13)] + ORDER:             # the medians first, then every stage in pipeline order
        assert same(got[key], want[key]), f"{name} {key}: {np.count_nonzero(got[key] != want[key])} elements differ"


@pytest.mark.parametrize("name", sorted(M.CHAIN_IMAGES))
def test_chain_of_medians_by_column_histograms(ctx, name):
    """Extractor::foreground on 1024 x 128 two-tone images with a patch over at most three of the host's 32 sample blocks, so that the host says "few
    values" and all eleven links take k_median_cols, each reading the presence map and the padded source that the link before it wrote.  Tiles whose
    footprint holds more than 129 values (windows of ranks), by the oracle's planes, per link from ksize 9 on:
      noise_patch 12 4 0 ...; ramp_patch 12 12 12 12 11 9 3 0 ... (hard tiles down to ksize 57); left_edge 14 14 14 14 16 14 12 10 12 10 6 (every link);
      right_edge 14 0 ...; values_130 20 0 ...; tiles of 65 to 129 values follow in every link of the noise and ramp images (noise_patch: 8 at ksize 17).
    values_64 / 65 / 129 / 130: the patch holds exactly that many values, so the first link meets footprints on either side of both limits.
    left_edge / right_edge: the patch lies on the image's side, where the x == 0 / x == W - 1 threads fill the padded source's replicated columns with
    medians that change from row to row."""
    if any(k in os.environ for k in MED_ENV):
        pytest.skip("a form of the medians is already forced in this process")
    plane = M.chain_plane(name)
    bgr = M.bgr_of(plane)
    want = oracle_foreground(name, bgr)
    assert np.array_equal(want["grey"], plane)
    assert capi.median_cols_hint(bgr) == 1
    first = M.footprint_presence(want["med1"], 9).sum(-1)             # the first real link reads the grey image (med1, the copy of ksize 1)
    second = M.footprint_presence(want["med2"], 17).sum(-1)
    if name.startswith("values_"):
        assert first.max() == int(name.split("_")[1])
    else:
        assert (first > 129).sum() >= 6 and first.max() == 256
        if name in ("noise_patch", "right_edge"):                     # the median of 9 leaves the noise on 65 to 129 values per tile
            assert ((second >= 65) & (second <= 129)).sum() >= 6
        else:                                                         # the ramp keeps windows of ranks busy for links more: still at ksize 41
            assert (second > 129).sum() >= 6 and (M.footprint_presence(want["med5"], 41).sum(-1) > 129).sum() >= 6
    got = ctx.foreground(bgr, debug=True)
    assert ctx.foreground_median_links(0) == (ALL_LINKS, capi.MEDIAN_BY_HINT)
    check_chain(name, got, want)
    assert np.array_equal(ctx.foreground(bgr), want["foreground"])   # the set-up's path (no stage planes): the same chain
    assert ctx.foreground_median_links(0) == (ALL_LINKS, capi.MEDIAN_BY_HINT)


def test_chain_on_noise_takes_the_lane_per_column_kernel(ctx):
    """and the report says so: the host sample finds no easy block, no link goes through k_median_cols"""
    if any(k in os.environ for k in MED_ENV):
        pytest.skip("a form of the medians is already forced in this process")
    bgr = M.bgr_of(M.noise(M.CHAIN_W, M.CHAIN_H, 3))
    assert capi.median_cols_hint(bgr) == 0
    got = ctx.foreground(bgr, debug=True)
    assert ctx.foreground_median_links(0) == (0, capi.MEDIAN_BY_HINT)
    check_chain("noise_full", got, oracle_foreground("noise_full", bgr))


# ---- the switches read once per process: a child each ----------------------------------------------------------------------------------------------
CHILD_CHAINS = ("ramp_patch", "right_edge", "noise_full", "small_97x61")
CHILD_FAMILY = (("ties", "ties_d64_r62"), ("ties", "ties_d130_r128"), ("extremes", "extremes_d129_top"), ("three_windows", "three_windows_low_minor"),
                ("runs", "stripes_64_at4"), ("uniform_dwords", "uniform_blocks_small"))
CHILD_KSIZES, CHILD_FORMS = (9, 89), (0, 1, 2, 6, 7)


def child_bgr(name):
    if name == "noise_full":
        return M.bgr_of(M.noise(M.CHAIN_W, M.CHAIN_H, 3))
    if name == "small_97x61":
        from poppy_amd import synth
        return synth.textured_bgr(97, 61, 2)
    return M.bgr_of(M.chain_plane(name))


def child_main(out):
    """what a child computes under its environment: the chains' median planes, final images and link reports, a few family images in a few forms"""
    res = {}
    c = capi.Context(0)
    try:
        for name in CHILD_CHAINS:
            got = c.foreground(child_bgr(name), debug=True)
            res[f"chain_{name}_meds"] = np.stack([got[f"med{i}"] for i in range(1, 13)])
            res[f"chain_{name}_foreground"] = got["foreground"]
            res[f"chain_{name}_links"] = np.array(c.foreground_median_links(0), np.int64)
        for family, name in CHILD_FAMILY:
            img = M.FAMILIES[family]()[name]
            for ksize in CHILD_KSIZES:
                for form in CHILD_FORMS:
                    res[f"median_{name}_{ksize}_{form}"] = c.median_blur(img, ksize, form)
        res["geom_chain"] = np.array(capi.median_cols_geom(M.CHAIN_W, M.CHAIN_H))
        res["geom_family"] = np.array(capi.median_cols_geom(300, 100))
    finally:
        c.close()
    np.savez(out, **res)


EASY, HARD = ("ramp_patch", "right_edge"), ("noise_full", "small_97x61")
# environment -> (links of the images the host calls easy, of the others, who decided, rows per tile at 1024 x 128 and at 300 x 100)
ENV_FORMS = {
    "force_1": ({"POPPY_MED_COLS_FORCE": "1"}, ALL_LINKS, ALL_LINKS, capi.MEDIAN_BY_ENV, 16, 16),       # the column chain on noise and at 97 x 61
    "force_0": ({"POPPY_MED_COLS_FORCE": "0"}, 0, 0, capi.MEDIAN_BY_ENV, 16, 16),
    "min_41": ({"POPPY_MED_COLS_MIN": "41"}, 0xfe0, 0, capi.MEDIAN_BY_HINT, 16, 16),                    # ksize 41 is link 5: a presence pass, then the column kernel
    "min_hard_33": ({"POPPY_MED_COLS_MIN_HARD": "33"}, ALL_LINKS, 0xff0, capi.MEDIAN_BY_HINT, 16, 16),  # hard images switch kernels at link 4, the presence map rebuilt
    "rows_17": ({"POPPY_MED_COLS_ROWS": "17"}, ALL_LINKS, 0, capi.MEDIAN_BY_HINT, 17, 17),
    "rows_31": ({"POPPY_MED_COLS_ROWS": "31"}, ALL_LINKS, 0, capi.MEDIAN_BY_HINT, 31, 31),
    "rows_128": ({"POPPY_MED_COLS_ROWS": "128"}, ALL_LINKS, 0, capi.MEDIAN_BY_HINT, 128, 100),
}


@pytest.mark.parametrize("form", sorted(ENV_FORMS))
def test_environment_forms_of_the_chain(form, tmp_path):
    if any(k in os.environ for k in MED_ENV):
        pytest.skip("a form of the medians is already forced in this process")
    env, easy_links, hard_links, by, rows_chain, rows_family = ENV_FORMS[form]
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out)
    assert z["geom_chain"][2] == rows_chain and z["geom_family"][2] == rows_family
    for name in CHILD_CHAINS:
        want = oracle_foreground(name, child_bgr(name))
        assert tuple(z[f"chain_{name}_links"]) == (easy_links if name in EASY else hard_links, by), f"{form} {name}: links {tuple(z[f'chain_{name}_links'])}"
        for i in range(12):
            assert np.array_equal(z[f"chain_{name}_meds"][i], want[f"med{i + 1}"]), f"{form} {name}: med{i + 1} differs"
        assert np.array_equal(z[f"chain_{name}_foreground"], want["foreground"]), f"{form} {name}: the final image differs"
    for family, name in CHILD_FAMILY:
        img = family_images(family)[name]
        for ksize in CHILD_KSIZES:
            for f in CHILD_FORMS:
                assert np.array_equal(z[f"median_{name}_{ksize}_{f}"], oracle_median(name, img, ksize)), f"{form}: {name} ksize {ksize} form {f}"


# ---- the device decides ----------------------------------------------------------------------------------------------------------------------------
def _to_device(img):
    hip = C.CDLL("libamdhip64.so")
    a = np.ascontiguousarray(img)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return hip, d


def _setup_state(c):
    nf, det = c.pair_begin_info()
    p1, p2 = c.pair_points()
    return nf, tuple(det), p1, p2


def _values_per_tile(hard_tiles, easy_values, hard_values):
    v = [easy_values] * 64
    for k in range(hard_tiles):
        v[(k * 9 + 4) % 64] = hard_values                           # spread over the image
    return v


@pytest.mark.parametrize("easy_values,hard_values", [(24, 25), (8, 256)], ids=["24_against_25_values", "58_against_57_tiles"])
def test_device_decided_route_at_its_thresholds(easy_values, hard_values):
    """A pair from device memory brings no host pixels: each image's chain counts its own tiles of at most 24 values (k_median_presence) and takes the
    column kernel when they are nine tenths of the 64 tiles - 58 are, 57 are not.  Image 1 has 58 tiles of `easy_values` values and 6 of `hard_values`,
    image 2 has 57 and 7: with 24 against 25 values the two images differ in ONE value of one tile."""
    if any(k in os.environ for k in MED_ENV):
        pytest.skip("a form of the medians is already forced in this process")
    planes = [M.tiles_plane(_values_per_tile(n, easy_values, hard_values), seed=n) for n in (6, 7)]
    for p, n in zip(planes, (58, 57)):
        assert int((M.tile_presence(p).sum(-1) <= 24).sum()) == n and M.tile_presence(p).shape[:2] == (8, 8)
    a, b = (M.bgr_of(p) for p in planes)
    c = capi.Context(0, number_of_frames=2)
    try:
        c.pair_begin(a, b)
        want = _setup_state(c)
    finally:
        c.close()
    c = capi.Context(0, number_of_frames=2)
    try:
        (hip, da), (_, db) = _to_device(a), _to_device(b)
        try:
            c.pair_begin_device(da.value, db.value, M.CHAIN_W, M.CHAIN_H)
        finally:
            hip.hipFree(da); hip.hipFree(db)
        assert c.foreground_median_links(0) == (ALL_LINKS, capi.MEDIAN_BY_DEVICE)
        assert c.foreground_median_links(1) == (0, capi.MEDIAN_BY_DEVICE)
        got = _setup_state(c)
    finally:
        c.close()
    assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert len(got[2]) > 4                                            # (no empty set-up)


if __name__ == "__main__":
    child_main(sys.argv[1])
