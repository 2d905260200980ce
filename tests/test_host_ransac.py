"""CPU tests of the RANSAC fundamental-matrix filter's host statement (include/poppy_hip.h: poppy_ransac_fundamental; poppy_amd/csrc/ransac_fundamental.cpp)
on the scenes of tests/ransac_util.py: planted outliers with and without noise, the reported F against numpy (its rank, and a float64 normalised 8-point
fit over the same inliers), the choice and every count against a numpy re-count in the rule's operation order, the sampler against a numpy restatement,
the degenerate scenes, the refusals and the edges of the distance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ransac_util as U
from poppy_amd import capi

E_ARG = -1
# (n_in, n_out, noise, seed).  The caps of the noisy scenes are conditions on the seeds: these meet them (asserted below, on the CPU).
NOISE_FREE = [(48, 16, 0.0, 0), (36, 24, 0.0, 1)]
NOISY = [(48, 16, 0.5, 2), (36, 24, 0.5, 3)]
# |F - F_numpy| (Frobenius, both of norm 1, the nearer sign): the largest value measured over the four scenes above is 5.63e-15
# (2.03e-15, 4.57e-15, 3.90e-15, 5.63e-15 in the order above); the bound is 100 x that.
F_BOUND = 100 * 5.63e-15


@pytest.fixture(scope="module")
def results():
    """The statement's result on every two-view scene, computed once."""
    out = {}
    for scene in NOISE_FREE + NOISY:
        p1, p2, planted = U.two_view(*scene)
        out[scene] = (p1, p2, planted, capi.ransac_fundamental(p1, p2, 3.0))
    return out


@pytest.mark.parametrize("scene", NOISE_FREE)
def test_noise_free_planted_outliers(results, scene):
    _, _, planted, r = results[scene]
    assert np.array_equal(r["inliers"].astype(bool), planted)
    assert r["n_inliers"] == planted.sum() and r["best"] >= 0


@pytest.mark.parametrize("scene", NOISY)
def test_noisy_planted_outliers(results, scene):
    _, _, planted, r = results[scene]
    kept = r["inliers"].astype(bool)
    assert not (kept & ~planted).any()
    assert (kept & planted).sum() >= 0.9 * planted.sum()
    assert r["n_inliers"] == kept.sum()


@pytest.mark.parametrize("scene", NOISE_FREE + NOISY)
def test_reported_f_against_numpy(results, scene):
    p1, p2, _, r = results[scene]
    sv = np.linalg.svd(r["f"])[1]
    print("third / first singular value", sv[2] / sv[0])
    assert sv[2] <= 1e-12 * sv[0]
    assert abs(np.linalg.norm(r["f"]) - 1) < 1e-15 * 8 and r["f"].flat[np.abs(r["f"]).argmax()] > 0
    kept = r["inliers"].astype(bool)
    want = U.eight_point(p1[kept], p2[kept])
    diff = min(np.linalg.norm(r["f"] - want), np.linalg.norm(r["f"] + want))
    print("Frobenius difference to the numpy fit", diff)
    assert diff <= F_BOUND


@pytest.mark.parametrize("scene", NOISE_FREE + NOISY)
def test_choice_and_counts(results, scene):
    p1, p2, _, r = results[scene]
    counts, valid = r["counts"], r["counts"] >= 0
    assert valid.any() and (counts[~valid] == -1).all() and not r["models"][~valid].any()
    assert r["best"] == int(np.flatnonzero(counts == counts.max())[0])
    again = U.recount(r["models"], p1, p2, 3.0)
    assert np.array_equal(again[valid], counts[valid])
    assert r["n_inliers"] == counts[r["best"]]
    assert np.array_equal(r["inliers"].astype(bool), U.inlier_matrix(r["models"][r["best"]][None], p1, p2, 3.0)[0])


@pytest.mark.parametrize("n", [8, 9, 1000])
def test_sampler(n):
    """The numpy restatement draws 8 distinct indices below n, and it is the statement's sampler: among unrelated pairs a model fits, to a ten-thousandth
    of a pixel, the 8 pairs it was solved from and no other, so every hypothesis that counts 8 there names its sample."""
    s = U.samples(n)
    assert s.shape == (capi.RANSAC_HYPOTHESES, 8) and (s >= 0).all() and (s < n).all()
    assert (np.diff(np.sort(s, axis=1), axis=1) > 0).all()
    p1, p2 = U.unrelated(n, 40 + n)
    r = capi.ransac_fundamental(p1, p2, 1e-4)
    eight = r["counts"] == 8
    assert eight.sum() >= 0.9 * capi.RANSAC_HYPOTHESES
    drawn = np.zeros((capi.RANSAC_HYPOTHESES, n), bool)
    drawn[np.arange(capi.RANSAC_HYPOTHESES)[:, None], s] = True
    assert np.array_equal(U.inlier_matrix(r["models"], p1, p2, 1e-4)[eight], drawn[eight])


def _no_model(r, n):
    return r["inliers"].all() and len(r["inliers"]) == n and not r["f"].any() and r["best"] == -1 and r["n_inliers"] == n


@pytest.mark.parametrize("name", ["identical", "copies"])
def test_degenerate_scenes_without_a_model(name):
    p1, p2 = U.degenerate()[name]
    assert _no_model(capi.ransac_fundamental(p1, p2, 3.0), len(p1))


@pytest.mark.parametrize("name", ["shift", "collinear"])
def test_degenerate_scenes_stay_finite(name):
    p1, p2 = U.degenerate()[name]
    r = capi.ransac_fundamental(p1, p2, 3.0)                        # (raises unless POPPY_OK)
    assert np.isfinite(r["f"]).all() and np.isfinite(r["models"]).all() and (r["counts"] >= -1).all() and (r["counts"] <= len(p1)).all()
    assert set(np.unique(r["inliers"])) <= {0, 1} and r["n_inliers"] == r["inliers"].sum()
    assert _no_model(r, len(p1)) or (r["best"] >= 0 and r["n_inliers"] >= 8)


def _raw_call(p1, p2, n, distance, null=None):
    inl = np.full(max(n, 1), 7, np.uint8); f = np.full(9, 7.0); counts = np.full(2048, 7, np.int32); models = np.full(2048 * 9, 7.0)
    n_in, best = C.c_int(7), C.c_int(7)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [vp(p1), vp(p2), n, distance, vp(inl), C.byref(n_in), vp(f), C.byref(best), vp(counts), vp(models)]
    if null is not None:
        args[null] = None
    rc = capi.lib().poppy_ransac_fundamental(*args)
    untouched = (inl == 7).all() and (f == 7).all() and (counts == 7).all() and (models == 7).all() and n_in.value == 7 and best.value == 7
    return rc, untouched


def test_refusals_leave_the_outputs_alone():
    big = np.zeros((65537, 2), np.float32)
    big[:] = np.random.RandomState(1).uniform(0, 1000, big.shape)
    assert _raw_call(big, big, 7, 3.0) == (E_ARG, True)
    assert _raw_call(big, big, 65537, 3.0) == (E_ARG, True)
    assert _raw_call(big, big, 64, -1.0) == (E_ARG, True)
    assert _raw_call(big, big, 64, float("nan")) == (E_ARG, True)
    assert _raw_call(big, big, 64, float("inf")) == (E_ARG, True)
    for null in (0, 1, 4, 5, 6, 7):
        assert _raw_call(big, big, 64, 3.0, null) == (E_ARG, True)
    for null in (8, 9):                                            # counts and models are optional
        assert _raw_call(big, big, 64, 3.0, null)[0] == 0


def test_distance_edges():
    p1, p2, planted = U.two_view(*NOISE_FREE[0])
    r0 = capi.ransac_fundamental(p1, p2, 0.0)
    valid = r0["counts"] >= 0
    assert np.array_equal(U.recount(r0["models"], p1, p2, 0.0)[valid], r0["counts"][valid]) and r0["counts"].max() <= len(p1)
    r9 = capi.ransac_fundamental(p1, p2, 1e9)
    valid = r9["counts"] >= 0
    assert np.array_equal(U.recount(r9["models"], p1, p2, 1e9)[valid], r9["counts"][valid])
    assert r9["best"] == int(np.flatnonzero(valid)[0]) and r9["inliers"].all() and np.isfinite(r9["f"]).all()      # a billion pixels: every pair fits every model
    assert np.array_equal(r0["models"].view(np.uint64), r9["models"].view(np.uint64))                                 # the models do not depend on the distance


def test_sizes_at_both_ends():
    for n in (8, 65536):
        p1, p2, planted = U.quarter_outliers(n, 11) if n > 8 else U.two_view(8, 0, 0.0, 11)
        r = capi.ransac_fundamental(p1, p2, 3.0)
        assert len(r["inliers"]) == n and r["n_inliers"] == r["inliers"].sum()
        if n > 8:
            assert not (r["inliers"].astype(bool) & ~planted).any() and r["n_inliers"] >= 0.9 * planted.sum()


def test_symbols_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "poppy_hip.h")).read()
    for name in ("poppy_ransac_fundamental", "poppy_hip_ransac_fundamental", "poppy_hip_pair_begin_descriptors_ransac", "poppy_hip_pair_fundamental"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert "is not provided" not in hdr
    for name, value in (("HYPOTHESES", 2048), ("MIN_POINTS", 8), ("MAX_POINTS", 65536)):
        assert re.search(r"#define POPPY_RANSAC_%s %d\b" % (name, value), hdr) and getattr(capi, "RANSAC_" + name) == value
