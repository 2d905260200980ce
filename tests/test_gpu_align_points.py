"""The auto-align scoring kernel (k_candidate_scores) and k_warp_affine on inputs built to reach their branches
(tests/align_points_util.py; tests/test_oracle_align_points.py asserts on the CPU that they do): every length around the
wave size up to the LDS limit of 4096 points, ties among equally near points, pairs that share their distance, exact
duplicates, the (-1, -1) marker and its near misses, 1 to 1080 candidates, coordinates up to +-1e6, walks of the translation
search past its first, second and third scoring call, and one-pixel-thin images.  Everything is compared with `==` against the
oracle: doubles by value, floats by bits.  NaN and infinities are not pinned.

Measured wall time on an MI355X, library call alone: the n = 4096 row of the scores takes 74 ms with its two candidates (73 ms
with one: the waves run side by side, the time is one wave's serial claim loop and addition chain), retranslate at n = 4096
(101 candidates, then one) 150 ms, reprocrustes (one candidate) 73 ms, the 1080 candidates at n = 70 1.4 ms.  With the oracle's
share every test of this file stays under 0.4 s, the whole file under 3 s."""
import ctypes as C

import numpy as np
import pytest

import align_points_util as U
import oracle_lib as O
from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu
E_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def image():
    return synth.textured_bgr(U.W, U.H, 5)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("family,label", [(f, l) for f, l, _ in U.score_cases()])
def test_scores_vs_oracle(ctx, family, label):
    build = next(b for f, l, b in U.score_cases() if (f, l) == (family, label))
    w, h, p1, sets = build()
    want_d, want_total, want_pairs, want_inner = U.oracle_scores(family, label)
    d, total, n_pairs, inner = ctx.align_scores(p1, sets, w, h)
    for a in range(len(sets)):
        where = f"{family} {label}: n = {len(p1)}, candidate {a} of {len(sets)}"
        assert n_pairs[a] == want_pairs[a], f"{where}: pair count {n_pairs[a]}, oracle {want_pairs[a]}"
        assert _bits(total)[a] == _bits(want_total)[a], f"{where}: float total {total[a]!r}, oracle {want_total[a]!r}"
        assert _bits(inner)[a] == _bits(want_inner)[a], f"{where}: raw offset sum {inner[a]!r}, oracle {want_inner[a]!r}"
        assert d[a] == want_d[a], f"{where}: morph distance {d[a]!r}, oracle {want_d[a]!r}"


def test_scores_outputs_are_optional(ctx):
    """Every output pointer may be NULL; the others are written as in the full call."""
    w, h, p1, sets = U.lengths(65)
    full = ctx.align_scores(p1, sets, w, h)
    L = capi.lib()
    for keep in range(4):
        outs = [np.zeros(len(sets), t) for t in (np.float64, np.float32, np.int32, np.float32)]
        args = [o.ctypes.data_as(C.c_void_p) if k == keep else None for k, o in enumerate(outs)]
        assert L.poppy_hip_align_scores(ctx.h, p1.ctypes.data_as(C.c_void_p), sets.ctypes.data_as(C.c_void_p), len(p1), len(sets), w, h, *args) == 0
        assert outs[keep].tobytes() == full[keep].tobytes()


def _check_step(ctx, image, step, p1, p2, where):
    want_img, want_p2, want_d = O.align_step(step, image, p1, p2)
    img, got_p2, d = ctx.align(step, image, p1, p2)
    assert np.array_equal(_bits(got_p2), _bits(want_p2)), f"{where}: points"
    assert d == want_d, f"{where}: distance {d!r}, oracle {want_d!r}"
    assert np.array_equal(img, want_img), f"{where}: image"
    return want_p2


@pytest.mark.parametrize("n", sorted(U.STEP_SETS))
@pytest.mark.parametrize("step", ["retranslate", "reprocrustes", "rerotate"])
def test_steps_on_tie_sets_vs_oracle(ctx, image, step, n):
    w, h, p1, p2 = U.step_set(n)
    _check_step(ctx, image, step, p1, p2, f"{step} on the ties set cut to n = {n}")


@pytest.mark.parametrize("step", ["retranslate", "reprocrustes"])
def test_steps_at_the_point_limit_vs_oracle(ctx, image, step):
    """n = 4096: 64 KiB of LDS per wave, 101 candidates in the translation search.  (rerotate is left at n <= 257: the oracle needs
    about 90 s for its 1080 candidates at 4096.)"""
    w, h, p1, sets = U.lengths(U.MAX_POINTS)
    _check_step(ctx, image, step, p1, sets[0], f"{step} at n = {U.MAX_POINTS}")


@pytest.mark.parametrize("name", [c[0] for c in U.WALKS])
def test_long_walks_vs_oracle(ctx, image, name):
    w, h, p1, p2 = U.walk(name)
    move = next(c[5] for c in U.WALKS if c[0] == name)
    after = _check_step(ctx, image, "retranslate", p1, p2, f"walk {name}")
    assert U.walk_steps(p2, after) == move and max(map(abs, move)) > 12


@pytest.mark.parametrize("kind", ["shifted", "rotated"])
def test_auto_align_vs_oracle(ctx, image, kind):
    w, h, p1, p2 = U.auto_set(kind)
    want_img, want_p2, want_d = O.align_step("auto", image, p1, p2)
    assert want_d < 1e-5 < O.morph_distance(p1, p2, w, h)          # the search finds its way back
    img, got_p2, d = ctx.align("auto", image, p1, p2)
    assert np.array_equal(_bits(got_p2), _bits(want_p2)), f"auto on the {kind} set: points"
    assert d == want_d, f"auto on the {kind} set: distance {d!r}, oracle {want_d!r}"
    assert np.array_equal(img, want_img), f"auto on the {kind} set: image"


def test_point_count_limits(ctx, image):
    """4096 point pairs are taken, 4097 and 3 are POPPY_E_ARG with the range in the message, and the context goes on working."""
    L = capi.lib()
    rng = np.random.default_rng(7)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    d = C.c_double(0)

    def step(n):
        img = image.copy()
        p1 = U._random_points(rng, n); p2 = p1[::-1].copy()
        return L.poppy_hip_align_step(ctx.h, 1, vp(img), U.W * 3, U.W, U.H, vp(p1), vp(p2), n, C.byref(d))

    def scores(n):
        p1 = U._random_points(rng, n); sets = p1[::-1].copy()
        out = np.zeros(1, np.float64)
        return L.poppy_hip_align_scores(ctx.h, vp(p1), vp(sets), n, 1, U.W, U.H, vp(out), None, None, None)

    for entry in (step, scores):
        assert entry(U.MAX_POINTS) == 0, L.poppy_hip_last_error(ctx.h)
        for n in (U.MAX_POINTS + 1, 3):
            assert entry(n) == E_ARG and b"4 .. 4096" in L.poppy_hip_last_error(ctx.h), (entry.__name__, n)
            assert entry(64) == 0, L.poppy_hip_last_error(ctx.h)              # the next valid call on the same context
    w, h, p1, sets = U.lengths(64)
    assert ctx.align_scores(p1, sets, w, h)[0].tobytes() == U.oracle_scores("lengths", "n64")[0].tobytes()


@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("w", [1, 255, 256, 257])
def test_warp_affine_sizes_vs_oracle(ctx, w, h):
    """Widths on both sides of the 256-thread block and one-pixel-thin images: identity, whole and 1/32-pixel translations, a rotation."""
    img = np.random.default_rng(100 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    maps = [[1, 0, 0, 0, 1, 0], [1, 0, -1, 0, 1, 0], [1, 0, w - 1, 0, 1, 0], [1, 0, 1 / 32, 0, 1, 0], [1, 0, 0, 0, 1, 1 / 32],
            [1, 0, -1 / 32, 0, 1, -1 / 32], O.rotation_matrix(np.float32(w / 2), np.float32(h / 2), 3.0).reshape(6)]
    assert np.array_equal(O.warp_affine(img, maps[0]), img)
    for M in maps:
        assert np.array_equal(ctx.warp_affine(img, M), O.warp_affine(img, M)), (w, h, list(M))
