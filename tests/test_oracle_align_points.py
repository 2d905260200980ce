"""The point-set families of tests/align_points_util.py reach what they are built for — asserted from the oracle and a plain
numpy restatement of the greedy claim alone, without the GPU.  These are conditions on the inputs, not measurements: a family
that stops meeting them no longer tests the branch of k_candidate_scores it is named after."""
import numpy as np
import pytest

import align_points_util as U
import oracle_lib as O
from poppy_amd import synth


def test_lengths_reach_the_wave_size_and_the_limit():
    rest = {n % 64 for n in U.LENGTHS}
    assert {0, 1, 63} <= rest
    assert U.MAX_POINTS in U.LENGTHS and U.MAX_POINTS - 1 in U.LENGTHS and max(U.LENGTHS) == U.MAX_POINTS
    assert sum(n >= 3 * 64 for n in U.LENGTHS) >= 3                 # more than two full blocks
    for n in U.LENGTHS:
        w, h, p1, sets = U.lengths(n)
        assert p1.shape == (n, 2) and sets.shape == (2 if n >= 4095 else 3, n, 2) and p1.dtype == sets.dtype == np.float32
        assert (p1 != np.rint(p1)).all() and (sets != np.rint(sets)).mean() > 0.999


@pytest.mark.parametrize("n,span,seed", U.TIES)
def test_ties_decide_claims_and_the_order_of_the_sum(n, span, seed):
    w, h, p1, sets = U.ties(n, span, seed)
    dist, tie_decided = U.greedy_claims(p1, sets[0])
    ascending, in_list_order, descending, shared = U.claim_totals(dist)
    total, n_pairs, _ = O.morph_distance_parts(p1, sets[0])
    assert n_pairs == n and (dist >= 0).all()
    assert total.tobytes() == ascending.tobytes()                  # the restatement is the oracle's pairing and its order
    assert tie_decided >= 10
    assert ascending != in_list_order and ascending != descending
    assert shared >= 50


def test_duplicates_are_exact():
    w, h, p1, sets = U.duplicates()
    total, n_pairs, _ = O.morph_distance_parts(p1, sets[0])
    assert total == 0 and n_pairs == len(p1)                        # p2 == p1
    total, n_pairs, _ = O.morph_distance_parts(p1, sets[1])
    assert n_pairs == len(p1) and sorted(map(tuple, sets[1])) == sorted(map(tuple, p1)) and not np.array_equal(sets[1], p1)
    assert len({tuple(p) for p in sets[2]}) == len(p1) - 20         # ten twins, one point eleven times
    assert U.greedy_claims(p1, sets[2])[1] >= 10                    # equal points are equally near


def test_tombstones_pair_with_nothing_and_near_misses_pair():
    w, h, p1, sets = U.tombstones()
    n = U.TOMBSTONE_N
    assert len(sets) == len(U.TOMBSTONE_M) == 10 and sorted(set(U.TOMBSTONE_M)) == [0, 1, 3, n - 1]
    assert (p1 == -1).all(1).sum() == 1
    for a, m in enumerate(U.TOMBSTONE_M):
        assert (sets[a] == -1).all(1).sum() == m
        total, n_pairs, _ = O.morph_distance_parts(p1, sets[a])
        assert n_pairs == n - m, (a, m)
        dist, _ = U.greedy_claims(p1, sets[a])
        assert (dist < 0).sum() == m and np.isfinite(total)
    near = sets[-1]
    assert ((near == -1).any(1) & ~(near == -1).all(1)).sum() >= 6 and (np.abs(near + 1) < 1e-6).all(1).sum() == 4


@pytest.mark.parametrize("k", U.CANDIDATE_COUNTS)
def test_candidates_all_differ(k):
    w, h, p1, sets = U.candidate_counts(k)
    assert sets.shape == (k, 70, 2)
    d, total, n_pairs, inner = U.oracle_scores("candidates", f"k{k}")
    assert (n_pairs == 70).all() and len(set(d)) == k               # a mix-up of two candidates changes a result
    assert len({t.tobytes() for t in total}) > k * 0.99 and len({t.tobytes() for t in inner}) > k * 0.9


def test_magnitudes_round_and_stay_finite():
    for label, build in (("near", U.magnitudes_near), ("far", U.magnitudes_far)):
        w, h, p1, sets = build()
        d, total, n_pairs, inner = U.oracle_scores("magnitudes", label)
        assert np.isfinite(d).all() and np.isfinite(total).all() and np.isfinite(inner).all() and (n_pairs == len(p1)).all()
        assert (sets < 0).any() and np.abs(sets).max() > 9e5
    w, h, p1, sets = U.magnitudes_far()
    exact = sets[0][:, 0].astype(np.float64) - p1[:, 0].astype(np.float64)
    assert (exact != (sets[0][:, 0] - p1[:, 0]).astype(np.float64)).any()      # the float differences round


def test_no_family_pins_nan():
    for family, label, build in U.score_cases():
        d, total, n_pairs, inner = U.oracle_scores(family, label)
        assert np.isfinite(d).all() and (n_pairs > 0).all(), (family, label)


@pytest.fixture(scope="module")
def walked():
    img = synth.textured_bgr(U.W, U.H, 5)
    out = {}
    for name, *_ in U.WALKS:
        w, h, p1, p2 = U.walk(name)
        out[name] = (p1, p2, O.align_step("retranslate", img, p1, p2)[1])
    return out


def test_long_walks_pass_the_first_scoring_call(walked):
    longest = 0
    for name, n, seed, shift, extra, move in U.WALKS:
        p1, p2, after = walked[name]
        steps = U.walk_steps(p2, after)
        assert steps == move, name
        assert max(abs(steps[0]), abs(steps[1])) > 12, name
        longest = max(longest, abs(steps[0]), abs(steps[1]))
    assert longest > 24
    moves = {name: move for name, *_, move in U.WALKS}
    assert any(m[1] == 0 for m in moves.values()) and any(m[0] == 0 for m in moves.values()) and any(m[0] and m[1] for m in moves.values())


@pytest.mark.parametrize("name,marker_step", [("origin", 30), ("origin_stop", 21)])
def test_walks_towards_the_origin_cross_the_marker(walked, name, marker_step):
    p1, p2, after = walked[name]
    k = marker_step - 1
    assert k > 12 and (p2 == k).all(1).sum() == 1                   # p2 holds (k, k)
    along = U.walk_candidates(p2, U.walk_steps(p2, after))
    counts = [O.morph_distance_parts(p1, s)[1] for s in along]
    assert counts[marker_step - 1] == len(p1) - 1 and counts.count(len(p1)) == len(counts) - 1
    assert len(along) >= marker_step
