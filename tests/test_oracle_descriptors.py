"""The describe and Hamming families of tests/descriptor_util.py reach what they are built for — asserted from the oracle and the plain
numpy restatements alone, without the GPU.  These are conditions on the inputs, not measurements: a family that stops meeting them no
longer tests the branch of k_orb_blur, k_orb_describe, k_hamming or k_hamming_knn2 it is named after.  Each switch of the restatement
(rounding="half_up", contract=1|2, strict=False) is a kernel error stated in numpy; that it changes its family's descriptors is the
evidence that the GPU comparison of tests/test_gpu_descriptors.py would catch that error.  NaN and infinite angles and coordinates are
not pinned."""
import numpy as np
import pytest

import descriptor_util as U
import oracle_lib as O
from poppy_amd import capi

DESCRIBE_FAMILIES = [f for f, _ in U.describe_cases()] + ["level_subsets"]


def _cases(family):
    return U.level_subsets() if family == "level_subsets" else dict(U.describe_cases())[family]()


@pytest.mark.parametrize("family", DESCRIBE_FAMILIES)
def test_oracle_equals_the_numpy_restatement_at_octave_0(family):
    octave0 = 0
    for label, img, kps in _cases(family):
        h, w = img.shape
        assert U.accepted(kps, w, h).all(), label
        rows = U.level0_rows(kps)
        octave0 += len(rows)
        want = U.describe_level0(img, kps[rows])
        got = U.oracle_describe(family)[label]
        assert got.shape == (len(kps), 32)
        assert np.array_equal(got[rows], want), f"{label}: rows {rows[(got[rows] != want).any(1)].tolist()} differ"
    assert octave0 > 0 or family == "counts0"


def test_half_ties_tie_where_they_claim():
    for angle, (ties, moved) in U.TIE_ANGLES.items():
        assert U.half_tie_count(np.float32(angle)) == (ties, moved) and moved > 0
    for angle in U.CONTRAST_ANGLES:
        assert U.half_tie_count(np.float32(angle)) == (0, 0)
    (label, img, kps), = U.half_ties()
    assert set(kps[:, 5].astype(int)) == set(range(U.LEVELS))
    rows = U.level0_rows(kps)
    plain = U.describe_level0(img, kps[rows])
    half_up = U.describe_level0(img, kps[rows], rounding="half_up")
    tied = np.isin(kps[rows, 3], np.array(list(U.TIE_ANGLES), np.float32))
    assert tied.sum() == len(U.TIE_ANGLES) * len(U.INTERIOR)
    assert (plain[tied] != half_up[tied]).any(1).all()               # round-half-up is seen in every row at 30 degrees
    assert np.array_equal(plain[~tied], half_up[~tied])               # and nowhere else: the contrast rows have no tie to move


def test_contraction_rows_see_a_fused_product():
    (label, img, kps), = U.contraction()
    assert len(kps) == len(U.CONTRACTION_ROWS) >= 16
    plain = U.describe_level0(img, kps)
    fused = {c: (U.describe_level0(img, kps, contract=c) != plain).any(1) for c in (1, 2)}
    assert (fused[1] | fused[2]).all()                                # every committed row qualifies
    assert fused[1].sum() >= 4 and fused[2].sum() >= 4
    for i, (angle, x, y, forms) in enumerate(U.CONTRACTION_ROWS):
        assert all(fused[c][i] for c in forms), (angle, forms)
        assert any((u != v).any() for c in forms for u, v in zip(U.offsets(np.float32(angle)), U.offsets(np.float32(angle), contract=c)))
    rng = np.random.default_rng(3)                                    # random angles do not: none of 2000 moves a coordinate
    for angle in rng.uniform(0, 360, 2000).astype(np.float32):
        p = U.offsets(angle)
        assert all(np.array_equal(u, v) for c in (1, 2) for u, v in zip(p, U.offsets(angle, contract=c)))


def test_flat_and_two_valued_rows_see_the_strict_compare():
    flat = two = 0
    for label, img, kps in U.flat_and_two_valued():
        rows = U.level0_rows(kps)
        oracle = U.oracle_describe("flat_and_two_valued")[label]
        loose = U.describe_level0(img, kps[rows], strict=False)
        assert len(np.unique(img)) == (1 if label.startswith("flat") else 2)
        if label.startswith("flat"):
            flat += 1
            assert (oracle == 0).all()                                # every octave, the positions in the ring included
            assert (loose == 255).all()
        else:
            two += 1
            assert (oracle[rows] != loose).any(1).all()
            assert oracle[rows].any(1).all()                          # and the rows are not empty either
    assert flat == 3 and two == 2


def test_border_rows_read_the_ring_and_many_reflections():
    for (label, img, kps), (w, h) in zip(U.border(), ((U.W, U.H), (U.SMALL_W, U.SMALL_H))):
        assert img.shape == (h, w)
        rows, labels = U.border_rows(w, h)
        assert np.array_equal(rows, kps)
        labels = np.array(labels)
        ring = U.reads_ring(kps, w, h)
        assert (ring[labels != "half"] > 0).all() and (ring > 0).sum() >= len(kps) - 4
        assert (labels == "corner").sum() == 4 * U.LEVELS and (labels == "edge").sum() == 4 * U.LEVELS + 2
        cx, cy = U.level_position(kps, w, h)
        lw = np.array([U.levels(w, h)[int(o)][0] for o in kps[:, 5]]); lh = np.array([U.levels(w, h)[int(o)][1] for o in kps[:, 5]])
        edge = labels == "edge"
        for o in range(U.LEVELS):                                     # both ends of the accepted range on both axes, at every octave
            at = edge & (kps[:, 5] == o)
            assert (cx[at] == U.ACCEPT_LO).any() and (cx[at] == lw[at] + U.ACCEPT_PAST - 1).any()
            assert (cy[at] == U.ACCEPT_LO).any() and (cy[at] == lh[at] + U.ACCEPT_PAST - 1).any()
        half = kps[labels == "half"]
        assert (half[:, :2] % 1 == 0.5).all()
        below = np.floor(half[:, :2]).astype(int) % 2
        assert {tuple(b) for b in below} == {(0, 0), (0, 1), (1, 0), (1, 1)}       # k + 0.5 for even and odd k on both axes
    assert U.levels(U.SMALL_W, U.SMALL_H)[7][:2] == (6, 4)
    kps, labels = U.border_rows(U.SMALL_W, U.SMALL_H)
    far = U.reads_past_one_reflection(kps, U.SMALL_W, U.SMALL_H)
    assert (far[np.array(labels) != "half"] > 0).all()                # every corner and edge row of the 20 x 16 image


def test_refused_rows_lie_one_past_the_accepted_range():
    for what, row in U.refused_rows():
        if 0 <= row[5] < U.LEVELS:
            assert not U.accepted([row], U.W, U.H)[0], what
            cx, cy = U.level_position([row], U.W, U.H)
            lw, lh = U.levels(U.W, U.H)[int(row[5])][:2]
            assert sum([cx[0] == U.ACCEPT_LO - 1, cx[0] == lw + U.ACCEPT_PAST, cy[0] == U.ACCEPT_LO - 1, cy[0] == lh + U.ACCEPT_PAST]) == 1, what


def test_counts_and_level_subsets():
    assert {1, 7, 8, 9} <= set(U.COUNTS) and U.KP_CAP in U.COUNTS and max(U.COUNTS) == U.KP_CAP + 1       # 8 keypoints per block
    k = U.random_keypoints(U.KP_CAP + 1)
    assert set(k[:, 5].astype(int)) == set(range(U.LEVELS)) and (k[:, 0] < 0).any() and (k[:, 1] > U.H).any()
    (_, a, ka), (_, b, k0), (_, b2, k7) = U.level_subsets()
    assert b is b2 and not np.array_equal(a, b)
    assert set(ka[:, 5].astype(int)) == set(range(U.LEVELS)) and (k0[:, 5] == 0).all() and (k7[:, 5] == 7).all() and len(k0) > 8 < len(k7)
    stale = O.orb_describe(a, k7)                                     # image A's level 7 under B's keypoints: a stale atlas shows
    assert not np.array_equal(stale, U.oracle_describe("level_subsets")["levels_octave7"])


@pytest.mark.parametrize("family", sorted({f for f, _, _ in U.hamming_cases()}))
def test_oracle_equals_the_numpy_hamming_references(family):
    for f, label, _ in U.hamming_cases():
        if f != family:
            continue
        q, t, match, knn = U.hamming_reference(f, label)
        assert q.shape[1:] == (32,) and t.shape[1:] == (32,)
        assert np.array_equal(O.hamming_match(q, t), match), label
        assert np.array_equal(O.hamming_knn2(q, t), knn), label


def test_hamming_lengths_tie():
    assert {1, 2, 3, 5} <= set(U.NQ) and {0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025} <= set(U.NT)
    tied = 0
    for nq in U.NQ:
        for nt in U.NT:
            q, t, match, knn = U.hamming_reference("lengths", f"nq{nq}_nt{nt}")
            assert q.shape == (nq, 32) and t.shape == (nt, 32) and len(match) == (nq if nt else 0) and knn.shape == (nq, 4)
            if nt >= 63:
                d = U.hamming_distances(q, t)
                tied += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
                assert ((d == d.min(1, keepdims=True)).sum(1) > 1).any(), (nq, nt)
            if nt < 2:
                assert (knn[:, 2:] == -1).all() and (knn[:, :2] == -1).all() == (nt == 0)
    assert tied > 100


def test_all_equal_complement_and_empty():
    for nt in U.ALL_EQUAL_NT:
        q, t, match, knn = U.hamming_reference("all_equal", f"nt{nt}")
        assert (match[:, 1:] == (0, 0)).all() and (knn == (0, 0, 1, 0)).all() and len(match) == len(q) == 5
        q, t, match, knn = U.hamming_reference("complement", f"nt{nt}")
        assert (match[:, 1:] == (0, 256)).all() and (knn == (0, 256, 1, 256)).all()
    q, t, match, knn = U.hamming_reference("empty", "nq0")
    assert len(q) == 0 and len(t) > 0 and match.shape == (0, 3) and knn.shape == (0, 4)
    q, t, match, knn = U.hamming_reference("empty", "nt0")
    assert len(t) == 0 and match.shape == (0, 3) and knn.shape == (len(q), 4) and (knn == -1).all()


def test_planted_neighbours_are_the_answers():
    cases = U.planted_cases()
    assert len(cases) == len(U.PLANT_NT) * (2 * len(U.PLANT_SINGLE) + 3 * len(U.PLANT_PAIRS))
    lanes = set()
    for label, nt, qi, plants in cases:
        q, t, match, knn = U.hamming_reference("planted", label)
        d = U.hamming_distances(q, t)
        for idx, dist in plants:
            assert 0 <= idx < nt and d[qi, idx] == dist               # the plant is there and as near as it claims
        others = np.delete(d[qi], [idx for idx, _ in plants])
        assert others.min() >= 64 and np.delete(d, qi, 0).min() >= 64
        want_qi, want_match, want_knn = U.planted_expectation(label)
        assert tuple(match[qi]) == want_match
        if want_knn is not None:
            assert tuple(knn[qi]) == want_knn
            (a, da), (b, db) = plants
            assert (da == db) == ("_d3_3" in label)                   # the ties really tie
            lanes.add((a % 512 % 64 == b % 512 % 64, a // 512 == b // 512, a < b))
        else:
            assert tuple(knn[qi][:2]) == want_match[1:] and knn[qi][3] >= 64
    assert (True, True, True) in lanes and (False, True, True) in lanes and (False, False, False) in lanes and (True, False, True) in lanes
    assert any(plants[0][0] == nt - 1 and (nt - 1) % 512 % 64 == 63 for _, nt, _, plants in cases)       # the last lane of the last, partial tile
    assert any(plants[0][0] == nt - 1 and (nt - 1) % 512 == 0 for _, nt, _, plants in cases)              # a last tile of one descriptor


# hand-made 2-NN tables (train0, distance0, train1, distance1); row i of both directions describes descriptor i of its set
KNN12 = [(0, 7, 1, 10),        # 7 / 10 at 0.7f: not greater, kept
         (1, 0, 2, 0),         # 0 / 0 is NaN: not greater, kept at every ratio
         (2, 5, 3, 0),         # 5 / 0 is +inf: dropped at every ratio
         (3, 4, -1, -1),       # one neighbour only: dropped
         (5, 1, 4, 9),         # kept by the ratio test, but 5 points back at 6: asymmetric, dropped
         (4, 1, 0, 9),         # 5 <-> 4, kept
         (6, 3, 0, 4),         # 3 / 4: dropped at 0.7, kept at 1
         (7, 0, 0, 5),         # 0 / 5 = 0: kept at ratio 0
         (8, 2, 0, 10)]        # kept here at 0.7, but the way back is 2 / 2 = 1: dropped at 0.7, kept at 1
KNN21 = [(0, 7, 1, 10), (1, 0, 2, 0), (2, 5, 3, 0), (3, 4, -1, -1), (5, 1, 0, 9), (6, 1, 4, 9), (6, 3, 0, 4), (7, 0, 0, 5), (8, 2, 0, 2)]
SYMMETRIC = {0.7: [(0, 0, 7), (1, 1, 0), (5, 4, 1), (7, 7, 0)],
             0.0: [(1, 1, 0), (7, 7, 0)],
             1.0: [(0, 0, 7), (1, 1, 0), (5, 4, 1), (6, 6, 3), (7, 7, 0), (8, 8, 2)]}


@pytest.mark.parametrize("ratio", sorted(SYMMETRIC))
def test_ratio_symmetry_rule(ratio):
    k12, k21 = np.array(KNN12, np.int32), np.array(KNN21, np.int32)
    keep1, keep2, sym = U.ratio_symmetry_ref(k12, k21, ratio)
    assert sym.tolist() == [list(r) for r in SYMMETRIC[ratio]]
    o1, o2, osym = O.ratio_symmetry(k12, k21, ratio)
    assert np.array_equal(o1, keep1) and np.array_equal(o2, keep2) and np.array_equal(osym, sym)
    assert np.array_equal(capi.ratio_symmetry(k12, k21, ratio), sym)
    assert keep1[1] == 1 and keep1[2] == 0 and keep1[3] == 0                           # NaN kept, +inf and a lone neighbour dropped
    assert keep1[4] == (ratio >= 0.7) and [4, 5, 1] not in sym.tolist()                # the asymmetric pair passes the ratio test alone
    if ratio == 0.7:
        assert keep1[0] == 1 and np.float32(7) / np.float32(10) == np.float32(0.7) and 7 / 10 > float(np.float32(0.7))     # a double division would drop it
        assert keep1[8] == 1 and keep2[8] == 0
    assert np.array_equal(capi.ratio_symmetry(k21, k12, ratio), U.ratio_symmetry_ref(k21, k12, ratio)[2])      # and in the other direction
