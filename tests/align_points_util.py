"""Point sets built to reach the branches of the auto-align scoring kernel (k_candidate_scores, kernels_align.hip) that the
reference fixtures (40, 60 and 150 well-separated, non-integer points) never do.  One builder per family, each returning
(w, h, p1, candidate sets) with sets of shape (candidates, n, 2); everything is deterministic from seeds.  NaN and
infinities are not pinned: no set consists of (-1, -1) points alone (0 pairs: 0 / 0) and no Procrustes fit sees identical
points.  tests/test_oracle_align_points.py asserts from the oracle and the numpy restatement below that every family reaches
what it is built for; tests/test_gpu_align_points.py compares the kernel with the oracle on them."""
import functools

import numpy as np

import oracle_lib as O

W, H = 256, 192
MAX_POINTS = 4096                                   # kAlignMaxPoints


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _random_points(rng, n, w=W, h=H):
    """Non-integer coordinates inside the image, as float32."""
    p = _f32(np.stack([rng.uniform(2, w - 2, n), rng.uniform(2, h - 2, n)], 1))
    p[p == np.rint(p)] += np.float32(0.5)           # one float in 65 536 is a whole number
    return p


# ---- lengths: the full 64-lane blocks and the tail of candidate_inner, the lane stride of candidate_pairs, the LDS limit ---------
LENGTHS = [4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000, 4095, 4096]


def lengths(n):
    rng = np.random.default_rng(1000 + n)
    p1 = _random_points(rng, n)
    k = 2 if n >= 4095 else 3
    sets = np.stack([_f32(p1[rng.permutation(n)] + rng.uniform(-6, 6, (n, 2))) for _ in range(k)])
    return W, H, p1, sets


# ---- ties: integer coordinates, so that claims are decided among equally near points and pairs share their distance ------------
TIES = [(65, 24, 1), (130, 24, 2), (200, 40, 3), (257, 64, 4)]


def ties(n, span, seed):
    rng = np.random.default_rng(seed)
    p1 = _f32(rng.integers(0, span, (n, 2)) + 20)
    p2 = _f32(rng.integers(0, span, (n, 2)) + 20)
    return W, H, p1, p2[None]


# the sets the single steps run on: n = 64 and 128 are the first points of the 65- and 130-point ties sets
STEP_SETS = {64: (TIES[0], 64), 65: (TIES[0], 65), 128: (TIES[1], 128), 257: (TIES[3], 257)}


def step_set(n):
    args, keep = STEP_SETS[n]
    w, h, p1, sets = ties(*args)
    return w, h, p1[:keep].copy(), sets[0][:keep].copy()


# ---- duplicates ---------------------------------------------------------------------------------------------------------------
def duplicates():
    """p2 == p1 (every distance 0), p2 a permutation of p1, p2 with exact duplicates of some of its own points."""
    n = 100
    rng = np.random.default_rng(11)
    p1 = _random_points(rng, n)
    repeated = _f32(p1 + rng.uniform(-3, 3, (n, 2)))
    repeated[10:20] = repeated[0:10]                # ten pairs of twins
    repeated[90:] = repeated[50]                    # and one point eleven times
    return W, H, p1, np.stack([p1.copy(), p1[rng.permutation(n)], repeated])


# ---- tombstones: a candidate point at exactly (-1, -1) is the reference's "claimed" marker and pairs with nothing ---------------
TOMBSTONE_N = 70


def _tombstone_layout():
    n = TOMBSTONE_N
    out = []
    for m in (1, 3, n - 1):
        scattered = np.random.default_rng(40 + m).permutation(n)[:m]
        out += [(m, np.arange(m)), (m, np.arange(n - m, n)), (m, np.sort(scattered))]
    return out


def tombstones():
    """Sets 0..8: m = 1, 3, n - 1 points at (-1, -1), at the front, at the back, scattered (TOMBSTONE_M).  Set 9: near misses that
    pair like any other point.  p1 holds a point at (-1, -1) itself, which is not special."""
    n = TOMBSTONE_N
    rng = np.random.default_rng(12)
    p1 = _random_points(rng, n)
    p1[7] = (-1, -1)
    base = _f32(p1[rng.permutation(n)] + rng.uniform(-4, 4, (n, 2)))
    sets = []
    for m, where in _tombstone_layout():
        s = base.copy()
        s[where] = (-1, -1)
        sets.append(s)
    near = base.copy()
    below = np.nextafter(np.float32(-1), np.float32(-2)); above = np.nextafter(np.float32(-1), np.float32(0))
    near[0] = (-1, 5); near[1] = (-1, -2); near[2] = (17, -1); near[3] = (-3, -1)
    near[4] = (below, -1); near[5] = (above, -1); near[6] = (-1, below); near[69] = (-1, above)
    sets.append(near)
    return W, H, p1, np.stack(sets)


TOMBSTONE_M = [m for m, _ in _tombstone_layout()] + [0]


# ---- candidate counts: the block index of every candidate ------------------------------------------------------------------------
CANDIDATE_COUNTS = [1, 2, 101, 1080]


def candidate_counts(k):
    n = 70
    rng = np.random.default_rng(13)
    p1 = _random_points(rng, n)
    base = p1[rng.permutation(n)]
    sets = _f32(base[None] + rng.uniform(-8, 8, (k, n, 2)))     # every candidate differs from every other in every point
    return W, H, p1, sets


# ---- magnitudes: negative coordinates and coordinates up to +-1e6, where the float differences round --------------------------------
def _magnitude_parts():
    n = 90
    rng = np.random.default_rng(14)
    p1 = _f32(rng.uniform(-200, 200, (n, 2)))
    far = _f32(rng.uniform(-1e6, 1e6, (n, 2)))
    sets = np.stack([_f32(rng.uniform(-200, 200, (n, 2))),            # both sets around the origin
                     far,                                             # small against huge
                     _f32(p1 + np.float32(1e6)), _f32(p1 - np.float32(1e6))])
    far1 = _f32(far[rng.permutation(n)] + rng.uniform(-50, 50, (n, 2)))
    return W, H, p1, sets, far1


def magnitudes_near():
    w, h, p1, sets, far1 = _magnitude_parts()
    return w, h, p1, sets


def magnitudes_far():
    """Both sets at up to +-1e6: every difference of two coordinates rounds."""
    w, h, p1, sets, far1 = _magnitude_parts()
    return w, h, far1, sets[1:]


# ---- long walks: retranslate on p2 = p1 + shift, for shifts the oracle walks back by more than 12 and more than 24 steps ----------
# (name, n, seed, shift, p1 point added, the move of the oracle's retranslate).  The shifts were picked by what the oracle's search
# does with them, which is not what one would expect: it counts its steps from 1, so a walk that finds its way back overshoots by
# one, and most x-only or y-only shifts make it walk diagonally and stop halfway ((40, 0) on seed 21 moves (-21, -21)).
# tests/test_oracle_align_points.py asserts the moves.  The GPU search scores 12 steps per call: the walks end in its second,
# third and fourth call, and two of them on the first step of a new call (13, 25).
WALKS = [
    ("x", 100, 22, (26, 0), None, (-27, 0)),
    ("y", 100, 21, (0, 40), None, (0, -41)),
    ("diagonal", 100, 21, (30, 30), None, (-31, -31)),
    ("diagonal_up", 100, 22, (20, -20), None, (-21, 21)),
    ("diagonal_13", 100, 21, (12, 12), None, (-13, -13)),
    ("diagonal_25", 100, 22, (24, 24), None, (-25, -25)),
    # towards the origin over a p2 point (29, 29): step 30 of the walk puts it on (-1, -1), where it pairs with nothing, and the walk goes on
    ("origin", 100, 24, (30, 30), (-1, -1), (-31, -31)),
    # the same over (20, 20): step 21 puts it on (-1, -1), the search takes that for worse and stops there, with the point on the marker
    ("origin_stop", 100, 24, (30, 30), (-10, -10), (-21, -21)),
]


def walk(name):
    """(w, h, p1, p2) of a walk case."""
    _, n, seed, shift, extra, _ = next(c for c in WALKS if c[0] == name)
    rng = np.random.default_rng(seed)
    p1 = _random_points(rng, n)
    if extra is not None:
        p1[n // 2] = extra
    p2 = _f32(p1 + _f32(shift))
    return W, H, p1, p2


def walk_steps(p2_before, p2_after):
    """(steps in x, steps in y) a retranslate moved the points by: output points minus input points."""
    d = np.rint(np.asarray(p2_after, np.float64) - np.asarray(p2_before, np.float64))     # the float additions round
    assert (d == d[0]).all(), "the points did not move as one"
    return int(d[0, 0]), int(d[0, 1])


def walk_candidates(p2, move):
    """The point sets the search scores along a walk that ends in `move`: one unit step after the other, each a float addition."""
    steps = max(abs(move[0]), abs(move[1]))
    unit = _f32([np.sign(move[0]), np.sign(move[1])])
    out, t = [], _f32(p2).copy()
    for _ in range(steps):
        t = _f32(t + unit)
        out.append(t)
    return np.stack(out)


# ---- whole searches: a shifted and a rotated copy of the first set ------------------------------------------------------------------
def auto_set(kind):
    """(w, h, p1, p2) for Matcher::autoAlign: 'shifted' = p1 + (40, -40); 'rotated' = p1 turned by 7 degrees about the image centre."""
    n = 100
    rng = np.random.default_rng(31)
    p1 = _random_points(rng, n)
    if kind == "shifted":
        return W, H, p1, _f32(p1 + _f32([40, -40]))
    a = np.deg2rad(7.0)
    c = np.array([W / 2, H / 2])
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return W, H, p1, _f32((p1 - c) @ rot.T + c)


# ---- every family's scoring cases -----------------------------------------------------------------------------------------------
def score_cases():
    """[(family, label, builder)]: builder() -> (w, h, p1, sets)."""
    out = [("lengths", f"n{n}", functools.partial(lengths, n)) for n in LENGTHS]
    out += [("ties", f"n{n}", functools.partial(ties, n, span, seed)) for n, span, seed in TIES]
    out += [("duplicates", "n100", duplicates), ("tombstones", f"n{TOMBSTONE_N}", tombstones)]
    out += [("candidates", f"k{k}", functools.partial(candidate_counts, k)) for k in CANDIDATE_COUNTS]
    out += [("magnitudes", "near", magnitudes_near), ("magnitudes", "far", magnitudes_far)]
    return out


@functools.lru_cache(maxsize=None)
def oracle_scores(family, label):
    """The oracle on one scoring case, computed once per session: (distances f64, totals f32, pair counts i32, offset sums f32)."""
    build = next(b for f, l, b in score_cases() if (f, l) == (family, label))
    w, h, p1, sets = build()
    k = len(sets)
    d = np.zeros(k, np.float64); total = np.zeros(k, np.float32); n_pairs = np.zeros(k, np.int32); inner = np.zeros(k, np.float32)
    for a in range(k):
        total[a], n_pairs[a], inner[a] = O.morph_distance_parts(p1, sets[a])
        d[a] = O.morph_distance(p1, sets[a], w, h)
    for r in (d, total, n_pairs, inner):
        r.setflags(write=False)
    return d, total, n_pairs, inner


# ---- the greedy claim in plain numpy (make_distance_map, src/util.cpp:351-383) ------------------------------------------------------
def hypotf(x, y):
    """glibc's hypotf: the double sum of the squares, its square root, rounded to float."""
    x = np.asarray(x, np.float32).astype(np.float64); y = np.asarray(y, np.float32).astype(np.float64)
    return np.sqrt(x * x + y * y).astype(np.float32)


def greedy_claims(p1, p2):
    """Every p1 point, in list order, takes the nearest unclaimed p2 point (strict <: the lowest index wins); (-1, -1) is skipped.
    Returns (dist f32 per p1 point, -1 where nothing was left; claims decided among equally near candidates)."""
    p1 = _f32(p1); pool = _f32(p2).copy()
    dist = np.full(len(p1), -1, np.float32)
    tie_decided = 0
    for i, q in enumerate(p1):
        free = np.flatnonzero(~((pool[:, 0] == -1) & (pool[:, 1] == -1)))
        if not len(free):
            continue
        d = hypotf(pool[free, 0] - q[0], pool[free, 1] - q[1])
        j = int(np.argmin(d))                       # the first of equal minima
        tie_decided += int((d == d[j]).sum() > 1)
        dist[i] = d[j]
        pool[free[j]] = (-1, -1)
    return dist, tie_decided


def float_total(d):
    """Sequential float32 sum in the given order."""
    t = np.float32(0)
    for v in np.asarray(d, np.float32):
        t = np.float32(t + v)
    return t


def claim_totals(dist):
    """(ascending order: the reference's, list order, descending order) float totals of the pairs' distances, and the number of
    pairs that share their distance with another pair."""
    d = dist[dist >= 0]
    asc = np.sort(d, kind="stable")
    _, counts = np.unique(d, return_counts=True)
    return float_total(asc), float_total(d), float_total(asc[::-1]), int(counts[counts > 1].sum())
