"""Point sets aimed at the branches of the fused raster + warp kernels (kernels_warp_bin.hip: k_tile_expand, k_warp_bin) and at the host's choice between
them and the id-map path, shared by tests/test_host_warp_geometry.py (which asserts on the CPU, from the planner itself, that every set reaches what it is
built for) and tests/test_gpu_warp_geometry.py (which compares the frames with the oracle, bit for bit).

What a set does to the kernels depends on the tile shape, 64 x 16 or 128 x 8.  Every image here is below 4 Mpx, so the tiles are 64 wide unless
POPPY_TILE_W forces 128 (read once per process by the library, and here): TILE_W is the width in force, CASES the sets chosen for it, cases(tile_w) those
of either width.

Rules of every family: the sources are independent uniform noise (a wrong triangle id or a wrong footprint changes the pixel), and the second point set
is the first moved by +-3..6 px with the sign alternating from point to point (no smooth field: neighbouring triangles carry different matrices)."""
import os
from collections import namedtuple

import numpy as np

from poppy_amd import capi, synth

TILE_W = 128 if os.environ.get("POPPY_TILE_W", "").strip() == "128" else 64
SLOTS, MAX_LIST = 32, 255                                        # kernels_warp_bin.hip: kSlots, kMaxTileEntries


def pass_len(tile_w):
    """Entries k_tile_expand rasterises per pass of its `base` loop: 256 / tile height."""
    return 256 // (1024 // tile_w)


def bins_cap(n_points, w, h, tile_w):
    """frame_plan.h: tile_bins_capacity — the list entries a context keeps room for.  (Restated only to report how near a set is; on which side a set falls
    is the planner's own bins_ok, and the host test checks that the two agree.)"""
    th = 1024 // tile_w
    return 64 * (2 * n_points + 16) + 16 * ((w + tile_w - 1) // tile_w) * ((h + th - 1) // th)


def shifts(n):
    """Point i moves by (+3, -5), (-4, +6), (+5, -3), (-6, +4), ... px"""
    i = np.arange(n)
    return np.stack([np.where(i & 1, -1, 1) * (3 + i % 4), np.where(i & 1, 1, -1) * (3 + (i + 2) % 4)], 1).astype(np.float64)


def moved(p1, w, h):
    """The second set: p1 + shifts; a coordinate that would leave the image moves the other way instead."""
    d = shifts(len(p1))
    for k, lim in ((0, w - 1), (1, h - 1)):
        out = (p1[:, k] + d[:, k] < 0) | (p1[:, k] + d[:, k] > lim)
        d[out, k] = -d[out, k]
    return (p1 + d).astype(np.float32)


def around(m, w, h, d=None):
    """Both sets for a frame at ratio 0.5 whose morphed points are exactly m (coordinates in quarter pixels: every step is exact in float):
    p1 = m - d / 2, p2 = m + d / 2.  A coordinate's shift changes sign, or is dropped, where it would leave the image."""
    m = np.asarray(m, np.float64)
    d = shifts(len(m)) if d is None else np.asarray(d, np.float64).copy()
    for k, lim in ((0, w - 1), (1, h - 1)):
        for retry in (-1, 0):
            out = (m[:, k] - d[:, k] / 2 < 0) | (m[:, k] - d[:, k] / 2 > lim) | (m[:, k] + d[:, k] / 2 < 0) | (m[:, k] + d[:, k] / 2 > lim)
            d[out, k] *= retry
    return (m - d / 2).astype(np.float32), (m + d / 2).astype(np.float32)


def sources(w, h, seed):
    return synth.uniform_noise(w, h, seed, channels=3), synth.uniform_noise(w, h, seed + 100, channels=3), synth.unit_field(w, h, seed + 200)


# ---- the families: each returns (w, h, p1, p2, shape ratios) ------------------------------------------------------------------------------------------
def density_ramp(n, seed):
    """256 x 192 = 4 x 12 tiles of 64 x 16 (2 x 24 of 128 x 8), no corner points: the density falls from the top left corner to nothing at the far sides,
    so one frame's list lengths run from 0 up to 148..247 (never past 255: the frame stays fused) with few gaps."""
    w, h = 256, 192
    u = np.random.default_rng(seed).uniform(0, 1, (n, 2)) ** 2.5
    p1 = (u * np.array([0.85 * (w - 1), 0.85 * (h - 1)]) + 3).astype(np.float32)
    return w, h, p1, moved(p1, w, h), (0.5,)


def dense(n, seed, w=128, h=96):
    """Uniformly scattered points on a small image (near_full, over_full): every tile's list is long."""
    rng = np.random.default_rng(seed)
    p1 = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1).astype(np.float32)
    return w, h, p1, moved(p1, w, h), (0.5,)


def dense_rotated(n, seed, w, h, ratios):
    """dense() with the second set rotated 35 degrees and scaled 0.8 about the centre before it is moved (the strong-deformation recipe of
    tests/test_gpu_fused_warp.py): records from the overflow area and footprints that leave the image in the same tiles."""
    _, _, p1, _, _ = dense(n, seed, w, h)
    a = np.deg2rad(35.0)
    c = np.array([(w - 1) / 2, (h - 1) / 2])
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) * 0.8
    q = (p1 - c) @ R.T + c
    q[:, 0] = np.clip(q[:, 0], 6, w - 7); q[:, 1] = np.clip(q[:, 1], 6, h - 7)
    return w, h, p1, moved(q, w, h), ratios


def chains(n):
    """512 x 384 (192 tiles of either shape), n points on two exactly collinear chains, one inside the first tile and one inside the last: the mesh is the
    n - 2 triangles between the chains, and every one of them has the whole image for its bounding box, so the lists hold 192 (n - 2) entries, against
    room for 64 (2 n + 16) + 16 * 192: equal at n = 70, over from n = 71.  (No set of 12 points or fewer can outgrow the room: it has at most 2 n - 5 = 19
    triangles, 19 * 192 = 3648 entries, and room for 5632.)  The points of a chain move along it by the alternating +-3..6 px and across it by one common
    step, so both sets stay collinear."""
    w, h = 512, 384
    na = n // 2
    m = np.concatenate([np.stack([np.linspace(6, 56, na), np.full(na, 3.0)], 1), np.stack([np.linspace(455, 505, n - na), np.full(n - na, 380.0)], 1)])
    d = shifts(n)
    d[:, 1] = np.where(np.arange(n) < na, 3, -4)
    p1, p2 = around(np.round(m * 4) / 4, w, h, d)
    return w, h, p1, p2, (0.5,)


RAIL_STEPS = (8, 1, 0, 4, 3, 8, 7, 3, 5, 5)                      # found by search: the Delaunay mesh of these rails has a rung of every minor 0..8


def rails(w, h):
    """Two rails of ten points on the image's short sides, 6 px apart on one and moved along by RAIL_STEPS on the other: rungs of major = long side - 1
    and minor = 0, 1, .., 8 (shallow on a wide image, steep on a tall one), and the rails' own edges, vertical or horizontal.  The points stay on the
    image's border: they move along their rail only."""
    k = len(RAIL_STEPS)
    along = 1 + 6 * np.arange(k)
    m = np.concatenate([np.stack([np.zeros(k), along], 1), np.stack([np.full(k, max(w, h) - 1.0), along + np.array(RAIL_STEPS)], 1)])
    d = shifts(2 * k)
    d[:, 0] = 0
    if h > w:
        m, d = m[:, ::-1], d[:, ::-1]
    p1, p2 = around(m, w, h, d)
    return w, h, p1, p2, (0.5,)


DIAGONAL_STEPS = (1, -1, 0, 1, 0, 1, 1, 1, 0, 1)                 # found by search: rungs with |dy| - |dx| = -1, 0 and +1 are all edges of the mesh


def diagonal_rails(mirror):
    """1024 x 1024: two rails of ten points across the main diagonal (the other one with `mirror`), 880 px apart along it, the far rail's points off by
    DIAGONAL_STEPS: rungs on the `dy > dx` line between steep and shallow, |dx| = |dy| and |dy| = |dx| +- 1, in both y directions."""
    w = h = 1024
    i = np.arange(len(DIAGONAL_STEPS))
    near = np.stack([20 + 10 * i, 120 - 10 * i], 1).astype(np.float64)
    m = np.concatenate([near, near + np.stack([np.full(len(i), 880), 880 + np.array(DIAGONAL_STEPS)], 1)])
    if mirror:
        m[:, 0] = w - 1 - m[:, 0]
    p1, p2 = around(m, w, h)
    return w, h, p1, p2, (0.5,)


def neighbouring_pixels():
    """96 x 64: two points inside one pixel and two on its neighbours, so that after truncation the mesh has edges of major 0 and of major 1."""
    w, h = 96, 64
    m = [[40.25, 30.25], [40.75, 30.5], [41.5, 30.25], [41.25, 31.5], [10, 10], [85, 12], [80, 55], [12, 50]]
    p1, p2 = around(m, w, h)
    return w, h, p1, p2, (0.5,)


# ---- what the planner hands the kernels ---------------------------------------------------------------------------------------------------------------
def tile_lists(w, h, p1, p2, ratio, tile_w):
    """(list length of every tile, their sum, bins_ok) from the planner itself: poppy_plan_tile_counts."""
    return capi.plan_tile_counts(w, h, p1, p2, ratio, tile_w)


def local_ids(w, h, p1, p2, ratio, tile_w, tri_map):
    """What k_tile_expand must write: for every pixel the number (1-based) its owning triangle has in its tile's list, 0 where no triangle paints, from
    the planner's lists (poppy_plan_tile_tris) and the oracle's triangle map (triangle number + 1).  Raises if a pixel's owner is not in its tile's list."""
    counts = capi.plan_tile_counts(w, h, p1, p2, ratio, tile_w)[0]
    lists = capi.plan_tile_tris(w, h, p1, p2, ratio, tile_w)
    th = 1024 // tile_w
    out = np.zeros((h, w), np.int32)
    for t, tris in enumerate(lists):
        ty, tx = divmod(t, counts.shape[1])
        owner = tri_map[ty * th:(ty + 1) * th, tx * tile_w:(tx + 1) * tile_w].astype(np.int64) - 1
        if len(tris) == 0:
            assert (owner < 0).all(), f"tile {t} has an empty list and painted pixels"
            continue
        at = np.minimum(np.searchsorted(tris, owner), len(tris) - 1)
        assert (tris[at] == owner)[owner >= 0].all(), f"tile {t}: a pixel's triangle is not in the tile's list"
        out[ty * th:(ty + 1) * th, tx * tile_w:(tx + 1) * tile_w] = np.where(owner >= 0, at + 1, 0)
    return out, counts


def last_entry_pixels(local, counts, tile_w):
    """Per tile: the pixels whose id is the tile's list length, i.e. that the LAST entry of the list owns (a length is only reached in the picture if
    that entry paints something: a list's last entry may touch the tile with its bounding box alone)."""
    th = 1024 // tile_w
    out = np.zeros(counts.shape, np.int64)
    for ty in range(counts.shape[0]):
        for tx in range(counts.shape[1]):
            if counts[ty, tx]:
                out[ty, tx] = (local[ty * th:(ty + 1) * th, tx * tile_w:(tx + 1) * tile_w] == counts[ty, tx]).sum()
    return out


def matrices_in_range(w, h, p1, p2, ratio):
    """frame_plan.cpp: warp_matrix_ok over every triangle's box, as pack_warp_records applies it in a context (the exported poppy_warp_records tests over
    the whole image, which near-degenerate triangles of a dense mesh do not pass): the number of triangles with a matrix outside the tiled warp kernels'
    range.  With one, the frame takes the general warp kernel on the id-map path (kind 0), whatever its lists."""
    plan = capi.plan_frame(w, h, p1, p2, ratio)
    bad = 0
    for v, pair in zip(plan["tri_xy"], zip(plan["inv1"], plan["inv2"])):
        x0, x1 = max(0, int(v[:, 0].min()) - 1), min(w - 1, int(v[:, 0].max()) + 1)
        y0, y1 = max(0, int(v[:, 1].min()) - 1), min(h - 1, int(v[:, 1].max()) + 1)
        for m in pair:
            m = m.ravel()
            ok = bool(np.isfinite(m).all()) and not (np.abs(m) > 2.0 ** 40).any() and not ((m[:6] != 0) & (np.abs(m[:6]) < 2.0 ** -100)).any()
            if ok and (m != 0).any():
                z = [float(m[6]) * x + float(m[7]) * y + float(m[8]) for x in (x0, x1) for y in (y0, y1)]
                ok = (min(z) >= 2.0 ** -20 and max(z) <= 2.0 ** 20) or (max(z) <= -2.0 ** -20 and min(z) >= -2.0 ** 20)
            bad += not ok
    return bad


def edge_steps(w, h, p1, p2, ratio):
    """(dx, dy) of every triangle edge of the frame's mesh, from plan_frame's integer corners (what build_outlines turns into segments; plan_frame clips the
    points into the image first, so no edge is ever clipped by clip_line_ref: that code cannot be reached and is not tested)."""
    t = capi.plan_frame(w, h, p1, p2, ratio)["tri_xy"].astype(np.int64)
    return np.concatenate([t[:, 0] - t[:, 2], t[:, 1] - t[:, 0], t[:, 2] - t[:, 1]])


# Not covered, and not coverable at these sizes: the `- (r < 0)` step of div_small_quotient (kernels_warp_bin.hip).  The float quotient a * rcp(b) can only
# come out one too HIGH when its error (about 2.4e-7 a / b: one ulp of the reciprocal and the product's rounding) reaches the distance 1 / b of a / b
# from the next integer, i.e. from a = major (2 d +- 1) of about 4e6 up: an edge of some 1500 px in BOTH directions.  The largest a here is 1.8e6 (the
# diagonal rails), and an image with such an edge costs the oracle several seconds per frame.  A build without that step passes every test here.
def has_edge(steps, shape, w, h):
    """Is an edge of this named shape among `steps`?  Shapes: ("shallow", minor) / ("steep", minor): image-spanning, major = w - 1 / h - 1;
    ("diagonal", k, sign): |dy| - |dx| = k on an edge longer than 500 px whose dx dy has this sign; "horizontal", "vertical", "major0", "major1"."""
    dx, dy = steps[:, 0], steps[:, 1]
    ax, ay = np.abs(dx), np.abs(dy)
    if shape == "horizontal":
        return bool(((dy == 0) & (ax > 1)).any())
    if shape == "vertical":
        return bool(((dx == 0) & (ay > 1)).any())
    if shape == "major0":
        return bool(((dx == 0) & (dy == 0)).any())
    if shape == "major1":
        return bool((np.maximum(ax, ay) == 1).any())
    if shape[0] == "shallow":
        return bool(((ax == w - 1) & (ay == shape[1])).any())
    if shape[0] == "steep":
        return bool(((ay == h - 1) & (ax == shape[1])).any())
    if shape[0] == "diagonal":
        return bool(((ay - ax == shape[1]) & (ax > 500) & (np.sign(dx * dy) == shape[2])).any())
    raise ValueError(shape)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------
# expect: lengths = list lengths that must occur in the frame, in a tile whose last entry owns at least OWNED pixels (0: an empty tile); longest = (lo, hi) for the longest list; every = (lo, hi) for every tile's list;
# bins_ok; fill = (lo, hi) for total / bins_cap; edges = shapes that must be in the mesh; leaves_image = the footprint of a pixel whose id
# is 32 or more (its record comes from the overflow area) leaves the image; admitted = every matrix is in the tiled warp kernels' range (matrices_in_range; asserted for every fused case too).  fused: the frame stays on k_tile_expand + k_warp_bin.
Case = namedtuple("Case", "name make fused about expect")
OWNED = 4

# the lengths the density ramps of a tile width must reach between them: 0 (the identity slot alone), 1, the last list of one pass and the first of two,
# 31 / 32 / 33 around the 32 record slots, and for the wide tile the same around its second pass (64 / 65)
RAMP_LENGTHS = {64: (0, 1, 16, 17, 31, 32, 33), 128: (0, 1, 31, 32, 33, 64, 65)}
_RAMPS = {64: ((425, 4, (0, 16, 17, 31, 32, 33)), (325, 8, (0, 1, 16, 17, 31, 32))),
          128: ((500, 2, (0, 32, 33, 64, 65)), (475, 6, (0, 31, 33, 64, 65)), (300, 33, (0, 1, 31, 32, 33)))}
_NEAR_FULL = {64: (932, 51), 128: (700, 56)}                     # (n, seed): the longest list is 255, and its last entry owns pixels
_OVER_FULL = {64: (946, 51), 128: (702, 56)}                       # a few points more: 256
_ROTATED_SMALL = {64: (620, 5), 128: (500, 2)}                   # fewer points than near_full: the mesh shrinks towards ratio 1, and the longest list must stay a byte
_ROTATED_ODD = {64: (6000, 3), 128: (6000, 3)}


def cases(tile_w):
    out = []
    for n, seed, lengths in _RAMPS[tile_w]:
        out.append(Case(f"density_ramp_{n}", lambda n=n, seed=seed: density_ramp(n, seed), True,
                        "list lengths from 0 up: empty tiles, one entry, both sides of a pass of k_tile_expand and of the 32 record slots",
                        dict(lengths=lengths, longest=(66, MAX_LIST), bins_ok=True)))
    n, seed = _NEAR_FULL[tile_w]
    out.append(Case("near_full", lambda: dense(n, seed), True, "the longest list the fused path takes: id 255 in a byte",
                    dict(lengths=(MAX_LIST,), longest=(MAX_LIST, MAX_LIST), every=(SLOTS + 1, MAX_LIST), bins_ok=True)))
    n2, seed2 = _OVER_FULL[tile_w]
    out.append(Case("over_full", lambda: dense(n2, seed2), False, "one entry more than a byte numbers: prepare_slot falls back to the id-map path",
                    dict(longest=(MAX_LIST + 1, MAX_LIST + 1), bins_ok=True, admitted=True)))
    out.append(Case("over_cap", lambda: chains(71), False, "the lists outgrow the plan blob's room: build_tile_bins gives up, the id-map path runs",
                    dict(bins_ok=False, fill=(1.0001, 1.01), admitted=True)))
    out.append(Case("under_cap", lambda: chains(70), True, "one point fewer: the lists fill the room to the last entry and stay fused",
                    dict(bins_ok=True, fill=(1.0, 1.0), longest=(68, 68))))
    n3, seed3 = _ROTATED_SMALL[tile_w]
    out.append(Case("dense_rotated_128x96", lambda: dense_rotated(n3, seed3, 128, 96, (0.25, 0.8)), True,
                    "records from the overflow area under footprints that leave the image (the border path's record lookup), rows of a multiple of 4",
                    dict(longest=(SLOTS + 1, MAX_LIST), bins_ok=True, leaves_image=True)))
    n4, seed4 = _ROTATED_ODD[tile_w]
    out.append(Case("dense_rotated_398x377", lambda: dense_rotated(n4, seed4, 398, 377, (0.4,)), True,
                    "the same on rows that are no multiple of 4 bytes (k_warp_bin<*, false>)",
                    dict(longest=(SLOTS + 1, MAX_LIST), bins_ok=True, leaves_image=True)))
    out.append(Case("rails_3840x64", lambda: rails(3840, 64), True, "image-spanning shallow outline runs: major 3839 over minor 0..8, and vertical edges",
                    dict(bins_ok=True, edges=[("shallow", k) for k in range(9)] + ["vertical", "horizontal"])))
    out.append(Case("rails_64x2160", lambda: rails(64, 2160), True, "their steep transposes: major 2159 over minor 0..8, and horizontal edges",
                    dict(bins_ok=True, edges=[("steep", k) for k in range(9)] + ["vertical", "horizontal"])))
    out.append(Case("rails_diagonal", lambda: diagonal_rails(False), True, "long edges on the steep / shallow line, y growing with x",
                    dict(bins_ok=True, edges=[("diagonal", k, 1) for k in (-1, 0, 1)])))
    out.append(Case("rails_antidiagonal", lambda: diagonal_rails(True), True, "long edges on the steep / shallow line, y falling with x",
                    dict(bins_ok=True, edges=[("diagonal", k, -1) for k in (-1, 0, 1)])))
    out.append(Case("neighbouring_pixels", neighbouring_pixels, True, "edges of major 0 (a single pixel) and major 1",
                    dict(bins_ok=True, edges=["major0", "major1"])))
    return out


CASES = cases(TILE_W)
