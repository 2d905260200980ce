"""The layout of a frame slot's plan blob (poppy_amd/csrc/plan_blob.h), checked on the CPU through poppy_plan_blob_layout: the groups lie in the documented
order on 16-byte boundaries with exactly the sizes the kernels read, a context's capacity holds both worst cases and is never above what was allocated
before the layout had one description, and the plans of the warp-geometry point sets fit it."""
import itertools

import numpy as np
import pytest

import warp_geometry_util as U
from poppy_amd import capi

HEADER, RECORD = 64, 20 * 4                                        # kBlobHeader; kWarpRecordFloats floats
RASTER_ROWS = 16                                                   # kPlanRasterRows


def pad16(b):
    return (b + 15) & ~15


def groups(t, n_work, n_toff, n_ttri, fused):
    """(offset field, bytes the kernels read) of every group in the documented order: records, fill-edge tables, then the path's own group."""
    common = [("rec", (t + 1) * RECORD), ("o_edges", t * 96)]
    if fused:
        return common + [("o_outl", t * 48), ("o_toff", 4 * n_toff), ("o_ttri", 2 * n_ttri)]
    return common + [("o_tri", 24 * t), ("o_inv", 72 * t), ("o_work", 8 * n_work)]


@pytest.mark.parametrize("fused", [False, True])
def test_groups_are_aligned_ordered_and_sized(fused):
    for t, n_work, n_toff, n_ttri in itertools.product((0, 1, 2, 7, 1000), (0, 1, 3), (1, 2, 3, 5), (0, 1, 7, 9)):
        lay = capi.plan_blob_layout(t, n_work, n_toff, n_ttri, fused)
        what = f"T {t}, work {n_work}, offsets {n_toff}, entries {n_ttri}, fused {fused}: {lay}"
        assert lay["rec_bytes"] == (t + 1) * RECORD, what
        end = HEADER                                               # the header, then group after group: each starts where the padded one before it ends
        for name, size in groups(t, n_work, n_toff, n_ttri, fused):
            start = HEADER if name == "rec" else lay[name]
            assert start % 16 == 0, f"{name} not on a 16-byte boundary; {what}"
            assert start == end, f"{name} starts at {start}, the group before it ends at {end} (padded); {what}"
            end = start + pad16(size)
            assert end - start >= size and end - start - size < 16, what
        assert lay["used"] == end, what
        other = ("o_tri", "o_inv", "o_work") if fused else ("o_outl", "o_toff", "o_ttri")
        assert all(lay[k] == 0 for k in other), f"the offsets of the group that is not uploaded are not 0; {what}"


def parent_sum(n_points, w, h, tile_w):
    """What ensure_ring allocated before plan_blob.h: both groups added, and a fixed allowance for the pads."""
    need = 2 * n_points + 16
    th = 1024 // tile_w
    ntiles = ((w + tile_w - 1) // tile_w) * ((h + th - 1) // th)
    bins_cap = 64 * need + 16 * ntiles
    items = need * (h // RASTER_ROWS + 3)
    return (HEADER + (need + 1) * RECORD + need * (6 * 4 + 18 * 4 + 96) + items * 8 + need * 3 * 16 + (ntiles + 1) * 4 + bins_cap * 2 + 64 + 6 * 16 + 15) // 16 * 16


@pytest.mark.parametrize("n_points,w,h", [(3, 1, 1), (4, 64, 48), (300, 256, 192), (300, 1920, 1080)])
@pytest.mark.parametrize("tile_w", [0, 64, 128])
def test_capacity_holds_both_worst_cases(n_points, w, h, tile_w):
    cap = capi.plan_blob_capacity(n_points, w, h, tile_w)
    tw = cap["tile_w"]
    assert tw in (64, 128) and (tile_w == 0 or tw == tile_w)
    assert cap["max_tris"] == 2 * n_points + 16 and cap["bins_cap"] == U.bins_cap(n_points, w, h, tw)
    assert cap["n_tiles"] == ((w + tw - 1) // tw) * ((h + 1024 // tw - 1) // (1024 // tw))
    t = cap["max_tris"]
    fused = capi.plan_blob_layout(t, 0, cap["n_tiles"] + 1, cap["bins_cap"], True)
    idmap = capi.plan_blob_layout(t, t * (h // RASTER_ROWS + 3), 0, 0, False)
    assert fused["used"] <= cap["capacity"] and idmap["used"] <= cap["capacity"]
    assert cap["capacity"] == max(fused["used"], idmap["used"])
    assert cap["capacity"] % 16 == 0
    assert cap["capacity"] <= parent_sum(n_points, w, h, tw)


def work_bound(tri_xy, h):
    """An upper bound of the id-map raster's work items from poppy_plan_frame's integer corners (frame_plan.cpp: build_raster): one outline item per triangle
    and one per 16 painted rows, and a triangle paints at most the rows ymin .. min(ymax, h - 1) + 1.  A plan whose bound fits, fits."""
    if len(tri_xy) == 0:
        return 0
    y = tri_xy[:, :, 1].astype(np.int64)
    rows = np.maximum(np.minimum(y.max(1), h - 1) + 1 - y.min(1), 0)
    return int(len(tri_xy) + ((rows + RASTER_ROWS - 1) // RASTER_ROWS).sum())


ALL = [(tw, c) for tw in (64, 128) for c in U.cases(tw)]


@pytest.mark.parametrize("tile_w,case", ALL, ids=[f"{tw}-{c.name}" for tw, c in ALL])
def test_real_plans_fit_the_capacity(tile_w, case):
    """Every warp-geometry point set, at its own size (the density ramps are the 256 x 192 ones): the layout its frame would use — fused where the planner's
    lists fit and no list is longer than a byte numbers, the id-map path otherwise, and the id-map path again for what POPPY_HIP_IDMAP or debug mode force — fits
    what a context with that many point pairs allocates."""
    w, h, p1, p2, ratios = case.make()
    cap = capi.plan_blob_capacity(len(p1), w, h, tile_w)
    for r in ratios:
        counts, total, ok = capi.plan_tile_counts(w, h, p1, p2, r, tile_w)
        tri_xy = capi.plan_frame(w, h, p1, p2, r)["tri_xy"]
        t, n_work = len(tri_xy), work_bound(tri_xy, h)
        assert t <= cap["max_tris"]
        fused = ok and int(counts.max()) <= U.MAX_LIST
        assert fused == case.fused
        if fused:
            assert total <= cap["bins_cap"] and counts.size == cap["n_tiles"]
            lay = capi.plan_blob_layout(t, n_work, counts.size + 1, total, True)
            assert lay["used"] <= cap["capacity"], f"{case.name}: the fused layout needs {lay['used']} bytes of {cap['capacity']}"
        lay = capi.plan_blob_layout(t, n_work, 0, 0, False)
        assert lay["used"] <= cap["capacity"], f"{case.name}: the id-map layout needs {lay['used']} bytes of {cap['capacity']}"
