"""The point sets of tests/warp_geometry_util.py reach what they are built for: checked on the CPU from the planner itself (poppy_plan_tile_counts: the
tile lists k_tile_expand and k_warp_bin would be handed; plan_frame: the mesh's integer corners), for both tile shapes.  These are not measurements: the
sets were chosen so that the conditions hold, and a planner or synth change after which a set no longer reaches its branch fails here, naming the branch."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import warp_geometry_util as U
from poppy_amd import capi

ALL = [(tw, c) for tw in (64, 128) for c in U.cases(tw)]


def test_tile_counts_entry():
    """One triangle: its bounding box, grown by a pixel, decides the tiles; bad arguments are refused."""
    p = np.array([[10, 5], [70, 5], [10, 20]], np.float32)
    counts, total, ok = capi.plan_tile_counts(256, 64, p, p, 0.5, 64)
    assert counts.shape == (4, 4) and ok and total == 4
    assert counts.tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    counts, total, ok = capi.plan_tile_counts(256, 64, p, p, 0.5, 128)
    assert counts.shape == (8, 2) and total == 3 and counts[:4, 0].tolist() == [1, 1, 1, 0]
    with pytest.raises(capi.PoppyError):
        capi.plan_tile_counts(256, 64, p, p, 0.5, 32)
    lists = capi.plan_tile_tris(256, 64, p, p, 0.5, 64)
    assert [l.tolist() for l in lists] == [[0], [0], [], []] + [[0], [0], [], []] + [[]] * 8
    q = np.array([[10, 5], [70, 5], [10, 20], [70, 20]], np.float32)             # two triangles: ascending numbers in every tile
    assert all(l.tolist() == sorted(l.tolist()) and len(l) <= 2 for l in capi.plan_tile_tris(256, 64, q, q, 0.5, 64))
    n_tiles = C.c_int(0)                                                         # counts is optional: the capacity is not looked at without it
    assert capi.lib().poppy_plan_tile_counts(256, 64, p.ctypes.data, p.ctypes.data, 3, 0.5, 64, None, 0, C.byref(n_tiles), None, None) == 0 and n_tiles.value == 16
    assert capi.lib().poppy_plan_tile_counts(256, 64, None, None, 3, 0.5, 64, None, 0, C.byref(n_tiles), None, None) != 0


@pytest.mark.parametrize("tile_w", [64, 128])
def test_density_ramps_reach_every_threshold(tile_w):
    ramps = [c for c in U.cases(tile_w) if c.name.startswith("density_ramp")]
    assert 1 <= len(ramps) <= 3
    seen = set()
    for c in ramps:
        w, h, p1, p2, ratios = c.make()
        assert (w, h) == (256, 192)
        assert set(c.expect["lengths"]) <= set(np.unique(U.tile_lists(w, h, p1, p2, ratios[0], tile_w)[0]).tolist())
        seen |= set(c.expect["lengths"])                          # test_case_reaches_its_branch: each in a tile whose last entry owns pixels
    k = U.pass_len(tile_w)
    assert {0, 1, k, k + 1, U.SLOTS - 1, U.SLOTS, U.SLOTS + 1} <= set(U.RAMP_LENGTHS[tile_w])
    missing = [v for v in U.RAMP_LENGTHS[tile_w] if v not in seen]
    assert not missing, f"tile width {tile_w}: no density ramp has a tile with a list of {missing} entries (empty tile / pass of k_tile_expand / record slots)"


@pytest.mark.parametrize("tile_w,case", ALL, ids=[f"{tw}-{c.name}" for tw, c in ALL])
def test_case_reaches_its_branch(tile_w, case):
    w, h, p1, p2, ratios = case.make()
    exp = case.expect
    what = f"{case.name}, tile width {tile_w} ({case.about})"
    for pts in (p1, p2):
        assert pts.dtype == np.float32 and (pts >= 0).all() and (pts[:, 0] <= w - 1).all() and (pts[:, 1] <= h - 1).all(), f"{what}: a point outside the image"
    assert max(w, h) <= 3840 and w * h <= 1024 * 1024
    for r in ratios:
        counts, total, ok = U.tile_lists(w, h, p1, p2, r, tile_w)
        cap = U.bins_cap(len(p1), w, h, tile_w)
        assert total == int(counts.sum())
        assert ok == (total <= cap), f"{what}: bins_ok = {ok} with {total} entries against room for {cap}"
        assert ok == exp["bins_ok"], f"{what}, ratio {r}: {total} entries against room for {cap}: build_tile_bins " + ("gave up" if not ok else "did not give up")
        longest = int(counts.max())
        # what prepare_slot decides from (fused: the frame stays on k_tile_expand + k_warp_bin)
        assert case.fused == (ok and longest <= U.MAX_LIST), f"{what}, ratio {r}: longest list {longest}, bins_ok {ok}"
        if case.fused or exp.get("admitted"):
            bad = U.matrices_in_range(w, h, p1, p2, r)
            assert bad == 0, f"{what}, ratio {r}: {bad} matrices outside the tiled warp kernels' range: the frame would take the general warp kernel on the id-map path"
        local = None
        if "lengths" in exp or exp.get("leaves_image"):
            c1, c2, g = U.sources(w, h, 1)
            d = O.morph_images(c1, c2, g, p1, p2, r, r, 64, debug=True)[2]
            local, counts2 = U.local_ids(w, h, p1, p2, r, tile_w, d["triMap"])
            assert (counts2 == counts).all()
        if "lengths" in exp:
            owned = U.last_entry_pixels(local, counts, tile_w)
            for v in exp["lengths"]:
                assert (counts == v).any(), f"{what}: no tile with a list of {v} entries"
                best = int(owned[counts == v].max())
                assert v == 0 or best >= U.OWNED, (f"{what}: in no tile with a list of {v} entries does entry {v} own {U.OWNED} pixels or more (at most {best}): "
                                                   f"id {v} never reaches the picture, the branch at list length {v} is not seen")
        if "longest" in exp:
            lo, hi = exp["longest"]
            assert lo <= longest <= hi, f"{what}, ratio {r}: the longest list has {longest} entries, not {lo}..{hi}"
        if "every" in exp:
            lo, hi = exp["every"]
            assert lo <= int(counts.min()) and longest <= hi, f"{what}, ratio {r}: lists of {int(counts.min())}..{longest} entries, not {lo}..{hi}"
        if "fill" in exp:
            lo, hi = exp["fill"]
            assert lo * cap <= total <= hi * cap, f"{what}: {total} entries are {total / cap:.4f} of the room ({cap}), not {lo}..{hi}"
        if "edges" in exp:
            steps = U.edge_steps(w, h, p1, p2, r)
            for shape in exp["edges"]:
                assert U.has_edge(steps, shape, w, h), f"{what}: the mesh has no {shape} edge"
        if exp.get("leaves_image"):
            for k in "12":
                x, y = d["mapx" + k], d["mapy" + k]
                out = (x < 0) | (y < 0) | (x > w - 1) | (y > h - 1)
                assert (out & (local >= U.SLOTS)).sum() >= U.OWNED, (f"{what}, ratio {r}: fewer than {U.OWNED} pixels with an id of {U.SLOTS} or more have a footprint in "
                                                                       f"source {k} that leaves the image: the border path does not read an overflow record")
