"""CPU tests of the content that tests/test_gpu_palette_content.py puts in front of the palette and I420 kernels (palette_util.adversarial_frames,
big_noise, primaries).  Two things: the host statements (poppy_bgr_to_pal8, poppy_bgr_frames_to_pal8, poppy_bgr_to_i420) equal the numpy rule on it, byte
for byte, so that the GPU file may compare with them; and the frames are what they claim to be — the figures of palette_util.cut_trace follow from how each
frame is built, and a frame that lost them would leave the GPU comparisons passing without reaching the code they are for."""
import numpy as np
import pytest

import palette_util as P
from palette_seq_util import frames_of_stacked, stacked
from poppy_amd import capi
from test_host_frame_format import i420_reference

FRAMES = {**P.adversarial_frames(), **P.big_noise()}
SEQUENCES = {"cube_noise": ("cube_uniform", "noise_256x128"), "cube_noise_cube": ("cube_uniform", "noise_256x128", "cube_uniform"),
             "lines_rg": ("line_r", "line_g"), "lines_rgb": ("line_r", "line_g", "line_b"),
             "lattice_tail": ("lattice512", "heavy_tail"), "lattice_tail_lattice": ("lattice512", "heavy_tail", "lattice512"),
             "slab_mirror": ("last_slab", "last_slab_mirror"), "slab_mirror_slab": ("last_slab", "last_slab_mirror", "last_slab"),
             "big_noise": ("noise_1280x1024_a", "noise_1280x1024_b")}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_bgr_to_pal8_matches_the_definition(name):
    f = FRAMES[name]
    h, w = f.shape[:2]
    want, boxes = P.pal8_reference(f)
    got = capi.bgr_to_pal8(f)
    assert got.size == w * h + 768
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{name}: {neq.size} bytes differ, first at {neq[0]} (index plane ends at {w * h}); {len(boxes)} boxes"


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_sequences_match_the_definition(name):
    """The sequence rule: the frames stacked into one image, by the numpy rule."""
    fr = np.stack([FRAMES[k] for k in SEQUENCES[name]])
    n, h, w = fr.shape[:3]
    want = frames_of_stacked(P.pal8_reference(stacked(fr))[0], n, w, h)
    got = capi.bgr_frames_to_pal8(fr)
    neq = np.argwhere(got != want)
    assert neq.size == 0, f"{name}: {len(neq)} bytes differ, first at frame {neq[0][0]}, byte {neq[0][1]} (index plane ends at {w * h})"


def test_the_cube_and_the_lattice_tie_across_register_banks():
    """Equal counts in every cell: 255 cuts, 146 / 73 / 36 along R / G / B, 247 of them with more than one best box, 64 with best boxes 64 or more indices apart."""
    for name in ("cube_uniform", "lattice512"):
        t = P.cut_trace(FRAMES[name])
        assert t == {"boxes": 256, "axis_cuts": [146, 73, 36], "clamped": 0, "tied": 247, "cross_bank": 64}, f"{name}: {t}"
    assert len(np.unique(FRAMES["cube_uniform"].reshape(-1, 3) >> 3, axis=0)) == 32768


def test_the_lines_cut_one_axis_each_and_stop_at_32_boxes():
    for axis, name in enumerate(("line_r", "line_g", "line_b")):
        t = P.cut_trace(FRAMES[name])
        want = [0, 0, 0]
        want[axis] = 31
        assert t["boxes"] == 32 and t["axis_cuts"] == want, f"{name}: {t}"
        got = capi.bgr_to_pal8(FRAMES[name])
        assert not got[64 * 32 + 3 * 32:].any(), f"{name}: palette entries behind the 32 boxes are not zero"


def test_clamped_medians():
    t = P.cut_trace(FRAMES["last_slab"])
    assert t["boxes"] == 4 and t["clamped"] >= 1, t
    t = P.cut_trace(FRAMES["heavy_tail"])
    cells = len(np.unique(FRAMES["heavy_tail"].reshape(-1, 3) >> 3, axis=0))
    assert cells == 41 and t["boxes"] == cells and t["clamped"] >= 1, t
    px = FRAMES["heavy_tail"].reshape(-1, 3) >> 3
    assert (px == 31).all(axis=1).sum() >= 0.99 * len(px)


def test_big_noise_overflows_a_workgroups_table():
    """More distinct cells in workgroup 0 than its LDS table has entries: some go to the global tables directly, whatever the hash does."""
    for name in ("noise_1280x1024_a", "noise_1280x1024_b"):
        f = FRAMES[name]
        assert f.shape[0] * f.shape[1] > P.HIST_SLOTS * P.HIST_MAX_BLOCKS
        assert P.first_workgroup_cells(f) > P.HIST_SLOTS, f"{name}: {P.first_workgroup_cells(f)} cells"
    assert P.first_workgroup_cells(FRAMES["noise_256x128"]) <= P.HIST_SLOTS          # (the small noise frame does not: that is why the large ones exist)


@pytest.mark.parametrize("w,h", P.PRIMARIES_SIZES, ids=[f"{w}x{h}" for w, h in P.PRIMARIES_SIZES])
def test_primaries_reach_both_chroma_clamps(w, h):
    """first = 1 / 4: the block at the origin is blue / red, so even the 1 x 1 frames reach U = 255 / V = 255."""
    for first in (1, 4):
        f = P.primaries(w, h, first)
        got = capi.bgr_to_i420(f)
        want = i420_reference(f)
        neq = np.flatnonzero(got != want)
        assert neq.size == 0, f"{w}x{h}, first {first}: {neq.size} bytes differ, first at {neq[0]}"
        n_c = ((w + 1) // 2) * ((h + 1) // 2)
        u, v = got[w * h:w * h + n_c], got[w * h + n_c:]
        if w * h == 1:
            assert (u[0] if first == 1 else v[0]) == 255
        else:
            assert u.max() == 255 and v.max() == 255 and min(u.min(), v.min()) == 1, f"{w}x{h}: U {u.min()}..{u.max()}, V {v.min()}..{v.max()}"
