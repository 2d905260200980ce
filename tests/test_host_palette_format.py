"""CPU tests of the PAL8 hand-off format (include/poppy_hip.h: POPPY_FRAME_PAL8): poppy_bgr_to_pal8 against a numpy restatement of the format's four
steps, bit for bit; the properties the format promises (exact frames, indices below the box count, cells inside their boxes, unused entries zero);
its quality against Pillow's median cut; poppy_frame_bytes; the pixel limit; and the GIF89a sink (POPPY_SINK_GIF) against a decoder written here
and against Pillow's."""
import os

import numpy as np
import pytest

from palette_util import GOLDEN, frames, gif_decode, pal8_reference, photo
from poppy_amd import capi, synth

E_ARG, E_UNSUPPORTED = -1, -6


def cars():
    return np.load(os.path.join(GOLDEN, "a_749x480_cars.npz"))["frame0"]


FRAMES = frames()


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_bgr_to_pal8_matches_the_definition(name):
    f = FRAMES[name]
    h, w = f.shape[:2]
    want, boxes = pal8_reference(f)
    got = capi.bgr_to_pal8(f)
    assert got.size == capi.frame_bytes(capi.FRAME_PAL8, w, h) == w * h + 768
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{name}: {neq.size} bytes differ, first at {neq[0]} (index plane ends at {w * h}); {len(boxes)} boxes"
    padded = capi.bgr_to_pal8(f, row_pad=13)
    assert np.array_equal(padded, want), f"{name}: a padded stride changes the frame"


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_promises_of_the_format(name):
    f = FRAMES[name]
    h, w = f.shape[:2]
    _, boxes = pal8_reference(f)
    got = capi.bgr_to_pal8(f)
    idx, pal = got[:w * h].astype(np.int64), got[w * h:].reshape(256, 3)
    assert idx.max() < len(boxes), f"{name}: index {idx.max()} with {len(boxes)} boxes"
    assert not pal[len(boxes):].any(), f"{name}: unused palette entries are not zero"
    rgb = f.reshape(-1, 3)[:, ::-1].astype(np.int64)
    lo = np.array([b[0] for b in boxes])[idx]; hi = np.array([b[1] for b in boxes])[idx]
    assert ((rgb >> 3) >= lo).all() and ((rgb >> 3) <= hi).all(), f"{name}: a pixel's cell lies outside its box"
    err = np.abs(pal[idx].astype(np.int64) - rgb)
    assert (err < 8 * (hi - lo + 1)).all(), f"{name}: a channel is further from its palette entry than its box is wide"


def test_exact_frames_and_box_counts():
    """At most 256 occupied cells with one colour per cell: palette[index] is the frame."""
    for name in ("cells_256", "flat", "two_tone", "1x1", "1x7", "5x3", "equal_scores", "equal_sides", "rb_tie_clamped", "lattice"):
        f = FRAMES[name]
        h, w = f.shape[:2]
        assert np.array_equal(capi.pal8_to_bgr(capi.bgr_to_pal8(f), w, h), f), f"{name} does not come back exactly"
    assert len(pal8_reference(FRAMES["cells_256"])[1]) == 256 and len(pal8_reference(FRAMES["cells_257"])[1]) == 256
    assert len(pal8_reference(FRAMES["flat"])[1]) == 1 and len(pal8_reference(FRAMES["two_tone"])[1]) == 2
    f = FRAMES["cells_257"]
    assert not np.array_equal(capi.pal8_to_bgr(capi.bgr_to_pal8(f), 64, 40), f)
    # the tie rules, spelled out: the cube's first cut is along G (box 1 = the high-G half), the second cut is box 0's, along R
    got = capi.bgr_to_pal8(FRAMES["equal_sides"])
    idx = got[:8 * 16].reshape(8, 16)[:, 0]                   # rows k: B bit 0, G bit 1, R bit 2 of k
    assert idx[0] == 0 and idx[2] == 1 and idx[4] == 2, idx


def psnr(a, b):
    m = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if m == 0 else 10 * np.log10(255.0 ** 2 / m)


def test_quality_against_pillow_median_cut(capsys):
    """An outside yardstick: on each image not more than 1.5 dB below Pillow's quantize(256, MEDIANCUT, dither NONE).  Measured with Pillow 12.2
    (ours / Pillow, dB): photo a 34.29 / 35.05, photo b 34.46 / 35.45, cars frame 0 41.06 / 38.55, textured 640x360 30.05 / 28.45."""
    Image = pytest.importorskip("PIL.Image")
    images = {"photo_a": photo("a"), "photo_b": photo("b"), "cars_frame0": cars(), "textured_640x360": synth.textured_bgr(640, 360, 3)}
    rows = []
    for name, im in images.items():
        h, w = im.shape[:2]
        ours = psnr(capi.pal8_to_bgr(capi.bgr_to_pal8(im), w, h), im)
        q = Image.fromarray(im[:, :, ::-1].copy()).quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB")
        theirs = psnr(np.asarray(q)[:, :, ::-1], im)
        rows.append((name, ours, theirs))
    with capsys.disabled():
        for name, ours, theirs in rows:
            print(f"\n  PAL8 quality {name}: {ours:.2f} dB, Pillow median cut {theirs:.2f} dB", end="")
    for name, ours, theirs in rows:
        assert ours >= theirs - 1.5, f"{name}: {ours:.2f} dB against Pillow's {theirs:.2f} dB"


def test_frame_bytes_and_limits():
    assert capi.FRAME_PAL8 == 8 and capi.SINK_GIF == 8
    assert capi.frame_bytes(capi.FRAME_PAL8, 1920, 1080) == 1920 * 1080 + 768
    assert capi.frame_bytes(capi.FRAME_PAL8, 3840, 2160) == 3840 * 2160 + 768
    assert capi.frame_bytes(capi.FRAME_PAL8, 1, 1) == 769 and capi.frame_bytes(capi.FRAME_PAL8, 5, 3) == 783
    assert capi.frame_bytes(capi.FRAME_PAL8, 0, 10) == 0 and capi.frame_bytes(capi.FRAME_PAL8, 10, -1) == 0
    assert capi.frame_bytes(2, 10, 10) == 0 and capi.frame_bytes(4, 10, 10) == 0 and capi.frame_bytes(7, 10, 10) == 0 and capi.frame_bytes(9, 10, 10) == 0
    assert "poppy_bgr_to_pal8" in capi.SYMBOLS and hasattr(capi.lib(), "poppy_bgr_to_pal8")
    out = np.zeros(800, np.uint8)
    assert capi.lib().poppy_bgr_to_pal8(None, 3, 1, 1, capi._p(out)) == E_ARG
    assert capi.lib().poppy_bgr_to_pal8(capi._p(out), 3, 0, 1, capi._p(out)) == E_ARG
    assert capi.lib().poppy_bgr_to_pal8(capi._p(out), 2, 1, 1, capi._p(out)) == E_ARG
    assert capi.lib().poppy_hip_set_frame_format(None, capi.FRAME_PAL8) == E_ARG
    assert capi.lib().poppy_hip_pool_set_frame_format(None, capi.FRAME_PAL8) == E_ARG


def test_pixel_limit_keeps_the_sums_in_32_bits():
    """2^24 pixels of 255 is the largest sum a cell can hold in 32 bits: that frame is taken (and exact), one more row is refused."""
    w, h = 4096, 4096
    f = np.full((h, w, 3), 255, np.uint8)
    got = capi.bgr_to_pal8(f)
    assert not got[:w * h].any() and tuple(got[w * h:w * h + 3]) == (255, 255, 255) and not got[w * h + 3:].any()
    del got
    f = np.full((h + 1, w, 3), 255, np.uint8)
    out = np.zeros(1, np.uint8)                                  # refused before a byte is read or written
    assert capi.lib().poppy_bgr_to_pal8(capi._p(f), w * 3, w, h + 1, capi._p(out)) == E_UNSUPPORTED
    with pytest.raises(capi.PoppyError, match=str(E_UNSUPPORTED)):
        capi.bgr_to_pal8(f)


# ---- the GIF sink ----------------------------------------------------------------------------------------------------------------------------
def write_gif(path, frames_pal8, w, h, fps=(25, 1)):
    s = capi.lib().poppy_sink_open(str(path).encode(), capi.SINK_GIF, w, h, fps[0], fps[1])
    assert s
    for f in frames_pal8:
        capi.lib().poppy_sink_write(s, capi._p(f), w, h, w)
    return capi.lib().poppy_sink_close(s)


def gif_cases():
    rng = np.random.default_rng(3)
    tex = synth.textured_bgr(640, 360, 5)
    three = [synth.textured_bgr(96, 64, k) for k in (1, 2)] + [rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)]
    return {"5x3": [rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)], "64x48": [synth.textured_bgr(64, 48, 7), rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)],
            "1x7": [rng.integers(0, 256, (7, 1, 3), dtype=np.uint8)], "textured_640x360": [tex], "flat": [np.full((40, 60, 3), (9, 99, 199), np.uint8)],
            "three_palettes": three}


GIFS = gif_cases()


@pytest.mark.parametrize("name", sorted(GIFS))
def test_gif_sink_decodes_to_the_frames(tmp_path, name):
    bgr = GIFS[name]
    h, w = bgr[0].shape[:2]
    pal8 = [capi.bgr_to_pal8(f) for f in bgr]
    path = tmp_path / "out.gif"
    assert write_gif(path, pal8, w, h) == len(bgr)
    data = path.read_bytes()
    g = gif_decode(data)
    assert g["header"] == b"GIF89a" and g["screen"] == (w, h, 0x70, 0, 0) and g["loop"] == 0
    assert data[13:32] == b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"
    assert len(g["frames"]) == len(bgr)
    for k, (delay, fw, fh, pal, idx) in enumerate(g["frames"]):
        assert (delay, fw, fh) == (4, w, h)                                    # 25 frames/s
        assert np.array_equal(pal.ravel(), pal8[k][w * h:]) and np.array_equal(idx, pal8[k][:w * h]), f"{name}: frame {k} differs"
        assert np.array_equal(pal[idx][:, ::-1].reshape(h, w, 3), capi.pal8_to_bgr(pal8[k], w, h))
    if name == "textured_640x360":
        assert g["clears"] > 1, "a frame this long fills the code table"
    if name == "three_palettes":
        assert len({g["frames"][k][3].tobytes() for k in range(3)}) == 3
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.n_frames == len(bgr) and im.size == (w, h) and im.info.get("loop") == 0
        for k in range(len(bgr)):
            im.seek(k)
            assert im.info.get("duration") == 40
            assert np.array_equal(np.asarray(im.convert("RGB"))[:, :, ::-1], capi.pal8_to_bgr(pal8[k], w, h)), f"{name}: Pillow's frame {k} differs"


@pytest.mark.parametrize("fps,cs", [((25, 1), 4), ((30, 1), 3), ((60, 1), 2), ((1000, 1), 1), ((1, 2), 200), ((30000, 1001), 3), ((0, 0), 3), ((8, 1), 13), ((3, 1), 33)])
def test_gif_delay(tmp_path, fps, cs):
    f = capi.bgr_to_pal8(GIFS["5x3"][0])
    path = tmp_path / "d.gif"
    assert write_gif(path, [f, f], 5, 3, fps) == 2
    assert [fr[0] for fr in gif_decode(path.read_bytes())["frames"]] == [cs, cs]


def test_gif_sink_refuses_other_frames(tmp_path):
    w, h = 8, 6
    f = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    L = capi.lib()
    s = L.poppy_sink_open(str(tmp_path / "a.gif").encode(), capi.SINK_GIF, w, h, 25, 1)
    L.poppy_sink_write(s, capi._p(capi.bgr_to_pal8(f)), w, h, w)
    L.poppy_sink_write(s, capi._p(f), w, h, w * 3)                             # a BGR frame poisons the sink
    L.poppy_sink_write(s, capi._p(capi.bgr_to_pal8(f)), w, h, w)
    assert L.poppy_sink_close(s) < 0
    s = L.poppy_sink_open(str(tmp_path / "b.gif").encode(), capi.SINK_GIF, w, h, 25, 1)
    L.poppy_sink_write(s, capi._p(capi.bgr_to_pal8(f)), w, h + 1, w)           # another geometry
    assert L.poppy_sink_close(s) < 0
    for fmt in (capi.SINK_RAW, capi.SINK_PPM, capi.SINK_Y4M):                  # a PAL8 frame at the BGR sinks
        s = L.poppy_sink_open(str(tmp_path / f"c{fmt}_%d.out").encode(), fmt, w, h, 25, 1)
        L.poppy_sink_write(s, capi._p(capi.bgr_to_pal8(f)), w, h, w)
        assert L.poppy_sink_close(s) < 0
    # GIF's screen is 16 bits wide and high: such a sink fails every frame
    for ww, hh in ((65536, 1), (1, 65536)):
        s = L.poppy_sink_open(str(tmp_path / "big.gif").encode(), capi.SINK_GIF, ww, hh, 25, 1)
        assert s
        L.poppy_sink_write(s, capi._p(np.zeros(ww * hh + 768, np.uint8)), ww, hh, ww)
        assert L.poppy_sink_close(s) < 0
    s = L.poppy_sink_open(str(tmp_path / "edge.gif").encode(), capi.SINK_GIF, 65535, 1, 25, 1)
    L.poppy_sink_write(s, capi._p(np.zeros(65535 + 768, np.uint8)), 65535, 1, 65535)
    assert L.poppy_sink_close(s) == 1
    for fmt in (4, 5, 6, 7, 9):
        assert not L.poppy_sink_open(b"/dev/null", fmt, 8, 8, 25, 1)
