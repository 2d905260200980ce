"""CPU tests of the GIF hand-off format (include/poppy_hip.h: POPPY_FRAME_GIF) and its sink (POPPY_SINK_GIF_CODED): poppy_pal8_to_gif_frame against a
plain-Python restatement of the segment rule, byte for byte; Pillow's decoding of the sink's file; the sub-block framing at its boundaries; the capacity;
the refusals; and the coded sizes of three inputs beside the sizes POPPY_SINK_GIF's whole-image coder gives for them."""
import os

import numpy as np
import pytest

import gif_coded_util as U
from poppy_amd import capi, synth

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
E_ARG, E_UNSUPPORTED = -1, -6
S = U.segment_pixels()


def write_sink(path, sink, frames, w, h, stride):
    s = capi.lib().poppy_sink_open(str(path).encode(), sink, w, h, 25, 1)
    assert s
    for f in frames:
        capi.lib().poppy_sink_write(s, capi._p(np.ascontiguousarray(f)), w, h, stride)
    return capi.lib().poppy_sink_close(s)


def check_pillow(path, pal8_frames, w, h):
    Image = pytest.importorskip("PIL.Image")
    with Image.open(path) as im:
        assert im.n_frames == len(pal8_frames) and im.size == (w, h) and im.info.get("loop") == 0
        for k, p in enumerate(pal8_frames):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert("RGB"))[:, :, ::-1], capi.pal8_to_bgr(p, w, h)), f"Pillow's frame {k} differs"


def test_segment_constant_and_values():
    assert S in (1024, 2048, 4096)
    assert capi.FRAME_GIF == 64 and capi.SINK_GIF_CODED == 64
    assert capi.frame_bytes(capi.FRAME_GIF, 8, 8) > 0 and capi.frame_bytes(32, 8, 8) == 0


@pytest.mark.parametrize("content", U.CONTENTS)
def test_pal8_to_gif_frame_matches_the_restatement(content):
    """Every pixel count around one and two segments, as one row and 67 wide.  All-zero gives the longest strings; noise a code per pixel (from 3839 pixels
    on that fills the table: a restart inside a segment when S = 4096); the restatement asserts byte-aligned segments with at most seven padding clears."""
    for w, h in U.shapes(S):
        pal8 = U.pal8_of(U.index_plane(content, w * h), seed=w)
        got = capi.pal8_to_gif_frame(pal8, w, h)
        want = U.gif_frame_reference(pal8, w, h, S)
        assert bytes(got) == want, f"{content} {w}x{h}: {len(got)} bytes against {len(want)}"
        total, pal, _ = U.split_frame(got)
        assert total == capi.gif_frame_bytes(got) and np.array_equal(pal, pal8[w * h:])
        assert total <= capi.frame_bytes(capi.FRAME_GIF, w, h)


def test_full_table_restart_is_reached():
    """4096 pixels that cost a code each fill the table after 3838 strings, whatever S is: the whole-image rule (one segment of the restatement) restarts, and
    with S = 4096 the segment does too."""
    n = 4096
    pal8 = U.pal8_of(U.all_distinct(n))
    bits = U.Bits()
    U.lzw_codes(pal8[:n], bits)
    assert bits.clears == 2                                 # the one in front and the restart
    assert bytes(capi.pal8_to_gif_frame(pal8, n, 1)) == U.gif_frame_reference(pal8, n, 1, S)


def test_sink_file_decodes_to_the_pal8_pixels(tmp_path):
    """The coded sink's file from the restatement cases and from textured frames, read by Pillow: palette[index] of the PAL8 frames, the pixels the GIF sink's
    file decodes to; and the coded sink writes POPPY_SINK_GIF's framing around the frames' own bytes."""
    for content in U.CONTENTS:
        for w, h in U.shapes(S)[3:]:                        # (Pillow takes a while on one-row images thousands wide: the planes 67 wide and S + 1, 2 S + 1 as rows)
            pal8 = [U.pal8_of(U.index_plane(content, w * h, seed=k), seed=k) for k in range(2)]
            coded = [capi.pal8_to_gif_frame(p, w, h) for p in pal8]
            path = tmp_path / f"{content}_{w}x{h}.gif"
            assert write_sink(path, capi.SINK_GIF_CODED, coded, w, h, 0) == 2
            check_pillow(path, pal8, w, h)
    for w, h in ((S + 1, 1), (2 * S + 1, 1)):
        pal8 = [U.pal8_of(U.index_plane("noise", w * h))]
        path = tmp_path / f"row_{w}.gif"
        assert write_sink(path, capi.SINK_GIF_CODED, [capi.pal8_to_gif_frame(pal8[0], w, h)], w, h, 0) == 1
        check_pillow(path, pal8, w, h)
    w, h = 96, 64
    bgr = [synth.textured_bgr(w, h, k) for k in (1, 2, 3)]
    pal8 = [capi.bgr_to_pal8(f) for f in bgr]
    coded = [capi.bgr_to_gif_frame(f) for f in bgr]
    for p, c in zip(pal8, coded):
        assert bytes(c) == bytes(capi.pal8_to_gif_frame(p, w, h))
    path, plain = tmp_path / "textured.gif", tmp_path / "plain.gif"
    assert write_sink(path, capi.SINK_GIF_CODED, coded, w, h, 0) == 3
    assert write_sink(plain, capi.SINK_GIF, pal8, w, h, w) == 3
    check_pillow(path, pal8, w, h)
    check_pillow(plain, pal8, w, h)
    data = path.read_bytes()
    assert data[:32] == plain.read_bytes()[:32] and data[-1] == 0x3B
    at = 32
    for c in coded:
        assert data[at:at + 8] == b"\x21\xf9\x04\x00\x04\x00\x00\x00" and data[at + 8] == 0x2C and data[at + 17] == 0x87
        assert data[at + 18:at + 18 + len(c) - 4] == bytes(c[4:])
        at += 18 + len(c) - 4
    assert at == len(data) - 1


def test_sub_block_framing_at_its_boundaries():
    """Noise of n = 200 .. 479 pixels in one row, three planes per count (a pixel more is nine or ten bits more, so one plane per count steps over some
    lengths): the payloads pass 254, 255, 256 and 510, 511 bytes (a full sub-block, one byte more, two full ones)."""
    seen = {}
    for n, seed in U.sweep_cases(1):
        pal8 = U.pal8_of(U.index_plane("noise", n, seed))
        got = capi.pal8_to_gif_frame(pal8, n, 1)
        total, _, payload = U.split_frame(got)              # (asserts: total = the bytes present, no empty sub-block, the terminator last)
        assert bytes(got) == U.gif_frame_reference(pal8, n, 1, S)
        assert total == 772 + 1 + len(payload) + (len(payload) + 254) // 255 + 1
        seen[len(payload)] = n
    for want in (254, 255, 256, 510, 511):
        assert want in seen, f"no payload of {want} bytes in the sweep: {sorted(seen)}"


def test_capacity_holds_for_incompressible_planes():
    """frame_bytes(FRAME_GIF) bounds any content: noise and a plane in which no pair of neighbours repeats (a code per pixel, the worst case of the header's
    derivation), at 3 S + 5 pixels and at segment sizes."""
    for n in (3 * S + 5, S, 1, S + 1):
        for idx in (U.index_plane("noise", n), U.all_distinct(n)):
            got = capi.pal8_to_gif_frame(U.pal8_of(idx), n, 1)
            assert len(got) <= capi.frame_bytes(capi.FRAME_GIF, n, 1), (n, len(got))
    n = 3 * S + 5
    got = capi.pal8_to_gif_frame(U.pal8_of(U.all_distinct(n)), n, 1)
    assert len(got) > 9 * n // 8                            # no pixel came cheaper than nine bits: the plane is the worst case it claims to be
    segments = -(-n // S)
    seg_bytes = (9 + 12 * (S + 2) + 63 + 7) // 8            # the header's bound
    payload = segments * seg_bytes
    assert capi.frame_bytes(capi.FRAME_GIF, n, 1) == 772 + 1 + payload + (payload + 254) // 255 + 1


def test_refusals_and_sinks(tmp_path):
    L = capi.lib()
    tiny = np.zeros(16, np.uint8)
    # refused on the arguments alone: the buffers are far too small for these frames, nothing may be read or written
    for w, h in ((4097, 4096), (65536, 1), (1, 65536)):
        assert L.poppy_pal8_to_gif_frame(capi._p(tiny), w, h, capi._p(tiny)) == E_UNSUPPORTED
        assert L.poppy_bgr_to_gif_frame(capi._p(tiny), w * 3, w, h, capi._p(tiny)) == E_UNSUPPORTED
    assert not tiny.any()
    assert L.poppy_pal8_to_gif_frame(None, 4, 4, capi._p(tiny)) == E_ARG and L.poppy_pal8_to_gif_frame(capi._p(tiny), 0, 4, capi._p(tiny)) == E_ARG
    assert capi.frame_bytes(capi.FRAME_GIF, 0, 4) == 0
    w, h = 8, 6
    f = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    pal8, coded = capi.bgr_to_pal8(f), capi.bgr_to_gif_frame(f)
    for sink, name in ((capi.SINK_RAW, "a.raw"), (capi.SINK_PPM, "a_%d.ppm"), (capi.SINK_Y4M, "a.y4m"), (capi.SINK_Y4M420, "b.y4m"), (capi.SINK_GIF, "a.gif"),
                       (capi.SINK_GIF_GLOBAL, "b.gif")):
        assert write_sink(tmp_path / name, sink, [coded], w, h, 0) < 0, f"sink {sink} took a coded frame"
    assert write_sink(tmp_path / "c.gif", capi.SINK_GIF_CODED, [pal8], w, h, w) < 0            # a PAL8 frame at the coded sink
    assert write_sink(tmp_path / "d.gif", capi.SINK_GIF_CODED, [f], w, h, w * 3) < 0           # a BGR frame
    assert write_sink(tmp_path / "e.gif", capi.SINK_GIF_CODED, [coded, coded], w, h, 0) == 2
    s = L.poppy_sink_open(str(tmp_path / "f.gif").encode(), capi.SINK_GIF_CODED, w, h + 1, 25, 1)      # another geometry
    L.poppy_sink_write(s, capi._p(coded), w, h, 0)
    assert L.poppy_sink_close(s) < 0
    s = L.poppy_sink_open(str(tmp_path / "g.gif").encode(), capi.SINK_GIF_CODED, 65536, 1, 25, 1)      # GIF's 16-bit screen
    assert s
    L.poppy_sink_write(s, capi._p(coded), 65536, 1, 0)
    assert L.poppy_sink_close(s) < 0
    for fmt in (32, 63, 65):
        assert not L.poppy_sink_open(b"/dev/null", fmt, 8, 8, 25, 1)


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------
def chained_256x192(n=60):
    """A 60-frame chained sequence at 256 x 192 on the CPU: the oracle's frame loop on the textured golden pair with the reference's own point pairs and mask field."""
    import golden_util as G
    import oracle_lib as O
    inp = G.astage_inputs("a_256x192_textured")
    setup = {"points1": G.full("a_256x192_textured", "prepared1"), "points2": G.full("a_256x192_textured", "prepared2"), "gabor2": G.full("a_256x192_textured", "gabor2")}
    return O.morph(inp["img1"], inp["img2"], n, setup=setup)


def sizes_of(frames, tmp_path, name):
    h, w = frames[0].shape[:2]
    pal8 = [capi.bgr_to_pal8(f) for f in frames]
    coded = [capi.pal8_to_gif_frame(p, w, h) for p in pal8]
    a, b = tmp_path / f"{name}_coded.gif", tmp_path / f"{name}_plain.gif"
    assert write_sink(a, capi.SINK_GIF_CODED, coded, w, h, 0) == len(frames)
    assert write_sink(b, capi.SINK_GIF, pal8, w, h, w) == len(frames)
    return sum(len(c) for c in coded), os.path.getsize(a), os.path.getsize(b)


# (the frames' bytes, the coded sink's file, the GIF sink's file) as the host statement produces them with POPPY_GIF_SEGMENT_PIXELS = 2048: measured, not capped
# (ratios of the two files: 1.1641, 1.0822, 0.9896 — every segment starts a new table, and a 256 x 192 frame's whole-image table is itself restarted often)
SIZES = {"cars_frame0": (132495, 132542, 113856), "textured_640x360": (191234, 191281, 176746), "chained_256x192_x60": (2235782, 2236655, 2260242)}


@pytest.mark.parametrize("name", sorted(SIZES))
def test_coded_sizes_are_pinned(tmp_path, name, capsys):
    if name == "cars_frame0":
        frames = [np.load(os.path.join(GOLDEN, "a_749x480_cars.npz"))["frame0"]]
    elif name == "textured_640x360":
        frames = [synth.textured_bgr(640, 360, 3)]
    else:
        frames = chained_256x192()
        assert len(frames) == 60 and frames[0].shape == (192, 256, 3)
    got = sizes_of(frames, tmp_path, name)
    with capsys.disabled():
        print(f"\n{name}: frames {got[0]} B, coded file {got[1]} B, plain file {got[2]} B, ratio {got[1] / got[2]:.4f}")
    assert S == 2048, "the pinned sizes are those of 2048-pixel segments"
    assert got == SIZES[name]
