"""CPU checks of the JPEG hand-off format (include/poppy_hip.h: POPPY_FRAME_JPEG) and the MJPEG sink: the header's tables against the files Pillow writes,
the integer DCT against a double-precision one at the standard's bound, the host statement poppy_i420_to_jpeg_frame byte for byte against the numpy
restatement in tests/jpeg_util.py, the branches the content reaches, decoding by Pillow, capacity and refusals, and the AVI file chunk by chunk."""
import io

import numpy as np
import pytest

import jpeg_util as U
from palette_util import textured
from poppy_amd import capi

Image = pytest.importorskip("PIL.Image")
E_ARG, E_UNSUPPORTED = -1, -6
R = U.restart_mcus()


def _pil_file(quality=None, qtables=None, size=(32, 32)):
    im = Image.fromarray(np.random.default_rng(5).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8))
    b = io.BytesIO()
    if qtables is None:
        im.save(b, "JPEG", quality=quality, subsampling=2, optimize=False)
    else:
        im.save(b, "JPEG", qtables=qtables, subsampling=2, optimize=False)
    return b.getvalue()


def _frame(data):
    """a JFIF file as a frame: `total` in front"""
    return np.frombuffer((len(data) + 4).to_bytes(4, "little") + data, np.uint8)


def test_constants():
    assert R == 8, "POPPY_JPEG_RESTART_MCUS (DESIGN.md section 4, JPEG hand-off)"
    assert capi.FRAME_JPEG == 256 and capi.SINK_MJPEG == 256 and capi.JPEG_QUALITY_DEFAULT == 90
    for fmt in (255, 257):
        assert capi.frame_bytes(fmt, 64, 64) == 0


def test_quantisation_tables_equal_pillows_at_every_quality():
    for q in range(1, 101):
        mine = U.walk_frame(capi.i420_to_jpeg_frame(U.i420_content("flat128", 16, 16), 16, 16, q))["qtables"]
        theirs = U.walk_frame(_frame(_pil_file(quality=q)))["qtables"]
        ql, qc = U.quant_tables(q)
        assert mine[0] == theirs[0] == [int(x) for x in ql[U.ZIGZAG]], f"quality {q}, table 0"
        assert mine[1] == theirs[1] == [int(x) for x in qc[U.ZIGZAG]], f"quality {q}, table 1"


def test_huffman_tables_equal_pillows():
    mine = U.walk_frame(capi.i420_to_jpeg_frame(U.i420_content("flat128", 16, 16), 16, 16, 75))["dht"]
    theirs = U.walk_frame(_frame(_pil_file(quality=75)))["dht"]
    assert sorted(mine) == [(0, 0), (0, 1), (1, 0), (1, 1)] and mine == theirs
    for t in range(2):
        assert mine[(0, t)] == (list(U.DC_BITS[t]), U.DC_VALS) and mine[(1, t)] == (list(U.AC_BITS[t]), list(U.AC_VALS[t]))


def test_dct_table_is_the_rounded_orthonormal_dct():
    u, x = np.mgrid[0:8, 0:8]
    a = np.where(u == 0, np.sqrt(1 / 8), 0.5)
    assert np.array_equal(U.dct_table(), np.rint(16384 * a * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64))
    assert U.K == [int(round(8192 * np.cos(k * np.pi / 16))) for k in range(8)]


def _extreme_blocks():
    """flat 0 and 255, and for every (v, u) the saturated sign pattern of that basis function, which maximises the coefficient, and its negative"""
    y, x = np.mgrid[0:8, 0:8]
    out = [np.zeros((8, 8)), np.full((8, 8), 255)]
    for v in range(8):
        for u in range(8):
            basis = np.cos((2 * y + 1) * v * np.pi / 16) * np.cos((2 * x + 1) * u * np.pi / 16)
            out += [(basis > 0) * 255, (basis < 0) * 255]
    return np.array(out, np.uint8)


def test_dct_is_within_one_of_a_double_precision_dct():
    """ITU-T T.83's bar: every quantised coefficient within 1 of the double-precision DCT's, quantised alike.  The bound is the standard's, not a measured one."""
    fft = pytest.importorskip("scipy.fft")
    blocks = np.concatenate([np.random.default_rng(83).integers(0, 256, (2000, 8, 8), dtype=np.uint8), _extreme_blocks()])
    exact = fft.dctn(blocks.astype(np.float64) - 128, axes=(1, 2), norm="ortho")
    F = U.fdct(blocks)
    assert np.abs(F - 8 * exact).max() < 2.0, "the integer transform itself: within a quarter of a coefficient unit"
    for q in (100, 90, 10):
        for table in U.quant_tables(q):
            Q = table.reshape(8, 8)
            want = np.sign(exact) * np.floor(np.abs(exact) / Q + 0.5)
            assert np.abs(U.quantise(F, table) - want).max() <= 1, f"quality {q}"


def test_coefficient_ranges_and_the_reciprocal_division():
    """What the capacity's proof and the device's quantiser rest on: DC in -1024 .. 1016, AC magnitudes below 1024 (at Q = 1, on the blocks that maximise each
    coefficient), and (n * ceil(2^32 / d)) >> 32 == n // d for every divisor d = 8 Q and every n < 2^15."""
    q = U.quantise(U.fdct(_extreme_blocks()), np.ones(64, np.int64))
    assert q[:, 0, 0].min() == -1024 and q[:, 0, 0].max() == 1016
    ac = np.abs(q).reshape(-1, 64)[:, 1:]
    assert 1000 <= ac.max() <= 1023
    n = np.arange(1 << 15, dtype=np.uint64)
    for Q in range(1, 256):
        d = 8 * Q
        m = np.uint64(((1 << 32) + d - 1) // d)
        assert np.array_equal((n * m) >> np.uint64(32), n // np.uint64(d)), Q


@pytest.fixture(scope="module")
def coded():
    """{(content, w, h, quality): (the restatement's frame, the host statement's)} and what the restatement reached; coded once for the module"""
    stats, out = U.Stats(), {}
    for name in U.CONTENTS:
        for w, h in U.SIZES:
            for q in U.QUALITIES:
                a = U.i420_content(name, w, h)
                out[(name, w, h, q)] = (U.jpeg_frame_reference(a, w, h, q, R, stats), capi.i420_to_jpeg_frame(a, w, h, q))
    return out, stats


def test_host_statement_equals_the_restatement(coded):
    for key, (want, got) in coded[0].items():
        assert got.tobytes() == want, f"{key}: {got.size} bytes, the restatement gives {len(want)}"


def test_sizes_reach_short_and_straddling_segments_and_wrap_the_rst_number(coded):
    assert 9 % R != 0 and 3 % R != 0, "48 x 48: a segment straddles MCU rows, the last is short"
    assert len(U.walk_frame(coded[0][("noise", 48, 48, 90)][1])["segments"]) == -(-9 // R)
    w = U.walk_frame(coded[0][("noise", 160, 128, 90)][1])
    assert len(w["segments"]) == 80 // R >= 10 and w["rst"] == [k % 8 for k in range(80 // R - 1)]
    assert w["restart"] == R and w["data_offset"] == U.HEADER_BYTES


def test_content_reaches_every_branch(coded):
    s = coded[1]
    assert s.stuffed > 0, "a stuffed FF 00"
    assert s.zrl > 0, "a ZRL symbol"
    assert s.no_eob > 0, "a block whose last coefficient is non-zero"
    assert s.eob_only > 0, "a block of EOB alone"
    assert {0, 11} <= s.dc_cats, "DC categories 0 and 11"
    assert 10 in s.ac_cats, "an AC category 10"
    assert {0, 7} <= s.pads, "padding of 0 and of 7 bits"


def test_chosen_interval_pins_these_sizes(coded):
    """The frame lengths of the chosen interval's row of DESIGN.md's table, on the content above (another interval gives other lengths)."""
    assert {k: v[1].size for k, v in coded[0].items() if k[0] in ("noise", "gradient") and k[1:3] == (160, 128)} == PINNED_SIZES


PINNED_SIZES = {("gradient", 160, 128, 10): 1312, ("gradient", 160, 128, 90): 4780, ("gradient", 160, 128, 100): 9566,
                ("noise", 160, 128, 10): 5848, ("noise", 160, 128, 90): 23994, ("noise", 160, 128, 100): 48469}


def test_pillow_decodes_every_frame(coded):
    for (name, w, h, q), (_, got) in coded[0].items():
        parts = U.walk_frame(got)
        assert parts["order"] == [0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA] and parts["app0"] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
        assert parts["size"] == (w, h) and parts["sampling"] == [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)]
        n_seg = -(-(((w + 15) // 16) * ((h + 15) // 16)) // R)
        assert len(parts["segments"]) == n_seg and parts["rst"] == [k % 8 for k in range(n_seg - 1)]
        with Image.open(io.BytesIO(got[4:].tobytes())) as im:
            im.load()
            assert im.size == (w, h)
            assert im.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
            ql, qc = U.quant_tables(q)
            assert list(im.quantization[0]) == [int(x) for x in ql] and list(im.quantization[1]) == [int(x) for x in qc], "(Pillow hands tables out in natural order)"


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_quality_beside_pillows_encoder():
    """PSNR of the decoded RGB against the source, beside Pillow's own encoder (libjpeg-turbo) on the same BGR with the same tables and 4:2:0, on the two
    images of the textured 256 x 192 pair at quality 90.  Measured on the CPU: image 41 this coder 28.261 dB, Pillow 28.260 dB; image 42 this coder 28.847 dB,
    Pillow 28.833 dB (the texture is close to noise, and both lose its chroma to 4:2:0).  The gap, Pillow's minus this coder's, is -0.001 and -0.014 dB; the test
    allows it rounded up to the next 0.25 dB, which is 0."""
    for seed in (41, 42):
        bgr = textured(256, 192, seed)
        rgb = np.ascontiguousarray(bgr[:, :, ::-1])
        with Image.open(io.BytesIO(capi.bgr_to_jpeg_frame(bgr, 90)[4:].tobytes())) as im:
            mine = _psnr(np.asarray(im.convert("RGB")), rgb)
            tables = [list(im.quantization[0]), list(im.quantization[1])]
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, "JPEG", qtables=tables, subsampling=2, optimize=False)
        assert U.walk_frame(_frame(b.getvalue()))["qtables"] == U.walk_frame(capi.bgr_to_jpeg_frame(bgr, 90))["qtables"], "both files carry the same tables"
        with Image.open(b) as im:
            theirs = _psnr(np.asarray(im.convert("RGB")), rgb)
        print(f"textured {seed}: this coder {mine:.3f} dB, Pillow {theirs:.3f} dB")
        assert theirs - mine <= PSNR_GAP_DB


PSNR_GAP_DB = 0.0


def test_capacity_holds_at_quality_100(coded):
    for (name, w, h, q), (_, got) in coded[0].items():
        if q == 100:
            assert got.size <= capi.frame_bytes(capi.FRAME_JPEG, w, h), (name, w, h)
    n_seg = lambda w, h: -(-(((w + 15) // 16) * ((h + 15) // 16)) // R)
    for w, h in ((1, 1), (16 * R, 16), (16 * R + 1, 16), (1920, 1080)):
        assert capi.frame_bytes(capi.FRAME_JPEG, w, h) == 4 + 613 + n_seg(w, h) * (2 * ((6 * 1660 * R + 7) // 8) + 2)


def test_refusals_on_the_arguments_alone():
    L = capi.lib()
    one = np.zeros(16, np.uint8)                                # (refused before a byte of it is read)
    for w, h in ((65536, 1), (1, 65536), (65535, 65535)):       # a side above SOF0's 16 bits; a capacity above `total`'s 32
        assert L.poppy_i420_to_jpeg_frame(capi._p(one), w, h, 90, capi._p(one)) == E_UNSUPPORTED
        assert L.poppy_bgr_to_jpeg_frame(capi._p(one), w * 3, w, h, 90, capi._p(one)) == E_UNSUPPORTED
    for q in (0, 101, -5):
        assert L.poppy_i420_to_jpeg_frame(capi._p(one), 2, 2, q, capi._p(one)) == E_ARG
        assert L.poppy_bgr_to_jpeg_frame(capi._p(one), 6, 2, 2, q, capi._p(one)) == E_ARG
    assert L.poppy_i420_to_jpeg_frame(None, 2, 2, 90, capi._p(one)) == E_ARG and L.poppy_i420_to_jpeg_frame(capi._p(one), 0, 2, 90, capi._p(one)) == E_ARG
    assert L.poppy_bgr_to_jpeg_frame(capi._p(one), 5, 2, 2, 90, capi._p(one)) == E_ARG, "a stride below 3 * width"


def test_bgr_statement_is_the_composition():
    bgr = textured(61, 47, 3)
    assert np.array_equal(capi.bgr_to_jpeg_frame(bgr, 77), capi.i420_to_jpeg_frame(capi.bgr_to_i420(bgr), 61, 47, 77))


# ---- the sink ---------------------------------------------------------------------------------------------------------------------------------------------
def _write(path, fmt, w, h, frames, fps=(25, 2)):
    L = capi.lib()
    s = L.poppy_sink_open(str(path).encode(), fmt, w, h, fps[0], fps[1])
    assert s
    for f, stride in frames:
        L.poppy_sink_write(s, capi._p(f), w, h, stride)
    return L.poppy_sink_close(s)


def test_mjpeg_sink_file_chunk_by_chunk(tmp_path):
    w = h = 48
    frames = [capi.i420_to_jpeg_frame(U.i420_content(name, w, h), w, h, q) for name, q in (("noise", 90), ("gradient", 90), ("flat0", 10), ("stripes4", 90))]
    assert any(f.size % 2 for f in frames) and any(f.size % 2 == 0 for f in frames), "an odd and an even chunk: the padding byte"
    path = tmp_path / "out.avi"
    assert _write(path, capi.SINK_MJPEG, w, h, [(f, 0) for f in frames]) == len(frames)
    data = path.read_bytes()
    (riff,) = U.walk_riff(data)
    assert riff[0] == b"RIFF" and riff[3] == b"AVI " and riff[2] == len(data) - 8, "the patched RIFF length"
    hdrl, movi, idx1 = riff[4]
    assert (hdrl[0], hdrl[3]) == (b"LIST", b"hdrl") and (movi[0], movi[3]) == (b"LIST", b"movi") and idx1[0] == b"idx1"
    avih, strl = hdrl[4]
    u32 = lambda at: int.from_bytes(data[at:at + 4], "little")
    assert avih[0] == b"avih" and avih[2] == 56
    assert u32(avih[1]) == 80000 and u32(avih[1] + 12) & 0x10 and u32(avih[1] + 16) == len(frames) and u32(avih[1] + 24) == 1
    assert (u32(avih[1] + 32), u32(avih[1] + 36)) == (w, h)
    strh, strf = strl[4]
    assert strh[0] == b"strh" and strh[2] == 56 and data[strh[1]:strh[1] + 8] == b"vidsMJPG"
    assert (u32(strh[1] + 20), u32(strh[1] + 24), u32(strh[1] + 32)) == (2, 25, len(frames)), "dwScale = fps_den, dwRate = fps_num, dwLength"
    assert strf[0] == b"strf" and strf[2] == 40 and u32(strf[1]) == 40 and (u32(strf[1] + 4), u32(strf[1] + 8)) == (w, h)
    assert data[strf[1] + 12:strf[1] + 20] == b"\x01\x00\x18\x00MJPG", "one plane, 24 bits, MJPG"
    chunks = movi[4]
    assert len(chunks) == len(frames) and idx1[2] == 16 * len(frames)
    largest = max(f.size - 4 for f in frames)
    assert u32(avih[1] + 28) == largest and u32(strh[1] + 36) == largest
    for k, (cc, at, n, _, _) in enumerate(chunks):
        assert cc == b"00dc" and data[at:at + n] == frames[k][4:].tobytes(), f"chunk {k} is the frame's bytes 4 .. total"
        e = idx1[1] + 16 * k
        assert data[e:e + 4] == b"00dc" and u32(e + 4) == 0x10 and u32(e + 12) == n
        assert movi[1] + u32(e + 8) == at - 8, "the index's offset counts from the movi fourcc to the chunk's header"
        with Image.open(io.BytesIO(data[at:at + n])) as im:
            im.load()
            assert im.size == (w, h)


def test_mjpeg_sink_without_frames_is_a_valid_file(tmp_path):
    path = tmp_path / "empty.avi"
    assert _write(path, capi.SINK_MJPEG, 48, 48, []) == 0
    data = path.read_bytes()
    (riff,) = U.walk_riff(data)
    assert riff[2] == len(data) - 8 and [c[0] for c in riff[4]] == [b"LIST", b"LIST", b"idx1"] and riff[4][1][4] == [] and riff[4][2][2] == 0


def test_sinks_refuse_frames_of_another_format(tmp_path):
    w = h = 48
    jpeg = capi.i420_to_jpeg_frame(U.i420_content("noise", w, h), w, h, 90)
    bgr = textured(w, h, 1)
    gif = capi.bgr_to_gif_frame(bgr)
    bad = lambda rc: rc < 0
    assert bad(_write(tmp_path / "a.avi", capi.SINK_MJPEG, w, h, [(jpeg, 0), (np.ascontiguousarray(bgr), w * 3)])), "a raster frame"
    assert bad(_write(tmp_path / "b.avi", capi.SINK_MJPEG, w, h, [(capi.bgr_to_i420(bgr), w)])), "an I420 frame"
    assert bad(_write(tmp_path / "c.avi", capi.SINK_MJPEG, w, h, [(gif, 0)])), "a GIF-coded frame"
    assert bad(_write(tmp_path / "d.gif", capi.SINK_GIF_CODED, w, h, [(jpeg, 0)])), "a JPEG frame at the coded GIF sink"
    assert bad(_write(tmp_path / "e.gif", capi.SINK_GIF_GLOBAL_CODED, w, h, [(jpeg, 0)]))
    for fmt in (capi.SINK_RAW, capi.SINK_Y4M420, capi.SINK_GIF):
        assert bad(_write(tmp_path / "f.bin", fmt, w, h, [(jpeg, 0)])), "a JPEG frame at a raster sink"
    other = capi.i420_to_jpeg_frame(U.i420_content("noise", 32, 48), 32, 48, 90)
    assert bad(_write(tmp_path / "g.avi", capi.SINK_MJPEG, w, h, [(jpeg, 0), (other, 0)])), "a frame whose SOF0 names another size"
    assert not capi.lib().poppy_sink_open(str(tmp_path / "h.avi").encode(), 255, w, h, 25, 1) and not capi.lib().poppy_sink_open(str(tmp_path / "h.avi").encode(), 257, w, h, 25, 1)
