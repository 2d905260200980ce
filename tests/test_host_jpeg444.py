"""CPU checks of the 4:4:4 JPEG hand-off format (include/poppy_hip.h: POPPY_FRAME_JPEG444): the I444 planes of poppy_bgr_to_i444 against the three formulas in
numpy, against I420's Y plane and against the file POPPY_SINK_Y4M writes; the host statement poppy_i444_to_jpeg_frame byte for byte against the numpy
restatement in tests/jpeg444_util.py; the branches the content reaches; the header beside POPPY_FRAME_JPEG's; decoding by Pillow; capacity and refusals; the
quality beside Pillow's 4:4:4 and above this coder's 4:2:0; and the MJPEG sink on a mix of both formats."""
import io

import numpy as np
import pytest

import jpeg_util as U
import jpeg444_util as V
from palette_util import textured
from poppy_amd import capi

Image = pytest.importorskip("PIL.Image")
E_ARG, E_UNSUPPORTED = -1, -6
R = V.restart_mcus444()
CUBE = np.array([[[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)]], np.uint8)      # 1 x 8: the corners of the RGB cube


def test_constants():
    assert R == 16, "POPPY_JPEG444_RESTART_MCUS"
    assert capi.FRAME_JPEG444 == 512 and capi.FRAME_JPEG444 in capi.FRAMES_CODED
    for fmt in (511, 513):
        assert capi.frame_bytes(fmt, 64, 64) == 0
    assert capi.frame_bytes(capi.FRAME_JPEG444, 64, 64) > 0


def test_unknown_sink_values(tmp_path):
    for fmt in (511, 512, 513):                                 # (the format has no sink value of its own)
        assert not capi.lib().poppy_sink_open(str(tmp_path / "x.avi").encode(), fmt, 48, 48, 25, 1)


def _frames():
    rng = np.random.default_rng(444)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in ((1, 1), (7, 3), (8, 2), (16, 5), (33, 17), (64, 48))] + [CUBE, np.repeat(CUBE, 3, axis=0)]


def test_i444_planes_are_the_three_formulas():
    B, G, Rr = (CUBE[0, :, k].astype(np.int64) for k in range(3))
    assert (((-11059 * Rr - 21709 * G + 32768 * B + 32768) >> 16) + 128).max() == 256, "pure blue: the clamp of U is live"
    assert (((32768 * Rr - 27439 * G - 5329 * B + 32768) >> 16) + 128).max() == 256, "pure red: the clamp of V is live"
    for bgr in _frames():
        want = V.i444_of(bgr)
        assert np.array_equal(capi.bgr_to_i444(bgr), want), bgr.shape
        for pad in (1, 5, 16):
            assert np.array_equal(capi.bgr_to_i444(bgr, row_pad=pad), want), (bgr.shape, pad)


def test_i444_luma_is_i420s_and_the_planes_are_the_y4m_sinks(tmp_path):
    for k, bgr in enumerate(_frames()):
        h, w = bgr.shape[:2]
        planes = capi.bgr_to_i444(bgr)
        assert np.array_equal(planes[:w * h], capi.bgr_to_i420(bgr)[:w * h])
        path = tmp_path / f"{k}.y4m"
        L = capi.lib()
        s = L.poppy_sink_open(str(path).encode(), capi.SINK_Y4M, w, h, 25, 1)
        a = np.ascontiguousarray(bgr)
        L.poppy_sink_write(s, capi._p(a), w, h, w * 3)
        assert L.poppy_sink_close(s) == 1
        data = path.read_bytes()
        at = data.index(b"FRAME\n") + 6
        assert data[at:] == planes.tobytes(), "the C444 payload"


def test_i444_refusals():
    L = capi.lib()
    one = np.zeros(16, np.uint8)
    assert L.poppy_bgr_to_i444(None, 6, 2, 2, capi._p(one)) == E_ARG and L.poppy_bgr_to_i444(capi._p(one), 6, 2, 2, None) == E_ARG
    assert L.poppy_bgr_to_i444(capi._p(one), 6, 0, 2, capi._p(one)) == E_ARG and L.poppy_bgr_to_i444(capi._p(one), 6, 2, 0, capi._p(one)) == E_ARG
    assert L.poppy_bgr_to_i444(capi._p(one), 5, 2, 2, capi._p(one)) == E_ARG, "a stride below 3 * width"


@pytest.fixture(scope="module")
def coded():
    """{(content, w, h, quality): (the restatement's frame, the host statement's)} and what the restatement reached; coded once for the module"""
    stats, out = V.Stats(), {}
    for name in V.CONTENTS:
        for w, h in V.SIZES:
            for q in V.QUALITIES:
                a = V.i444_content(name, w, h)
                out[(name, w, h, q)] = (V.jpeg444_frame_reference(a, w, h, q, R, stats), capi.i444_to_jpeg_frame(a, w, h, q))
    return out, stats


def test_host_statement_equals_the_restatement(coded):
    for key, (want, got) in coded[0].items():
        assert got.tobytes() == want, f"{key}: {got.size} bytes, the restatement gives {len(want)}"


def test_sizes_reach_short_and_straddling_segments_and_wrap_the_rst_number(coded):
    assert len(V.walk_frame(coded[0][("noise", 40, 40, 90)][1])["segments"]) == 2, "25 MCUs in rows of 5: an interval straddles MCU rows, the last is short"
    assert len(V.walk_frame(coded[0][("noise", 128, 8, 90)][1])["segments"]) == 1 and len(V.walk_frame(coded[0][("noise", 129, 8, 90)][1])["segments"]) == 2
    w = V.walk_frame(coded[0][("noise", 160, 128, 90)][1])
    assert len(w["segments"]) == 20 and w["rst"] == [k % 8 for k in range(19)]
    assert w["restart"] == R and w["data_offset"] == U.HEADER_BYTES


def test_content_reaches_every_branch(coded):
    s = coded[1]
    assert s.segments == 720
    assert s.stuffed > 0, "a stuffed FF 00"
    assert s.zrl > 0, "a ZRL symbol"
    assert s.no_eob > 0, "a block whose last coefficient is non-zero"
    assert s.eob_only > 0, "a block of EOB alone"
    assert s.dc_cats == set(range(12)), "every DC category"
    assert s.ac_cats == set(range(1, 11)), "every AC category"
    assert s.pads == set(range(8)), "every padding"
    assert s.longest + 2 == 4738 and s.longest <= 19920, "the longest segment with its marker, against the scratch slot"


def test_the_interval_pins_these_sizes(coded):
    """The frame lengths on the 160 x 128 noise and gradient content, taken from the restatement (another interval or block order gives other lengths)."""
    assert {k: len(v[0]) for k, v in coded[0].items() if k[0] in ("noise", "gradient") and k[1:3] == (160, 128)} == PINNED_SIZES
    assert {k: v[1].size for k, v in coded[0].items() if k[0] in ("noise", "gradient") and k[1:3] == (160, 128)} == PINNED_SIZES


PINNED_SIZES = {("gradient", 160, 128, 10): 1852, ("gradient", 160, 128, 90): 8136, ("gradient", 160, 128, 100): 18272,
                ("noise", 160, 128, 10): 9886, ("noise", 160, 128, 90): 45853, ("noise", 160, 128, 100): 94899}


def test_header_differs_from_jpegs_in_exactly_two_bytes():
    for w, h in V.SIZES:
        for q in V.QUALITIES:
            mine = capi.i444_to_jpeg_frame(V.i444_content("gradient", w, h), w, h, q)
            theirs = capi.i420_to_jpeg_frame(U.i420_content("gradient", w, h), w, h, q)
            a, b = mine[4:4 + U.HEADER_BYTES], theirs[4:4 + U.HEADER_BYTES]
            at = np.flatnonzero(a != b)
            assert list(at) == [V.OFF_SOF_SAMPLING, V.OFF_DRI_LOW], at
            assert (a[at[0]], b[at[0]]) == (0x11, 0x22) and (a[at[1]], b[at[1]]) == (16, 8)
            pa, pb = V.walk_frame(mine), V.walk_frame(theirs)
            assert pa["order"] == pb["order"] == [0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA] and pa["data_offset"] == pb["data_offset"] == 613


def test_pillow_decodes_every_frame(coded):
    for (name, w, h, q), (_, got) in coded[0].items():
        parts = V.walk_frame(got)
        assert parts["size"] == (w, h) and parts["sampling"] == V.SAMPLING and parts["restart"] == R
        n_seg = -(-(((w + 7) // 8) * ((h + 7) // 8)) // R)
        assert len(parts["segments"]) == n_seg and parts["rst"] == [k % 8 for k in range(n_seg - 1)]
        with Image.open(io.BytesIO(got[4:].tobytes())) as im:
            im.load()
            assert im.size == (w, h)
            assert im.layer == V.LAYERS
            ql, qc = U.quant_tables(q)
            assert list(im.quantization[0]) == [int(x) for x in ql] and list(im.quantization[1]) == [int(x) for x in qc], "(Pillow hands tables out in natural order)"


def test_capacity(coded):
    for (name, w, h, q), (_, got) in coded[0].items():
        if q == 100:
            assert got.size <= capi.frame_bytes(capi.FRAME_JPEG444, w, h), (name, w, h)
    n_seg = lambda w, h: -(-(((w + 7) // 8) * ((h + 7) // 8)) // 16)
    for w, h in ((1, 1), (128, 8), (129, 8), (1920, 1080)):
        assert capi.frame_bytes(capi.FRAME_JPEG444, w, h) == 617 + n_seg(w, h) * (2 * ((6 * 1660 * 8 + 7) // 8) + 2) == V.capacity(w, h)
    assert capi.frame_bytes(capi.FRAME_JPEG444, 1920, 1080) == 617 + 2025 * 19922


def test_refusals_on_the_arguments_alone():
    L = capi.lib()
    one = np.zeros(16, np.uint8)                                # (refused before a byte of it is read)
    # a side above SOF0's 16 bits; a capacity above `total`'s 32 (16000 x 16000 is one that POPPY_FRAME_JPEG still takes: this format has twice the blocks)
    assert capi.frame_bytes(capi.FRAME_JPEG, 16000, 16000) < 1 << 32 <= capi.frame_bytes(capi.FRAME_JPEG444, 16000, 16000)
    for w, h in ((65536, 1), (1, 65536), (65535, 65535), (16000, 16000)):
        assert L.poppy_i444_to_jpeg_frame(capi._p(one), w, h, 90, capi._p(one)) == E_UNSUPPORTED
        assert L.poppy_bgr_to_jpeg444_frame(capi._p(one), w * 3, w, h, 90, capi._p(one)) == E_UNSUPPORTED
    for q in (0, 101, -5):
        assert L.poppy_i444_to_jpeg_frame(capi._p(one), 2, 2, q, capi._p(one)) == E_ARG
        assert L.poppy_bgr_to_jpeg444_frame(capi._p(one), 6, 2, 2, q, capi._p(one)) == E_ARG
    assert L.poppy_i444_to_jpeg_frame(None, 2, 2, 90, capi._p(one)) == E_ARG and L.poppy_i444_to_jpeg_frame(capi._p(one), 0, 2, 90, capi._p(one)) == E_ARG
    assert L.poppy_i444_to_jpeg_frame(capi._p(one), 2, 2, 90, None) == E_ARG
    assert L.poppy_bgr_to_jpeg444_frame(capi._p(one), 5, 2, 2, 90, capi._p(one)) == E_ARG, "a stride below 3 * width"


def test_bgr_statement_is_the_composition():
    bgr = textured(61, 47, 3)
    assert np.array_equal(capi.bgr_to_jpeg444_frame(bgr, 77), capi.i444_to_jpeg_frame(capi.bgr_to_i444(bgr), 61, 47, 77))


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_quality_beside_pillows_444_and_above_this_coders_420():
    """PSNR of the decoded RGB against the source on the two images of the textured 256 x 192 pair at quality 90.  Measured on the CPU:
        image 41: this coder 33.774 dB (24 499 bytes), Pillow at subsampling=0 with the same tables 33.776 dB (24 357 bytes), this coder's 4:2:0 28.261 dB
        image 42: this coder 33.676 dB (24 093 bytes), Pillow 33.674 dB (23 980 bytes), this coder's 4:2:0 28.847 dB
    The gap, Pillow's minus this coder's, is +0.002 and -0.002 dB; the test allows it rounded up to the next 0.25 dB, which is 0.25.  The gain over
    poppy_bgr_to_jpeg_frame is 5.513 and 4.829 dB; rounded down to 0.25 dB, 5.5 and 4.75 are asserted."""
    for seed in (41, 42):
        bgr = textured(256, 192, seed)
        rgb = np.ascontiguousarray(bgr[:, :, ::-1])
        frame = capi.bgr_to_jpeg444_frame(bgr, 90)
        with Image.open(io.BytesIO(frame[4:].tobytes())) as im:
            mine = _psnr(np.asarray(im.convert("RGB")), rgb)
            tables = [list(im.quantization[0]), list(im.quantization[1])]
        with Image.open(io.BytesIO(capi.bgr_to_jpeg_frame(bgr, 90)[4:].tobytes())) as im:
            mine420 = _psnr(np.asarray(im.convert("RGB")), rgb)
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, "JPEG", qtables=tables, subsampling=0, optimize=False)
        assert U.walk_frame(np.frombuffer((len(b.getvalue()) + 4).to_bytes(4, "little") + b.getvalue(), np.uint8))["qtables"] == V.walk_frame(frame)["qtables"], "both files carry the same tables"
        with Image.open(b) as im:
            assert im.layer == V.LAYERS
            theirs = _psnr(np.asarray(im.convert("RGB")), rgb)
        print(f"textured {seed}: this coder {mine:.3f} dB in {frame.size} bytes, Pillow 4:4:4 {theirs:.3f} dB in {len(b.getvalue())}, this coder's 4:2:0 {mine420:.3f} dB")
        assert theirs - mine <= PSNR_GAP_DB
        assert mine - mine420 >= PSNR_GAIN_DB[seed]


PSNR_GAP_DB = 0.25
PSNR_GAIN_DB = {41: 5.5, 42: 4.75}


# ---- the sink ---------------------------------------------------------------------------------------------------------------------------------------------
def _write(path, fmt, w, h, frames, fps=(25, 1)):
    L = capi.lib()
    s = L.poppy_sink_open(str(path).encode(), fmt, w, h, fps[0], fps[1])
    assert s
    for f, stride in frames:
        L.poppy_sink_write(s, capi._p(f), w, h, stride)
    return L.poppy_sink_close(s)


def test_mjpeg_sink_takes_a_mix_of_both_formats(tmp_path):
    w = h = 48
    f420 = [capi.i420_to_jpeg_frame(U.i420_content(name, w, h), w, h, 90) for name in ("noise", "gradient")]
    f444 = capi.i444_to_jpeg_frame(V.i444_content("noise", w, h), w, h, 90)
    frames = [f420[0], f444, f420[1]]
    path = tmp_path / "mix.avi"
    assert _write(path, capi.SINK_MJPEG, w, h, [(f, 0) for f in frames]) == 3
    data = path.read_bytes()
    (riff,) = V.walk_riff(data)
    chunks = riff[4][1][4]
    assert riff[2] == len(data) - 8 and len(chunks) == 3
    layers = [[(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)], V.LAYERS, [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]]
    for k, (cc, at, n, _, _) in enumerate(chunks):
        assert cc == b"00dc" and data[at:at + n] == frames[k][4:].tobytes(), f"chunk {k} is the frame's bytes 4 .. total"
        with Image.open(io.BytesIO(data[at:at + n])) as im:
            im.load()
            assert im.size == (w, h) and im.layer == layers[k]


def test_mjpeg_sink_holds_each_frame_to_its_own_capacity(tmp_path):
    w = h = 48
    cap444, cap420 = capi.frame_bytes(capi.FRAME_JPEG444, w, h), capi.frame_bytes(capi.FRAME_JPEG, w, h)
    assert cap420 < cap444
    for fmt, frame, cap in ((capi.FRAME_JPEG444, capi.i444_to_jpeg_frame(V.i444_content("noise", w, h), w, h, 90), cap444),
                            (capi.FRAME_JPEG, capi.i420_to_jpeg_frame(U.i420_content("noise", w, h), w, h, 90), cap420)):
        for total, ok in ((cap, True), (cap + 1, False)):       # (the sink reads `total` and the header; the buffer is as long as `total` says)
            big = np.zeros(total, np.uint8)
            big[:frame.size] = frame
            big[:4] = np.frombuffer(int(total).to_bytes(4, "little"), np.uint8)
            rc = _write(tmp_path / "cap.avi", capi.SINK_MJPEG, w, h, [(big, 0)])
            assert (rc == 1) if ok else (rc < 0), (fmt, total, rc)


def test_every_other_sink_refuses_a_jpeg444_frame(tmp_path):
    w = h = 48
    frame = capi.i444_to_jpeg_frame(V.i444_content("noise", w, h), w, h, 90)
    for fmt in (capi.SINK_RAW, capi.SINK_PPM, capi.SINK_Y4M, capi.SINK_Y4M420, capi.SINK_GIF, capi.SINK_GIF_GLOBAL, capi.SINK_GIF_CODED, capi.SINK_GIF_GLOBAL_CODED):
        name = "f%03d.ppm" if fmt == capi.SINK_PPM else "f.bin"
        assert _write(tmp_path / name, fmt, w, h, [(frame, 0)]) < 0, fmt
    other = capi.i444_to_jpeg_frame(V.i444_content("noise", 32, 48), 32, 48, 90)
    assert _write(tmp_path / "g.avi", capi.SINK_MJPEG, w, h, [(frame, 0), (other, 0)]) < 0, "a frame whose SOF0 names another size"
