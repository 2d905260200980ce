"""CPU checks of the JPEG hand-off on per-frame Huffman tables (include/poppy_hip.h: POPPY_FRAME_JPEG_OPT, POPPY_FRAME_JPEG444_OPT): the table rule and the
host coders (frame_jpeg.cpp) against the plain-Python restatement of tests/jpeg_opt_util.py, == throughout; what Pillow decodes; capacity, `least`, refusals;
the MJPEG sink."""
import io

import numpy as np
import pytest

import jpeg444_util as U4
import jpeg_opt_util as O
import jpeg_util as U
from poppy_amd import capi, synth

E_ARG, E_UNSUPPORTED = -1, -6
KEYS = ((0, 0), (1, 0), (0, 1), (1, 1))


def _frame_counts(planes, w, h, quality, sampling=420):
    st = {}
    O.jpeg_opt_frame_reference(planes, w, h, quality, sampling, st)
    return st["counts"]


@pytest.fixture(scope="module")
def families():
    fam = dict(O.count_families())
    real = _frame_counts(capi.bgr_to_i420(synth.textured_bgr(160, 128)), 160, 128, 90)
    for key in KEYS:
        fam[f"textured_{key[0]}{key[1]}"] = real[key]
    real = _frame_counts(U4.i444_of(synth.gen_pair(160, 128)[0]), 160, 128, 90, 444)
    for key in KEYS:
        fam[f"pair444_{key[0]}{key[1]}"] = real[key]
    return fam


def test_table_rule_is_the_restatement(families):
    for name, counts in families.items():
        info = {}
        bits, vals = O.optimal_table(counts, info)
        got_bits, got_vals = capi.jpeg_optimal_table(counts)
        assert [int(b) for b in got_bits] == bits and [int(v) for v in got_vals] == vals, name
        assert O.kraft_ok(bits), f"{name}: Kraft's sum reaches 2^16, or a length passes 16"
        assert sum(bits) == len(vals) == sum(1 for c in counts if c), name
    assert [len(O.optimal_table(families[n])[1]) for n in ("one", "two", "all_equal", "dc12")] == [1, 2, 256, 12]
    assert O.optimal_table(families["one"]) == ([1] + [0] * 15, [5])


def test_fibonacci_counts_pass_libjpegs_32_lengths():
    counts = O.fibonacci_counts()
    info = {}
    O.optimal_table(counts, info)
    assert sum(counts) < 1 << 32 and info["depth"] > 32 and info["limited"]


def test_table_rule_refuses():
    L = capi.lib()
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), np.zeros(1, np.int32)

    def rc(counts, b=bits, v=vals, nn=n):
        a = None if counts is None else np.asarray(counts, np.uint32)
        return L.poppy_jpeg_optimal_table(None if a is None else capi._p(a), None if b is None else capi._p(b), None if v is None else capi._p(v),
                                          None if nn is None else capi._p(nn))
    assert rc([0] * 256) == E_ARG
    assert rc([0xffffffff] + [0] * 255) == E_ARG                 # a sum of 2^32 - 1
    assert rc([0xfffffffe, 1] + [0] * 254) == E_ARG
    assert rc([0x80000000] * 2 + [0] * 254) == E_ARG             # ... and above 32 bits
    assert rc([0xfffffffe] + [0] * 255) == 0 and n[0] == 1
    assert rc([0xfffffffd, 1] + [0] * 254) == 0 and n[0] == 2
    one = [1] + [0] * 255
    assert rc(None) == E_ARG and rc(one, b=None) == E_ARG and rc(one, v=None) == E_ARG and rc(one, nn=None) == E_ARG


@pytest.mark.parametrize("quality", U.QUALITIES)
def test_frames_are_the_restatement_420(quality):
    reached = {"one_symbol": False, "zrl": 0, "stuffed": 0}
    for name in U.CONTENTS:
        for w, h in U.SIZES:
            a = U.i420_content(name, w, h)
            st = {}
            want = O.jpeg_opt_frame_reference(a, w, h, quality, 420, st)
            got = capi.i420_to_jpeg_opt_frame(a, w, h, quality)
            assert got.tobytes() == want, f"{name} {w}x{h} q{quality}"
            assert O.LEAST <= got.size <= capi.frame_bytes(capi.FRAME_JPEG_OPT, w, h)
            reached["one_symbol"] |= st["one_symbol"]
            reached["zrl"] += st["zrl"]
            reached["stuffed"] += st["stuffed"]
    assert reached["one_symbol"] and reached["stuffed"], reached
    bgr = synth.textured_bgr(160, 128)
    st = {}
    assert capi.bgr_to_jpeg_opt_frame(bgr, quality).tobytes() == O.jpeg_opt_frame_reference(capi.bgr_to_i420(bgr), 160, 128, quality, 420, st)
    if quality == 90:
        assert st["zrl"] > 0, "the textured frame at quality 90 has no ZRL"


@pytest.mark.parametrize("quality", U4.QUALITIES)
def test_frames_are_the_restatement_444(quality):
    one_symbol = False
    for name in U4.CONTENTS:
        for w, h in U4.SIZES:
            a = U4.i444_content(name, w, h)
            st = {}
            want = O.jpeg_opt_frame_reference(a, w, h, quality, 444, st)
            got = capi.i444_to_jpeg_opt_frame(a, w, h, quality)
            assert got.tobytes() == want, f"{name} {w}x{h} q{quality}"
            assert O.LEAST <= got.size <= capi.frame_bytes(capi.FRAME_JPEG444_OPT, w, h)
            one_symbol |= st["one_symbol"]
    assert one_symbol
    bgr = synth.textured_bgr(160, 128)
    assert capi.bgr_to_jpeg444_opt_frame(bgr, quality).tobytes() == O.jpeg_opt_frame_reference(capi.bgr_to_i444(bgr), 160, 128, quality, 444)


@pytest.mark.parametrize("quality", (100, 90))
def test_noise_frame_runs_the_length_limit(quality):
    """640 x 360 uniform noise: the luma AC table reaches lengths above 16 before limiting (the restatement says so), so Annex K.3 runs inside a whole frame"""
    w, h = 640, 360
    a = O.noise_i420(w, h, 5)
    st = {}
    want = O.jpeg_opt_frame_reference(a, w, h, quality, 420, st)
    assert st["limited"][(1, 0)] and st["depth"][(1, 0)] > 16, st["depth"]
    assert capi.i420_to_jpeg_opt_frame(a, w, h, quality).tobytes() == want
    f = U.walk_frame(np.frombuffer(want, np.uint8))
    assert len(f["segments"]) == 115 and all(O.kraft_ok(bits) for bits, _ in f["dht"].values())


def test_smallest_frame_is_least():
    """a flat 1 x 1 frame: four one-symbol tables, every code one bit.  4:4:4 has three blocks, 6 bits, one byte of data: `least`; 4:2:0 has six, 12 bits, two"""
    got = capi.i444_to_jpeg_opt_frame(U4.i444_content("flat128", 1, 1), 1, 1, 90)
    f = U.walk_frame(got)
    assert got.size == O.LEAST == 276 and [len(v) for _, v in f["dht"].values()] == [1, 1, 1, 1] and f["data_offset"] == 197 + 4 * 18
    assert capi.i420_to_jpeg_opt_frame(U.i420_content("flat128", 1, 1), 1, 1, 90).size == O.LEAST + 1


def _photo_crop():
    return np.ascontiguousarray(synth.photo_pair(720, 405)[0][100:228, 200:360])


def test_pillow_decodes_the_pixels_of_the_standard_tables():
    Image = pytest.importorskip("PIL.Image")

    def pixels(frame):
        with Image.open(io.BytesIO(frame[4:].tobytes())) as im:
            im.load()
            return np.asarray(im).copy(), im.layer

    def same(what, opt, std):
        (p_opt, l_opt), (p_std, l_std) = pixels(opt), pixels(std)
        assert l_opt == l_std and p_opt.shape == p_std.shape and (p_opt == p_std).all(), what
    for quality in U.QUALITIES:
        for name in U.CONTENTS:
            for w, h in U.SIZES:
                a = U.i420_content(name, w, h)
                same(f"{name} {w}x{h} q{quality}", capi.i420_to_jpeg_opt_frame(a, w, h, quality), capi.i420_to_jpeg_frame(a, w, h, quality))
            for w, h in U4.SIZES:
                b = U4.i444_content(name, w, h)
                same(f"4:4:4 {name} {w}x{h} q{quality}", capi.i444_to_jpeg_opt_frame(b, w, h, quality), capi.i444_to_jpeg_frame(b, w, h, quality))
        for bgr in (_photo_crop(), synth.textured_bgr(160, 128)):
            assert (pixels(capi.bgr_to_jpeg_opt_frame(bgr, quality))[0] == pixels(capi.bgr_to_jpeg_frame(bgr, quality))[0]).all()
            assert (pixels(capi.bgr_to_jpeg444_opt_frame(bgr, quality))[0] == pixels(capi.bgr_to_jpeg444_frame(bgr, quality))[0]).all()
    a = O.noise_i420(640, 360, 5)                           # the frames whose luma AC table went through Annex K.3 (test_noise_frame_runs_the_length_limit)
    for quality in (100, 90):
        same(f"noise 640x360 q{quality}", capi.i420_to_jpeg_opt_frame(a, 640, 360, quality), capi.i420_to_jpeg_frame(a, 640, 360, quality))


def test_fewer_bytes_than_the_standard_tables():
    for what, bgr in (("photograph", _photo_crop()), ("textured", synth.textured_bgr(160, 128)), ("pair", synth.gen_pair(160, 128)[0])):
        for quality in U.QUALITIES:
            opt, std = capi.bgr_to_jpeg_opt_frame(bgr, quality).size, capi.bgr_to_jpeg_frame(bgr, quality).size
            assert opt < std, f"{what} q{quality}: {opt} bytes on its own tables, {std} on the standard ones"


def test_capacity_is_the_headers_formula_and_the_refusals_are_jpegs():
    for w, h in ((1, 1), (16, 16), (17, 16), (128, 16), (129, 16), (1920, 1080), (3840, 2160), (65535, 1)):
        assert capi.frame_bytes(capi.FRAME_JPEG_OPT, w, h) == O.capacity(w, h), (w, h)
        assert capi.frame_bytes(capi.FRAME_JPEG444_OPT, w, h) == O.capacity(w, h, 444), (w, h)
        assert capi.frame_bytes(capi.FRAME_JPEG_OPT, w, h) > capi.frame_bytes(capi.FRAME_JPEG, w, h)
    L = capi.lib()
    one = np.zeros(16, np.uint8)
    for call in (L.poppy_i420_to_jpeg_opt_frame, L.poppy_i444_to_jpeg_opt_frame):
        assert call(capi._p(one), 65536, 1, 90, capi._p(one)) == E_UNSUPPORTED
        assert call(capi._p(one), 65535, 65535, 90, capi._p(one)) == E_UNSUPPORTED      # a capacity above 2^32
        assert call(capi._p(one), 2, 2, 0, capi._p(one)) == E_ARG and call(capi._p(one), 2, 2, 101, capi._p(one)) == E_ARG
        assert call(None, 2, 2, 90, capi._p(one)) == E_ARG and call(capi._p(one), 0, 2, 90, capi._p(one)) == E_ARG
    for call in (L.poppy_bgr_to_jpeg_opt_frame, L.poppy_bgr_to_jpeg444_opt_frame):
        assert call(capi._p(one), 3 * 65536, 65536, 1, 90, capi._p(one)) == E_UNSUPPORTED
        assert call(capi._p(one), 5, 2, 2, 90, capi._p(one)) == E_ARG
    assert O.capacity(65535, 65535) > 1 << 32


def test_neighbouring_format_values_are_unknown():
    for fmt in (4095, 4097, 8191, 8193):
        assert capi.frame_bytes(fmt, 16, 16) == 0
    assert (capi.FRAME_JPEG_OPT, capi.FRAME_JPEG444_OPT) == (4096, 8192)
    assert capi.FRAME_JPEG_OPT in capi.FRAMES_CODED and capi.FRAME_JPEG444_OPT in capi.FRAMES_CODED
    L = capi.lib()
    for name in capi.SYMBOLS:
        assert hasattr(L, name), name


# ---- the MJPEG sink ---------------------------------------------------------------------------------------------------------------------------------------
def _write(path, fmt, w, h, frames):
    L = capi.lib()
    s = L.poppy_sink_open(str(path).encode(), fmt, w, h, 25, 1)
    assert s
    for f in frames:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    return L.poppy_sink_close(s)


def test_mjpeg_sink_takes_a_mix_with_the_opt_formats(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    w = h = 48
    a, b = U.i420_content("noise", w, h), U4.i444_content("gradient", w, h)
    frames = [capi.i420_to_jpeg_frame(a, w, h, 90), capi.i420_to_jpeg_opt_frame(a, w, h, 90), capi.i444_to_jpeg_opt_frame(b, w, h, 90), capi.i444_to_jpeg_frame(b, w, h, 90),
              capi.i420_to_jpeg_opt_frame(U.i420_content("flat128", w, h), w, h, 10)]
    path = tmp_path / "mix.avi"
    assert _write(path, capi.SINK_MJPEG, w, h, frames) == len(frames)
    data = path.read_bytes()
    (riff,) = U.walk_riff(data)
    movi = riff[4][1]
    assert riff[2] == len(data) - 8 and movi[3] == b"movi" and len(movi[4]) == len(frames)
    for k, (cc, at, n, _, _) in enumerate(movi[4]):
        assert cc == b"00dc" and data[at:at + n] == frames[k][4:].tobytes()
        with Image.open(io.BytesIO(data[at:at + n])) as im:
            im.load()
            assert im.size == (w, h)


def test_mjpeg_sink_holds_an_opt_frame_to_the_opt_capacity(tmp_path):
    w = h = 48
    for fmt, frame in ((capi.FRAME_JPEG_OPT, capi.i420_to_jpeg_opt_frame(U.i420_content("noise", w, h), w, h, 90)),
                       (capi.FRAME_JPEG444_OPT, capi.i444_to_jpeg_opt_frame(U4.i444_content("noise", w, h), w, h, 90))):
        cap = capi.frame_bytes(fmt, w, h)
        assert cap > capi.frame_bytes(capi.FRAME_JPEG if fmt == capi.FRAME_JPEG_OPT else capi.FRAME_JPEG444, w, h)
        for total, ok in ((cap, True), (cap + 1, False)):
            big = np.zeros(total, np.uint8)
            big[:frame.size] = frame
            big[:4] = np.frombuffer(int(total).to_bytes(4, "little"), np.uint8)
            rc = _write(tmp_path / "cap.avi", capi.SINK_MJPEG, w, h, [big])
            assert (rc == 1) if ok else (rc < 0), (fmt, total, rc)


def test_every_other_sink_refuses_an_opt_frame(tmp_path):
    w = h = 48
    for frame in (capi.i420_to_jpeg_opt_frame(U.i420_content("noise", w, h), w, h, 90), capi.i444_to_jpeg_opt_frame(U4.i444_content("noise", w, h), w, h, 90)):
        for fmt in (capi.SINK_RAW, capi.SINK_PPM, capi.SINK_Y4M, capi.SINK_Y4M420, capi.SINK_GIF, capi.SINK_GIF_GLOBAL, capi.SINK_GIF_CODED, capi.SINK_GIF_GLOBAL_CODED,
                    capi.SINK_PNG):
            name = "f%03d.ppm" if fmt == capi.SINK_PPM else "f%03d.png" if fmt == capi.SINK_PNG else "f.bin"
            assert _write(tmp_path / name, fmt, w, h, [frame]) < 0, fmt
