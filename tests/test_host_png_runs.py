"""The POPPY_FRAME_PNG_RUNS hand-off on the host (include/poppy_hip.h has the rule): poppy_bgr_to_png_runs_frame against a numpy restatement built from the tables
that poppy_png_runs_table hands out (png_runs_util.py), and, independently of any restatement, against zlib's and Pillow's decoders; the tables and their headers;
the capacity; the refusals; the PNG sink on a mix of both PNG formats.  The content set is png_runs_util.cases(), and every case asserts what it reaches."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_runs_util as R
import png_util as P
from poppy_amd import capi

E_ARG, E_UNSUPPORTED = -1, -6
CASES = list(R.cases())


@pytest.fixture(scope="module")
def host_frames():
    """name -> the host statement's whole destination buffer (canary-filled before the call)"""
    return {name: capi.bgr_to_png_runs_frame(bgr, whole=True) for name, bgr in R.cases().items()}


def _frame(buf):
    return buf[:capi.png_frame_bytes(buf)]


@pytest.mark.parametrize("name", CASES)
def test_host_statement_is_the_restated_rule(host_frames, name):
    R.check_case(name)
    P.equal(name, _frame(host_frames[name]), R.restated(name)[0])


@pytest.mark.parametrize("name", CASES)
def test_decoders_give_back_the_frame(host_frames, name):
    Image = pytest.importorskip("PIL.Image")
    bgr, buf = R.cases()[name], host_frames[name]
    h, w = bgr.shape[:2]
    total = capi.png_frame_bytes(buf)
    capacity = capi.frame_bytes(capi.FRAME_PNG_RUNS, w, h)
    assert 0 < total <= capacity and buf.size == capacity + 64
    assert (buf[total:] == capi.PNG_CANARY).all(), "bytes behind `total` were written"
    chunks = P.walk_frame(buf[:total])
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0) and chunks[2][1] == b""
    idat = chunks[1][1]
    assert idat[:2] == b"\x78\x01"
    stream, _ = P.filtered_stream(bgr)
    assert zlib.decompress(idat) == stream.tobytes()
    with Image.open(io.BytesIO(buf[4:total].tobytes())) as im:
        im.load()
        assert im.mode == "RGB" and im.size == (w, h)
        assert (np.asarray(im) == bgr[:, :, ::-1]).all()


def test_row_pads_do_not_matter():
    for name in ("segment cuts", "333x97 cuts mid-row"):
        bgr = R.cases()[name]
        want = capi.bgr_to_png_runs_frame(bgr)
        for pad in (1, 7, 64):
            P.equal(f"{name} pad {pad}", capi.bgr_to_png_runs_frame(bgr, row_pad=pad), want)


def test_content_set_reaches_every_table_and_both_kinds_of_token():
    tables_seen, symbols_seen = set(), set()
    for name in CASES:
        _, _, _, tokens, choice = R.restated(name)
        tables_seen |= set(choice)
        for sym, _, _ in tokens:
            symbols_seen |= set(sym[sym > 256].tolist())
    assert tables_seen == set(range(capi.PNG_TABLES))
    assert {285, 284, 257, 262, 263, 264} <= symbols_seen      # 258; a long remainder; 3; the shortest matches of a run: 8, 9, 10


@pytest.mark.parametrize("name", R.RUN_FREE)
def test_run_free_content_is_the_literals_of_the_png_format(name):
    """No run with a tail of POPPY_PNG_RUN_MIN: the tokens are the filtered stream's bytes, one literal each — POPPY_FRAME_PNG's token stream."""
    _, stream, _, tokens, _ = R.restated(name)
    assert (np.concatenate([sym for sym, _, _ in tokens]) == stream).all()
    assert all(not eb.any() and not ex.any() for _, eb, ex in tokens)
    # ... and the host statement's file holds that stream (the literals' codes differ: the tables have 29 symbols more)
    idat = P.walk_frame(capi.bgr_to_png_runs_frame(R.cases()[name]))[1][1]
    assert zlib.decompress(idat) == zlib.decompress(P.walk_frame(capi.bgr_to_png_frame(R.cases()[name]))[1][1]) == stream.tobytes()


@pytest.mark.parametrize("name", ("341x24 black", "21x130 black stub", "341x16 flat"))
def test_flat_frames_come_out_under_a_bit_per_byte(host_frames, name):
    """A Huffman-only block pays a bit per byte at the least: no such coder gets under n / 8."""
    bgr = R.cases()[name]
    n = bgr.shape[0] * (1 + 3 * bgr.shape[1])
    assert capi.png_frame_bytes(host_frames[name]) < n / 8
    assert capi.bgr_to_png_frame(bgr).size > n / 8


@pytest.mark.parametrize("k", range(capi.PNG_TABLES))
def test_tables_are_complete_codes_and_headers_decode_to_them(k):
    lengths, codes, header = R.tables()[k]
    assert lengths.size == 286 and lengths.min() >= 1 and lengths.max() <= 15
    assert sum(1 << (15 - int(l)) for l in lengths) == 1 << 15, "the Kraft sum is exactly 1"
    # BFINAL 0, BTYPE 10, HLIT 29, HDIST 0
    assert 17 + 4 * 3 <= header.size <= 8 * capi.PNG_HEADER_BYTES and header[:13].tolist() == [0, 0, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    # the header followed by end-of-block alone: an empty final block that inflate accepts
    head = header.copy(); head[0] = 1
    eob = [(int(codes[256]) >> i) & 1 for i in range(int(lengths[256]))]
    d = zlib.decompressobj(wbits=-15)
    assert d.decompress(np.packbits(np.r_[head, eob].astype(np.uint8), bitorder="little").tobytes()) == b"" and d.eof
    # one final block holding every literal once and a match of every length symbol: inflate reads the same lengths from the header
    sym = np.r_[np.arange(256)[::-1], 7, np.arange(257, 286)]
    ex = np.zeros(sym.size, np.int64)
    eb = np.r_[np.zeros(257, np.int64), np.array(R.LENGTH_EXTRA, np.int64)]
    want = bytes(range(256))[::-1] + b"\x07" + b"\x07" * sum(R.LENGTH_BASE)
    raw = R.deflate_bits([(sym, eb, ex)], [k])
    d = zlib.decompressobj(wbits=-15)
    assert d.decompress(raw) == want and d.eof


def test_length_symbols_are_rfc_1951s():
    """the restatement's list against zlib: a run of every length 3..258 behind a literal, coded as one match, decodes to that run"""
    for length in range(3, 259):
        a, b, c = R.length_symbol(length)
        raw = R.deflate_bits([(np.array([65, a]), np.array([0, b]), np.array([0, c]))], [7])
        d = zlib.decompressobj(wbits=-15)
        assert d.decompress(raw) == b"A" * (1 + length) and d.eof, length
    assert R.length_symbol(258) == (285, 0, 0) and R.length_symbol(257) == (284, 5, 30)


def test_table_seven_bounds_the_capacity():
    lengths, _, header = R.tables()[7]
    literal = int(lengths[:256].max())
    assert literal <= 9
    for s in range(257, 286):                               # a match costs no more than the three literals it covers at the least
        assert int(lengths[s]) + R.LENGTH_EXTRA[s - 257] + 1 <= 3 * literal
    for w, h in ((1, 1), (341, 8), (683, 4), (1920, 1080)):
        n = h * (1 + 3 * w)
        n_seg = -(-n // P.SEGMENT)
        assert capi.frame_bytes(capi.FRAME_PNG_RUNS, w, h) == 67 + -(-(n_seg * (header.size + int(lengths[256])) + literal * n) // 8)
    # uniform noise, the capacity's case: inside the bound
    noise = R.cases()["341x24 uniform noise"]
    total = capi.bgr_to_png_runs_frame(noise).size
    assert noise.size < total <= capi.frame_bytes(capi.FRAME_PNG_RUNS, 341, 24)
    for name, bgr in R.cases().items():
        assert capi.bgr_to_png_runs_frame(bgr).size <= capi.frame_bytes(capi.FRAME_PNG_RUNS, bgr.shape[1], bgr.shape[0]), name


def test_refusals_symbols_and_unknown_values(tmp_path):
    L = capi.lib()
    one = np.zeros(256, np.uint8)
    f = L.poppy_bgr_to_png_runs_frame
    assert f(None, 6, 2, 2, capi._p(one)) == E_ARG and f(capi._p(one), 6, 2, 2, None) == E_ARG
    assert f(capi._p(one), 5, 2, 2, capi._p(one)) == E_ARG
    assert f(capi._p(one), 6, 0, 2, capi._p(one)) == E_ARG and f(capi._p(one), 6, 2, -1, capi._p(one)) == E_ARG
    assert 0 < capi.frame_bytes(capi.FRAME_PNG_RUNS, 25000, 25000) < 1 << 31
    for w, h in ((26000, 26000), (1 << 30, 1), (1, 1 << 30), (65536, 65536)):
        assert capi.frame_bytes(capi.FRAME_PNG_RUNS, w, h) == 0
        assert f(capi._p(one), 3 * w, w, h, capi._p(one)) == E_UNSUPPORTED
    assert L.poppy_png_runs_table(-1, None, None, None) == E_ARG and L.poppy_png_runs_table(8, None, None, None) == E_ARG and L.poppy_png_runs_table(3, None, None, None) == 0
    for name in ("poppy_png_runs_table", "poppy_bgr_to_png_runs_frame", "poppy_hip_bgr_to_png_runs_frame"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert (capi.FRAME_PNG_RUNS, capi.PNG_RUN_MIN) == (2048, 8) and capi.FRAME_PNG_RUNS in capi.FRAMES_CODED
    for value in (2047, 2049):
        assert capi.frame_bytes(value, 16, 16) == 0
        assert not L.poppy_sink_open(str(tmp_path / "x%d").encode(), value, 16, 16, 25, 1)
    assert not L.poppy_sink_open(str(tmp_path / "x%d").encode(), 2048, 16, 16, 25, 1), "there is no sink value for the format: POPPY_SINK_PNG takes it"


def test_png_sink_takes_both_formats_in_a_mix(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    L = capi.lib()
    w, h = 65, 3
    frames = [np.roll(P.cases()["65x3 gradient"], k, 1) for k in range(3)] + [np.zeros((h, w, 3), np.uint8)]
    coded = [(capi.bgr_to_png_runs_frame if k % 2 == 0 else capi.bgr_to_png_frame)(f) for k, f in enumerate(frames)]
    s = L.poppy_sink_open(str(tmp_path / "f_%03d.png").encode(), capi.SINK_PNG, w, h, 25, 1)
    assert s
    for f in coded:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(frames)
    for k, f in enumerate(frames):
        path = tmp_path / f"f_{k:03d}.png"
        assert path.read_bytes() == coded[k][4:].tobytes()
        with Image.open(path) as im:
            assert (np.asarray(im.convert("RGB")) == f[:, :, ::-1]).all()

    def fails(frame, size=(w, h)):
        s = L.poppy_sink_open(str(tmp_path / "o_%d.bin").encode(), capi.SINK_PNG, size[0], size[1], 25, 1)
        assert s
        L.poppy_sink_write(s, capi._p(frame), w, h, 0)
        return L.poppy_sink_close(s) < 0
    big = np.zeros(1024, np.uint8)
    runs = np.concatenate([coded[0], big])
    assert not fails(runs)
    # `total` is held to the larger of the two capacities
    larger = max(capi.frame_bytes(capi.FRAME_PNG, w, h), capi.frame_bytes(capi.FRAME_PNG_RUNS, w, h))
    at = runs.copy(); at[:4] = np.frombuffer(struct.pack("<I", larger), np.uint8)
    past = runs.copy(); past[:4] = np.frombuffer(struct.pack("<I", larger + 1), np.uint8)
    assert not fails(np.concatenate([at, big])) and fails(np.concatenate([past, big]))
    # a frame of another size fails it, and a PNG_RUNS frame fails every other sink
    assert fails(np.concatenate([capi.bgr_to_png_runs_frame(P.cases()["64x3 gradient"]), big]))
    for sink in (capi.SINK_RAW, capi.SINK_PPM, capi.SINK_Y4M, capi.SINK_Y4M420, capi.SINK_GIF, capi.SINK_GIF_GLOBAL, capi.SINK_GIF_CODED, capi.SINK_GIF_GLOBAL_CODED, capi.SINK_MJPEG):
        s = L.poppy_sink_open(str(tmp_path / "p_%d.bin").encode(), sink, w, h, 25, 1)
        assert s
        L.poppy_sink_write(s, capi._p(runs), w, h, 0)
        assert L.poppy_sink_close(s) < 0, f"sink {sink} took a PNG_RUNS frame"
