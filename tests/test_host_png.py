"""The POPPY_FRAME_PNG hand-off on the host (include/poppy_hip.h has the rule): poppy_bgr_to_png_frame against a numpy restatement built from the tables that
poppy_png_table hands out (png_util.py), and, independently of any restatement, against zlib's and Pillow's decoders; the tables themselves; the refusals; the
PNG sink.  The content set is png_util.cases(); this file asserts that it reaches every filter type and every table."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_util as P
from poppy_amd import capi

E_ARG, E_UNSUPPORTED = -1, -6
CASES = list(P.cases())


@pytest.fixture(scope="module")
def host_frames():
    """name -> the host statement's whole destination buffer (canary-filled before the call)"""
    return {name: capi.bgr_to_png_frame(bgr, whole=True) for name, bgr in P.cases().items()}


def _frame(buf):
    return buf[:capi.png_frame_bytes(buf)]


@pytest.mark.parametrize("name", CASES)
def test_host_statement_is_the_restated_rule(host_frames, name):
    want, _, _ = P.restated_frame(P.cases()[name])
    P.equal(name, _frame(host_frames[name]), want)


@pytest.mark.parametrize("name", CASES)
def test_decoders_give_back_the_frame(host_frames, name):
    Image = pytest.importorskip("PIL.Image")
    bgr, buf = P.cases()[name], host_frames[name]
    h, w = bgr.shape[:2]
    total = capi.png_frame_bytes(buf)
    capacity = capi.frame_bytes(capi.FRAME_PNG, w, h)
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
    for name in ("333x97 cuts mid-row", "5x1 no row above"):
        bgr = P.cases()[name]
        want = capi.bgr_to_png_frame(bgr)
        for pad in (1, 7, 64):
            P.equal(f"{name} pad {pad}", capi.bgr_to_png_frame(bgr, row_pad=pad), want)


def test_content_set_reaches_every_filter_and_every_table(host_frames):
    """From the host statement's output alone for the filters (the first byte of every decompressed row); the tables from the restatement's choice, which
    test_host_statement_is_the_restated_rule ties to the same bytes."""
    filters, tables_seen, residuals = set(), set(), set()
    for name, bgr in P.cases().items():
        h, w = bgr.shape[:2]
        idat = P.walk_frame(_frame(host_frames[name]))[1][1]
        rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
        filters |= set(rows[:, 0].tolist())
        stream, _ = P.filtered_stream(bgr)
        tables_seen |= set(P.table_choice(stream))
        if name == "256x6 every residual":
            residuals = set(rows[:, 1:].ravel().tolist())
    assert filters == {0, 1, 2, 3, 4}
    assert tables_seen == set(range(capi.PNG_TABLES))
    assert residuals == set(range(256))


def test_named_cases_take_the_path_they_are_named_for():
    c = P.cases()
    assert [bgr.shape[0] * (1 + 3 * bgr.shape[1]) for bgr in (c["682x4 just under a segment"], c["683x4 just over a segment"], c["341x8 one segment"])] == [8188, 8200, 8192]
    stream, types = P.filtered_stream(c["341x16 flat"])
    assert P.table_choice(stream) == [0, 0]
    assert P.table_choice(P.filtered_stream(c["341x24 uniform noise"])[0]) == [7, 7, 7]
    assert P.filtered_stream(c["341x128 whole segments"])[0].size == 16 * P.SEGMENT
    stub = P.filtered_stream(c["21x130 stub segment"])[0]
    assert stub.size % P.SEGMENT == 128 and P.table_choice(stub)[-1] == 7      # the header dominates a 128-byte block
    assert (P.filtered_stream(c["90x40 columns"])[1][1:] == 2).all()
    # noise at capacity: every byte on table 7 at close to its longest code, and still inside the bound
    noise = c["341x24 uniform noise"]
    assert capi.png_frame_bytes(capi.bgr_to_png_frame(noise)) > noise.size


@pytest.mark.parametrize("k", range(capi.PNG_TABLES))
def test_tables_are_complete_codes_and_headers_decode_to_them(k):
    lengths, codes, header = P.tables()[k]
    assert lengths.size == 257 and lengths.min() >= 1 and lengths.max() <= 15
    assert sum(1 << (15 - int(l)) for l in lengths) == 1 << 15, "the Kraft sum is exactly 1"
    assert 17 + 4 * 3 <= header.size <= 8 * capi.PNG_HEADER_BYTES and header[0] == 0 and header[1:3].tolist() == [0, 1] and not header[3:13].any()
    # one final block on this table holding every literal once: zlib's inflate decodes the header, so it reads the same lengths
    literals = np.arange(256)[::-1].copy()
    head = header.copy(); head[0] = 1
    values = np.concatenate([head, codes[literals], codes[256:257]])
    widths = np.concatenate([np.ones(head.size, np.int64), lengths[literals], lengths[256:257]])
    starts = np.cumsum(widths) - widths
    symbol = np.repeat(np.arange(values.size), widths)
    bits = (values[symbol] >> (np.arange(symbol.size) - starts[symbol])) & 1
    raw = np.packbits(bits.astype(np.uint8), bitorder="little").tobytes()
    d = zlib.decompressobj(wbits=-15)
    assert d.decompress(raw) == bytes(literals.tolist()) and d.eof


def test_table_seven_bounds_the_capacity():
    lengths, _, header = P.tables()[7]
    assert lengths[:256].max() <= 9
    for w, h in ((1, 1), (341, 8), (683, 4), (1920, 1080)):
        n = h * (1 + 3 * w)
        n_seg = -(-n // P.SEGMENT)
        assert capi.frame_bytes(capi.FRAME_PNG, w, h) == 67 + -(-(n_seg * (header.size + int(lengths[256])) + int(lengths[:256].max()) * n) // 8)


def test_refusals_symbols_and_unknown_values(tmp_path):
    L = capi.lib()
    one = np.zeros(256, np.uint8)
    assert L.poppy_bgr_to_png_frame(None, 6, 2, 2, capi._p(one)) == E_ARG and L.poppy_bgr_to_png_frame(capi._p(one), 6, 2, 2, None) == E_ARG
    assert L.poppy_bgr_to_png_frame(capi._p(one), 5, 2, 2, capi._p(one)) == E_ARG
    assert L.poppy_bgr_to_png_frame(capi._p(one), 6, 0, 2, capi._p(one)) == E_ARG and L.poppy_bgr_to_png_frame(capi._p(one), 6, 2, -1, capi._p(one)) == E_ARG
    # 25000 x 25000 is the format's: its capacity is below 2^31; 26000 x 26000 is not, and is refused before a byte is read
    assert 0 < capi.frame_bytes(capi.FRAME_PNG, 25000, 25000) < 1 << 31
    for w, h in ((26000, 26000), (1 << 30, 1), (1, 1 << 30), (65536, 65536)):
        assert capi.frame_bytes(capi.FRAME_PNG, w, h) == 0
        assert L.poppy_bgr_to_png_frame(capi._p(one), 3 * w, w, h, capi._p(one)) == E_UNSUPPORTED
    assert L.poppy_png_table(-1, None, None, None) == E_ARG and L.poppy_png_table(8, None, None, None) == E_ARG and L.poppy_png_table(3, None, None, None) == 0
    assert L.poppy_png_frame_bytes(None) == 0
    for name in ("poppy_png_frame_bytes", "poppy_png_table", "poppy_bgr_to_png_frame", "poppy_hip_bgr_to_png_frame"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert (capi.FRAME_PNG, capi.SINK_PNG, capi.PNG_SEGMENT_BYTES, capi.PNG_TABLES) == (1024, 1024, 8192, 8)
    for value in (1023, 1025):
        assert capi.frame_bytes(value, 16, 16) == 0
        assert not L.poppy_sink_open(str(tmp_path / "x%d").encode(), value, 16, 16, 25, 1)


def test_png_sink_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    L = capi.lib()
    w, h = 65, 3
    frames = [np.roll(P.cases()["65x3 gradient"], k, 1) for k in range(3)]
    coded = [capi.bgr_to_png_frame(f) for f in frames]
    s = L.poppy_sink_open(str(tmp_path / "f_%03d.png").encode(), capi.SINK_PNG, w, h, 25, 1)
    assert s
    for f in coded:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == 3
    for k, f in enumerate(frames):
        path = tmp_path / f"f_{k:03d}.png"
        assert path.read_bytes() == coded[k][4:].tobytes()
        with Image.open(path) as im:
            assert (np.asarray(im.convert("RGB")) == f[:, :, ::-1]).all()
    # the path follows PPM's rule: exactly one %d conversion
    for bad in ("plain.png", "a_%s.png", "a_%d_%d.png"):
        assert not L.poppy_sink_open(str(tmp_path / bad).encode(), capi.SINK_PNG, w, h, 25, 1)

    def fails(sink_format, frame, stride, path="o_%d.bin", size=(w, h)):
        s = L.poppy_sink_open(str(tmp_path / path).encode(), sink_format, size[0], size[1], 25, 1)
        assert s
        L.poppy_sink_write(s, capi._p(frame), w, h, stride)
        return L.poppy_sink_close(s) < 0
    bgr = np.ascontiguousarray(frames[0])
    big = np.zeros(1024, np.uint8)                          # (room for every read a sink makes before it refuses)
    jpeg = big.copy(); j = capi.bgr_to_jpeg_frame(bgr); jpeg = np.concatenate([j, big])
    gif = np.concatenate([capi.bgr_to_gif_frame(bgr), big])
    png = np.concatenate([coded[0], big])
    # frames of any other format fail the PNG sink ...
    assert fails(capi.SINK_PNG, jpeg, 0) and fails(capi.SINK_PNG, gif, 0) and fails(capi.SINK_PNG, bgr, w * 3) and fails(capi.SINK_PNG, png, w * 3)
    # ... as does a PNG frame of another size, or one whose `total` is past the capacity
    other = np.concatenate([capi.bgr_to_png_frame(P.cases()["64x3 gradient"]), big])
    assert fails(capi.SINK_PNG, other, 0)
    long = png.copy(); long[:4] = np.frombuffer(struct.pack("<I", capi.frame_bytes(capi.FRAME_PNG, w, h) + 1), np.uint8)
    assert fails(capi.SINK_PNG, long, 0)
    assert not fails(capi.SINK_PNG, png, 0)
    # ... and a PNG frame fails every other sink
    for sink in (capi.SINK_RAW, capi.SINK_PPM, capi.SINK_Y4M, capi.SINK_Y4M420, capi.SINK_GIF, capi.SINK_GIF_GLOBAL, capi.SINK_GIF_CODED, capi.SINK_GIF_GLOBAL_CODED, capi.SINK_MJPEG):
        assert fails(sink, png, 0), f"sink {sink} took a PNG frame"
