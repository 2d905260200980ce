"""The POPPY_FRAME_PNG_OPT hand-off on the host (include/poppy_hip.h has the rule): poppy_bgr_to_png_opt_frame against a numpy restatement of the rule
(png_opt_util.py) and, independently of any restatement, against zlib's and Pillow's decoders; never more bytes than POPPY_FRAME_PNG_RUNS; poppy_png_optimal_lengths
on every count family against the restatement, with a Kraft sum of exactly 1; the refusals and the unknown values.  The content set is png_opt_util.cases(), and
every case asserts what it reaches."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_opt_util as O
import png_util as P
from poppy_amd import capi

E_ARG, E_UNSUPPORTED = -1, -6
CASES = list(O.cases())
FAMILIES = [(name, limit) for name, (_, limits) in O.count_families().items() for limit in limits]


@pytest.fixture(scope="module")
def host_frames():
    """name -> the host statement's whole destination buffer (canary-filled before the call)"""
    return {name: capi.bgr_to_png_opt_frame(bgr, whole=True) for name, bgr in O.cases().items()}


def _frame(buf):
    return buf[:capi.png_frame_bytes(buf)]


@pytest.mark.parametrize("name", CASES)
def test_host_statement_is_the_restated_rule(host_frames, name):
    O.check_case(name)
    P.equal(name, _frame(host_frames[name]), O.restated(name)[0])


@pytest.mark.parametrize("name", CASES)
def test_decoders_give_back_the_frame_and_runs_is_no_smaller(host_frames, name):
    bgr, buf = O.cases()[name], host_frames[name]
    h, w = bgr.shape[:2]
    total = capi.png_frame_bytes(buf)
    capacity = capi.frame_bytes(capi.FRAME_PNG_OPT, w, h)
    assert 0 < total <= capacity and buf.size == capacity + 64
    assert (buf[total:] == capi.PNG_CANARY).all(), "bytes behind `total` were written"
    assert total <= capi.bgr_to_png_runs_frame(bgr).size, "a PNG_OPT frame is never longer than the PNG_RUNS frame"
    chunks = P.walk_frame(buf[:total])
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0) and chunks[2][1] == b""
    idat = chunks[1][1]
    assert idat[:2] == b"\x78\x01"
    stream, _ = P.filtered_stream(bgr)
    assert zlib.decompress(idat) == stream.tobytes()


@pytest.mark.parametrize("name", CASES)
def test_pillow_decodes_the_file_to_the_frame(host_frames, name):
    Image = pytest.importorskip("PIL.Image")
    bgr, buf = O.cases()[name], host_frames[name]
    h, w = bgr.shape[:2]
    with Image.open(io.BytesIO(_frame(buf)[4:].tobytes())) as im:
        im.load()
        assert im.mode == "RGB" and im.size == (w, h)
        assert (np.asarray(im) == bgr[:, :, ::-1]).all()


def test_row_pads_do_not_matter():
    for name in O.PADDED:
        bgr = O.cases()[name]
        want = capi.bgr_to_png_opt_frame(bgr)
        for pad in (1, 7, 64):
            P.equal(f"{name} pad {pad}", capi.bgr_to_png_opt_frame(bgr, row_pad=pad), want)


def test_content_set_reaches_both_kinds_of_choice_and_every_entry_of_the_header():
    choices, zero_runs, other_runs, sent, deepest = set(), set(), set(), set(), 0
    for name in CASES:
        for p in O.restated(name)[4]:
            choices.add(p["choice"])
            if p["choice"] != O.OWN:
                continue
            zero_runs |= {r for v, r in p["runs"] if v == 0}
            other_runs |= {r for v, r in p["runs"] if v != 0}
            sent |= {s for s, _, _ in O.header_sequence(p["lengths"])[1]}
            deepest = max(deepest, int(p["depth"].max()))
    assert O.OWN in choices and min(choices) < O.OWN
    assert {2, 3, 10, 11, 138, 139, 149} <= zero_runs and {3, 4, 7, 8} <= other_runs
    assert {0, 16, 17, 18} <= sent
    assert deepest == 17
    # a code-length code deeper than 7 before the adjustment is not asked of the frames (19 symbols over fewer than 290 entries): the count family has it
    lengths, depth = O.optimal_lengths([1, 2, 3, 5, 8, 13, 21, 34, 55], 7)
    assert depth.max() == 8 and lengths.max() == 7


@pytest.mark.parametrize("name,limit", FAMILIES)
def test_optimal_lengths_on_the_count_families(name, limit):
    counts = O.count_families()[name][0]
    got = capi.png_optimal_lengths(counts, limit).astype(np.int64)
    want, _ = O.optimal_lengths(counts, limit)
    assert got.tolist() == want.tolist()
    used = np.flatnonzero(counts)
    assert (got[used] >= 1).all() and got.max() <= limit and not got[np.asarray(counts) == 0].any()
    if used.size > 1:
        assert sum(1 << (limit - int(l)) for l in got[used]) == 1 << limit, "the Kraft sum is exactly 1"
    else:
        assert got[used].tolist() == [1]


def test_deep_trees_are_limited_and_ties_take_the_larger_index():
    lengths, depth = O.optimal_lengths(O.fibonacci(18), 15)
    assert depth.max() == 17 and lengths.max() == 15
    # every family that 7 bits hold is built at both limits, and trees of depth 16 and more are among those squeezed into 7 bits
    for name, (counts, limits) in O.count_families().items():
        assert limits == ((7, 15) if np.count_nonzero(counts) <= 128 else (15,)), name
    deep_at_7 = [name for name, limit in FAMILIES if limit == 7 and O.optimal_lengths(O.count_families()[name][0], 7)[1].max() >= 16]
    assert len(deep_at_7) >= 4 and any(np.count_nonzero(O.count_families()[name][0]) == 128 for name in deep_at_7), deep_at_7
    # 1, 1, 1, 1: two merges of equals, then the two trees; 1, 1, 2: the tie between the tree and the 2 goes to the larger index, the tree at symbol 1
    assert capi.png_optimal_lengths([1, 1, 1, 1]).tolist() == [2, 2, 2, 2]
    assert capi.png_optimal_lengths([1, 1, 2]).tolist() == [2, 2, 1]
    assert capi.png_optimal_lengths([2, 1, 1, 1]).tolist() == O.optimal_lengths([2, 1, 1, 1], 15)[0].tolist()


def test_refusals_symbols_and_unknown_values(tmp_path):
    L = capi.lib()
    one = np.zeros(256, np.uint8)
    f = L.poppy_bgr_to_png_opt_frame
    assert f(None, 6, 2, 2, capi._p(one)) == E_ARG and f(capi._p(one), 6, 2, 2, None) == E_ARG
    assert f(capi._p(one), 5, 2, 2, capi._p(one)) == E_ARG
    assert f(capi._p(one), 6, 0, 2, capi._p(one)) == E_ARG and f(capi._p(one), 6, 2, -1, capi._p(one)) == E_ARG
    for w, h in ((1, 1), (341, 8), (683, 4), (1920, 1080), (25000, 25000)):
        assert 0 < capi.frame_bytes(capi.FRAME_PNG_OPT, w, h) == capi.frame_bytes(capi.FRAME_PNG_RUNS, w, h)
    for w, h in ((26000, 26000), (1 << 30, 1), (1, 1 << 30), (65536, 65536)):
        assert capi.frame_bytes(capi.FRAME_PNG_OPT, w, h) == 0
        assert f(capi._p(one), 3 * w, w, h, capi._p(one)) == E_UNSUPPORTED
    g = L.poppy_png_optimal_lengths
    counts, out = np.ones(286, np.uint32), np.zeros(286, np.uint8)
    assert g(capi._p(counts), 286, 15, capi._p(out)) == 0
    assert g(None, 286, 15, capi._p(out)) == E_ARG and g(capi._p(counts), 286, 15, None) == E_ARG
    for n in (0, -1, 287):
        assert g(capi._p(counts), n, 15, capi._p(out)) == E_ARG
    for limit in (0, 6, 8, 14, 16):
        assert g(capi._p(counts), 19, limit, capi._p(out)) == E_ARG
    assert g(capi._p(np.zeros(286, np.uint32)), 286, 15, capi._p(out)) == E_ARG
    big = np.array([1 << 31, 1 << 31], np.uint32)
    assert g(capi._p(big), 2, 15, capi._p(out)) == E_ARG, "a sum of 2^32"
    big[1] -= 1
    assert g(capi._p(big), 2, 15, capi._p(out)) == 0 and out[:2].tolist() == [1, 1]
    assert g(capi._p(counts), 128, 7, capi._p(out)) == 0 and g(capi._p(counts), 129, 7, capi._p(out)) == E_ARG, "129 symbols have no code of 7 bits"
    for name in ("poppy_png_optimal_lengths", "poppy_bgr_to_png_opt_frame", "poppy_hip_bgr_to_png_opt_frame", "poppy_hip_png_optimal_lengths"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert capi.FRAME_PNG_OPT == 16384 and capi.FRAME_PNG_OPT in capi.FRAMES_CODED
    for value in (16383, 16385):
        assert capi.frame_bytes(value, 16, 16) == 0
        assert not L.poppy_sink_open(str(tmp_path / "x%d").encode(), value, 16, 16, 25, 1)
    assert not L.poppy_sink_open(str(tmp_path / "x%d").encode(), 16384, 16, 16, 25, 1), "there is no sink value for the format: POPPY_SINK_PNG takes it"


def test_png_sink_takes_the_format_among_the_others(tmp_path):
    L = capi.lib()
    w, h = 65, 3
    frames = [np.roll(P.cases()["65x3 gradient"], k, 1) for k in range(3)] + [np.zeros((h, w, 3), np.uint8)]
    coders = (capi.bgr_to_png_opt_frame, capi.bgr_to_png_frame, capi.bgr_to_png_runs_frame, capi.bgr_to_png_opt_frame)
    coded = [coder(f) for coder, f in zip(coders, frames)]
    s = L.poppy_sink_open(str(tmp_path / "f_%03d.png").encode(), capi.SINK_PNG, w, h, 25, 1)
    assert s
    for f in coded:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(frames)
    for k in range(len(frames)):
        assert (tmp_path / f"f_{k:03d}.png").read_bytes() == coded[k][4:].tobytes()
    for sink in (capi.SINK_RAW, capi.SINK_PPM, capi.SINK_Y4M, capi.SINK_MJPEG, capi.SINK_GIF_CODED):
        s = L.poppy_sink_open(str(tmp_path / "p_%d.bin").encode(), sink, w, h, 25, 1)
        assert s
        L.poppy_sink_write(s, capi._p(np.concatenate([coded[0], np.zeros(1024, np.uint8)])), w, h, 0)
        assert L.poppy_sink_close(s) < 0, f"sink {sink} took a PNG_OPT frame"
