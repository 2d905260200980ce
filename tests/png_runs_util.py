"""What the POPPY_FRAME_PNG_RUNS tests share: a numpy restatement of the rule (include/poppy_hip.h) from the tables that poppy_png_runs_table hands out, and a
content set built to reach every branch of it.  The filtered stream, the chunks and the walk over a frame are png_util's: the two formats share them.  The
restatement finds the runs from np.diff, takes RFC 1951's length table as a list (the library computes the symbol from the length's leading bit), and packs every
field of the frame in one repeat / shift / packbits.  check_case() asserts, from the restatement alone, that a case reaches what it is built for."""
import functools
import struct
import zlib

import numpy as np

import png_util as P
from poppy_amd import capi

SEGMENT = P.SEGMENT
RUN_MIN = capi.PNG_RUN_MIN
# RFC 1951, 3.2.5: the length symbols 257..285, their extra bits and the smallest length of each
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258; 258 is symbol 285"""
    i = max(i for i in range(29) if LENGTH_BASE[i] <= length)
    return 257 + i, LENGTH_EXTRA[i], length - LENGTH_BASE[i]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables():
    """per table: lengths (286), canonical codes bit-reversed (286), the header's bits"""
    out = []
    for k in range(capi.PNG_TABLES):
        lengths, header = capi.png_runs_table(k)
        lengths = lengths.astype(np.int64)
        codes, code = np.zeros(lengths.size, np.int64), 0
        for bits in range(1, 16):
            for s in np.flatnonzero(lengths == bits):
                codes[s] = int(format(code, f"0{bits}b")[::-1], 2)
                code += 1
            code <<= 1
        out.append((lengths, codes, header.astype(np.int64)))
    return out


def segment_tokens(seg):
    """a segment's tokens in order: (symbols, extra bits, extra values), int64 arrays; a literal has no extra bits, every match is at distance 1"""
    seg = np.asarray(seg)
    n = seg.size
    starts = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
    runs = np.diff(np.r_[starts, n])
    literal = np.ones(n, bool)
    at, sym, eb, ex = [], [], [], []
    for s, r in zip(starts[runs - 1 >= RUN_MIN].tolist(), runs[runs - 1 >= RUN_MIN].tolist()):
        m, p = r - 1, s + 1
        literal[p:s + r] = False
        lengths = [258] * (m // 258) + ([m % 258] if m % 258 >= 3 else [])
        for length in lengths:
            a, b, c = length_symbol(length)
            at.append(p); sym.append(a); eb.append(b); ex.append(c)
            p += length
        literal[p:s + r] = True                             # a remainder of 1 or 2
    lit = np.flatnonzero(literal)
    order = np.argsort(np.r_[lit, np.array(at, np.int64)], kind="stable")
    z = np.zeros(lit.size, np.int64)
    return (np.r_[seg[lit].astype(np.int64), np.array(sym, np.int64)][order], np.r_[z, np.array(eb, np.int64)][order], np.r_[z, np.array(ex, np.int64)][order])


def stream_tokens(stream):
    return [segment_tokens(stream[first:first + SEGMENT]) for first in range(0, stream.size, SEGMENT)]


def table_choice(tokens):
    """per segment the table that codes its tokens in the fewest bits, the first of equals"""
    T = tables()
    out = []
    for sym, eb, _ in tokens:
        beside = int((eb[sym > 256] + 1).sum())             # the matches' extra bits and distance codes
        out.append(int(np.argmin([header.size + lengths[sym].sum() + beside + lengths[256] for lengths, _, header in T])))
    return out


def deflate_bits(tokens, choice):
    T = tables()
    values, widths = [], []
    for s, (k, (sym, eb, ex)) in enumerate(zip(choice, tokens)):
        lengths, codes, header = T[k]
        head = header.copy()
        head[0] = 1 if s == len(choice) - 1 else 0
        match = sym > 256
        body_v = np.stack([codes[sym], ex], 1).ravel()      # a code, then the match's extra bits with the distance code's 0 bit on top (no bits behind a literal)
        body_w = np.stack([lengths[sym], np.where(match, eb + 1, 0)], 1).ravel()
        values += [head, body_v, codes[256:257]]
        widths += [np.ones(head.size, np.int64), body_w, lengths[256:257]]
    values, widths = np.concatenate(values), np.concatenate(widths)
    starts = np.cumsum(widths) - widths
    field = np.repeat(np.arange(values.size), widths)
    bits = (values[field] >> (np.arange(field.size) - starts[field])) & 1
    return np.packbits(bits.astype(np.uint8), bitorder="little").tobytes()


@functools.lru_cache(maxsize=None)
def _restated(name):
    bgr = cases()[name]
    h, w = bgr.shape[:2]
    stream, types = P.filtered_stream(bgr)
    tokens = stream_tokens(stream)
    choice = table_choice(tokens)
    idat = b"\x78\x01" + deflate_bits(tokens, choice) + struct.pack(">I", zlib.adler32(stream.tobytes()))
    file = P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + P.chunk(b"IDAT", idat) + P.chunk(b"IEND", b"")
    frame = np.frombuffer(struct.pack("<I", 4 + len(file)) + file, np.uint8)
    return frame, stream, types, tokens, choice


def restated(name):
    """of a case of the set: (the frame as uint8, the filtered stream, the filter types, the segments' tokens, the tables chosen); computed once"""
    return _restated(name)


# ---- the content set ----------------------------------------------------------------------------------------------------------------------------------------------
def from_residuals(n, runs, first=(100, 90, 80)):
    """A one-row frame whose filtered stream is built: stream byte 0 is the filter type (Sub: the frame is the residuals summed along the row per channel), and the
    n - 1 bytes behind it are 3, 5, 7, 3, ... (no two neighbours equal) with `runs` = [(start, length, value)] laid over them at those STREAM positions.  The row's
    first pixel is `first`, far from 0, so that None and Average score worse than Sub.  check_case asserts the type and the stream from the restatement."""
    assert (n - 1) % 3 == 0
    resid = np.array([3, 5, 7], np.int64)[np.arange(1, n) % 3]
    resid[:3] = first
    for start, length, value in runs:
        assert 4 <= start and start + length <= n
        resid[start - 1:start - 1 + length] = value
    rgb = np.cumsum(resid.reshape(-1, 3), 0) % 256
    return np.ascontiguousarray(rgb[None, :, ::-1].astype(np.uint8)), np.r_[1, resid].astype(np.uint8)


def _built():
    """name -> (bgr, the stream it is built to have, the runs laid into it)"""
    b = {}

    def add(name, n, runs):
        bgr, stream = from_residuals(n, runs)
        b[name] = (bgr, stream, runs)
    # tails m = 7, 8, 9: runs of 8, 9, 10 bytes
    add("tails 7 8 9", 1 + 3 * 40, [(10, 8, 0), (30, 9, 0), (60, 10, 0)])
    # m = 257 .. 261, 516, 519, at odd places
    runs, at = [], 5
    for m in (257, 258, 259, 260, 261, 516, 519):
        runs.append((at, m + 1, 0))
        at += m + 1 + 7
    add("remainders", 1 + 3 * ((at + 2) // 3), runs)
    # a thread's 32 bytes are the stream's 32 j .. 32 j + 31: a run from byte 31 of thread 2, one whose last byte is byte 0 of thread 5, one over threads 7 .. 9
    add("thread boundaries", 1 + 3 * 135, [(95, 12, 0), (150, 11, 0), (200, 150, 0)])
    # one row of 24577 bytes: cuts at 8192 and 16384 and a last segment of ONE byte; a run of 8 + 9 bytes over the first cut, one of 9 + 8 over the second
    add("segment cuts", 1 + 3 * 8192, [(8192 - 8, 17, 0), (16384 - 9, 17, 0), (24577 - 40, 20, 0)])
    # one row of 16384 bytes: a run that ends with the first segment, one that ends with the second and with the stream
    add("segment ends", 1 + 3 * 5461, [(8192 - 300, 300, 0), (16384 - 12, 12, 0)])
    # runs of a byte other than 0
    add("runs of 1 and 200", 1 + 3 * 333, [(20, 9, 1), (40, 270, 1), (400, 8, 1), (500, 300, 200), (900, 3, 0)])
    return b


@functools.lru_cache(maxsize=None)
def cases():
    c = {name: v[0] for name, v in _built().items()}
    c["341x24 black"] = np.zeros((24, 341, 3), np.uint8)                  # three whole segments of zeros, the rows' filter types (0) among them
    c["21x130 black stub"] = np.zeros((130, 21, 3), np.uint8)             # n = 8320: a segment and a stub of 128 bytes, each one run
    y, x = np.mgrid[0:6, 0:200]
    c["200x6 gradient"] = np.ascontiguousarray(np.repeat((x + 7 * y)[:, :, None], 3, 2).astype(np.uint8))      # Sub leaves 1 everywhere, the type byte 1 too
    for name, bgr in P.cases().items():
        c[name] = bgr
    frame = P.band_frame(341, 8, BAND_AMPLITUDES).copy()     # a segment per band: 8 rows of 1024 bytes
    frame[:, :200] = 0                                      # a black margin of 600 bytes per row beside every band: every table with matches among its tokens
    c["bands with margins"] = frame
    for v in c.values():
        v.setflags(write=False)
    return c


BAND_AMPLITUDES = (0, 2, 5, 9, 17, 20, 64, 128)             # 128 +- A noise that the tables 0 .. 7 code best, in this order (check_case asserts it)
PADDED = ("segment cuts", "333x97 cuts mid-row", "40x137 A=20")      # the segment-cut case (a width of 4 n), an odd width, a width of 4 n


def _matches(tokens):
    """per segment the list of match lengths, in order"""
    out = []
    for sym, eb, ex in tokens:
        m = sym > 256
        out.append([LENGTH_BASE[s - 257] + e for s, e in zip(sym[m].tolist(), ex[m].tolist())])
    return out


def check_case(name):
    """asserts, from the restatement, that the case reaches what it is built for"""
    _, stream, types, tokens, choice = restated(name)
    matches = _matches(tokens)
    literals = [int((sym < 256).sum()) for sym, _, _ in tokens]
    built = _built()
    if name in built:
        assert types.tolist() == [1] and (stream == built[name][1]).all(), f"{name}: the stream is not the one it was built to be"
    if name == "tails 7 8 9":
        assert matches == [[8, 9]] and literals == [stream.size - 17]
    elif name == "remainders":
        assert matches == [[257, 258, 258, 258, 258, 3, 258, 258, 258, 258, 3]] and literals[0] == stream.size - sum(matches[0])
    elif name == "thread boundaries":
        assert matches == [[11, 10, 149]]
    elif name == "segment cuts":
        assert stream.size == 3 * SEGMENT + 1 and len(tokens) == 4 and tokens[3][0].size == 1
        assert matches == [[], [8, 8], [19], []]            # tails of 7 in front of the first cut and behind the second: literals
        assert tokens[1][0][:2].tolist() == [0, length_symbol(8)[0]]      # the second segment begins with a literal 0, then the match of 8
        assert tokens[2][0][:9].tolist() == [0] * 8 + [int(stream[2 * SEGMENT + 8])]
    elif name == "segment ends":
        assert stream.size == 2 * SEGMENT and matches == [[258, 41], [11]]
        assert tokens[0][0][-1] == length_symbol(41)[0] and tokens[1][0][-1] == length_symbol(11)[0]      # the blocks' last tokens are the matches
    elif name == "runs of 1 and 200":
        assert matches == [[8, 258, 11, 258, 41]]
        assert set(stream[40:310].tolist()) == {1} and set(stream[500:800].tolist()) == {200}
    elif name == "341x24 black":
        assert not stream.any() and len(tokens) == 3
        assert all(m == [258] * 31 + [193] and n == 1 for m, n in zip(matches, literals))
    elif name == "21x130 black stub":
        assert not stream.any() and matches == [[258] * 31 + [193], [127]] and literals == [1, 1]
    elif name == "341x16 flat":
        rows = stream.reshape(16, 1024)
        assert (rows[:, 0] != 0).all() and not rows[1:, 4:].any()         # every row's type byte breaks the zeros
        assert matches[0] == [258, 258, 258, 245] + [258, 258, 258, 248] * 7
    elif name == "200x6 gradient":
        assert types.tolist() == [1, 1, 4, 4, 4, 4] and set(stream.reshape(6, 601)[:, 4:].ravel().tolist()) == {1}      # (Paeth is Sub here but for the row's first pixel)
        assert sum(len(m) for m in matches) >= 6 * 3
    elif name == "bands with margins":
        assert choice == list(range(8)) and all(len(m) >= 8 for m in matches)
    if name in RUN_FREE:
        assert all(not m for m in matches), f"{name}: built to have no run with a tail of {RUN_MIN}"
    return choice


# the cases of png_util.cases() in which no run has a tail of RUN_MIN bytes or more: their token streams are POPPY_FRAME_PNG's literals
RUN_FREE = ("1x1", "1x5 no left neighbour", "5x1 no row above", "63x3 gradient", "64x3 gradient", "65x3 gradient", "682x4 just under a segment",
            "683x4 just over a segment", "341x8 one segment", "341x128 whole segments", "333x97 cuts mid-row", "341x24 uniform noise", "256x6 every residual",
            "40x137 A=20", "40x137 A=64")
