"""What the POPPY_FRAME_PNG_SEQ tests share: a numpy restatement of the rule (include/poppy_hip.h) and a set of sequences built to reach every branch of it.  The
filtered stream, the chunks and the walk over a frame are png_util's; the tokens, the eight fixed tables and from_residuals png_runs_util's; optimal_lengths,
own_header, canonical_codes, the frame's bits and _stream_case png_opt_util's, all imported unchanged.  New here: the sum of the frames' counts, the choice among
nine candidates whose ninth is the sequence's table, and the frames' assembly.  check_case() asserts, from the restatement alone, that a sequence reaches what it is
built for."""
import functools
import struct
import zlib

import numpy as np

import png_opt_util as O
import png_runs_util as R
import png_util as P
from poppy_amd import capi, synth

SEGMENT = P.SEGMENT
SEQ = O.OWN                                                  # the ninth candidate: the sequence's table
MAX_SYMBOLS = (1 << 32) - 1
HEADER_BITS_MAX = 2083


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------------
def segment_counts(tokens):
    counts = np.bincount(tokens[0], minlength=286)
    counts[256] = 1                                         # one end-of-block per block
    return counts


def seq_table(counts):
    """the sequence's table from its summed counts: dict(lengths, depth before the adjustment, header bits (BFINAL 0), the header sequence's runs)"""
    lengths, depth = O.optimal_lengths(counts, 15)
    header, runs, _ = O.own_header(lengths)
    return dict(lengths=lengths, depth=depth, header=header, runs=runs)


def segment_choice(tokens, table):
    """(the nine costs, the choice: the first of equals, so the sequence's table wins only outright)"""
    sym, eb, _ = tokens
    counts = segment_counts(tokens)
    beside = int((eb[sym > 256] + 1).sum())                 # the matches' extra bits and distance codes
    costs = [int(h.size + (counts * l).sum() + beside) for l, _, h in R.tables()]
    costs.append(int(table["header"].size + (counts * table["lengths"]).sum() + beside))
    return costs, int(np.argmin(costs))


def assemble(bgr, stream, tokens, plans):
    h, w = bgr.shape[:2]
    idat = b"\x78\x01" + O.deflate_bits(tokens, plans) + struct.pack(">I", zlib.adler32(stream.tobytes()))
    file = P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + P.chunk(b"IDAT", idat) + P.chunk(b"IEND", b"")
    return np.frombuffer(struct.pack("<I", 4 + len(file)) + file, np.uint8)


def seq_reference(frames):
    """of a list of HxWx3 BGR frames of one geometry: dict(frames: the coded frames as uint8 arrays, counts: the summed counts, table: seq_table's,
    frame_counts: each frame's own counts, streams, types, choices: per frame the segments' choices, costs: per frame the segments' nine costs)"""
    streams, types, tokens = [], [], []
    for bgr in frames:
        s, t = P.filtered_stream(bgr)
        streams.append(s); types.append(t); tokens.append(R.stream_tokens(s))
    frame_counts = [sum(segment_counts(t) for t in toks) for toks in tokens]
    counts = sum(frame_counts)
    table = seq_table(counts)
    coded, choices, costs = [], [], []
    for bgr, s, toks in zip(frames, streams, tokens):
        picked = [segment_choice(t, table) for t in toks]
        plans = [dict(choice=k, lengths=table["lengths"], header=table["header"]) for _, k in picked]
        coded.append(assemble(bgr, s, toks, plans))
        costs.append([c for c, _ in picked]); choices.append([k for _, k in picked])
    return dict(frames=coded, counts=counts, table=table, frame_counts=frame_counts, streams=streams, types=types, choices=choices, costs=costs)


def unfilter(stream, w, h):
    """the HxWx3 BGR frame of a filtered stream: PNG's five filters undone row by row"""
    rows = np.asarray(stream, np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), np.int64)
    for y in range(h):
        t, line = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(3 * w, np.int64)
        if t == 0:
            out[y] = line
        elif t == 1:
            out[y] = np.cumsum(line.reshape(w, 3), 0).ravel() % 256
        elif t == 2:
            out[y] = (line + up) % 256
        else:
            cur = out[y]
            for i in range(3 * w):
                a = int(cur[i - 3]) if i >= 3 else 0
                b = int(up[i])
                c = int(up[i - 3]) if i >= 3 else 0
                if t == 3:
                    pred = (a + b) // 2
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (int(line[i]) + pred) % 256
    return np.ascontiguousarray(out.reshape(h, w, 3)[:, :, ::-1].astype(np.uint8))


def decoded(frame, w, h):
    """a coded frame through zlib's decoder and unfilter: the BGR frame"""
    chunks = P.walk_frame(frame)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    assert chunks[1][1][:2] == b"\x78\x01"
    return unfilter(np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8), w, h)


def decodes_to(frame, bgr):
    """whether a coded frame, through zlib's decoder and the filters undone, is the BGR frame — without the byte-by-byte walk of unfilter(): every filter is a
    bijection of a row given the rows above it, so undoing the stream's filters gives `bgr` exactly when filtering `bgr` with the stream's own types gives the stream"""
    h, w = bgr.shape[:2]
    chunks = P.walk_frame(frame)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    stream = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8)
    if stream.size != h * (1 + 3 * w):
        return False
    rows = stream.reshape(h, 1 + 3 * w)
    types = rows[:, 0].astype(np.int64)
    if types.max() > 4:
        return False
    cur = bgr[:, :, ::-1].reshape(h, 3 * w).astype(np.int64)
    a = np.zeros_like(cur); a[:, 3:] = cur[:, :-3]
    b = np.zeros_like(cur); b[1:] = cur[:-1]
    c = np.zeros_like(cur); c[1:, 3:] = cur[:-1, :-3]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    candidates = np.stack([cur, cur - a, cur - b, cur - (a + b) // 2, cur - paeth]) % 256
    return bool((candidates[types, np.arange(h)] == rows[:, 1:]).all())


def seq_fits(n_frames, w, h):
    """the sequence limit (include/poppy_hip.h: Limits), the per-frame limits aside"""
    n = h * (1 + 3 * w)
    return n_frames >= 1 and n_frames * (n + -(-n // SEGMENT)) <= MAX_SYMBOLS


# ---- the sequences ------------------------------------------------------------------------------------------------------------------------------------------------
def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _margins(frame, step):
    frame = frame.copy()
    for y in range(frame.shape[0]):
        frame[y, :(3 + step * y) % frame.shape[1]] = 0
    return frame


def _disjoint_pair():
    """two one-row frames whose literal sets share only the forced bytes (the filter-type byte 1 and the first pixel 100, 90, 80); skewed counts, so that a code built
    from them beats every fixed table by more than its header"""
    def counts(values):
        c = {v: 1 for v in (1, 100, 90, 80)}
        for i, v in enumerate(values):
            c[v] = 120 if i < 4 else 40 if i < 12 else 6
        c[values[0]] += (1 - sum(c.values())) % 3
        return c
    return [O._stream_case(counts(list(range(2, 34)))), O._stream_case(counts(list(range(224, 256))))]      # (residuals near 0 either way: Sub stays the row's filter)


def _stream_of(counts):
    """png_opt_util._stream_case for counts of which one is more than half of all: its _spread cannot keep equal neighbours apart then, so here the most frequent
    symbol of those left may stand up to four times in a row — a run of four has a tail of three, below POPPY_PNG_RUN_MIN, and stays four literals"""
    left = dict(counts)
    for v in (1, 100, 90, 80):
        assert left.get(v, 0) >= 1
        left[v] -= 1
    body = []
    while any(left.values()):
        blocked = body[-1] if len(body) >= 4 and len(set(body[-4:])) == 1 else None
        v = max((v for v in left if left[v] and v != blocked), key=lambda v: (left[v], -v))
        body.append(v)
        left[v] -= 1
    return R.from_residuals(4 + len(body), [(4 + i, 1, v) for i, v in enumerate(body)])


def _split_fibonacci(n_symbols):
    """two frames (_stream_of) that split a Fibonacci-like series of counts by symbol: the four forced bytes stand once in either frame, every other symbol in one
    frame alone, alternately.  Behind the forced bytes and the two end-of-blocks (six counts of 2: a tree of 12) the series grows so that every further symbol
    joins the whole tree so far: the summed counts are one chain, each frame's own counts are two interleaved halves of it."""
    series = [12, 12]
    while len(series) < n_symbols:
        series.append(series[-1] + series[-2])
    values = list(range(2, 2 + n_symbols))
    halves = [{v: 1 for v in (1, 100, 90, 80)}, {v: 1 for v in (1, 100, 90, 80)}]
    for i, (v, c) in enumerate(zip(values, series)):
        halves[i % 2][v] = c
    # one geometry: the shorter frame's most frequent symbol takes the difference (the chain's last links only grow), then both are 1 + 3 k bytes long
    size = [sum(h.values()) for h in halves]
    top = [max(h, key=h.get) for h in halves]
    halves[int(np.argmin(size))][top[int(np.argmin(size))]] += abs(size[0] - size[1])
    pad = (1 - sum(halves[0].values())) % 3
    for h, t in zip(halves, top):
        h[t] += pad
    return [_stream_of(h) for h in halves]


def _every_symbol_pair():
    """two one-row frames (png_runs_util.from_residuals) that together hold every literal and a match of every length 3..258: a run of L + 1 equal bytes for L >= 8,
    of 258 + L + 1 for L < 8 (a full match and the remainder), none across a segment cut; the 256 literals stand one by one in the first frame"""
    def lay(lengths, literals):
        runs, at = [], 8
        for v in literals:
            runs.append((at, 1, v)); at += 2
        for L in lengths:
            r = L + 1 if L >= R.RUN_MIN else 258 + L + 1
            if at // SEGMENT != (at + r + 1) // SEGMENT:
                at = (at // SEGMENT + 1) * SEGMENT + 8      # not across a cut
            runs.append((at, r, 0 if L % 2 else 200)); at += r + 5
        return runs, at
    first, n1 = lay(list(range(3, 185)), list(range(256)))
    second, n2 = lay(list(range(185, 259)), [])
    n = max(n1, n2) + 8
    n += (1 - n) % 3
    return [R.from_residuals(n, first), R.from_residuals(n, second)]


def _fades(a, b, n=3):
    a, b = a.astype(np.int64), b.astype(np.int64)
    return [((a * (n + 1 - k) + b * k + (n + 1) // 2) // (n + 1)).astype(np.uint8) for k in range(1, n + 1)]


@functools.lru_cache(maxsize=None)
def _built():
    """name -> [(bgr, the stream it is built to have)] of the sequences made from residuals"""
    return {"disjoint alphabets": _disjoint_pair(), "depth 16 in the sums": _split_fibonacci(13), "depth 17 in the sums": _split_fibonacci(14),
            "all 286 symbols": _every_symbol_pair()}


@functools.lru_cache(maxsize=None)
def sequences():
    """name -> list of HxWx3 BGR frames of one geometry"""
    s = {}
    s["one frame, one segment"] = [O.cases()["341x8 noise with margins"]]
    s["21x128 one full segment"] = [_margins(_noise(21, 128, 31), 5), _noise(21, 128, 32)]        # n = 8192
    s["21x129 a second segment of 64 bytes"] = [_margins(_noise(21, 129, 33), 5), _noise(21, 129, 34)]      # n = 8256
    for name, pair in _built().items():
        s[name] = [bgr for bgr, _ in pair]
    s["341x24 black twice"] = [R.cases()["341x24 black"]] * 2
    s["21x1 noise, four frames"] = [_noise(21, 1, 40 + k) for k in range(4)]      # 64 bytes a frame: no table of 250 symbols earns its header back on one of them
    s["40x137 noise, two seeds"] = [O.cases()["40x137 uniform noise"], _noise(40, 137, 5)]
    s["40x137 noise and flat"] = [O.cases()["40x137 uniform noise"], np.full((137, 40, 3), 77, np.uint8)]
    s["128x96 textured fades"] = _fades(synth.textured_bgr(128, 96, 7), synth.textured_bgr(128, 96, 9))
    s["128x96 photograph fades"] = _fades(*synth.photo_pair(128, 96))
    for frames in s.values():
        for f in frames:
            f.setflags(write=False)
    return s


PAYS = ("128x96 textured fades", "128x96 photograph fades")    # content where the format pays: every frame strictly smaller than its PNG_RUNS frame
LOSES = "21x1 noise, four frames"                           # the sequence whose frames are their PNG_RUNS frames byte for byte
LARGEST = "all 286 symbols"                                  # the sequence with the most segments per frame


@functools.lru_cache(maxsize=None)
def restated(name):
    """seq_reference of a sequence of the set; computed once"""
    return seq_reference(sequences()[name])


def kraft_is_one(lengths):
    return sum(1 << (15 - int(l)) for l in lengths if l) == 1 << 15


def check_case(name):
    """asserts, from the restatement, that the sequence reaches what it is built for; returns the frames' choices"""
    frames, r = sequences()[name], restated(name)
    t, choices = r["table"], r["choices"]
    n_seg = sum(len(c) for c in choices)
    assert r["counts"][256] == n_seg and int(r["counts"].sum()) <= MAX_SYMBOLS
    assert t["lengths"].max() <= 15 and kraft_is_one(t["lengths"]) and 17 <= t["header"].size <= HEADER_BITS_MAX
    assert ((t["lengths"] > 0) == (r["counts"] > 0)).all(), "a symbol has a code exactly where some segment gave it a count"
    for costs, picked in zip(r["costs"], choices):
        for c, k in zip(costs, picked):
            assert (k == SEQ) == all(c[SEQ] < x for x in c[:SEQ]), "the sequence's table wins only outright"
    flat = [k for c in choices for k in c]
    if name in _built():
        for (bgr, stream), got, types in zip(_built()[name], r["streams"], r["types"]):
            assert types.tolist() == [1] and (got == stream).all(), f"{name}: a stream is not the one it was built to be"
    if name == "one frame, one segment":
        assert flat == [SEQ]
    elif name == "21x128 one full segment":
        assert all(s.size == SEGMENT for s in r["streams"]) and [len(c) for c in choices] == [1, 1]
    elif name == "21x129 a second segment of 64 bytes":
        assert all(s.size == SEGMENT + 64 for s in r["streams"]) and [len(c) for c in choices] == [2, 2]
    elif name == "disjoint alphabets":
        a, b = (set(np.flatnonzero(c[:256]).tolist()) for c in r["frame_counts"])
        assert a & b == {1, 100, 90, 80} and len(a) > 4 and len(b) > 4
        assert all(t["lengths"][v] for v in a | b), "the table holds codes for symbols each frame lacks"
        assert flat == [SEQ, SEQ], "table 8 wins in both frames"
    elif name.startswith("depth "):
        d = int(name.split()[1])
        own = [int(O.optimal_lengths(c, 15)[1].max()) for c in r["frame_counts"]]
        assert max(own) < 16 and int(t["depth"].max()) == d and t["lengths"].max() == 15, (own, int(t["depth"].max()))
    elif name == "341x24 black twice":
        # by the rule the table of an all-black sequence is four symbols (0, end-of-block, two match lengths) and a header about half as long as the shortest
        # fixed table's: it wins every segment, and the frames are their PNG_OPT frames' size, not their PNG_RUNS frames'
        assert np.count_nonzero(r["counts"]) == 4 and t["header"].size < min(h.size for _, _, h in R.tables()) and all(k == SEQ for k in flat)
    elif name == "21x1 noise, four frames":
        assert all(k < SEQ for k in flat), "the shared table loses everywhere"
    elif name == "40x137 noise, two seeds":
        assert len(flat) == 6
    elif name == "40x137 noise and flat":
        assert SEQ in choices[0] and min(choices[0] + choices[1]) < SEQ, "both the sequence's table and a fixed one occur"
    elif name == "all 286 symbols":
        assert (r["counts"] > 0).all() and (t["lengths"] > 0).all() and max(len(c) for c in choices) >= 3
    return choices


# ---- the table alone: name -> 286 counts ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_families():
    """Every family of png_opt_util.count_families() of 286 or fewer entries, padded with zeros to 286, that then has a count for symbol 256; a family whose entries
    end below 256 stands a second time moved up so that its LAST entry is symbol 256's (the same counts on other symbols: "a sum just under 2^32" and Fibonacci 40
    with its depth of 39 reach the build this way)."""
    f = {}
    for name, (counts, _) in O.count_families().items():
        if len(counts) > 286:
            continue
        padded = np.zeros(286, np.uint64)
        padded[:len(counts)] = counts
        if padded[256]:
            f[name] = padded
        elif counts[-1]:
            moved = np.zeros(286, np.uint64)
            moved[257 - len(counts):257] = counts
            f[name + ", ending at 256"] = moved
    for name in ("286 equal counts", "a ramp of 286", "a sum just under 2^32, ending at 256", "fibonacci 40: depth 39, ending at 256"):
        assert name in f, name
    return f


def table_reference(counts):
    """(lengths, header bits) of the restatement"""
    t = seq_table([int(c) for c in counts])
    return t["lengths"], t["header"]


def host_frames(frames, **pads):
    return capi.bgr_frames_to_png_seq_frames(np.stack(frames), **pads)
