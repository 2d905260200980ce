"""What the POPPY_FRAME_PNG_OPT tests share: a numpy restatement of the rule (include/poppy_hip.h) — the lengths of a segment's own table, its run-coded block
header, the choice among nine candidates and the frame's bits — and a content set built to reach every branch of it.  The filtered stream, the chunks and the
walk over a frame are png_util's, the tokens, the eight fixed tables and from_residuals png_runs_util's.  The restatement keeps the trees of the length rule as
sets of symbols where the library keeps a root per symbol, reads the header's sequence with itertools.groupby, and packs every field of the frame in one
repeat / shift / packbits.  check_case() asserts, from the restatement alone, that a case reaches what it is built for."""
import functools
import itertools
import struct
import zlib

import numpy as np

import png_runs_util as R
import png_util as P

SEGMENT = P.SEGMENT
OWN = 8                                                      # the ninth candidate
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------------
def optimal_lengths(counts, limit):
    """(lengths, depths before the adjustment) of the counts by the rule's seven steps"""
    count = [int(c) for c in counts]
    n = len(count)
    trees = {s: {s} for s in range(n) if count[s]}
    depth = [0] * n
    while len(trees) > 1:
        # the smallest non-zero count, the largest index among equals; the same among the rest
        c1 = min(trees, key=lambda s: (count[s], -s))
        c2 = min((s for s in trees if s != c1), key=lambda s: (count[s], -s))
        count[c1] += count[c2]
        count[c2] = 0
        trees[c1] |= trees.pop(c2)
        for s in trees[c1]:
            depth[s] += 1
    if len(trees) == 1 and max(depth) == 0:
        depth[next(iter(trees))] = 1                        # a single symbol with a count
    of = [0] * (max(max(depth), limit) + 2)
    for d in depth:
        if d:
            of[d] += 1
    for i in range(len(of) - 1, limit, -1):                 # Annex K.3 with `limit` in the place of 16
        while of[i] > 0:
            j = i - 2
            while of[j] == 0:
                j -= 1
            of[i] -= 2
            of[i - 1] += 1
            of[j + 1] += 2
            of[j] -= 1
    ascending = [l for l in range(1, limit + 1) for _ in range(of[l])]
    lengths = [0] * n
    for l, s in zip(ascending, sorted((s for s in range(n) if depth[s]), key=lambda s: (depth[s], s))):
        lengths[s] = l
    return np.array(lengths, np.int64), np.array(depth, np.int64)


def canonical_codes(lengths):
    """deflate's canonical codes by (length, symbol), bit-reversed"""
    codes, code = np.zeros(len(lengths), np.int64), 0
    for bits in range(1, 16):
        for s in np.flatnonzero(np.asarray(lengths) == bits):
            codes[s] = int(format(code, f"0{bits}b")[::-1], 2)
            code += 1
        code <<= 1
    return codes


def header_sequence(lengths):
    """the HLIT + 258 lengths as one sequence, run-coded: (HLIT, [(code-length symbol, extra bits, extra value)], [(value, run length)])"""
    used = np.flatnonzero(lengths)
    n_lit = max(257, int(used.max()) + 1)
    seq = list(lengths[:n_lit]) + [1]
    sent, runs = [], []
    for value, group in itertools.groupby(seq):
        r = len(list(group))
        runs.append((int(value), r))
        if value == 0:
            while r >= 11:
                c = min(r, 138)
                sent.append((18, 7, c - 11))
                r -= c
            if r >= 3:
                sent.append((17, 3, r - 3))
            else:
                sent += [(0, 0, 0)] * r
        else:
            sent.append((int(value), 0, 0))
            rest = r - 1
            while rest >= 3:
                c = min(rest, 6)
                sent.append((16, 2, c - 3))
                rest -= c
            sent += [(int(value), 0, 0)] * rest
    return n_lit - 257, sent, runs


def own_header(lengths):
    """the own header's bits in stream order (BFINAL 0), and what it is made of: (bits, runs of the sequence, the code-length code's depths before the adjustment)"""
    hlit, sent, runs = header_sequence(lengths)
    cl_counts = np.bincount([s for s, _, _ in sent], minlength=19)
    cl_len, cl_depth = optimal_lengths(cl_counts, 7)
    cl_code = canonical_codes(cl_len)
    n_cl = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_len[s]))
    fields = [(0, 1), (2, 2), (hlit, 5), (0, 5), (n_cl - 4, 4)] + [(int(cl_len[s]), 3) for s in CL_ORDER[:n_cl]]
    for s, eb, ex in sent:
        fields.append((int(cl_code[s]), int(cl_len[s])))
        if eb:
            fields.append((ex, eb))
    bits = [(v >> i) & 1 for v, w in fields for i in range(w)]
    return np.array(bits, np.int64), runs, cl_depth


def segment_plan(tokens):
    """a segment's nine candidates from its tokens: a dict with counts, the own lengths, depths, header, the nine costs and the choice (the first of equals)"""
    sym, eb, _ = tokens
    counts = np.bincount(sym, minlength=286)
    counts[256] = 1
    lengths, depth = optimal_lengths(counts, 15)
    header, runs, cl_depth = own_header(lengths)
    beside = int((eb[sym > 256] + 1).sum())                 # the matches' extra bits and distance codes
    costs = [int(h.size + (counts * l).sum() + beside) for l, _, h in R.tables()] + [int(header.size + (counts * lengths).sum() + beside)]
    return dict(counts=counts, lengths=lengths, depth=depth, header=header, runs=runs, cl_depth=cl_depth, costs=costs, choice=int(np.argmin(costs)))


def deflate_bits(tokens, plans):
    values, widths = [], []
    for s, (plan, (sym, eb, ex)) in enumerate(zip(plans, tokens)):
        if plan["choice"] == OWN:
            lengths, codes, header = plan["lengths"], canonical_codes(plan["lengths"]), plan["header"]
        else:
            lengths, codes, header = R.tables()[plan["choice"]]
        head = header.copy()
        head[0] = 1 if s == len(plans) - 1 else 0
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
    tokens = R.stream_tokens(stream)
    plans = [segment_plan(t) for t in tokens]
    idat = b"\x78\x01" + deflate_bits(tokens, plans) + struct.pack(">I", zlib.adler32(stream.tobytes()))
    file = P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + P.chunk(b"IDAT", idat) + P.chunk(b"IEND", b"")
    frame = np.frombuffer(struct.pack("<I", 4 + len(file)) + file, np.uint8)
    return frame, stream, types, tokens, plans


def restated(name):
    """of a case of the set: (the frame as uint8, the filtered stream, the filter types, the segments' tokens, the segments' plans); computed once"""
    return _restated(name)


# ---- the content set ----------------------------------------------------------------------------------------------------------------------------------------------
def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _spread(counts):
    """the symbols of `counts` (value -> count) in an order in which no two neighbours are equal: the most frequent of the others, every time"""
    left, out = dict(counts), []
    while any(left.values()):
        v = max((v for v in left if left[v] and (not out or v != out[-1])), key=lambda v: (left[v], -v))
        out.append(v)
        left[v] -= 1
    return out


def _stream_case(counts):
    """a one-row frame (png_runs_util.from_residuals) whose filtered stream holds literal v exactly counts[v] times and no run to speak of: the row's type byte 1
    and its first pixel 100, 90, 80 are among them, the rest is _spread's order"""
    counts = dict(counts)
    for v in (1, 100, 90, 80):
        assert counts.get(v, 0) >= 1
        counts[v] -= 1
    body = _spread(counts)
    n = 4 + len(body)
    bgr, stream = R.from_residuals(n, [(4 + i, 1, v) for i, v in enumerate(body)])
    return bgr, stream


def _fibonacci_counts(n_literals):
    """eob's 1 is the first of the series: literals 100, 90, 80, 1, 2, 3, ... count 1, 2, 3, 5, 8, ...; the largest takes what makes the stream 1 + 3 k bytes"""
    values = [100, 90, 80, 1] + list(range(2, n_literals - 2))
    counts = dict(zip(values, fibonacci(n_literals + 1)[1:]))
    counts[values[-1]] += (1 - sum(counts.values())) % 3
    return counts


# literal values in use, chosen for the zero-runs between them in the header's sequence; every one twice, so the lengths are equal where the symbols are 2^k
GAPS_SMALL = [1, 2, 3, 6, 7, 8, 9, 13, 14, 15, 16, 17, 18, 19, 30, 31, 32, 33, 34, 35, 36, 37] + list(range(49, 88)) + [90, 100]      # 63, and end-of-block
GAPS_LARGE = {"zero-run of 138": 239, "zero-run of 139": 240, "zero-run of 149": 250}


@functools.lru_cache(maxsize=None)
def _built():
    """name -> (bgr, the stream it is built to have)"""
    b = {}
    b["depth 16"] = _stream_case(_fibonacci_counts(16))
    b["depth 17"] = _stream_case(_fibonacci_counts(17))
    values = [1, 100, 90, 80] + list(range(2, 32)) + list(range(226, 256))
    b["every count equal"] = _stream_case({v: 1 for v in values})       # 64 bytes, all different; end-of-block counts 1 as well
    counts = {v: 2 for v in GAPS_SMALL}
    counts[100] += (1 - sum(counts.values())) % 3
    b["zero-runs of 2 3 10 11"] = _stream_case(counts)
    for name, far in GAPS_LARGE.items():
        counts = {1: 300, far: 250, 100: 50, 90: 50, 80: 50}
        counts[1] += (1 - sum(counts.values())) % 3
        b[name] = _stream_case(counts)
    return b


@functools.lru_cache(maxsize=None)
def cases():
    c = dict(R.cases())
    for name, (bgr, _) in _built().items():
        c[name] = bgr
    frame = np.random.default_rng(21).integers(0, 256, (8, 341, 3), dtype=np.uint8)      # one segment: 8 rows of 1024 bytes
    for y in range(8):
        frame[y, :20 + 37 * y] = 0                          # black margins of eight widths: matches of several lengths beside every literal
    c["341x8 noise with margins"] = frame
    c["40x137 uniform noise"] = np.random.default_rng(NOISE_SEED).integers(0, 256, (137, 40, 3), dtype=np.uint8)      # n = 16577: two segments and 193 bytes
    for v in c.values():
        v.setflags(write=False)
    return c


NOISE_SEED = 3
PADDED = R.PADDED


def _run_lengths(runs, zero):
    return [r for v, r in runs if (v == 0) == zero]


def check_case(name):
    """asserts, from the restatement, that the case reaches what it is built for; returns the segments' choices"""
    _, stream, types, tokens, plans = restated(name)
    choice = [p["choice"] for p in plans]
    for p in plans:
        assert all(p["costs"][OWN] < c for c in p["costs"][:OWN]) == (p["choice"] == OWN)
        assert p["lengths"].max() <= 15 and sum(1 << (15 - int(l)) for l in p["lengths"] if l) == 1 << 15 and p["header"].size <= 2083
    if name in _built():
        assert types.tolist() == [1] and (stream == _built()[name][1]).all(), f"{name}: the stream is not the one it was built to be"
        assert all((sym < 256).all() for sym, _, _ in tokens), f"{name}: built to have no run with a tail of {R.RUN_MIN}"
        assert choice == [OWN], f"{name}: the own header is not in the frame"
    if name in R.cases():
        R.check_case(name)
    if name in ("depth 16", "depth 17"):
        d = int(name.split()[1])
        assert plans[0]["depth"].max() == d and np.count_nonzero(plans[0]["counts"]) == d + 1 and plans[0]["lengths"].max() == 15
    elif name == "every count equal":
        assert set(plans[0]["counts"].tolist()) == {0, 1} and np.count_nonzero(plans[0]["counts"]) == 65
    elif name == "zero-runs of 2 3 10 11":
        zeros, others = _run_lengths(plans[0]["runs"], True), _run_lengths(plans[0]["runs"], False)
        assert {2, 3, 10, 11} <= set(zeros) and {3, 4, 7, 8} <= set(others), (zeros, others)
    elif name in GAPS_LARGE:
        assert int(name.split()[-1]) in _run_lengths(plans[0]["runs"], True)
    elif name == "341x16 flat":
        assert set(stream[SEGMENT:].tolist()) == {0, 2}     # the second segment: two byte values
    elif name == "segment cuts":
        assert tokens[3][0].size == 1 and np.count_nonzero(plans[3]["counts"]) == 2 and plans[3]["lengths"].max() == 1      # a last segment of one byte
    elif name == "341x8 noise with margins":
        sym = tokens[0][0]
        assert len(tokens) == 1 and set(range(256)) <= set(sym.tolist()) and len(set(sym[sym > 256].tolist())) >= 4 and choice == [OWN]
    elif name == "40x137 uniform noise":
        assert stream.size == 2 * SEGMENT + 193 and choice[:2] == [OWN, OWN] and choice[2] < OWN      # a fixed table wins the short tail
    elif name == "341x24 black":
        assert all(p["costs"][p["choice"]] < 256 for p in plans)      # tiny blocks: they share words
    return choice


# ---- the count families of the length rule: name -> (counts, the limits they are built at: 15, and 7 wherever 7 bits hold the symbols in use) ---------------------
@functools.lru_cache(maxsize=None)
def count_families():
    f = {}
    f["fibonacci 17: depth 16"] = fibonacci(17)
    f["fibonacci 18: depth 17"] = fibonacci(18)
    f["fibonacci 9 from 1, 2: deeper than 7"] = [1, 2, 3, 5, 8, 13, 21, 34, 55]
    f["fibonacci 40: depth 39"] = fibonacci(40)
    f["286 equal counts"] = [7] * 286
    f["128 equal counts"] = [1] * 128
    f["100 equal counts"] = [3] * 100
    f["two symbols"] = [0, 4, 0, 9]
    f["one symbol"] = [0, 0, 5]
    f["one count alone"] = [1]
    f["a ramp of 286"] = list(range(1, 287))
    f["128 symbols, 40 of them Fibonacci"] = fibonacci(40) + [3] * 88          # as many as 7 bits hold, under a tree of depth 39 and more
    f["powers of two"] = [1 << k for k in range(20)]
    f["a sum just under 2^32"] = [(1 << 32) - 1 - 18] + [1] * 18
    rng = np.random.default_rng(4)
    f["random, sparse"] = (rng.integers(0, 50, 286) * (rng.random(286) < 0.3)).tolist()
    f["random, 19 symbols"] = rng.integers(0, 300, 19).tolist()
    for name in ("341x8 noise with margins", "depth 16", "every count equal", "341x16 flat"):
        for s, p in enumerate(restated(name)[4]):
            f[f"{name}, segment {s}"] = p["counts"].tolist()
    return {name: (counts, (7, 15) if np.count_nonzero(counts) <= 128 else (15,)) for name, counts in f.items()}
