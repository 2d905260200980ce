"""Shared by the CPU and GPU tests of the JPEG hand-off on per-frame Huffman tables (include/poppy_hip.h: POPPY_FRAME_JPEG_OPT, POPPY_FRAME_JPEG444_OPT): a
plain-Python restatement of the table rule written from the header's text (lists and loops, nothing of the C++), the symbol counts of a frame, the OPT header
and the whole frame, on the quantised MCUs and the fixed header of tests/jpeg_util.py and tests/jpeg444_util.py; the count families that pin the rule; and the
frames both suites code."""
import struct

import numpy as np

import jpeg444_util as U4
import jpeg_util as U

OFF_DHT = 2 + 18 + 134 + 19                                     # in the JFIF file: SOI, APP0, DQT, SOF0
STD_DHT_BYTES = 420                                             # the fixed header's DHT segment with its marker
SEGMENT_BYTES = 2 * ((6 * 1661 * 8 + 7) // 8) + 2               # the header's bound: a block is at most 12 + 11 + 63 * 26 bits
LEAST = 4 + 197 + 4 * 18 + 1 + 2


# ---- the table rule --------------------------------------------------------------------------------------------------------------------------------------
def optimal_lengths(counts):
    """steps 1 and 2: the code length of every entry 0..256 before limiting (0: no count)"""
    freq = [int(c) for c in counts] + [1]
    assert len(freq) == 257
    tree = [[i] for i in range(257)]                            # the symbols of the tree whose count entry i holds
    length = [0] * 257
    while True:
        c1 = None
        for i in range(257):
            if freq[i] and (c1 is None or freq[i] <= freq[c1]):
                c1 = i                                          # the smallest non-zero count, the largest index among equals
        c2 = None
        for i in range(257):
            if freq[i] and i != c1 and (c2 is None or freq[i] <= freq[c2]):
                c2 = i
        if c2 is None:
            return length
        freq[c1] += freq[c2]
        freq[c2] = 0
        for s in tree[c1] + tree[c2]:
            length[s] += 1
        tree[c1] += tree[c2]
        tree[c2] = []


def optimal_table(counts, info=None):
    """(bits[16], vals) of 256 counts by the header's six steps; info (a dict) receives the unlimited depth and whether step 4 changed anything"""
    length = optimal_lengths(counts)
    n = [0] * 258
    for s in range(257):
        if length[s]:
            n[length[s]] += 1
    if info is not None:
        info["depth"] = max(length)
        info["limited"] = max(length) > 16
    for i in range(256, 16, -1):
        while n[i] > 0:
            j = i - 2
            while n[j] == 0:
                j -= 1
            n[i] -= 2
            n[i - 1] += 1
            n[j + 1] += 2
            n[j] -= 1
    i = 16
    while n[i] == 0:
        i -= 1
    n[i] -= 1
    vals = [s for l in range(1, 257) for s in range(256) if length[s] == l]
    return n[1:17], vals


def kraft_ok(bits):
    """no length above 16 (bits has 16 entries), and with the reserved all-ones code left free the codes' Kraft sum stays below 2^16"""
    return len(bits) == 16 and sum(b << (16 - l) for l, b in enumerate(bits, 1)) < 1 << 16


# ---- the count families -------------------------------------------------------------------------------------------------------------------------------------
def fibonacci_counts():
    c = [1, 2]
    while len(c) < 42:
        c.append(c[-1] + c[-2] + 1)
    return c + [0] * (256 - 42)


def count_families():
    rng = np.random.default_rng(11)
    pairs = [0] * 256
    for i in range(0, 60, 2):
        pairs[i] = pairs[i + 1] = 5 + i // 2
    scattered = [0] * 256
    for i in (0, 1, 2, 3, 4, 0x11, 0x12, 0x21, 0xF0, 0xFA, 0xFF):
        scattered[i] = 7
    return {
        "one": [0] * 5 + [9] + [0] * 250,
        "two": [3] + [0] * 254 + [3],
        "all_equal": [1] * 256,
        "all_equal_large": [16000000] * 256,
        "pairs": pairs,
        "dc12": [900, 4000, 3000, 2500, 1200, 700, 300, 90, 30, 7, 2, 1] + [0] * 244,
        "fibonacci": fibonacci_counts(),
        "fibonacci_reversed": fibonacci_counts()[41::-1] + [0] * 214,
        "scattered_ties": scattered,
        "random_small": [int(x) for x in rng.integers(0, 4, 256)],
        "random_wide": [int(x) for x in rng.integers(0, 1 << 20, 256) * (rng.integers(0, 3, 256) > 0)],
        "steep": [1 << min(i, 23) for i in range(162)] + [0] * 94,
    }


# ---- a frame ------------------------------------------------------------------------------------------------------------------------------------------------
def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, cat):
    return (v - 1 if v < 0 else v) & ((1 << cat) - 1)


def segment_symbols(coefs):
    """the symbols of a segment's MCUs (n x blocks x 64, zig-zag; 6 blocks: 4:2:0, 3: 4:4:4) in coding order: (class 0 DC / 1 AC, table, symbol, value, category)"""
    blocks = coefs.shape[1]
    luma = blocks - 2
    pred = [0, 0, 0]
    out = []
    for mcu in coefs:
        for b in range(blocks):
            comp, t = (0, 0) if b < luma else (b - luma + 1, 1)
            zz = [int(x) for x in mcu[b]]
            diff = zz[0] - pred[comp]
            pred[comp] = zz[0]
            out.append((0, t, _category(diff), diff, _category(diff)))
            run = 0
            for k in range(1, 64):
                if zz[k] == 0:
                    run += 1
                    continue
                while run >= 16:
                    out.append((1, t, 0xF0, 0, 0))
                    run -= 16
                cat = _category(zz[k])
                out.append((1, t, run * 16 + cat, zz[k], cat))
                run = 0
            if run:
                out.append((1, t, 0, 0, 0))
    return out


def code_symbols(symbols, codes, stats=None):
    """a segment's symbols on codes[(class, table)] = {symbol: (code, length)} -> its bytes behind padding and stuffing"""
    acc, n = 0, 0
    for cls, t, sym, v, cat in symbols:
        code, length = codes[(cls, t)][sym]
        acc = (acc << length | code) << cat | _value_bits(v, cat)
        n += length + cat
    pad = -n % 8
    acc = acc << pad | ((1 << pad) - 1)
    raw = acc.to_bytes((n + pad) // 8, "big")
    if stats is not None:
        stats["stuffed"] = stats.get("stuffed", 0) + raw.count(b"\xff")
        stats["zrl"] = stats.get("zrl", 0) + sum(1 for s in symbols if s[0] == 1 and s[2] == 0xF0)
    return raw.replace(b"\xff", b"\xff\x00")


def frame_counts(segments):
    """{(class, id): 256 counts}, in the DHT's order DC 0, AC 0, DC 1, AC 1"""
    counts = {(0, 0): [0] * 256, (1, 0): [0] * 256, (0, 1): [0] * 256, (1, 1): [0] * 256}
    for seg in segments:
        for cls, t, sym, _, _ in seg:
            counts[(cls, t)][sym] += 1
    return counts


def opt_header(fixed, tables):
    """the fixed header (jpeg_util.header / jpeg444_util.header) with its DHT segment replaced by one that holds `tables` = {(class, id): (bits, vals)}"""
    assert fixed[OFF_DHT:OFF_DHT + 2] == b"\xff\xc4" and fixed[OFF_DHT + STD_DHT_BYTES:OFF_DHT + STD_DHT_BYTES + 2] == b"\xff\xdd"
    dht = bytearray()
    for key in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = tables[key]
        dht += bytes([key[0] << 4 | key[1]]) + bytes(bits) + bytes(vals)
    out = fixed[:OFF_DHT] + b"\xff\xc4" + struct.pack(">H", 2 + len(dht)) + bytes(dht) + fixed[OFF_DHT + STD_DHT_BYTES:]
    assert len(out) == 197 + sum(17 + len(v) for _, v in tables.values())
    return out


def jpeg_opt_frame_reference(planes, w, h, quality, sampling=420, stats=None):
    """The POPPY_FRAME_JPEG_OPT (sampling 444: POPPY_FRAME_JPEG444_OPT) frame of flat planes, as bytes.  stats (a dict) receives what the frame reached: `limited`
    per table (step 4 ran), `one_symbol` (a table with a single symbol), `zrl`, `stuffed`, the tables."""
    if sampling == 444:
        q, restart, fixed = U4.quantised_mcus(planes, w, h, quality), 16, U4.header(w, h, quality, 16)
    else:
        q, restart, fixed = U.quantised_mcus(planes, w, h, quality), 8, U.header(w, h, quality, 8)
    n_seg = -(-len(q) // restart)
    segments = [segment_symbols(q[k * restart:(k + 1) * restart]) for k in range(n_seg)]
    tables, codes = {}, {}
    for key, counts in frame_counts(segments).items():
        info = {}
        tables[key] = optimal_table(counts, info)
        codes[key] = U.huffman_codes(*tables[key])
        if stats is not None:
            stats.setdefault("limited", {})[key] = info["limited"]
            stats.setdefault("depth", {})[key] = info["depth"]
            stats["one_symbol"] = stats.get("one_symbol", False) or len(tables[key][1]) == 1
            stats.setdefault("counts", {})[key] = counts
    out = bytearray(opt_header(fixed, tables))
    for k, seg in enumerate(segments):
        out += code_symbols(seg, codes, stats)
        out += bytes([0xFF, 0xD0 + k % 8]) if k + 1 < n_seg else b"\xff\xd9"
    return (len(out) + 4).to_bytes(4, "little") + bytes(out)


def capacity(w, h, sampling=420):
    """the header's formula"""
    side, restart = (8, 16) if sampling == 444 else (16, 8)
    n_mcu = -(-w // side) * -(-h // side)
    return 4 + 613 + -(-n_mcu // restart) * SEGMENT_BYTES


def noise_i420(w=640, h=360, seed=5):
    """uniform noise in all three planes: the frame whose luma AC table passes 16 bits before limiting"""
    return np.random.default_rng(seed).integers(0, 256, w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2), dtype=np.uint8)
