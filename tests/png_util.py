"""What the PNG hand-off tests share: the content set, a numpy restatement of the POPPY_FRAME_PNG rule (include/poppy_hip.h) from the tables that poppy_png_table
hands out, and a walk over a frame's chunks.  The restatement is whole arrays where the library is loops: filters from shifted copies of the row matrix, the table
choice from per-segment sums of looked-up lengths, the bit string from one repeat / shift / packbits over every symbol of the frame."""
import functools
import struct
import zlib

import numpy as np

from poppy_amd import capi, synth

SEGMENT = capi.PNG_SEGMENT_BYTES
SIGNATURE = bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])


# ---- the content set: the smallest shapes at which each thing can go wrong (name -> HxWx3 BGR) ------------------------------------------------------------------
def _noise(w, h, seed, lo=0, hi=255):
    return np.random.default_rng(seed).integers(lo, hi + 1, (h, w, 3), dtype=np.uint8)


def _gradient(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(3 * x + y) % 256, (x + 5 * y) % 256, (2 * x + 2 * y + (x * y) // 7) % 256], -1).astype(np.uint8)


def band_frame(w=341, rows=16, amplitudes=(0, 1, 2, 4, 8, 16, 40, 128)):
    """`rows`-row bands of 128 +- A noise, one under the other"""
    return np.concatenate([_noise(w, rows, 900 + a, max(0, 128 - a), min(255, 128 + a)) for a in amplitudes], 0)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["1x1"] = _noise(1, 1, 1)
    c["1x5 no left neighbour"] = _noise(1, 5, 2)
    c["5x1 no row above"] = _noise(5, 1, 3)
    for w in (63, 64, 65):
        c[f"{w}x3 gradient"] = _gradient(w, 3)
    c["682x4 just under a segment"] = synth.textured_bgr(682, 4, 5)
    c["683x4 just over a segment"] = synth.textured_bgr(683, 4, 6)
    c["341x8 one segment"] = _gradient(341, 8)
    c["341x128 whole segments"] = synth.textured_bgr(341, 128, 7)      # rows of 1024 bytes: every segment cut falls on a row's first byte
    c["21x130 stub segment"] = _noise(21, 130, 14, 88, 168)            # rows of 64 bytes, n = 8320: the last segment has 128 bytes
    c["333x97 cuts mid-row"] = synth.textured_bgr(333, 97, 8)
    c["341x16 flat"] = np.full((16, 341, 3), 77, np.uint8)
    c["341x24 uniform noise"] = _noise(341, 24, 9)
    c["256x6 every residual"] = _noise(256, 6, 10)
    c["341x128 bands"] = band_frame()
    c["40x137 A=20"] = _noise(40, 137, 11, 108, 148)
    c["40x137 A=64"] = _noise(40, 137, 12, 64, 192)
    c["90x40 columns"] = np.ascontiguousarray(np.broadcast_to(_noise(90, 1, 13), (40, 90, 3)))      # every row the row above: Up
    for v in c.values():
        v.setflags(write=False)
    return c


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables():
    """per table: lengths (257), canonical codes bit-reversed (257), the header's bits"""
    out = []
    for k in range(capi.PNG_TABLES):
        lengths, header = capi.png_table(k)
        lengths = lengths.astype(np.int64)
        codes, code = np.zeros(257, np.int64), 0
        for bits in range(1, 16):
            for s in np.flatnonzero(lengths == bits):
                codes[s] = int(format(code, f"0{bits}b")[::-1], 2)
                code += 1
            code <<= 1
        out.append((lengths, codes, header.astype(np.int64)))
    return out


def filtered_stream(bgr):
    """(the filtered stream as uint8, the rows' filter types)"""
    h, w = bgr.shape[:2]
    cur = bgr[:, :, ::-1].reshape(h, 3 * w).astype(np.int64)
    a = np.zeros_like(cur); a[:, 3:] = cur[:, :-3]
    b = np.zeros_like(cur); b[1:] = cur[:-1]
    c = np.zeros_like(cur); c[1:, 3:] = cur[:-1, :-3]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    candidates = np.stack([cur, cur - a, cur - b, cur - (a + b) // 2, cur - paeth]) % 256        # (5, h, 3w)
    types = np.minimum(candidates, 256 - candidates).sum(2).argmin(0)                            # argmin: the first of equals
    rows = candidates[types, np.arange(h)]
    return np.concatenate([types[:, None], rows], 1).astype(np.uint8).ravel(), types


def table_choice(stream):
    """per segment the table that codes it in the fewest bits, the first of equals"""
    T = tables()
    choice = []
    for first in range(0, stream.size, SEGMENT):
        seg = stream[first:first + SEGMENT]
        choice.append(int(np.argmin([header.size + lengths[seg].sum() + lengths[256] for lengths, _, header in T])))
    return choice


def deflate_bits(stream, choice):
    """the deflate bit string of the stream on the segments' tables, as bytes (zero bits up to the boundary)"""
    T = tables()
    values, widths = [], []
    n_seg = len(choice)
    for s, k in enumerate(choice):
        lengths, codes, header = T[k]
        seg = stream[s * SEGMENT:(s + 1) * SEGMENT].astype(np.int64)
        head = header.copy()
        head[0] = 1 if s == n_seg - 1 else 0
        values += [head, codes[seg], codes[256:257]]
        widths += [np.ones(head.size, np.int64), lengths[seg], lengths[256:257]]
    values, widths = np.concatenate(values), np.concatenate(widths)
    starts = np.cumsum(widths) - widths
    symbol = np.repeat(np.arange(values.size), widths)
    bits = (values[symbol] >> (np.arange(symbol.size) - starts[symbol])) & 1
    return np.packbits(bits.astype(np.uint8), bitorder="little").tobytes()


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def restated_frame(bgr):
    """(the frame as uint8, the filter types, the tables chosen)"""
    h, w = bgr.shape[:2]
    stream, types = filtered_stream(bgr)
    choice = table_choice(stream)
    idat = b"\x78\x01" + deflate_bits(stream, choice) + struct.pack(">I", zlib.adler32(stream.tobytes()))
    file = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")
    frame = struct.pack("<I", 4 + len(file)) + file
    return np.frombuffer(frame, np.uint8), types, choice


# ---- a frame's chunks ---------------------------------------------------------------------------------------------------------------------------------------------
def walk_frame(frame):
    """[(type, data)] of the PNG file in a frame, every length, CRC and the frame's `total` checked"""
    f = np.asarray(frame, np.uint8).tobytes()
    total = struct.unpack("<I", f[:4])[0]
    assert total == len(f), f"total says {total}, the frame has {len(f)} bytes"
    assert f[4:12] == SIGNATURE
    at, out = 12, []
    while at < total:
        n, kind = struct.unpack(">I", f[at:at + 4])[0], f[at + 4:at + 8]
        data = f[at + 8:at + 8 + n]
        assert len(data) == n and struct.unpack(">I", f[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data), f"chunk {kind} at {at}"
        out.append((kind, data))
        at += 12 + n
    assert at == total
    return out


def equal(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.ndim == 1 and got.size == want.size, f"{what}: {got.size} bytes, expected {want.size}"
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{what}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"
