"""Shared by the CPU and GPU tests of the JPEG hand-off format (include/poppy_hip.h: POPPY_FRAME_JPEG): a numpy restatement of the rule written from the
header's text and independent of the C++ (planes -> MCUs -> DCT -> quantisation -> Huffman -> segments -> file), a marker walker that takes a frame apart
again, a RIFF walker for the MJPEG sink's AVI, and the content both suites code."""
import struct

import numpy as np

# ---- the rule's constants, typed from ITU-T T.81 Annex K ------------------------------------------------------------------------------------------------
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HEADER_BYTES = 613
K = [8192, 8035, 7568, 6811, 5793, 4551, 3135, 1598]


def restart_mcus():
    """R, read back from the library's capacity: frame_bytes(FRAME_JPEG) steps when a one-MCU-high frame gains a segment."""
    from poppy_amd import capi
    for r in range(1, 65):
        if capi.frame_bytes(capi.FRAME_JPEG, 16 * r, 1) < capi.frame_bytes(capi.FRAME_JPEG, 16 * r + 1, 1):
            return r
    raise AssertionError("POPPY_JPEG_RESTART_MCUS is above 64")


def dct_table():
    """T[u][x] by the header's formula; equal to round(2^14 a(u) cos((2 x + 1) u pi / 16))."""
    t = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            if u == 0:
                t[u, x] = K[4]
                continue
            k = ((2 * x + 1) * u) % 32
            if k > 16:
                k = 32 - k
            t[u, x] = 0 if k == 8 else K[k] if k < 8 else -K[16 - k]
    return t


def quant_tables(quality):
    """(luma, chroma) in natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((base * scale + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA)]


def fdct(blocks):
    """n x 8 x 8 samples (0..255) -> F, 8 times the DCT coefficients, by the two integer passes"""
    s = np.asarray(blocks, np.int64) - 128
    T = dct_table()
    t = (s @ T.T + 1024) >> 11                                  # t[y][u] = sum over x of T[u][x] s[y][x]
    return (T @ t + 8192) >> 14                                 # F[v][u] = sum over y of T[v][y] t[y][u]


def quantise(F, q_natural):
    Q = np.asarray(q_natural, np.int64).reshape(8, 8)
    m = (np.abs(F) + 4 * Q) // (8 * Q)
    return np.where(F < 0, -m, m)


def huffman_codes(bits, vals):
    """symbol -> (code, length)"""
    out, code, at = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[at]] = (code, length)
            at += 1
            code += 1
        code <<= 1
    return out


HUFF_DC = [huffman_codes(DC_BITS[t], DC_VALS) for t in range(2)]
HUFF_AC = [huffman_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def planes_of(i420, w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    a = np.asarray(i420, np.uint8).ravel()
    return a[:w * h].reshape(h, w), a[w * h:w * h + cw * ch].reshape(ch, cw), a[w * h + cw * ch:].reshape(ch, cw)


def mcu_blocks(i420, w, h):
    """n_mcu x 6 x 8 x 8 samples in the rule's order; a sample outside a plane is the nearest inside (edge padding per axis)"""
    mw, mh = (w + 15) // 16, (h + 15) // 16
    y, u, v = planes_of(i420, w, h)
    yp = np.pad(y, ((0, 16 * mh - h), (0, 16 * mw - w)), mode="edge")
    up, vp = (np.pad(p, ((0, 8 * mh - p.shape[0]), (0, 8 * mw - p.shape[1])), mode="edge") for p in (u, v))
    out = np.zeros((mh, mw, 6, 8, 8), np.uint8)
    yb = yp.reshape(mh, 2, 8, mw, 2, 8)                          # [my][j][row][mx][i][col]
    for j in range(2):
        for i in range(2):
            out[:, :, 2 * j + i] = yb[:, j, :, :, i, :].transpose(0, 2, 1, 3)
    out[:, :, 4] = up.reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3)
    out[:, :, 5] = vp.reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3)
    return out.reshape(mh * mw, 6, 8, 8)


class Stats:
    """what the coded content reached (the branch assertions of tests/test_host_jpeg.py)"""
    def __init__(self):
        self.stuffed = self.zrl = self.no_eob = self.eob_only = 0
        self.dc_cats, self.ac_cats, self.pads, self.segments = set(), set(), set(), 0


def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, cat):
    return (v - 1 if v < 0 else v) & ((1 << cat) - 1)


def code_segment(coefs, stats=None):
    """the MCUs' quantised coefficients (n x 6 x 64 in zig-zag order) -> the segment's bytes behind padding and stuffing"""
    acc, n = 0, 0
    pred = [0, 0, 0]
    for mcu in coefs:
        for b in range(6):
            comp, t = (0, 0) if b < 4 else (b - 3, 1)
            zz = [int(x) for x in mcu[b]]
            diff = zz[0] - pred[comp]
            pred[comp] = zz[0]
            cat = _category(diff)
            code, length = HUFF_DC[t][cat]
            acc = (acc << length | code) << cat | _value_bits(diff, cat)
            n += length + cat
            run, symbols = 0, 0
            for k in range(1, 64):
                if zz[k] == 0:
                    run += 1
                    continue
                while run >= 16:
                    code, length = HUFF_AC[t][0xF0]
                    acc = acc << length | code
                    n += length
                    run -= 16
                    if stats:
                        stats.zrl += 1
                cat = _category(zz[k])
                code, length = HUFF_AC[t][run * 16 + cat]
                acc = (acc << length | code) << cat | _value_bits(zz[k], cat)
                n += length + cat
                run = 0
                symbols += 1
                if stats:
                    stats.ac_cats.add(cat)
            if run:
                code, length = HUFF_AC[t][0]
                acc = acc << length | code
                n += length
            if stats:
                stats.dc_cats.add(_category(diff))
                stats.no_eob += run == 0
                stats.eob_only += symbols == 0
    pad = -n % 8
    acc = acc << pad | ((1 << pad) - 1)
    n += pad
    raw = acc.to_bytes(n // 8, "big")
    if stats:
        stats.pads.add(pad)
        stats.stuffed += raw.count(b"\xff")
        stats.segments += 1
    return raw.replace(b"\xff", b"\xff\x00")


def header(w, h, quality, restart):
    ql, qc = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0" + struct.pack(">H", 16) + b"JFIF\x00\x01\x01\x00" + struct.pack(">HH", 1, 1) + b"\x00\x00")
    out += b"\xff\xdb" + struct.pack(">H", 2 + 65 + 65) + b"\x00" + bytes(int(x) for x in ql[ZIGZAG]) + b"\x01" + bytes(int(x) for x in qc[ZIGZAG])
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    dht = bytearray()
    for t in range(2):
        dht += bytes([t]) + bytes(DC_BITS[t]) + bytes(DC_VALS) + bytes([0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t])
    out += b"\xff\xc4" + struct.pack(">H", 2 + len(dht)) + dht
    out += b"\xff\xdd" + struct.pack(">HH", 4, restart)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return bytes(out)


def quantised_mcus(i420, w, h, quality):
    """n_mcu x 6 x 64, zig-zag order"""
    blocks = mcu_blocks(i420, w, h)
    ql, qc = quant_tables(quality)
    F = fdct(blocks.reshape(-1, 8, 8)).reshape(-1, 6, 8, 8)
    q = np.concatenate([quantise(F[:, :4], ql), quantise(F[:, 4:], qc)], axis=1)
    return q.reshape(-1, 6, 64)[:, :, ZIGZAG]


def jpeg_frame_reference(i420, w, h, quality, restart, stats=None):
    """The POPPY_FRAME_JPEG frame of a flat I420 frame with restart intervals of `restart` MCUs, as bytes."""
    q = quantised_mcus(i420, w, h, quality)
    out = bytearray(header(w, h, quality, restart))
    n_seg = -(-len(q) // restart)
    for k in range(n_seg):
        out += code_segment(q[k * restart:(k + 1) * restart], stats)
        out += bytes([0xFF, 0xD0 + k % 8]) if k + 1 < n_seg else b"\xff\xd9"
    return (len(out) + 4).to_bytes(4, "little") + bytes(out)


# ---- taking a frame apart again --------------------------------------------------------------------------------------------------------------------------
def walk_frame(frame):
    """{total, size: (w, h), sampling, qtables: [64 zig-zag entries] per table, dht: {(class, id): (bits, vals)}, restart, segments: [bytes], rst: [n],
    app0, order: the markers in the header}; asserts the layout: `total`, SOI first, EOI last, nothing behind it."""
    f = bytes(np.asarray(frame, np.uint8))
    total = int.from_bytes(f[:4], "little")
    assert total == len(f), (total, len(f))
    j = f[4:]
    assert j[:2] == b"\xff\xd8" and j[-2:] == b"\xff\xd9"
    out = {"total": total, "qtables": {}, "dht": {}, "order": [], "segments": [], "rst": []}
    at = 2
    while True:
        assert j[at] == 0xFF, f"no marker at {at}"
        m, n = j[at + 1], int.from_bytes(j[at + 2:at + 4], "big")
        body = j[at + 4:at + 2 + n]
        out["order"].append(m)
        if m == 0xE0:
            out["app0"] = body
        elif m == 0xDB:
            for p in range(0, len(body), 65):
                assert body[p] >> 4 == 0, "8-bit entries"
                out["qtables"][body[p] & 15] = list(body[p + 1:p + 65])
        elif m == 0xC0:
            prec, hh, ww, nc = struct.unpack(">BHHB", body[:6])
            assert prec == 8 and nc == 3
            out["size"] = (ww, hh)
            out["sampling"] = [(body[6 + 3 * k], body[7 + 3 * k], body[8 + 3 * k]) for k in range(3)]
        elif m == 0xC4:
            p = 0
            while p < len(body):
                bits = list(body[p + 1:p + 17])
                out["dht"][(body[p] >> 4, body[p] & 15)] = (bits, list(body[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif m == 0xDD:
            out["restart"] = int.from_bytes(body, "big")
        elif m == 0xDA:
            out["sos"] = body
            at += 2 + n
            break
        at += 2 + n
    out["data_offset"] = at
    start = at
    while True:
        k = j.index(b"\xff", at)
        nxt = j[k + 1]
        if nxt == 0:
            at = k + 2
            continue
        out["segments"].append(j[start:k])
        if nxt == 0xD9:
            assert k + 2 == len(j), "bytes behind EOI"
            return out
        assert 0xD0 <= nxt <= 0xD7, f"marker {nxt:#x} inside the scan"
        out["rst"].append(nxt - 0xD0)
        at = start = k + 2


def walk_riff(data):
    """The chunks of a RIFF file as a tree: [(fourcc, payload offset, payload length, list type or None, children)]; asserts that lengths nest and pad to even."""
    def chunks(at, end):
        out = []
        while at < end:
            cc, n = data[at:at + 4], int.from_bytes(data[at + 4:at + 8], "little")
            assert at + 8 + n <= end, f"chunk {cc} at {at} runs past its parent"
            if cc in (b"RIFF", b"LIST"):
                out.append((cc, at + 8, n, data[at + 8:at + 12], chunks(at + 12, at + 8 + n)))
            else:
                out.append((cc, at + 8, n, None, []))
            at += 8 + n + (n & 1)
        assert at == end or at == end + 1
        return out
    return chunks(0, len(data))


# ---- content ---------------------------------------------------------------------------------------------------------------------------------------------
CONTENTS = ("noise", "flat0", "flat255", "flat128", "checker", "stripes4", "mcu_alternation", "gradient")
SIZES = ((1, 1), (2, 2), (16, 16), (17, 17), (15, 33), (48, 48), (160, 128))
QUALITIES = (100, 90, 10)


def i420_content(name, w, h, seed=0):
    """a flat I420 frame, the content written into the planes directly (so that flat 0 and flat 255 are what the coder sees)"""
    cw, ch = (w + 1) // 2, (h + 1) // 2

    def plane(pw, ph, kind):
        yy, xx = np.mgrid[0:ph, 0:pw]
        if name == "noise":
            return np.random.default_rng(7000 + seed + kind + 3 * pw + ph).integers(0, 256, (ph, pw), dtype=np.uint8)
        if name.startswith("flat"):
            return np.full((ph, pw), int(name[4:]), np.uint8)
        if name == "checker":                                   # the saturated pixel checkerboard: the block's energy sits in the last coefficients
            return (((xx + yy) & 1) * 255).astype(np.uint8)
        if name == "stripes4":                                  # the sign pattern of cos((2 x + 1) 4 pi / 16): + - - + + - - +, which maximises F(0, 4)
            return (np.isin(xx % 8, (0, 3, 4, 7)) * 255).astype(np.uint8)
        if name == "mcu_alternation":                           # flat 0 beside flat 255, MCU by MCU (a block of the chroma planes): the largest DC differences
            s = 16 if kind == 0 else 8
            return ((((xx // s) + (yy // s)) & 1) * 255).astype(np.uint8)
        if name == "gradient":
            return ((xx * 3 + yy * 2 + 40 * kind) % 256 // 2 + 40).astype(np.uint8)
        raise KeyError(name)
    return np.concatenate([plane(w, h, 0).ravel(), plane(cw, ch, 1).ravel(), plane(cw, ch, 2).ravel()])
