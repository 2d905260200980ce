"""Shared by the CPU and GPU tests of the 4:4:4 JPEG hand-off format (include/poppy_hip.h: POPPY_FRAME_JPEG444): a numpy restatement of the rule written from
the header's text (I444 planes -> 8 x 8 MCUs of three blocks -> segments of 16 MCUs -> file), on the constants, the transform, the quantiser, the Huffman
tables and the walkers of tests/jpeg_util.py — the parts of POPPY_FRAME_JPEG's rule that the header takes over unchanged —, and the content both suites code."""
import numpy as np

import jpeg_util as U
from jpeg_util import HUFF_AC, HUFF_DC, ZIGZAG, fdct, quant_tables, quantise, walk_frame, walk_riff  # noqa: F401  (the walkers: for the tests)

LAYERS = [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]              # Pillow's (id, h, v, table) of a 4:4:4 file
SAMPLING = [(1, 0x11, 0), (2, 0x11, 1), (3, 0x11, 1)]           # walk_frame's
OFF_SOF_SAMPLING = 2 + 18 + 134 + 11                            # in the JFIF file: SOI, APP0, DQT, then SOF0's FF C0, length, precision, height, width, count, id
OFF_DRI_LOW = 2 + 18 + 134 + 19 + 420 + 5


class Stats(U.Stats):
    """the branches reached, and the longest segment behind stuffing (against the scratch slot)"""
    longest = 0


def restart_mcus444():
    """R, read back from the library's capacity: frame_bytes(FRAME_JPEG444) steps when a one-MCU-high frame gains a segment (an MCU is 8 pixels wide)."""
    from poppy_amd import capi
    for r in range(1, 65):
        if capi.frame_bytes(capi.FRAME_JPEG444, 8 * r, 1) < capi.frame_bytes(capi.FRAME_JPEG444, 8 * r + 1, 1):
            return r
    raise AssertionError("POPPY_JPEG444_RESTART_MCUS is above 64")


def i444_of(bgr):
    """The three formulas of the header in numpy int64 (>> on a negative int64 is arithmetic): the flat planes Y, U, V."""
    a = np.asarray(bgr, np.uint8).astype(np.int64)
    B, G, R = a[..., 0], a[..., 1], a[..., 2]
    y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    u = ((-11059 * R - 21709 * G + 32768 * B + 32768) >> 16) + 128
    v = ((32768 * R - 27439 * G - 5329 * B + 32768) >> 16) + 128
    return np.concatenate([np.clip(p, 0, 255).astype(np.uint8).ravel() for p in (y, u, v)])


def planes_of(i444, w, h):
    return np.asarray(i444, np.uint8).reshape(3, h, w)


def mcu_blocks(i444, w, h):
    """n_mcu x 3 x 8 x 8 samples, Y, Cb, Cr, MCUs in raster order; a sample outside the plane is the nearest inside (edge padding per axis)"""
    mw, mh = (w + 7) // 8, (h + 7) // 8
    out = np.zeros((mh, mw, 3, 8, 8), np.uint8)
    for k, p in enumerate(planes_of(i444, w, h)):
        out[:, :, k] = np.pad(p, ((0, 8 * mh - h), (0, 8 * mw - w)), mode="edge").reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3)
    return out.reshape(mh * mw, 3, 8, 8)


def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, cat):
    return (v - 1 if v < 0 else v) & ((1 << cat) - 1)


def code_segment(coefs, stats=None):
    """the MCUs' quantised coefficients (n x 3 x 64 in zig-zag order) -> the segment's bytes behind padding and stuffing.  Component k's block is block k: table 0
    for Y, table 1 for Cb and Cr, one DC predictor each, 0 at the segment's start."""
    acc, n = 0, 0
    pred = [0, 0, 0]
    for mcu in coefs:
        for comp in range(3):
            t = 0 if comp == 0 else 1
            zz = [int(x) for x in mcu[comp]]
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
        stats.longest = max(stats.longest, len(raw) + raw.count(b"\xff"))
    return raw.replace(b"\xff", b"\xff\x00")


def header(w, h, quality, restart):
    """JPEG's header for the same size and quality, except in two bytes: component 1's sampling byte is 0x11, DRI names this format's interval"""
    out = bytearray(U.header(w, h, quality, restart))
    assert out[OFF_SOF_SAMPLING - 11:OFF_SOF_SAMPLING - 9] == b"\xff\xc0" and out[OFF_SOF_SAMPLING] == 0x22
    assert out[OFF_DRI_LOW - 5:OFF_DRI_LOW - 3] == b"\xff\xdd" and out[OFF_DRI_LOW] == restart
    out[OFF_SOF_SAMPLING] = 0x11
    return bytes(out)


def quantised_mcus(i444, w, h, quality):
    """n_mcu x 3 x 64, zig-zag order"""
    blocks = mcu_blocks(i444, w, h)
    ql, qc = quant_tables(quality)
    F = fdct(blocks.reshape(-1, 8, 8)).reshape(-1, 3, 8, 8)
    q = np.concatenate([quantise(F[:, :1], ql), quantise(F[:, 1:], qc)], axis=1)
    return q.reshape(-1, 3, 64)[:, :, ZIGZAG]


def jpeg444_frame_reference(i444, w, h, quality, restart, stats=None):
    """The POPPY_FRAME_JPEG444 frame of flat I444 planes with restart intervals of `restart` MCUs, as bytes."""
    q = quantised_mcus(i444, w, h, quality)
    out = bytearray(header(w, h, quality, restart))
    n_seg = -(-len(q) // restart)
    for k in range(n_seg):
        out += code_segment(q[k * restart:(k + 1) * restart], stats)
        out += bytes([0xFF, 0xD0 + k % 8]) if k + 1 < n_seg else b"\xff\xd9"
    return (len(out) + 4).to_bytes(4, "little") + bytes(out)


def capacity(w, h, restart=16):
    """the header's formula"""
    n_mcu = ((w + 7) // 8) * ((h + 7) // 8)
    return 617 + -(-n_mcu // restart) * (2 * ((6 * 1660 * 8 + 7) // 8) + 2)


# ---- content ---------------------------------------------------------------------------------------------------------------------------------------------
CONTENTS = U.CONTENTS
SIZES = ((1, 1), (2, 2), (8, 8), (9, 9), (7, 17), (40, 40), (128, 8), (129, 8), (160, 128))
QUALITIES = (100, 90, 10)


def i444_content(name, w, h, seed=0):
    """flat I444 planes, jpeg_util's content written into three full-size planes directly (mcu_alternation: 8-pixel squares in every plane, an MCU each)"""
    def plane(kind):
        yy, xx = np.mgrid[0:h, 0:w]
        if name == "noise":
            return np.random.default_rng(7000 + seed + kind + 3 * w + h).integers(0, 256, (h, w), dtype=np.uint8)
        if name.startswith("flat"):
            return np.full((h, w), int(name[4:]), np.uint8)
        if name == "checker":
            return (((xx + yy) & 1) * 255).astype(np.uint8)
        if name == "stripes4":
            return (np.isin(xx % 8, (0, 3, 4, 7)) * 255).astype(np.uint8)
        if name == "mcu_alternation":
            return ((((xx // 8) + (yy // 8)) & 1) * 255).astype(np.uint8)
        if name == "gradient":
            return ((xx * 3 + yy * 2 + 40 * kind) % 256 // 2 + 40).astype(np.uint8)
        raise KeyError(name)
    return np.concatenate([plane(k).ravel() for k in range(3)])
