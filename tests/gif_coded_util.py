"""Shared by the CPU and GPU tests of the GIF hand-off format (include/poppy_hip.h: POPPY_FRAME_GIF): a plain-Python restatement of the segment rule, written
from the header's text and independent of the C++, the index planes both suites code, and a reader of a coded frame's layout."""
import numpy as np

CLEAR, END = 256, 257


def segment_pixels():
    """S, read back from the library's capacity: frame_bytes(FRAME_GIF) steps when a frame gains a segment."""
    from poppy_amd import capi
    for s in (1024, 2048, 4096):
        if capi.frame_bytes(capi.FRAME_GIF, s, 1) < capi.frame_bytes(capi.FRAME_GIF, s + 1, 1):
            return s
    raise AssertionError("POPPY_GIF_SEGMENT_PIXELS is none of 1024, 2048, 4096")


class Bits:
    def __init__(self):
        self.acc, self.n, self.out, self.clears = 0, 0, bytearray(), 0

    def put(self, code, width):
        self.clears += code == CLEAR                        # (256 is never a string's code)
        self.acc |= code << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8


def lzw_codes(px, bits):
    """A clear code at 9 bits and the codes of px; returns the width of the code that follows."""
    width, nxt, table = 9, 258, {}
    bits.put(CLEAR, 9)
    prefix = int(px[0])
    for b in px[1:]:
        b = int(b)
        if (prefix, b) in table:
            prefix = table[(prefix, b)]
            continue
        bits.put(prefix, width)
        if nxt == 4096:                                     # the table is full: a clear code, and everything starts again
            bits.put(CLEAR, width)
            width, nxt, table = 9, 258, {}
        else:
            table[(prefix, b)] = nxt
            if nxt == 1 << width:
                width += 1
            nxt += 1
        prefix = b
    bits.put(prefix, width)
    return width


def gif_frame_reference(pal8, w, h, seg):
    """The POPPY_FRAME_GIF frame of a flat PAL8 frame with segments of `seg` pixels, as bytes."""
    n = w * h
    idx = np.asarray(pal8[:n], np.uint8)
    bits = Bits()
    for at in range(0, n, seg):
        assert bits.n == 0, "a segment begins on a byte boundary"
        width = lzw_codes(idx[at:at + seg], bits)
        if at + seg < n:
            bits.put(CLEAR, width)
            pads = 0
            while bits.n:
                bits.put(CLEAR, 9)
                pads += 1
            assert pads <= 7, "at most seven padding clear codes"
        else:
            bits.put(END, width)
            if bits.n:
                bits.put(0, 8 - bits.n)
    assert bits.n == 0
    payload = bytes(bits.out)
    data = bytearray([8])
    for at in range(0, len(payload), 255):
        block = payload[at:at + 255]
        data.append(len(block))
        data += block
    data.append(0)
    total = 4 + 768 + len(data)
    return total.to_bytes(4, "little") + bytes(np.asarray(pal8[n:], np.uint8)) + bytes(data)


def split_frame(frame):
    """(total, palette, payload) of a coded frame; asserts the layout: the minimum code size, sub-blocks of 255 with only the last one shorter and none empty,
    the terminator as the frame's last byte."""
    f = bytes(np.asarray(frame, np.uint8))
    total = int.from_bytes(f[:4], "little")
    assert total == len(f), (total, len(f))
    assert f[772] == 8
    at, payload, sizes = 773, bytearray(), []
    while f[at]:
        sizes.append(f[at])
        payload += f[at + 1:at + 1 + f[at]]
        at += 1 + f[at]
    assert at == total - 1, "the terminator is the last byte"
    assert sizes and all(s == 255 for s in sizes[:-1]) and 1 <= sizes[-1] <= 255
    return total, np.frombuffer(f[4:772], np.uint8), bytes(payload)


CONTENTS = ("zero", "noise", "period2", "ramp")


def index_plane(content, n, seed=0):
    if content == "zero":
        return np.zeros(n, np.uint8)
    if content == "noise":
        return np.random.default_rng(1000 + seed + n).integers(0, 256, n, dtype=np.uint8)
    if content == "period2":
        return np.tile(np.array([7, 200], np.uint8), n // 2 + 1)[:n]
    if content == "ramp":
        return (np.arange(n) & 255).astype(np.uint8)
    raise KeyError(content)


SWEEP_LENGTHS = (254, 255, 256, 510, 511)


def sweep_cases(step):
    """(n, seed) of the sub-block sweep: noise rows of 200 .. 479 pixels, three planes each; step > 1: every step-th count, and always the ones that hit
    SWEEP_LENGTHS in the full sweep (tests/test_host_gif_coded.py asserts that they do)."""
    keep = {(223, 7919), (224, 0), (225, 0), (432, 0), (432, 15838)}
    return [(n, seed) for n in range(200, 480) for seed in (0, 7919, 15838) if ((n - 200) % step == 0 and (step == 1 or seed == 0)) or (n, seed) in keep]


def pal8_of(idx, seed=0):
    """A PAL8 frame around an index plane: a palette of noise (the coder copies it, whatever it holds)."""
    pal = np.random.default_rng(77 + seed).integers(0, 256, 768, dtype=np.uint8)
    return np.concatenate([np.asarray(idx, np.uint8).ravel(), pal])


def pixel_counts(seg):
    return (1, 2, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1)


def shapes(seg):
    """(w, h): every pixel count as one row, and planes 67 wide around one and two segments."""
    return [(n, 1) for n in pixel_counts(seg)] + [(67, seg // 67), (67, seg // 67 + 1), (67, 2 * seg // 67 + 1)]


def all_distinct(n):
    """n index bytes in which no pair of neighbours repeats inside 4096 pixels (runs of 256 values a fixed odd step apart, another step per run): the coder
    finds no string twice, every pixel costs a code."""
    out = np.empty(n, np.uint8)
    for k in range(0, n, 256):
        step = 2 * ((k // 256) % 128) + 1
        m = min(256, n - k)
        out[k:k + m] = (np.arange(m) * step) & 255
    return out
