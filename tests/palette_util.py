"""Helpers shared by tests/test_host_palette_format.py and tests/test_gpu_palette_format.py: the PAL8 format restated in numpy (the reference both
compare the library with), a GIF89a decoder written for the tests, and the pair inputs of the GPU cases."""
import struct

import numpy as np

from poppy_amd import synth


def pal8_reference(bgr):
    """(flat PAL8 frame, boxes) by the header's rule, in numpy / Python integers.  boxes: [(lo[3], hi[3], count)] over the axes R, G, B."""
    h, w = bgr.shape[:2]
    px = bgr.reshape(-1, 3).astype(np.int64)
    b, g, r = px[:, 0], px[:, 1], px[:, 2]
    cell = ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3)
    n = np.bincount(cell, minlength=32768).reshape(32, 32, 32)                      # [r, g, b]
    sums = [np.bincount(cell, weights=c, minlength=32768).astype(np.int64).reshape(32, 32, 32) for c in (r, g, b)]

    def shrink(lo, hi):
        sub = n[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        lo2, hi2 = list(lo), list(hi)
        for a in range(3):
            nz = np.flatnonzero(sub.sum(axis=tuple(x for x in range(3) if x != a)))
            lo2[a], hi2[a] = lo[a] + int(nz[0]), lo[a] + int(nz[-1])
        return lo2, hi2, int(sub.sum())

    boxes = [shrink([0, 0, 0], [31, 31, 31])]
    while len(boxes) < 256:
        best, best_score = -1, 0
        for i, (lo, hi, c) in enumerate(boxes):
            side = max(hi[a] - lo[a] + 1 for a in range(3))
            if side > 1 and c * side > best_score:                                   # ties: the lowest index
                best, best_score = i, c * side
        if best < 0:
            break
        lo, hi, c = boxes[best]
        ext = [hi[a] - lo[a] for a in range(3)]
        axis = 1                                                                     # ties: G, then R, then B
        if ext[0] > ext[axis]:
            axis = 0
        if ext[2] > ext[axis]:
            axis = 2
        sub = n[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        cum = np.cumsum(sub.sum(axis=tuple(x for x in range(3) if x != axis)))
        k = min(int(np.searchsorted(cum, (c + 1) // 2)), ext[axis] - 1)
        hi1, lo2 = list(hi), list(lo)
        hi1[axis], lo2[axis] = lo[axis] + k, lo[axis] + k + 1
        boxes[best] = shrink(lo, hi1)
        boxes.append(shrink(lo2, hi))
    table = np.zeros((32, 32, 32), np.uint8)
    pal = np.zeros((256, 3), np.uint8)
    for i, (lo, hi, c) in enumerate(boxes):
        sl = (slice(lo[0], hi[0] + 1), slice(lo[1], hi[1] + 1), slice(lo[2], hi[2] + 1))
        table[sl] = i
        pal[i] = [(int(s[sl].sum()) + c // 2) // c for s in sums]
    return np.concatenate([table.reshape(-1)[cell], pal.ravel()]).astype(np.uint8), boxes


def gif_decode(data):
    """{header, screen, loop, frames: [(delay, w, h, palette (256 x 3), indices)]} of a GIF89a file: blocks, sub-blocks, LZW.  Counts the clear codes."""
    out = {"header": data[:6], "screen": struct.unpack("<HHBBB", data[6:13]), "loop": None, "frames": [], "clears": 0}
    assert not out["screen"][2] & 0x80, "a global colour table"
    pos, delay = 13, None

    def sub_blocks(pos):
        buf = bytearray()
        while data[pos]:
            buf += data[pos + 1:pos + 1 + data[pos]]
            pos += 1 + data[pos]
        return bytes(buf), pos + 1

    while True:
        tag = data[pos]
        if tag == 0x3B:
            assert pos == len(data) - 1, "bytes behind the trailer"
            return out
        if tag == 0x21:
            label = data[pos + 1]
            body, pos = sub_blocks(pos + 2)
            if label == 0xF9:
                assert len(body) == 4
                delay = struct.unpack("<BHB", body)[1]
            elif label == 0xFF:
                assert body[:11] == b"NETSCAPE2.0" and body[11] == 1
                out["loop"] = struct.unpack("<H", body[12:14])[0]
            continue
        assert tag == 0x2C, f"block {tag:#x} at {pos}"
        x, y, w, h, flags = struct.unpack("<HHHHB", data[pos + 1:pos + 10])
        assert (x, y) == (0, 0) and flags == 0x87, "a 256-entry local colour table, not interlaced"
        pal = np.frombuffer(data[pos + 10:pos + 10 + 768], np.uint8).reshape(256, 3)
        min_code = data[pos + 778]
        assert min_code == 8
        body, pos = sub_blocks(pos + 779)
        # LZW
        clear, end = 256, 257
        px = bytearray()
        width, nxt, prev = 9, 258, None
        acc, n_acc, at = 0, 0, 0                                 # a bit reader over the sub-blocks' bytes
        table = {}
        while True:
            while n_acc < width:
                acc |= body[at] << n_acc
                at += 1
                n_acc += 8
            code = acc & ((1 << width) - 1)
            acc >>= width
            n_acc -= width
            if code == clear:
                out["clears"] += 1
                table, width, nxt, prev = {}, 9, 258, None
                continue
            if code == end:
                break
            if code < 256:
                s = bytes([code])
            elif code in table:
                s = table[code]
            else:
                assert code == nxt and prev is not None, "a code beyond the table"
                s = prev + prev[:1]
            px += s
            if prev is not None and nxt < 4096:
                table[nxt] = prev + s[:1]
                nxt += 1
                if nxt == (1 << width) and width < 12:
                    width += 1
            prev = s
        assert at == len(body), "bytes behind the end code"
        assert len(px) == w * h, f"{len(px)} pixels decoded, the image has {w * h}"
        out["frames"].append((delay, w, h, pal, np.frombuffer(bytes(px), np.uint8)))
        delay = None


def collect(c, call, *args, **kw):
    frames = []
    call(*args, write=lambda v: frames.append(v.copy()), **kw)
    return frames


def textured(w, h, seed):
    if w * h <= 1 << 20:
        return synth.textured_bgr(w, h, seed)
    t = synth.textured_bgr(960, 540, seed)
    return np.ascontiguousarray(np.tile(t, (-(-h // 540), -(-w // 960), 1))[:h, :w])


def inputs(w, h, n=40):
    """(image 1, image 2, gabor2, points 1, points 2) for pair_load; random bytes and corner points where the frame is thin"""
    rng = np.random.default_rng(w * 7919 + h)
    if min(w, h) < 33:
        c1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8); c2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        g = (rng.integers(0, 1025, (h, w, 3)) / 1024.0).astype(np.float32)
        corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
        inner = np.stack([rng.integers(0, 4 * (w - 1) + 1, 4), rng.integers(0, 4 * (h - 1) + 1, 4)], 1) / 4.0
        moved = np.clip(inner + rng.integers(-3, 4, inner.shape) / 4.0, 0, [w - 1, h - 1])
        return c1, c2, g, np.concatenate([corners, inner]).astype(np.float32), np.concatenate([corners, moved]).astype(np.float32)
    c1 = textured(w, h, 41); c2 = textured(w, h, 42); g = synth.unit_field(w, h, 7)
    p1 = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1).astype(np.float32)
    p2 = np.clip(p1 + rng.normal(0, 4.0, (n, 2)), 0, [w - 1, h - 1]).astype(np.float32)
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
    return c1, c2, g, np.concatenate([p1, corners]), np.concatenate([p2, corners])


def loaded(w, h):
    def run_with(fn):
        def run(c):
            c1, c2, g, p1, p2 = inputs(w, h)
            c.pair_load(c1, c2, g, p1, p2)
            return fn(c)
        return run
    return run_with
