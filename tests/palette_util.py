"""Helpers shared by the palette tests (tests/test_host_palette_*.py, tests/test_gpu_palette_*.py): the PAL8 format restated in numpy (the reference they
compare the library with) and a trace of its cuts, a GIF89a decoder written for the tests, the pair inputs of the GPU cases, and the content the formats are
pinned on: the host tests' frames, frames built to reach what rendered frames never reach in the palette kernels (equal scores in different register banks of
the build's arg-max, every axis and tie order, clamped medians, fewer than 256 boxes, a workgroup with more cells than its LDS table has entries) and, for
I420, saturated 2 x 2 blocks (the chroma clamp)."""
import os
import struct

import numpy as np

from poppy_amd import synth

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
HIST_SLOTS, HIST_MAX_BLOCKS = 2048, 512                          # kernels_frame_pal8.hip: kHistSlots, the hist launch's largest grid


def pal8_reference(bgr, trace=None):
    """(flat PAL8 frame, boxes) by the header's rule, in numpy / Python integers.  boxes: [(lo[3], hi[3], count)] over the axes R, G, B.
    trace (a dict, filled if given): see cut_trace."""
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
    if trace is not None:
        trace.update(axis_cuts=[0, 0, 0], clamped=0, tied=0, cross_bank=0)
    while len(boxes) < 256:
        best, best_score = -1, 0
        for i, (lo, hi, c) in enumerate(boxes):
            side = max(hi[a] - lo[a] + 1 for a in range(3))
            if side > 1 and c * side > best_score:                                   # ties: the lowest index
                best, best_score = i, c * side
        if best < 0:
            break
        if trace is not None:
            tied = [i for i, (lo, hi, c) in enumerate(boxes) if c * max(hi[a] - lo[a] + 1 for a in range(3)) == best_score]
            trace["tied"] += len(tied) > 1
            trace["cross_bank"] += len({i // 64 for i in tied}) > 1
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
        if trace is not None:
            trace["axis_cuts"][axis] += 1
            trace["clamped"] += int(np.searchsorted(cum, (c + 1) // 2)) > ext[axis] - 1
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
    if trace is not None:
        trace["boxes"] = len(boxes)
    return np.concatenate([table.reshape(-1)[cell], pal.ravel()]).astype(np.uint8), boxes


def cut_trace(bgr):
    """What the rule does on this frame: {boxes, axis_cuts: [cuts along R, G, B], clamped: cuts whose median fell on the last position (k = hi - 1 instead),
    tied: cuts whose best score more than one box had, cross_bank: those of them whose tied boxes differ in index // 64 (the build kernel keeps boxes
    lane, lane + 64, lane + 128, lane + 192 in four registers per lane and must take the lowest index over all four)}."""
    trace = {}
    pal8_reference(bgr, trace)
    return trace


def first_workgroup_cells(bgr, max_blocks=HIST_MAX_BLOCKS):
    """The distinct cells workgroup 0 of k_pal8_hist / k_pal8_seq_pass reads, by the launch's rule: quads of 4 pixels, 256 per workgroup, a grid stride over
    min(ceil(quads / 256), max_blocks) workgroups.  Above HIST_SLOTS its LDS table cannot hold them and cells go to the global tables directly."""
    px = bgr.reshape(-1, 3).astype(np.int64)
    n_quads = (len(px) + 3) // 4
    grid = min((n_quads + 255) // 256, max_blocks)
    mine = ((np.arange(len(px)) // 4 // 256) % grid) == 0
    b, g, r = px[mine, 0], px[mine, 1], px[mine, 2]
    return len(np.unique(((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3)))


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


def inputs(w, h, n=40, c1=None, c2=None):
    """(image 1, image 2, gabor2, points 1, points 2) for pair_load; random bytes and corner points where the frame is thin.  c1, c2: these images instead"""
    rng = np.random.default_rng(w * 7919 + h)
    if min(w, h) < 33:
        r1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8); r2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        g = (rng.integers(0, 1025, (h, w, 3)) / 1024.0).astype(np.float32)
        corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float32)
        inner = np.stack([rng.integers(0, 4 * (w - 1) + 1, 4), rng.integers(0, 4 * (h - 1) + 1, 4)], 1) / 4.0
        moved = np.clip(inner + rng.integers(-3, 4, inner.shape) / 4.0, 0, [w - 1, h - 1])
        return (r1 if c1 is None else c1, r2 if c2 is None else c2, g,
                np.concatenate([corners, inner]).astype(np.float32), np.concatenate([corners, moved]).astype(np.float32))
    c1 = textured(w, h, 41) if c1 is None else c1; c2 = textured(w, h, 42) if c2 is None else c2; g = synth.unit_field(w, h, 7)
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


# ---- content ---------------------------------------------------------------------------------------------------------------------------------------------
def cells_frame(cells, w, h, seed, one_colour=True):
    """A w x h frame whose pixels occupy exactly the given cells (every cell at least once); one colour per cell, or any colour of the cell."""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells)
    assert len(cells) <= w * h
    pick = np.concatenate([np.arange(len(cells)), rng.integers(0, len(cells), w * h - len(cells))])
    rng.shuffle(pick)
    low = rng.integers(0, 8, (len(cells), 3)) if one_colour else None
    c = cells[pick]
    rgb = np.stack([(c >> 10) & 31, (c >> 5) & 31, c & 31], 1) * 8 + (low[pick] if one_colour else rng.integers(0, 8, (w * h, 3)))
    return np.ascontiguousarray(rgb[:, ::-1].reshape(h, w, 3).astype(np.uint8))


def photo(name):
    return np.load(os.path.join(GOLDEN, "photo_pair_720x405.npz"))[name]


def tie_frames():
    out = {}
    # two boxes of equal score: four colours, two pairs of equal count, each pair one cell apart on another axis
    f = np.zeros((8, 8, 3), np.uint8)
    f[:2, :] = (0, 0, 0); f[2:4, :] = (0, 0, 8); f[4:6, :] = (200, 200, 200); f[6:, :] = (200, 208, 200)
    out["equal_scores"] = f
    # sides of equal length: the corners of a cube of cells, equal counts -> the first cut is along G, then R, then B
    f = np.zeros((8, 16, 3), np.uint8)
    for k in range(8):
        f[k, :] = (40 + 80 * (k & 1), 40 + 80 * ((k >> 1) & 1), 40 + 80 * ((k >> 2) & 1))
    out["equal_sides"] = f
    # equal sides on R and B only (G flat), and a median that falls on the last position (clamped to k < hi)
    f = np.zeros((4, 10, 3), np.uint8)
    f[:, :9] = (16, 100, 16); f[:, 9] = (48, 100, 48)
    out["rb_tie_clamped"] = f
    rng = np.random.default_rng(5)
    g = rng.integers(0, 4, (40, 40, 3)) * 64                                         # 64 colours on a lattice: many equal extents and counts
    out["lattice"] = g.astype(np.uint8)
    return out


def frames():
    rng = np.random.default_rng(11)
    out = {"random_97x61": rng.integers(0, 256, (61, 97, 3), dtype=np.uint8),
           "random_256x256": rng.integers(0, 256, (256, 256, 3), dtype=np.uint8),
           "textured_640x360": synth.textured_bgr(640, 360, 3),
           "photo_a": photo("a"), "photo_b": photo("b"),
           "flat": np.full((30, 50, 3), (12, 200, 99), np.uint8),
           "cells_256": cells_frame(rng.choice(32768, 256, replace=False), 64, 40, 1),
           "cells_257": cells_frame(rng.choice(32768, 257, replace=False), 64, 40, 2),
           "cells_257_any_colour": cells_frame(rng.choice(32768, 257, replace=False), 64, 40, 3, one_colour=False),
           "1x1": rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), "1x7": rng.integers(0, 256, (7, 1, 3), dtype=np.uint8),
           "5x3": rng.integers(0, 256, (3, 5, 3), dtype=np.uint8), "odd_749x31": synth.textured_bgr(749, 31, 9)}
    two = np.zeros((20, 33, 3), np.uint8)
    two[:, :11] = (250, 3, 77); two[:, 11:] = (4, 180, 90)
    out["two_tone"] = two
    out.update(tie_frames())
    return out


def _of_cells(cells, w, h, rng):
    """the pixels of the given cells (one entry per pixel), shuffled, random low three bits, as an h x w BGR frame"""
    cells = rng.permutation(np.asarray(cells))
    assert len(cells) == w * h
    rgb = np.stack([(cells >> 10) & 31, (cells >> 5) & 31, cells & 31], 1) * 8 + rng.integers(0, 8, (w * h, 3))
    return np.ascontiguousarray(rgb[:, ::-1].reshape(h, w, 3).astype(np.uint8))


def _cell(r, g, b):
    return (np.asarray(r) << 10) | (np.asarray(g) << 5) | np.asarray(b)


def adversarial_frames():
    """Frames that reach what rendered frames do not (the module's docstring); what each is built for is asserted in tests/test_host_palette_content.py."""
    rng = np.random.default_rng(2026)
    out = {"cube_uniform": _of_cells(np.arange(32768), 256, 128, rng)}               # every cell once: equal counts everywhere, ties in nearly every cut
    q = np.arange(0, 32, 4)
    r, g, b = np.meshgrid(q, q, q, indexing="ij")
    out["lattice512"] = _of_cells(np.repeat(_cell(r, g, b).ravel(), 8), 64, 64, rng)
    line = np.repeat(np.arange(32), 64)                                              # every cut along one axis (the other two sides are one cell)
    out["line_r"] = _of_cells(_cell(line, 9, 21), 64, 32, rng)
    out["line_g"] = _of_cells(_cell(17, line, 5), 64, 32, rng)
    out["line_b"] = _of_cells(_cell(3, 28, line), 64, 32, rng)
    slab = np.full(64 * 16, 31)
    slab[:3] = (0, 1, 2)                                                             # the median falls on G's last position: clamped, and 4 boxes in all
    out["last_slab"] = _of_cells(_cell(12, slab, 7), 64, 16, rng)
    out["last_slab_mirror"] = 255 - out["last_slab"]                                 # mirrored in colour: the median on the first position
    tail = np.full(64 * 64, 32767)                                                   # the heavy cell is the last on every axis: the median of its box is clamped
    tail[:40] = rng.choice(32767, 40, replace=False)
    out["heavy_tail"] = _of_cells(tail, 64, 64, rng)
    out["noise_256x128"] = rng.integers(0, 256, (128, 256, 3), dtype=np.uint8)
    return out


def big_noise():
    """Uniform noise above 2048 * 512 pixels, the smallest frames in which a hist workgroup reads more pixels than its table has entries (1280 x 1024:
    3072 pixels).  Built where they are used: 3.9 MB each."""
    rng = np.random.default_rng(1280)
    return {"noise_1280x1024_a": rng.integers(0, 256, (1024, 1280, 3), dtype=np.uint8), "noise_1280x1024_b": rng.integers(0, 256, (1024, 1280, 3), dtype=np.uint8)}


def white_4096():
    """2^24 pixels of 255: the largest sums PAL8's packed 32-bit fields hold.  50 MB: built where it is used."""
    return np.full((4096, 4096, 3), 255, np.uint8)


PRIMARIES_SIZES = [(16, 4), (16, 5), (18, 4), (17, 5), (1, 1)]      # the wide I420 kernel alone, with the tail kernel for the last row, the tail kernel alone (clipped blocks)


def primaries(w, h, first=0):
    """2 x 2-flat blocks that cycle through the eight corners of the colour cube (corner k: B = bit 0, G = bit 1, R = bit 2 of k, times 255), block (bx, by)
    taking corner first + bx + 3 by.  Blue and red blocks reach U = 256 and V = 256 before the clamp, yellow and cyan the smallest chroma value, 1."""
    by, bx = np.mgrid[0:h, 0:w] // 2
    k = (first + bx + 3 * by) % 8
    return np.ascontiguousarray((np.stack([k & 1, (k >> 1) & 1, (k >> 2) & 1], 2) * 255).astype(np.uint8))
