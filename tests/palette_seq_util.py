"""Helpers shared by tests/test_host_palette_seq.py and tests/test_gpu_palette_seq.py (POPPY_FRAME_PAL8_SEQ, POPPY_SINK_GIF_GLOBAL): sequences stacked into
one image (the way the sequence rule is pinned to the single-frame one), and a GIF89a decoder that takes files with and without a global colour table
(palette_util.gif_decode asserts that there is none)."""
import struct

import numpy as np

from palette_util import collect, inputs, loaded, pal8_reference, textured      # noqa: F401  (re-exported for the two test files)
from poppy_amd import capi


def stacked(frames):
    """n frames of H x W as one (n * H) x W image"""
    a = np.ascontiguousarray(frames, np.uint8)
    n, h, w = a.shape[:3]
    return a.reshape(n * h, w, 3)


def frames_of_stacked(flat, n, w, h):
    """a flat PAL8 frame of the stacked image, cut into the n PAL8_SEQ frames it stands for: n x (w * h + 768)"""
    idx, pal = flat[:n * w * h].reshape(n, w * h), flat[n * w * h:]
    return np.concatenate([idx, np.broadcast_to(pal, (n, 768))], axis=1)


def host_seq(bgr_frames):
    """what a PAL8_SEQ context must hand out for these BGR frames: the host statement"""
    return capi.bgr_frames_to_pal8(np.stack(bgr_frames))


def same_seq(what, bgr_frames, seq_frames):
    assert len(bgr_frames) == len(seq_frames) and len(bgr_frames) > 0, f"{what}: {len(bgr_frames)} BGR frames, {len(seq_frames)} PAL8_SEQ frames"
    want = host_seq(bgr_frames)
    n_idx = want.shape[1] - 768
    for k, p in enumerate(seq_frames):
        assert p.ndim == 1 and p.shape == want[k].shape, f"{what}: frame {k} has shape {p.shape}, the format has {want[k].shape}"
        neq = np.flatnonzero(p != want[k])
        assert neq.size == 0, f"{what}: frame {k}: {neq.size} of {p.size} bytes differ ({(neq >= n_idx).sum()} of them in the palette), first at {neq[0]}"


def _lzw(body, counts):
    clear, end = 256, 257
    px = bytearray()
    width, nxt, prev = 9, 258, None
    acc, n_acc, at = 0, 0, 0
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
            counts["clears"] += 1
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
    return bytes(px)


def gif_decode_any(data):
    """{header, screen, global (256 x 3 or None), loop, loop_at, frames: [(delay, w, h, palette in force (256 x 3), indices, has a local table)]}"""
    out = {"header": data[:6], "screen": struct.unpack("<HHBBB", data[6:13]), "global": None, "loop": None, "loop_at": None, "frames": [], "clears": 0}
    pos, delay = 13, None
    if out["screen"][2] & 0x80:
        assert out["screen"][2] & 7 == 7, "a global colour table of 256 entries"
        out["global"] = np.frombuffer(data[13:13 + 768], np.uint8).reshape(256, 3)
        pos += 768

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
            label, at = data[pos + 1], pos
            body, pos = sub_blocks(pos + 2)
            if label == 0xF9:
                assert len(body) == 4
                delay = struct.unpack("<BHB", body)[1]
            elif label == 0xFF:
                assert body[:11] == b"NETSCAPE2.0" and body[11] == 1
                out["loop"], out["loop_at"] = struct.unpack("<H", body[12:14])[0], at
            continue
        assert tag == 0x2C, f"block {tag:#x} at {pos}"
        x, y, w, h, flags = struct.unpack("<HHHHB", data[pos + 1:pos + 10])
        assert (x, y) == (0, 0) and flags in (0x87, 0x00), "a 256-entry local colour table or none, not interlaced"
        pos += 10
        if flags:
            pal = np.frombuffer(data[pos:pos + 768], np.uint8).reshape(256, 3)
            pos += 768
        else:
            assert out["global"] is not None, "a frame without a local table in a file without a global one"
            pal = out["global"]
        assert data[pos] == 8
        body, pos = sub_blocks(pos + 1)
        px = _lzw(body, out)
        assert len(px) == w * h, f"{len(px)} pixels decoded, the image has {w * h}"
        out["frames"].append((delay, w, h, pal, np.frombuffer(px, np.uint8), bool(flags)))
        delay = None


def write_gif(path, frames_pal8, w, h, sink, fps=(25, 1)):
    s = capi.lib().poppy_sink_open(str(path).encode(), sink, w, h, fps[0], fps[1])
    assert s
    for f in frames_pal8:
        capi.lib().poppy_sink_write(s, capi._p(np.ascontiguousarray(f)), w, h, w)
    return capi.lib().poppy_sink_close(s)
