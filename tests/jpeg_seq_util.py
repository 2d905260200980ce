"""Shared by the CPU and GPU tests of the JPEG hand-off on one Huffman table set per sequence (include/poppy_hip.h: POPPY_FRAME_JPEG_SEQ,
POPPY_FRAME_JPEG444_SEQ): the reference sequence in plain Python on the restatement of tests/jpeg_opt_util.py — every frame's symbol counts summed, ONE call of
the table rule per table, every frame coded on what it gave behind the one header — and the sequences both suites code."""
import numpy as np

import jpeg444_util as U4
import jpeg_opt_util as O
import jpeg_util as U
from poppy_amd import capi, synth

FORMATS = (capi.FRAME_JPEG_SEQ, capi.FRAME_JPEG444_SEQ)
SAMPLING = {capi.FRAME_JPEG_SEQ: 420, capi.FRAME_JPEG444_SEQ: 444}
OPT_OF = {capi.FRAME_JPEG_SEQ: capi.FRAME_JPEG_OPT, capi.FRAME_JPEG444_SEQ: capi.FRAME_JPEG444_OPT}
HOST_OPT = {capi.FRAME_JPEG_SEQ: capi.bgr_to_jpeg_opt_frame, capi.FRAME_JPEG444_SEQ: capi.bgr_to_jpeg444_opt_frame}
HOST_JPEG = {capi.FRAME_JPEG_SEQ: capi.bgr_to_jpeg_frame, capi.FRAME_JPEG444_SEQ: capi.bgr_to_jpeg444_frame}
PLANES_OF = {capi.FRAME_JPEG_SEQ: capi.bgr_to_i420, capi.FRAME_JPEG444_SEQ: capi.bgr_to_i444}
QUALITIES = (100, 90, 25)
SIZES = ((8, 8), (17, 9), (48, 48), (160, 128))                # 17 x 9: the last MCU column and row are clamped
LENGTHS = (1, 2, 5)
SEQ_MAX_SYMBOLS = (1 << 32) - 2


def frame_segments(planes, w, h, quality, sampling):
    """(the symbols of every segment of a frame of flat planes, the fixed header)"""
    if sampling == 444:
        q, restart, fixed = U4.quantised_mcus(planes, w, h, quality), 16, U4.header(w, h, quality, 16)
    else:
        q, restart, fixed = U.quantised_mcus(planes, w, h, quality), 8, U.header(w, h, quality, 8)
    n_seg = -(-len(q) // restart)
    return [O.segment_symbols(q[k * restart:(k + 1) * restart]) for k in range(n_seg)], fixed


def seq_reference(planes_list, w, h, quality, sampling=420, stats=None):
    """The frames of a POPPY_FRAME_JPEG_SEQ (sampling 444: JPEG444_SEQ) sequence of flat planes, as a list of bytes.  stats (a dict) receives per table the summed
    counts (`counts`), whether step 4 ran on them (`limited`) and their unlimited depth (`depth`), and per frame its own counts (`frame_counts`)."""
    frames = [frame_segments(p, w, h, quality, sampling) for p in planes_list]
    own = [O.frame_counts(segments) for segments, _ in frames]
    sums = {key: [sum(c[key][s] for c in own) for s in range(256)] for key in own[0]}
    tables, codes = {}, {}
    for key, counts in sums.items():
        info = {}
        tables[key] = O.optimal_table(counts, info)
        codes[key] = U.huffman_codes(*tables[key])
        if stats is not None:
            stats.setdefault("limited", {})[key] = info["limited"]
            stats.setdefault("depth", {})[key] = info["depth"]
    if stats is not None:
        stats["counts"], stats["frame_counts"] = sums, own
    out = []
    for segments, fixed in frames:
        f = bytearray(O.opt_header(fixed, tables))
        for k, seg in enumerate(segments):
            f += O.code_symbols(seg, codes)
            f += bytes([0xFF, 0xD0 + k % 8]) if k + 1 < len(segments) else b"\xff\xd9"
        out.append((len(f) + 4).to_bytes(4, "little") + bytes(f))
    return out


def _huffman_lookup(bits, vals):
    """(symbol, length) of every 16-bit prefix of a canonical code given as a DHT holds it; length 0: no code begins so"""
    sym, length = [0] * 65536, [0] * 65536
    code, at = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            lo, hi = code << (16 - l), (code + 1) << (16 - l)
            sym[lo:hi] = [vals[at]] * (hi - lo)
            length[lo:hi] = [l] * (hi - lo)
            at += 1
            code += 1
        code <<= 1
    return sym, length


def frame_coefficients(frame, sampling=420):
    """The quantised coefficients that a frame's entropy-coded data holds, decoded on the frame's OWN DHT tables: an array MCUs x blocks x 64, zig-zag, the DC
    values absolute — what a decoder dequantises, so two frames of one header that agree here decode to the same pixels.  Asserts that every segment ends in
    fewer than 8 padding bits, all ones."""
    f = U.walk_frame(frame)
    w, h = f["size"]
    side, blocks, restart = (8, 3, 16) if sampling == 444 else (16, 6, 8)
    assert f["restart"] == restart
    n_mcu = -(-w // side) * -(-h // side)
    assert len(f["segments"]) == -(-n_mcu // restart)
    look = {key: _huffman_lookup(*f["dht"][key]) for key in ((0, 0), (1, 0), (0, 1), (1, 1))}
    luma = blocks - 2
    out = np.zeros((n_mcu, blocks, 64), np.int64)
    for k, seg in enumerate(f["segments"]):
        data = seg.replace(b"\xff\x00", b"\xff")
        total = len(data) * 8 + 16
        acc = int.from_bytes(data, "big") << 16 | 0xFFFF      # (16 bits behind the end, so that a peek never runs out)
        pos = 0

        def symbol(key):
            nonlocal pos
            peek = (acc >> (total - 16 - pos)) & 0xFFFF
            n = look[key][1][peek]
            assert n, f"segment {k}: no code at bit {pos}"
            pos += n
            return look[key][0][peek]

        def value(cat):
            nonlocal pos
            if not cat:
                return 0
            v = (acc >> (total - pos - cat)) & ((1 << cat) - 1)
            pos += cat
            return v if v >> (cat - 1) else v - (1 << cat) + 1
        pred = [0, 0, 0]
        for m in range(k * restart, min((k + 1) * restart, n_mcu)):
            for b in range(blocks):
                comp, t = (0, 0) if b < luma else (b - luma + 1, 1)
                pred[comp] += value(symbol((0, t)))
                out[m, b, 0] = pred[comp]
                at = 1
                while at < 64:
                    s = symbol((1, t))
                    if s == 0:
                        break
                    if s == 0xF0:
                        at += 16
                        continue
                    at += s >> 4
                    assert at < 64, f"segment {k}: a run past coefficient 63"
                    out[m, b, at] = value(s & 15)
                    at += 1
        left = total - 16 - pos
        assert 0 <= left < 8 and (acc >> 16) & ((1 << left) - 1) == (1 << left) - 1, f"segment {k}: {left} bits behind its last block"
    return out


def blocks_per_frame(w, h, sampling=420):
    """B of the header's limit: the 8 x 8 blocks of a frame over all components"""
    side, blocks = (8, 3) if sampling == 444 else (16, 6)
    return -(-w // side) * -(-h // side) * blocks


def gradient_bgr(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], 2).astype(np.uint8))


def noise_bgr(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def sequence(n, w, h, seed=0):
    """n different BGR frames: textured, the synthetic pair's image, noise, a gradient, flat — in an order that depends on nothing but n"""
    kinds = [lambda: synth.textured_bgr(w, h, 3 + seed) if min(w, h) >= 16 else noise_bgr(w, h, 50 + seed), lambda: gradient_bgr(w, h),
             lambda: noise_bgr(w, h, 7 + seed), lambda: np.full((h, w, 3), (40, 90, 200), np.uint8), lambda: synth.gen(w, h, 77, 0, 0) if min(w, h) >= 16 else noise_bgr(w, h, 60 + seed)]
    return np.stack([np.ascontiguousarray(kinds[k % len(kinds)]()[:h, :w]) for k in range(n)])


def flat_noise_gradient(w=48, h=48):
    """the sequence in which the sum matters: a flat frame, then noise, then a smooth gradient"""
    return np.stack([np.full((h, w, 3), 128, np.uint8), noise_bgr(w, h, 21), gradient_bgr(w, h)])


def two_noise_frames(w=640, h=360):
    """two noise frames of different seeds: at quality 100 their SUMMED luma AC table passes 16 bits before limiting; 115 segments each, 29 counting workgroups"""
    return np.stack([noise_bgr(w, h, 5), noise_bgr(w, h, 6)])


def host_seq(frames, quality, fmt):
    return capi.bgr_frames_to_jpeg_seq_frames(np.stack(frames), quality, fmt)
