"""Shared by the CPU and GPU tests of the JPEG byte budget (include/poppy_hip.h, "JPEG byte budget"): the contents, small frames named for what they reach in
the coder and in the search, each content's table of the 100 file sizes (coded once per process by the fixed-quality host statement, which tests/test_host_jpeg.py
pins to the rule), a numpy restatement of the search written from the header's text, and the budgets and highest qualities every case runs over."""
import functools

import numpy as np

from poppy_amd import capi

QMAXES = (100, 90, 50, 2, 1)
NAMED_QUALITIES = (1, 2, 37, 50, 89, 90, 100)
SAMPLINGS = (capi.FRAME_JPEG, capi.FRAME_JPEG444)


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _saturated(w, h, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)


def _dithered_ramp(w, h, seed):
    x = np.arange(w)[None, :, None] * 255 // max(w - 1, 1)
    y = np.arange(h)[:, None, None] * 255 // max(h - 1, 1)
    base = (x * np.array([1, 0, 1]) + y * np.array([0, 1, 1])) // np.array([1, 1, 2])
    return np.clip(base + np.random.default_rng(seed).integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)


def _flat(w, h, seed):
    return np.full((h, w, 3), (90, 140, 200), np.uint8)


# name -> (generator, width, height, seed).  The seeds of the three small frames were searched on the CPU for frames whose size table has inversions
# (size(q + 1) < size(q)) at which the search and "the highest quality that fits" disagree: test_host_jpeg_budget.py asserts that they still do.
CONTENTS = {
    "noise_8x8": (_noise, 8, 8, 1),                          # one MCU, one segment
    "noise_17x9": (_noise, 17, 9, 2),                        # the last column and row clamped
    "noise_40x24": (_noise, 40, 24, 3),
    "saturated_40x24": (_saturated, 40, 24, 4),              # 0 / 255 noise: long codes, FF bytes, stuffing
    "ramp_64x48": (_dithered_ramp, 64, 48, 5),
    "flat_24x24": (_flat, 24, 24, 0),                        # every quality the same size
    "noise_136x24": (_noise, 136, 24, 6),                    # more than one segment, the last one short (18 MCUs of 4:2:0, 51 of 4:4:4)
    "ramp_200x120": (_dithered_ramp, 200, 120, 7),
}


@functools.lru_cache(maxsize=None)
def bgr(name):
    gen, w, h, seed = CONTENTS[name]
    a = gen(w, h, seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def planes(name, fmt):
    """the planes the format's coder reads: I420 for FRAME_JPEG, I444 for FRAME_JPEG444"""
    a = (capi.bgr_to_i444 if fmt == capi.FRAME_JPEG444 else capi.bgr_to_i420)(bgr(name))
    a = np.ascontiguousarray(a, np.uint8).ravel()
    a.setflags(write=False)
    return a


def fixed_frame(pl, w, h, fmt, quality):
    return (capi.i444_to_jpeg_frame if fmt == capi.FRAME_JPEG444 else capi.i420_to_jpeg_frame)(pl, w, h, quality)


@functools.lru_cache(maxsize=None)
def frames(name, fmt):
    """the content's fixed-quality frames, [None, frame at quality 1, ..., frame at quality 100]"""
    _, w, h, _ = CONTENTS[name]
    return [None] + [fixed_frame(planes(name, fmt), w, h, fmt, q) for q in range(1, 101)]


def size_table(all_frames):
    """sizes[q] = the JFIF file's length at quality q (`total` - 4), entry 0 unused"""
    return np.array([0] + [f.size - 4 for f in all_frames[1:]], np.uint32)


@functools.lru_cache(maxsize=None)
def sizes(name, fmt):
    t = size_table(frames(name, fmt))
    t.setflags(write=False)
    return t


def pick(table, qmax, budget):
    """the header's search, restated"""
    if table[qmax] <= budget:
        return qmax
    lo, hi = 0, qmax
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if table[mid] <= budget:
            lo = mid
        else:
            hi = mid
    return max(lo, 1)


def probes(table, qmax, budget):
    """how many qualities the search asks about"""
    return len(asked(table, qmax, budget))


def asked(table, qmax, budget):
    """the qualities the search asks about"""
    asked = {qmax}
    if table[qmax] > budget:
        lo, hi = 0, qmax
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            asked.add(mid)
            lo, hi = (mid, hi) if table[mid] <= budget else (lo, mid)
    return asked


def highest_fitting(table, qmax, budget):
    """the rule the search is NOT: the highest quality whose file fits, 1 if none does"""
    fit = [q for q in range(1, qmax + 1) if table[q] <= budget]
    return max(fit) if fit else 1


def disagreements(table, qmax=100):
    """every budget of the form size(q), size(q) - 1 at which the search and "highest fitting" differ"""
    out = []
    for q in range(1, qmax + 1):
        for b in (int(table[q]), int(table[q]) - 1):
            if b > 0 and b not in out and pick(table, qmax, b) != highest_fitting(table, qmax, b):
                out.append(b)
    return out


def budgets_of(table, capacity):
    """a content's budgets from its own table: the named qualities' sizes and one byte less, every disagreement, one below size(1), the format's capacity"""
    out = []
    for b in [int(table[q]) - d for q in NAMED_QUALITIES for d in (0, 1)] + disagreements(table) + [int(table[1]) // 2, int(capacity)]:
        if b > 0 and b not in out:
            out.append(b)
    return out


def budgets(name, fmt):
    _, w, h, _ = CONTENTS[name]
    return budgets_of(sizes(name, fmt), capi.frame_bytes(fmt, w, h))


def cases(name, fmt):
    """(qmax, budget, the quality the restated search picks) over every highest quality and budget of the content"""
    t = sizes(name, fmt)
    return [(qmax, b, pick(t, qmax, b)) for qmax in QMAXES for b in budgets(name, fmt)]
