"""Shared by the CPU and GPU tests of the JPEG sequence budget (include/poppy_hip.h, "JPEG sequence budget"): the sequences, built from jpeg_budget_util's
contents and generators and named for what they reach in the kernels and in the search; every frame's table of the 100 file sizes (coded once per process by the
fixed-quality host statement) and their element-wise sum, on which jpeg_budget_util's restated search is the restated rule; and the budgets every case runs over."""
import functools

import numpy as np

import jpeg_budget_util as B
from poppy_amd import capi

QMAXES, SAMPLINGS = B.QMAXES, B.SAMPLINGS


def _content(name):
    return B.CONTENTS[name]


# name -> the frames' specs (generator, width, height, seed); the frames of one sequence share a size
SEQUENCES = {
    # single-segment frames
    "noise_saturated_2": [_content("noise_40x24"), _content("saturated_40x24")],
    "noise_saturated_3": [_content("noise_40x24"), _content("saturated_40x24"), (B._noise, 40, 24, 13)],
    # several segments, the last one short (18 MCUs of 4:2:0, 51 of 4:4:4): blockIdx.y up to 4 beside blockIdx.x > 0
    "noise_5_136x24": [(B._noise, 136, 24, 6 + k) for k in range(5)],
    # mixed content: a flat frame (every quality one size), a ramp and noise, whose per-frame picks differ from the sequence's one
    "flat_ramp_noise_64x48": [(B._flat, 64, 48, 0), (B._dithered_ramp, 64, 48, 5), (B._noise, 64, 48, 9)],
    "ramp_4_200x120": [(B._dithered_ramp, 200, 120, 7 + k) for k in range(4)],
    "single_ramp_64x48": [_content("ramp_64x48")],
}


def size_of(name):
    _, w, h, _ = SEQUENCES[name][0]
    return w, h


@functools.lru_cache(maxsize=None)
def _frame_bgr(spec):
    gen, w, h, seed = spec
    a = gen(w, h, seed)
    a.setflags(write=False)
    return a


def bgr(name):
    """the sequence's BGR frames, a list"""
    return [_frame_bgr(spec) for spec in SEQUENCES[name]]


@functools.lru_cache(maxsize=None)
def _frame_fixed(spec, fmt):
    """one frame's fixed-quality frames, [None, frame at quality 1, ..., frame at quality 100]"""
    _, w, h, _ = spec
    pl = np.ascontiguousarray((capi.bgr_to_i444 if fmt == capi.FRAME_JPEG444 else capi.bgr_to_i420)(_frame_bgr(spec)), np.uint8).ravel()
    return [None] + [B.fixed_frame(pl, w, h, fmt, q) for q in range(1, 101)]


def fixed(name, fmt, quality):
    """the sequence's frames at one fixed quality"""
    return [_frame_fixed(spec, fmt)[quality] for spec in SEQUENCES[name]]


def frame_sizes(name, fmt):
    """per frame its table of 100 sizes, uint64"""
    return [B.size_table(_frame_fixed(spec, fmt)).astype(np.uint64) for spec in SEQUENCES[name]]


@functools.lru_cache(maxsize=None)
def sizes(name, fmt):
    """size(q) of the sequence: the element-wise sum of its frames' tables"""
    t = np.sum(frame_sizes(name, fmt), axis=0).astype(np.uint64)
    t.setflags(write=False)
    return t


def int_table(table):
    """a table as Python integers (the restated search compares them with budgets above 2^63 / without numpy's mixed-sign promotion)"""
    return [int(x) for x in table]


def pick(table, qmax, budget):
    return B.pick(int_table(table), qmax, budget)


def budgets_of(table, capacity):
    """a sequence's budgets from its summed table: jpeg_budget_util's (the named qualities' sizes and one byte less, every disagreement of the search with "highest
    fitting", half of size(1), the capacity) and 2^32 + size(50), which a budget cut to 32 bits would take for about size(50)"""
    t = int_table(table)
    return B.budgets_of(t, capacity) + [(1 << 32) + t[50]]


def budgets(name, fmt):
    w, h = size_of(name)
    return budgets_of(sizes(name, fmt), len(SEQUENCES[name]) * capi.frame_bytes(fmt, w, h))


def cases(name, fmt):
    """(qmax, budget, the quality the restated search picks on the summed table)"""
    t = sizes(name, fmt)
    return [(qmax, b, pick(t, qmax, b)) for qmax in QMAXES for b in budgets(name, fmt)]


def equal(what, got, want):
    assert got.ndim == 1 and got.size == want.size, f"{what}: {got.size} bytes, the reference has {want.size}"
    neq = np.flatnonzero(got != want)
    assert neq.size == 0, f"{what}: {neq.size} of {want.size} bytes differ, first at {neq[0]}"


def equal_seq(what, got, want):
    assert len(got) == len(want) and len(want) > 0, f"{what}: {len(got)} frames, the reference has {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        equal(f"{what}: frame {k}", g, w)
