"""GPU check of the writer path's grow-only buffers (poppy_amd/csrc/writer_buffers.h: DeviceBuffer) while ONE context lives: the scale and format scratch of the
frames that no slot renders (the t = 0 / 1 copies of render_phases go through download_frame), the sequence's store and its rings of index planes and coded
frames.  A 64 x 48 pair, then a 160 x 120 pair (every buffer grows), then the small pair again (a larger buffer than needed is reused); under the sequence
formats a 3-frame and then a 9-frame sequence at 160 x 120 as well (the store grows behind rings that stay).  Every frame must equal, byte for byte, what a
fresh context gives for the same pair, format, scale and phases.  The two sizes are the smallest whose buffers differ by more than an allocation's granularity
in every format (the scaled BGR scratch: 2.3 KB against 14 KB)."""
import numpy as np
import pytest

import test_gpu_frame_format as FF
from poppy_amd import capi

pytestmark = pytest.mark.gpu
BGR, I420, PAL8, PAL8_SEQ, GIF, GIF_SEQ = capi.FRAME_BGR, capi.FRAME_I420, capi.FRAME_PAL8, capi.FRAME_PAL8_SEQ, capi.FRAME_GIF, capi.FRAME_GIF_SEQ
SMALL, LARGE = (64, 48), (160, 120)
TS = (0.0, 0.3, 0.7, 1.0)                   # t = 0 and 1: copies of the images, through the scratch; the inner frames through the slots
TS3, TS9 = (0.0, 0.5, 1.0), tuple(np.linspace(0.0, 1.0, 9))
_FRESH = {}


def _configured(fmt, scale):
    c = capi.Context(0)
    if fmt != BGR:
        c.set_frame_format(fmt)
    if scale != 1:
        c.set_frame_scale(scale)
    return c


def _frames(c, size, ts):
    c.pair_load(*FF._inputs(*size))
    return FF._collect(c, c.render_phases, list(ts))


def _fresh(fmt, scale, size, ts):
    key = (fmt, scale, size, ts)
    if key not in _FRESH:
        c = _configured(fmt, scale)
        try:
            _FRESH[key] = _frames(c, size, ts)
        finally:
            c.close()
    return _FRESH[key]


def _grows_and_reuses(fmt, scale, steps):
    c = _configured(fmt, scale)
    try:
        for n, (size, ts) in enumerate(steps):
            got, want = _frames(c, size, ts), _fresh(fmt, scale, size, ts)
            what = f"format {fmt}, scale {scale}, step {n} ({size[0]} x {size[1]}, {len(ts)} frames)"
            assert len(got) == len(want) == len(ts), f"{what}: {len(got)} frames, a fresh context gives {len(want)}"
            for k, (a, b) in enumerate(zip(want, got)):
                assert a.shape == b.shape, f"{what}, frame {k}: {b.shape}, a fresh context gives {a.shape}"
                neq = np.flatnonzero(a.ravel() != b.ravel())
                assert neq.size == 0, f"{what}, frame {k}: {neq.size} of {a.size} bytes differ from a fresh context's, first at {neq[0]}"
    finally:
        c.close()


@pytest.mark.parametrize("fmt", [BGR, I420, PAL8, GIF])
def test_scratch_grows_and_is_reused(fmt):
    _grows_and_reuses(fmt, 2, [(SMALL, TS), (LARGE, TS), (SMALL, TS)])


@pytest.mark.parametrize("fmt", [PAL8_SEQ, GIF_SEQ])
def test_sequence_store_and_rings_grow(fmt):
    _grows_and_reuses(fmt, 1, [(SMALL, TS), (LARGE, TS), (SMALL, TS), (LARGE, TS3), (LARGE, TS9)])
