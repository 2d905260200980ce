"""The writer ring under its environment switches, for every hand-off format: POPPY_HIP_DL_EVENTS (one download stream + an event per copy) and POPPY_HIP_RING are
read once per process, so every case runs in a fresh child.  One ring serves the slots' frames of all formats and the PAL8_SEQ hand-over; a ring of 1 forces a
delivery before every copy, a ring of 8 is capped by the slot count.  64 x 48 is two GIF segments, the second one short.  Every frame must equal the host
function of its format applied to the BGR frame of a BGR context in the same child, in every byte."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
from poppy_amd import capi
import gif_coded_util as U
import palette_seq_util as PS
import test_gpu_frame_format as T
import test_gpu_gif_coded as TG
import test_gpu_palette_format as TP

W, H = 64, 48
assert U.segment_pixels() < W * H < 2 * U.segment_pixels()
calls = {"render_many": lambda c: PS.collect(c, c.render_many, [0.1, 0.25, 0.4, 0.55, 0.7, 0.85], chain=True),
         "render_phases": lambda c: PS.collect(c, c.render_phases, [0.0, 0.3, 0.5, 1.0, 0.7])}


def frames(fmt, call):
    c = capi.Context(0)
    try:
        c.pair_load(*T._inputs(W, H))
        c.set_frame_format(fmt)
        return call(c)
    finally:
        c.close()


for name, call in calls.items():
    bgr = frames(capi.FRAME_BGR, call)
    assert len(bgr) == (6 if name == "render_many" else 5)
    T._same_frames(name + " I420", bgr, frames(capi.FRAME_I420, call))
    TP._same_frames(name + " PAL8", bgr, frames(capi.FRAME_PAL8, call))
    PS.same_seq(name + " PAL8_SEQ", bgr, frames(capi.FRAME_PAL8_SEQ, call))
    gif = frames(capi.FRAME_GIF, call)
    TG._same(name + " GIF", [capi.bgr_to_pal8(b) for b in bgr], gif, W, H)
    for k, (b, g) in enumerate(zip(bgr, gif)):
        assert np.array_equal(g, capi.bgr_to_gif_frame(b)), f"{name} GIF: frame {k} differs from poppy_bgr_to_gif_frame"
print("child ok")
"""


@pytest.mark.parametrize("env", [{"POPPY_HIP_DL_EVENTS": "1", "POPPY_HIP_RING": "1"}, {"POPPY_HIP_RING": "1"}, {"POPPY_HIP_RING": "8"}],
                         ids=["events_ring1", "ring1", "ring8"])
def test_every_format_through_the_ring_in_a_child_process(env):
    base = {k: v for k, v in os.environ.items() if k not in ("POPPY_HIP_DL_EVENTS", "POPPY_HIP_DL_DEVWAIT", "POPPY_HIP_RING", "POPPY_HIP_SLOTS")}
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=dict(base, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
