"""Image-list timing: the CLI's loop over a list of images on ONE context (src/poppy.cpp:266-328), in two forms.

  pairs  pair after pair, each pair set up from scratch (poppy_hip_pair_begin_device + poppy_hip_morph_frames): bench.py's sequential_fps form
  list   poppy_hip_morph_list: pair 0 by pair_begin, every later pair by pair_begin_next (image 1's filter chain reused)

Both hand every frame to the library's counting writer (pinned host copies) and read the images from device memory.  Printed per form:
frames/s over --reps timed runs of the whole list (after one warm-up run), and the host gap between the end of pair k's last frame and the
start of pair k + 1's first frame (one extra run with a Python writer that stamps frames, median over the pairs).  One JSON line at the end.

    python tools/image_list_timing.py [--w 1920 --h 1080 --images 9 --frames 60 --reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppy_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--images", type=int, default=9)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import ctypes as C
    W, H, n = a.w, a.h, a.images
    ctx = capi.Context(0, number_of_frames=a.frames)
    hip = C.CDLL("libamdhip64.so")
    ptrs = []
    for k in range(n):                                           # the images in device memory, as a decoder on the GPU would leave them
        img = np.ascontiguousarray(synth.gen(W, H, 1234, k * W // 50, k * W // 100))
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(img.nbytes)) == 0
        assert hip.hipMemcpy(d, img.ctypes.data_as(C.c_void_p), C.c_size_t(img.nbytes), 1) == 0
        ptrs.append(d.value)

    def pairs():
        k = 0
        for i in range(n - 1):
            ctx.pair_begin_device(ptrs[i], ptrs[i + 1], W, H)
            k += ctx.morph_frames_counted(-1.0)
        return k

    def listed():
        rc, cnt, _, done = ctx.morph_list([(p, W, H) for p in ptrs], on_device=True, counted=True)
        assert rc == 0 and done == n - 1
        return cnt[0]

    def gap_ms(form):
        stamps = {}

        def wr(k, j, view):
            stamps.setdefault(k, []).append(time.perf_counter())
        if form == "list":
            ctx.morph_list([(p, W, H) for p in ptrs], on_device=True, write=wr)
        else:
            for i in range(n - 1):
                ctx.pair_begin_device(ptrs[i], ptrs[i + 1], W, H)
                ctx.render_many([capi.lib().poppy_frame_ratio(j, a.frames, -1.0) for j in range(a.frames)], chain=True,
                                write=lambda v, i=i: wr(i, 0, v))
        g = [(stamps[k + 1][0] - stamps[k][-1]) * 1e3 for k in range(n - 2)]
        return float(np.median(g))

    out = {"w": W, "h": H, "images": n, "frames_per_pair": a.frames}
    for name, fn in (("pairs", pairs), ("list", listed)):
        fn()                                                     # warm-up
        fps = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            k = fn()
            fps.append(k / (time.perf_counter() - t0))
        out[name + "_fps"] = [round(x, 1) for x in fps]
        out[name + "_gap_ms"] = round(gap_ms(name), 3)
        print(f"{name:6s} frames/s {' '.join(f'{x:8.1f}' for x in fps)}   gap between pairs (median) {out[name + '_gap_ms']:.3f} ms", flush=True)
    run, reused = ctx.chain_counts()
    out["chains_run"], out["chains_reused"] = run, reused
    ctx.close()
    for p in ptrs:
        hip.hipFree(C.c_void_p(p))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
