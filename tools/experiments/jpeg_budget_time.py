"""POPPY_FRAME_JPEG under a byte budget (poppy_hip_set_jpeg_budget) against JPEG at quality 90 at 1080p on one context, ONE process (processes differ by +-10 %:
DESIGN.md section 4): 60 chained frames of a resident pair, handed to a writer that reads every frame's length.

Per pair (the tool's synthetic pair, a textured pair, the photograph pair tiled to 1080p), three settings alternating run by run — budget off, a budget of 0.5 and
of 0.25 of the pair's median JPEG frame file at quality 90 —, `--warm` rounds dropped, `--runs` rounds kept:
  * frames/s of the whole call — the host clock around render_many with a writer and a synchronise behind it —: the median, the extremes, and the ratio of medians
    to budget off;
  * bytes per frame (the median over the 60 frames), the largest frame against the budget, and the qualities picked (lowest, median, highest);
  * the jpeg_measure, jpeg_pick, jpeg_code and jpeg_pack times of timing mode 1 per frame, in a run of its own (the marks serialise the streams; these are kernel
    times, not rates), and the launches of each per frame.
--parent-lib PATH --parent-capi PATH: budget off also on another build of the library through ITS binding (the parent commit's libpoppy_hip.so and capi.py, built
beside this tree), alternating with this build's run by run in the same process: the ratio says whether the fixed-quality path moved.

    python tools/experiments/jpeg_budget_time.py [--runs 15] [--warm 3] [--pairs synthetic,textured,photo] [--parent-lib P --parent-capi C]
One JSON line at the end; needs an MI355X (there is no fallback).
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from poppy_amd import capi, synth  # noqa: E402

W, H, N = 1920, 1080, 60
Q = capi.JPEG_QUALITY_DEFAULT
MARKS = ("frame_format", "jpeg_measure", "jpeg_pick", "jpeg_code", "jpeg_pack")
FRACTIONS = (0.5, 0.25)
PHOTOS = os.path.join(ROOT, "tests", "golden", "photo_pair_720x405.npz")


def pairs_of(names):
    out = {}
    if "synthetic" in names:
        out["synthetic"] = (synth.gen(W, H, 1234, 0, 0), synth.gen(W, H, 1234, W // 60, H // 90))
    if "textured" in names:
        out["textured"] = tuple(np.ascontiguousarray(np.tile(synth.textured_bgr(960, 540, sd), (2, 2, 1))) for sd in (41, 42))
    if "photo" in names:
        if not os.path.exists(PHOTOS):
            sys.exit(f"the photograph pair {PHOTOS} is missing: name the pairs to measure with --pairs, so that no table comes back short unnoticed")
        z = np.load(PHOTOS)
        out["photo"] = tuple(np.ascontiguousarray(np.tile(z[k], (-(-H // 405), -(-W // 720), 1))[:H, :W]) for k in ("a", "b"))
    unknown = set(names) - set(out)
    if unknown:
        sys.exit(f"unknown pairs: {sorted(unknown)}")
    return out


def parent_binding(lib_path, capi_path):
    """the other build's own binding, loaded beside this one's (a binding reads POPPY_HIP_LIB once, when it is imported)"""
    os.environ["POPPY_HIP_LIB"] = os.path.abspath(lib_path)
    try:
        spec = importlib.util.spec_from_file_location("parent_capi", capi_path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        del os.environ["POPPY_HIP_LIB"]
    return mod


def timed_run(ctx, shapes, quality_of=None):
    """(seconds, the frames' lengths, their qualities) of one call: 60 chained frames to a writer, synchronised"""
    sizes, used = [], []

    def write(f):
        sizes.append(int(f.size))
        if quality_of:
            used.append(quality_of(f))
    ctx.reset(); ctx.sync()
    t0 = time.perf_counter()
    ctx.render_many(shapes, chain=True, write=write)
    ctx.sync()
    return time.perf_counter() - t0, sizes, used


def marks_of(ctx, shapes):
    ctx.set_timing(1)
    ctx.reset(); ctx.render_many(shapes, chain=True, write=lambda f: None)
    t = {n: (ms, k) for n, ms, k in ctx.timing_summary() if n in MARKS}
    ctx.set_timing(0)
    return {n: {"us_per_frame": round(ms / N * 1e3, 2), "launches_per_frame": round(k / N, 2)} for n, (ms, k) in t.items()}


def rate(v):
    v = sorted(v)
    return {"median": round(N / statistics.median(v), 1), "min": round(N / v[-1], 1), "max": round(N / v[0], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--pairs", default="synthetic,textured,photo")
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-capi")
    ap.add_argument("--parent-first", action="store_true", help="create the other build's context before this build's (the second context of a process gets other hardware queues)")
    a = ap.parse_args()
    a.warm = max(a.warm, 1)                                         # (the first round reads the qualities back and is never kept)
    shapes = np.array([capi.lib().poppy_frame_ratio(j, N, -1.0) for j in range(N)])
    parent = parent_ctx = ctx = None
    for which in ((1, 0) if a.parent_first else (0, 1)):
        if which == 0:
            ctx = capi.Context(0, number_of_frames=N)
            ctx.set_frame_format(capi.FRAME_JPEG)
        elif a.parent_lib:
            parent = parent_binding(a.parent_lib, a.parent_capi or os.path.join(ROOT, "poppy_amd", "capi.py"))
            parent_ctx = parent.Context(0, number_of_frames=N)
            parent_ctx.set_frame_format(parent.FRAME_JPEG)
    out = {"frames": N, "size": [W, H], "quality": Q, "runs": a.runs, "warm": a.warm, "pairs": {}}
    for name, (x, y) in pairs_of(a.pairs.split(",")).items():
        ctx.pair_begin(x, y)
        if parent_ctx:
            parent_ctx.pair_begin(x, y)
        ctx.set_jpeg_budget(0)
        _, sizes_off, _ = timed_run(ctx, shapes)
        median_file = int(statistics.median(sizes_off)) - 4
        settings = [("off", 0)] + [(f"budget_{f}", int(f * median_file)) for f in FRACTIONS]
        secs = {s: [] for s, _ in settings}
        secs_parent = []
        sizes, used = {}, {}
        for rep in range(a.warm + a.runs):                          # the settings alternate run by run; the first rounds are dropped
            for s, b in settings:
                ctx.set_jpeg_budget(b)
                if rep == 0:                                        # (a warm round: reading the qualities back costs the writer time)
                    _, sizes[s], used[s] = timed_run(ctx, shapes, capi.jpeg_frame_quality)
                    continue
                t, sz, _ = timed_run(ctx, shapes)
                assert sz == sizes[s], "a frame is a pure function of its planes, the quality and the budget"
                if rep >= a.warm:
                    secs[s].append(t)
            if parent_ctx:
                t, sz, _ = timed_run(parent_ctx, shapes)
                assert sz == sizes["off"], "the parent's frames have other lengths"
                if rep >= a.warm:
                    secs_parent.append(t)
        base = statistics.median(secs["off"])
        res = {"median_jpeg_file_bytes": median_file}
        for s, b in settings:
            ctx.set_jpeg_budget(b)
            res[s] = {"budget": b, "frames_per_s": rate(secs[s]), "ratio_to_off": round(base / statistics.median(secs[s]), 3),
                      "call_ms_median": round(statistics.median(secs[s]) * 1e3, 2), "file_bytes_median": int(statistics.median(sizes[s])) - 4,
                      "file_bytes_max": max(sizes[s]) - 4, "qualities": [min(used[s]), int(statistics.median(used[s])), max(used[s])],
                      "timing_mode1": marks_of(ctx, shapes)}
        if parent_ctx:
            res["parent_off"] = {"frames_per_s": rate(secs_parent), "ratio_of_this_build_to_parent": round(statistics.median(secs_parent) / base, 3)}
        ctx.set_jpeg_budget(0)
        print(name, json.dumps(res), flush=True)
        out["pairs"][name] = res
    ctx.close()
    if parent_ctx:
        parent_ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
