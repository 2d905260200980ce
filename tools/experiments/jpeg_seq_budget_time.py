"""POPPY_FRAME_JPEG under a sequence budget (poppy_hip_set_jpeg_sequence_budget) at 1080p on one context, ONE process (processes differ by +-10 %: DESIGN.md
section 4): 60 chained frames of a resident pair, handed to a writer that reads every frame's length.

Per pair (the tool's synthetic pair, the photograph pair tiled to 1080p), four settings alternating run by run, `--warm` rounds dropped, `--runs` rounds kept:
    fixed          POPPY_FRAME_JPEG at the default quality
    frame_budget   POPPY_FRAME_JPEG with the per-frame budget B / 60
    seq_budget     POPPY_FRAME_JPEG with the sequence budget B
    jpeg_seq       POPPY_FRAME_JPEG_SEQ (one table set per sequence, fixed quality)
with B = `--fraction` of the 60 files' bytes at the default quality.  Reported:
  * frames/s of the whole call — the host clock around render_many with a writer and a synchronise behind it —: the median and the extremes;
  * the GPU time of the search — jpeg_measure + jpeg_pick of timing mode 1, all steps — per frame, for the per-frame budget and for the sequence budget, with the
    launches of each per frame (the marks serialise the streams: kernel times, not rates);
  * the qualities the per-frame budget picks at B / 60 (lowest, median, highest, how many different) against the one quality picked here, and the bytes of B each
    leaves unused.
--parent-lib PATH --parent-capi PATH: the per-frame budget also on another build of the library through ITS binding (the parent commit's libpoppy_hip.so and
capi.py, built beside this tree), alternating with this build's run by run in the same process, its search's GPU time beside it: the comparison the search's cost is
judged by.

    python tools/experiments/jpeg_seq_budget_time.py [--runs 9] [--warm 2] [--pairs synthetic,photo] [--fraction 0.5] [--parent-lib P --parent-capi C]
One JSON line at the end; needs an MI355X (there is no fallback).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from poppy_amd import capi  # noqa: E402
from jpeg_budget_time import N, Q, W, H, pairs_of, parent_binding, rate, timed_run  # noqa: E402

SEARCH = ("jpeg_measure", "jpeg_pick")


def search_time(ctx, shapes):
    """the search's kernels in timing mode 1: GPU microseconds per frame (all steps), launches per frame"""
    ctx.set_timing(1)
    ctx.timing_summary()
    ctx.reset(); ctx.render_many(shapes, chain=True, write=lambda f: None)
    t = {n: (ms, k) for n, ms, k in ctx.timing_summary() if n in SEARCH}
    ctx.set_timing(0)
    return {"us_per_frame": round(sum(ms for ms, _ in t.values()) / N * 1e3, 2), "launches_per_frame": round(sum(k for _, k in t.values()) / N, 2),
            "by_kernel_us_per_frame": {n: round(ms / N * 1e3, 2) for n, (ms, _) in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--pairs", default="synthetic,photo")
    ap.add_argument("--fraction", type=float, default=0.5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-capi")
    a = ap.parse_args()
    a.warm = max(a.warm, 1)                                         # (the first round reads the qualities back and is never kept)
    shapes = np.array([capi.lib().poppy_frame_ratio(j, N, -1.0) for j in range(N)])
    ctx = capi.Context(0, number_of_frames=N)
    parent = parent_ctx = None
    if a.parent_lib:
        parent = parent_binding(a.parent_lib, a.parent_capi or os.path.join(ROOT, "poppy_amd", "capi.py"))
        parent_ctx = parent.Context(0, number_of_frames=N)
        parent_ctx.set_frame_format(parent.FRAME_JPEG)

    def apply(setting, budget):
        ctx.set_jpeg_budget(0); ctx.set_jpeg_sequence_budget(0)
        ctx.set_frame_format(capi.FRAME_JPEG_SEQ if setting == "jpeg_seq" else capi.FRAME_JPEG)
        if setting == "frame_budget":
            ctx.set_jpeg_budget(budget // N)
        elif setting == "seq_budget":
            ctx.set_jpeg_sequence_budget(budget)

    out = {"frames": N, "size": [W, H], "quality": Q, "runs": a.runs, "warm": a.warm, "fraction": a.fraction, "pairs": {}}
    for name, (x, y) in pairs_of(a.pairs.split(",")).items():
        ctx.pair_begin(x, y)
        if parent_ctx:
            parent_ctx.pair_begin(x, y)
        apply("fixed", 0)
        _, sizes_fixed, _ = timed_run(ctx, shapes)
        budget = int(a.fraction * sum(s - 4 for s in sizes_fixed))
        settings = ("fixed", "frame_budget", "seq_budget", "jpeg_seq")
        secs = {s: [] for s in settings}
        secs_parent = []
        sizes, used = {}, {}
        for rep in range(a.warm + a.runs):                          # the settings alternate run by run; the first rounds are dropped
            for s in settings:
                apply(s, budget)
                if rep == 0:                                        # (a warm round: reading the qualities back costs the writer time)
                    _, sizes[s], used[s] = timed_run(ctx, shapes, capi.jpeg_frame_quality)
                    continue
                t, sz, _ = timed_run(ctx, shapes)
                assert sz == sizes[s], "a frame is a pure function of its sequence and the settings"
                if rep >= a.warm:
                    secs[s].append(t)
            if parent_ctx:
                parent_ctx.set_jpeg_budget(budget // N)
                t, sz, _ = timed_run(parent_ctx, shapes)
                assert sz == sizes["frame_budget"], "the parent's frames under the per-frame budget have other lengths"
                if rep >= a.warm:
                    secs_parent.append(t)
        res = {"budget": budget, "files_bytes_at_fixed_quality": sum(s - 4 for s in sizes_fixed)}
        for s in settings:
            apply(s, budget)
            q = used[s]
            res[s] = {"frames_per_s": rate(secs[s]), "call_ms_median": round(statistics.median(secs[s]) * 1e3, 2), "files_bytes": sum(v - 4 for v in sizes[s]),
                      "qualities": {"min": min(q), "median": int(statistics.median(q)), "max": max(q), "different": len(set(q))}}
            if s in ("frame_budget", "seq_budget"):
                res[s]["bytes_unused"] = budget - res[s]["files_bytes"]
                res[s]["search_timing_mode1"] = search_time(ctx, shapes)
        if parent_ctx:
            res["parent_frame_budget"] = {"frames_per_s": rate(secs_parent), "search_timing_mode1": search_time(parent_ctx, shapes)}
        apply("fixed", 0)
        print(name, json.dumps(res), flush=True)
        out["pairs"][name] = res
    ctx.close()
    if parent_ctx:
        parent_ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
