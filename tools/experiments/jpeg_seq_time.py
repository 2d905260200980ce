"""POPPY_FRAME_JPEG_SEQ / JPEG444_SEQ against JPEG and JPEG_OPT at 1080p on one context, ONE process (processes differ by +-10 %: DESIGN.md section 4):
60 chained frames of a resident pair, handed to a writer that reads every frame's length.

Per pair (the tool's synthetic pair, a textured pair, the photograph pair tiled to 1080p) and per family (4:2:0: JPEG, JPEG_OPT, JPEG_SEQ; 4:4:4 likewise):
  * frames/s of the whole call — the host clock around render_many with a writer and a synchronise behind it —, the three formats alternating run by run,
    `--warm` rounds dropped, `--runs` rounds kept: the median, the extremes, and the ratio of medians to the family's JPEG;
  * the call's time and the time until the writer's first call (under a sequence format: every frame rendered and counted, the tables built, frame 0 coded; what is
    left of the call is the hand-over loop coding and copying the other 59);
  * bytes per frame, the median over the 60 frames, and per sequence;
  * the jpeg_count, jpeg_tables, jpeg_code and jpeg_pack times of timing mode 1, in a run of its own (the marks serialise the streams; these are kernel times, not rates),
    per frame, and jpeg_tables per call as well.

    python tools/experiments/jpeg_seq_time.py [--runs 15] [--warm 3] [--pairs synthetic,textured,photo]
One JSON line at the end; needs an MI355X (there is no fallback).
"""
import argparse
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
MARKS = ("frame_format", "jpeg_count", "jpeg_tables", "jpeg_code", "jpeg_pack")
FAMILIES = {"420": (("jpeg", capi.FRAME_JPEG), ("jpeg_opt", capi.FRAME_JPEG_OPT), ("jpeg_seq", capi.FRAME_JPEG_SEQ)),
            "444": (("jpeg444", capi.FRAME_JPEG444), ("jpeg444_opt", capi.FRAME_JPEG444_OPT), ("jpeg444_seq", capi.FRAME_JPEG444_SEQ))}
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


def timed_run(ctx, shapes):
    """(seconds, seconds until the writer's first call, the frames' lengths) of one call: 60 chained frames to a writer, synchronised"""
    sizes, first = [], []

    def write(f):
        if not sizes:
            first.append(time.perf_counter())
        sizes.append(int(f.size))
    ctx.reset(); ctx.sync()
    t0 = time.perf_counter()
    ctx.render_many(shapes, chain=True, write=write)
    ctx.sync()
    return time.perf_counter() - t0, first[0] - t0, sizes


def marks_of(ctx, shapes):
    ctx.set_timing(1)
    ctx.reset(); ctx.render_many(shapes, chain=True, write=lambda f: None)
    t = {n: (ms, k) for n, ms, k in ctx.timing_summary() if n in MARKS}
    ctx.set_timing(0)
    out = {n: round(ms / k * 1e3, 2) for n, (ms, k) in t.items()}
    if "jpeg_tables" in t:
        out["jpeg_tables_calls"] = t["jpeg_tables"][1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--pairs", default="synthetic,textured,photo")
    a = ap.parse_args()
    shapes = np.array([capi.lib().poppy_frame_ratio(j, N, -1.0) for j in range(N)])
    ctx = capi.Context(0, number_of_frames=N)
    out = {"frames": N, "size": [W, H], "runs": a.runs, "warm": a.warm, "pairs": {}}
    for name, (x, y) in pairs_of(a.pairs.split(",")).items():
        ctx.pair_begin(x, y)
        res = {}
        for family, fmts in FAMILIES.items():
            secs, until_first = {f: [] for f, _ in fmts}, {f: [] for f, _ in fmts}
            sizes = {}
            for rep in range(a.warm + a.runs):                      # the formats alternate run by run; the first rounds warm every format's buffers and are dropped
                for f, fmt in fmts:
                    ctx.set_frame_format(fmt)
                    s, s_first, sz = timed_run(ctx, shapes)
                    assert len(sz) == N
                    sizes[f] = sz
                    if rep >= a.warm:
                        secs[f].append(s)
                        until_first[f].append(s_first)
            base = statistics.median(secs[fmts[0][0]])
            for f, fmt in fmts:
                v = sorted(secs[f])
                ctx.set_frame_format(fmt)
                res[f] = {"frames_per_s": {"median": round(N / statistics.median(v), 1), "min": round(N / v[-1], 1), "max": round(N / v[0], 1)},
                          "ratio_to_" + fmts[0][0]: round(base / statistics.median(v), 3),
                          "call_ms_median": round(statistics.median(v) * 1e3, 2), "ms_until_the_writers_first_call_median": round(statistics.median(until_first[f]) * 1e3, 2),
                          "bytes_per_frame_median": int(statistics.median(sizes[f])), "bytes_per_sequence": int(sum(sizes[f])),
                          "timing_mode1_us": marks_of(ctx, shapes)}
            print(name, family, json.dumps({f: res[f] for f, _ in fmts}), flush=True)
        out["pairs"][name] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
