"""POPPY_FRAME_PNG_SEQ against BGR, PNG, PNG_RUNS and PNG_OPT at 1080p on one context, ONE process (processes differ by +-10 %: DESIGN.md section 4):
60 chained frames of a resident pair.

Per pair (the tool's synthetic pair, a textured pair, the photograph pair tiled to 1080p) and per format:
  * frames/s of the whole call to a writer in Python that reads every frame's length, and to the library's counting writer (no Python per frame) — the host
    clock around render_many and a synchronise behind it —, the five formats alternating run by run, `--warm` rounds dropped, `--runs` rounds kept: the median,
    the extremes, and the ratio of medians to BGR's;
  * the time until the writer's first call (under PNG_SEQ: every frame rendered, filtered and counted, the table built, frame 0 coded; what is left of the call is
    the hand-over loop coding and copying the other 59);
  * bytes per frame, the median over the 60 frames, and per sequence;
  * the kernel times of timing mode 1 in a run of its own (the marks serialise the streams; these are kernel times, not rates), per frame, and png_seq_table per call;
  * the sequence store's bytes for the 60 frames (what the filtered streams and their coder words take: the library's own figure, png_scratch_bytes, restated).

    python tools/experiments/png_seq_time.py [--runs 11] [--warm 2] [--pairs synthetic,textured,photo] [--size 1920x1080]
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

N = 60
MARKS = ("png_filter", "png_cost", "png_scan", "png_pack", "png_crc", "png_finish", "png_seq_count", "png_seq_table", "png_seq_cost", "png_seq_pack")
FORMATS = (("bgr", capi.FRAME_BGR), ("png", capi.FRAME_PNG), ("png_runs", capi.FRAME_PNG_RUNS), ("png_opt", capi.FRAME_PNG_OPT), ("png_seq", capi.FRAME_PNG_SEQ))
PHOTOS = os.path.join(ROOT, "tests", "golden", "photo_pair_720x405.npz")


def pairs_of(names, W, H):
    out = {}
    if "synthetic" in names:
        out["synthetic"] = (synth.gen(W, H, 1234, 0, 0), synth.gen(W, H, 1234, W // 60, H // 90))
    if "textured" in names:
        out["textured"] = tuple(np.ascontiguousarray(np.tile(synth.textured_bgr(960, 540, sd), (-(-H // 540), -(-W // 960), 1))[:H, :W]) for sd in (41, 42))
    if "photo" in names:
        if not os.path.exists(PHOTOS):
            sys.exit(f"the photograph pair {PHOTOS} is missing: name the pairs to measure with --pairs, so that no table comes back short unnoticed")
        z = np.load(PHOTOS)
        out["photo"] = tuple(np.ascontiguousarray(np.tile(z[k], (-(-H // 405), -(-W // 720), 1))[:H, :W]) for k in ("a", "b"))
    unknown = set(names) - set(out)
    if unknown:
        sys.exit(f"unknown pairs: {sorted(unknown)}")
    return out


def timed_run(ctx, shapes, coded):
    """(seconds, seconds until the writer's first call, the frames' lengths) of one call: 60 chained frames to a writer in Python, synchronised"""
    sizes, first = [], []

    def write(f):
        if not sizes:
            first.append(time.perf_counter())
        sizes.append(int(f.size) if coded else int(f.nbytes))
    ctx.reset(); ctx.sync()
    t0 = time.perf_counter()
    ctx.render_many(shapes, chain=True, write=write)
    ctx.sync()
    return time.perf_counter() - t0, first[0] - t0, sizes


def counted_run(ctx, shapes):
    ctx.reset(); ctx.sync()
    t0 = time.perf_counter()
    n = ctx.render_many_counted(shapes, chain=True)
    ctx.sync()
    assert n == len(shapes)
    return time.perf_counter() - t0


def marks_of(ctx, shapes):
    ctx.set_timing(1)
    ctx.reset(); ctx.render_many(shapes, chain=True, write=lambda f: None)
    t = {n: (ms, k) for n, ms, k in ctx.timing_summary() if n in MARKS}
    ctx.set_timing(0)
    out = {n: round(ms / k * 1e3, 2) for n, (ms, k) in t.items()}
    if "png_seq_table" in t:
        out["png_seq_table_calls"] = t["png_seq_table"][1]
    return out


def store_bytes(W, H, n):
    """n places of the sequence store (kernels_frame_png.hip: png_scratch_bytes of the run formats, rounded up to 16)"""
    stream = H * (1 + 3 * W)
    seg = -(-stream // capi.PNG_SEGMENT_BYTES)
    crc = -(-capi.frame_bytes(capi.FRAME_PNG_SEQ, W, H) // 8192)
    place = seg * (capi.PNG_SEGMENT_BYTES + 16 + 8) + crc * 4 + 16 + 16
    return n * (-(-place // 16) * 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--pairs", default="synthetic,textured,photo")
    ap.add_argument("--size", default="1920x1080")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    shapes = np.array([capi.lib().poppy_frame_ratio(j, N, -1.0) for j in range(N)])
    ctx = capi.Context(0, number_of_frames=N)
    out = {"frames": N, "size": [W, H], "runs": a.runs, "warm": a.warm, "sequence_store_bytes": store_bytes(W, H, N), "pairs": {}}
    for name, (x, y) in pairs_of(a.pairs.split(","), W, H).items():
        ctx.pair_begin(x, y)
        secs, counted, until_first = ({f: [] for f, _ in FORMATS} for _ in range(3))
        sizes = {}
        for rep in range(a.warm + a.runs):                          # the formats alternate run by run; the first rounds warm every format's buffers and are dropped
            for f, fmt in FORMATS:
                ctx.set_frame_format(fmt)
                s, s_first, sz = timed_run(ctx, shapes, fmt != capi.FRAME_BGR)
                c = counted_run(ctx, shapes)
                assert len(sz) == N
                sizes[f] = sz
                if rep >= a.warm:
                    secs[f].append(s); counted[f].append(c); until_first[f].append(s_first)
        res = {}
        for f, fmt in FORMATS:
            v, c = sorted(secs[f]), sorted(counted[f])
            ctx.set_frame_format(fmt)
            res[f] = {"python_writer_frames_per_s": {"median": round(N / statistics.median(v), 1), "min": round(N / v[-1], 1), "max": round(N / v[0], 1)},
                      "python_writer_ratio_to_bgr": round(statistics.median(secs["bgr"]) / statistics.median(v), 3),
                      "counting_writer_frames_per_s": {"median": round(N / statistics.median(c), 1), "min": round(N / c[-1], 1), "max": round(N / c[0], 1)},
                      "counting_writer_ratio_to_bgr": round(statistics.median(counted["bgr"]) / statistics.median(c), 3),
                      "call_ms_median": round(statistics.median(v) * 1e3, 2), "ms_until_the_writers_first_call_median": round(statistics.median(until_first[f]) * 1e3, 2),
                      "bytes_per_frame_median": int(statistics.median(sizes[f])), "bytes_per_sequence": int(sum(sizes[f])),
                      "timing_mode1_us": marks_of(ctx, shapes) if fmt != capi.FRAME_BGR else {}}
            print(name, f, json.dumps(res[f]), flush=True)
        out["pairs"][name] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
