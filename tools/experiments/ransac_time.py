"""RANSAC fundamental-matrix filter: the host statement (poppy_ransac_fundamental) against the GPU form (poppy_hip_ransac_fundamental) at n = 64, 512
and 4096 point pairs (two views, a quarter planted outliers, d = 3), and the descriptor set-up without and with the filter on the 1080p synthetic pair.
Medians of --reps calls after --warmup calls, wall time of the whole call (uploads, both launches, download, choice, mask and refit included), on an
otherwise idle GPU.  One JSON line at the end.

    python tools/experiments/ransac_time.py [--reps 15 --warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ransac_util as U  # noqa: E402
from poppy_amd import capi, synth  # noqa: E402


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = capi.Context(0)
    out = {"reps": a.reps}
    for n in (64, 512, 4096):
        p1, p2, _ = U.quarter_outliers(n, n)
        host = median_ms(lambda: capi.ransac_fundamental(p1, p2, 3.0), a.reps, a.warmup)
        gpu = median_ms(lambda: ctx.ransac_fundamental(p1, p2, 3.0), a.reps, a.warmup)
        same = all(np.array_equal(x, y) for x, y in zip(capi.ransac_fundamental(p1, p2, 3.0).values(), ctx.ransac_fundamental(p1, p2, 3.0).values()))
        out[f"n{n}"] = {"host_ms": round(host, 3), "gpu_ms": round(gpu, 3), "same": bool(same)}
        print(f"n = {n:5d}: host statement {host:8.3f} ms, GPU form {gpu:8.3f} ms, same result: {same}", flush=True)
    img1, img2 = synth.gen_pair(1920, 1080, seed=1234)
    plain = median_ms(lambda: ctx.pair_begin_descriptors(img1, img2, 0.7), a.reps, a.warmup)
    n_plain = len(ctx.pair_points()[0]) - 4
    filtered = median_ms(lambda: ctx.pair_begin_descriptors_ransac(img1, img2, 0.7, 3.0), a.reps, a.warmup)
    f = ctx.pair_fundamental()
    out["setup_1080p"] = {"descriptors_ms": round(plain, 3), "descriptors_ransac_ms": round(filtered, 3), "pairs": n_plain, "pairs_into_filter": f["n_matches"],
                          "pairs_kept": f["n_inliers"], "best": f["best"]}
    print(f"1080p synthetic pair: pair_begin_descriptors {plain:.3f} ms ({n_plain} pairs), with the filter {filtered:.3f} ms "
          f"({f['n_matches']} -> {f['n_inliers']} pairs, hypothesis {f['best']})", flush=True)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
