"""Non-local-means denoise: poppy_hip_denoise_device at 1920 x 1080 for (hs, tw, sw) = (3, 7, 21), (10, 7, 21), (100, 7, 21) and (10, 3, 7) — a host clock
around the call and the stream synchronise behind it, device image in and out — the host statement poppy_bgr_denoise at 480 x 270 for scale, and a list of
four 1080p images through poppy_hip_morph_list (frames kept on the device) without and with poppy_hip_set_denoise(10, 7, 21).  Medians of --reps calls
after --warmup calls, on an otherwise idle GPU.  Every GPU result is compared with the host statement at 480 x 270 first.  One JSON line at the end.

    python tools/experiments/denoise_time.py [--reps 15 --warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from poppy_amd import capi, synth  # noqa: E402

PARAMS = [(3.0, 7, 21), (10.0, 7, 21), (100.0, 7, 21), (10.0, 3, 7)]


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def noisy(w, h, seed, dx=0, dy=0):
    noise = np.rint(6.0 * np.random.RandomState(seed).randn(h, w, 3))
    return np.clip(synth.gen(w, h, 1234, dx, dy).astype(np.float64) + noise, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = capi.Context(0, number_of_frames=60)
    hip = C.CDLL("libamdhip64.so")
    out = {"reps": a.reps}

    small = noisy(480, 270, 1)
    for p in PARAMS:
        host = median_ms(lambda: capi.bgr_denoise(small, *p), a.reps, a.warmup) if p == PARAMS[1] else None
        same = bool(np.array_equal(ctx.denoise(small, *p), capi.bgr_denoise(small, *p)))
        out[f"same_480x270_hs{p[0]:g}_{p[1]}_{p[2]}"] = same
        if host is not None:
            out["host_480x270_ms"] = round(host, 1)
            print(f"host statement, 480 x 270, {p}: {host:.1f} ms", flush=True)
        print(f"GPU == host statement at 480 x 270, {p}: {same}", flush=True)

    w, h = 1920, 1080
    img = noisy(w, h, 2)
    d_src, d_dst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_src), C.c_size_t(img.nbytes)) == 0 and hip.hipMalloc(C.byref(d_dst), C.c_size_t(img.nbytes)) == 0
    assert hip.hipMemcpy(d_src, img.ctypes.data_as(C.c_void_p), C.c_size_t(img.nbytes), 1) == 0

    def device_call(p):
        ctx.denoise_device(d_src.value, d_dst.value, w, h, *p)
        ctx.sync()
    for p in PARAMS:
        ms = median_ms(lambda: device_call(p), a.reps, a.warmup)
        out[f"device_1080p_hs{p[0]:g}_{p[1]}_{p[2]}_ms"] = round(ms, 3)
        print(f"poppy_hip_denoise_device, 1920 x 1080, {p}, L = {capi.denoise_weights(*p)['L']}: {ms:.3f} ms", flush=True)
    hip.hipFree(d_src); hip.hipFree(d_dst)

    images = [noisy(w, h, 10 + k, k * w // 50, k * w // 100) for k in range(4)]
    for name, setting in (("list_1080p_x4_ms", 0.0), ("list_1080p_x4_denoise_ms", 10.0)):
        ctx.set_denoise(setting, 7, 21)
        ms = median_ms(lambda: ctx.morph_list(images, collect=False), a.reps, a.warmup)
        out[name] = round(ms, 1)
        print(f"morph_list, four 1080p images, 60 frames per pair kept on the device, denoise {'off' if setting == 0 else '(10, 7, 21)'}: {ms:.1f} ms", flush=True)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
