"""POPPY_FRAME_GIF_SEQ at 1080p on one context, ONE process (processes differ by +-10 %: DESIGN.md section 4), 60 chained frames of a resident pair.

  1. timing mode 1: the coder's marks under GIF_SEQ in its two forms, alternating sequence by sequence — the fused k_gif_lzw_bgr (`gif_lzw`) against the two-dispatch
     form, k_pal8_remap into an index plane and k_gif_lzw on it (`frame_format` + `gif_lzw`).  The second form exists only in the experiments build
     (`python -m poppy_amd.build --experiments`, POPPY_HIP_LIB=poppy_amd/libpoppy_hip_experiments.so), where POPPY_GIF_SEQ_TWO_DISPATCH is read per sequence; on the
     shipped library that half is left out.  On the tool's synthetic pair (tools/frame_format_timing.py) and on a textured pair.
  2. frames/s of the whole sequence to a writer that discards, under GIF_SEQ, PAL8_SEQ and GIF, alternating, and PAL8 beside them (what chained PAL8_SEQ runs below).
  3. host arithmetic, no GPU: the file of the 60-frame 256 x 192 chain (tests/test_host_gif_coded.py's input) under POPPY_SINK_GIF_GLOBAL_CODED, POPPY_SINK_GIF_CODED,
     POPPY_SINK_GIF_GLOBAL and POPPY_SINK_GIF (--sizes; needs oracle/liboracle.so).

    python tools/experiments/gif_seq_timing.py [--repeats 5] [--sizes]
One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from poppy_amd import capi, synth  # noqa: E402

W, H, N = 1920, 1080, 60
MARKS = ("pal8_seq_hist", "pal8_seq_build", "frame_format", "gif_lzw", "gif_pack")


def synthetic_pair():
    return synth.gen(W, H, 1234, 0, 0), synth.gen(W, H, 1234, W // 60, H // 90)


def textured_pair():
    def tiled(seed):
        t = synth.textured_bgr(960, 540, seed)
        return np.ascontiguousarray(np.tile(t, (2, 2, 1)))
    return tiled(41), tiled(42)


def load(ctx, pair, name):
    a, b = pair
    if name == "synthetic":
        ctx.pair_begin(a, b)
        return
    rng = np.random.default_rng(W * 7919 + H)
    p1 = np.stack([rng.uniform(0, W - 1, 40), rng.uniform(0, H - 1, 40)], 1).astype(np.float32)
    p2 = np.clip(p1 + rng.normal(0, 4.0, (40, 2)), 0, [W - 1, H - 1]).astype(np.float32)
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.float32)
    ctx.pair_load(a, b, synth.unit_field(W, H, 7), np.concatenate([p1, corners]), np.concatenate([p2, corners]))


def marks_of(ctx, shapes):
    ctx.set_timing(1)
    ctx.reset(); ctx.render_many_counted(shapes, chain=True)
    t = {n: ms / k * 1e3 for n, ms, k in ctx.timing_summary() if n in MARKS}
    ctx.set_timing(0)
    return t


def sizes():
    from test_host_gif_coded import chained_256x192, write_sink
    frames = chained_256x192()
    h, w = frames[0].shape[:2]
    seq = capi.bgr_frames_to_pal8(np.stack(frames))
    pal8 = [capi.bgr_to_pal8(f) for f in frames]
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, sink, fr, stride in (("gif_global_coded", capi.SINK_GIF_GLOBAL_CODED, capi.bgr_frames_to_gif_frames(np.stack(frames)), 0),
                                       ("gif_coded", capi.SINK_GIF_CODED, [capi.pal8_to_gif_frame(p, w, h) for p in pal8], 0),
                                       ("gif_global", capi.SINK_GIF_GLOBAL, list(seq), w), ("gif", capi.SINK_GIF, pal8, w)):
            path = os.path.join(d, name + ".gif")
            assert write_sink(path, sink, fr, w, h, stride) == len(frames)
            out[name] = os.path.getsize(path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    out = {}
    if a.sizes:
        out["file_bytes_chained_256x192_x60"] = sizes()
        print(out, flush=True)
    if a.no_gpu:
        print(json.dumps(out))
        return
    experiments = "experiments" in os.path.basename(capi.SO_PATH)
    shapes = np.array([capi.lib().poppy_frame_ratio(j, N, -1.0) for j in range(N)])
    ctx = capi.Context(0, number_of_frames=N)
    out["library"] = os.path.basename(capi.SO_PATH)
    out["timing_mode1_us"] = {}
    out["frames_per_s"] = {}
    for name, pair in (("synthetic", synthetic_pair()), ("textured", textured_pair())):
        load(ctx, pair, name)
        ctx.set_frame_format(capi.FRAME_GIF_SEQ)
        ctx.reset(); ctx.render_many_counted(shapes, chain=True); ctx.sync()      # warm: buffers, rings, captured nothing
        forms = {"fused": []}
        if experiments:
            forms["two_dispatch"] = []
        for _ in range(a.repeats):
            for form in forms:
                os.environ.pop("POPPY_GIF_SEQ_TWO_DISPATCH", None)
                if form == "two_dispatch":
                    os.environ["POPPY_GIF_SEQ_TWO_DISPATCH"] = "1"
                forms[form].append(marks_of(ctx, shapes))
        os.environ.pop("POPPY_GIF_SEQ_TWO_DISPATCH", None)
        out["timing_mode1_us"][name] = {form: {m: [round(r[m], 2) for r in runs if m in r] for m in MARKS if any(m in r for r in runs)} for form, runs in forms.items()}
        print(name, json.dumps(out["timing_mode1_us"][name]), flush=True)
        rates = {f: [] for f in ("gif_seq", "pal8_seq", "gif", "pal8")}
        fmts = {"gif_seq": capi.FRAME_GIF_SEQ, "pal8_seq": capi.FRAME_PAL8_SEQ, "gif": capi.FRAME_GIF, "pal8": capi.FRAME_PAL8}
        for rep in range(a.repeats + 1):                            # (the first round warms every format's buffers and is dropped)
            for f, fmt in fmts.items():
                ctx.set_frame_format(fmt)
                ctx.reset(); ctx.sync()
                t0 = time.perf_counter()
                for _ in range(3):
                    ctx.reset(); n = ctx.render_many_counted(shapes, chain=True)
                ctx.sync()
                if rep:
                    rates[f].append(3 * N / (time.perf_counter() - t0))
        out["frames_per_s"][name] = {f: {"min": round(min(v), 1), "median": round(statistics.median(v), 1), "max": round(max(v), 1)} for f, v in rates.items()}
        print(name, json.dumps(out["frames_per_s"][name]), flush=True)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
