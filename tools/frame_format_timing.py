"""BGR against I420 against PAL8 against PAL8_SEQ against GIF against JPEG against JPEG444 against PNG against PNG_RUNS against PNG_OPT frame hand-off (poppy_hip_set_frame_format), alternated in ONE process: processes differ by up to +-10 %, so every run
times each row once per format, one format right after the other, and the rows report min / median / max over --runs runs.

  pool_1080p    bench.py's `value` set-up: a pool of --contexts contexts, --steps queued batches of six 1080p pairs from device images, 60 chained
                frames per pair to the library's counting writer (pinned host copies)
  pool_4k       the same at 3840 x 2160 (--steps-4k batches)
  job480        ONE 480-frame 1080p phase-mode job on one context: pair set-up from device images + poppy_hip_render_phases to the counting writer
  chained       one context, pair after pair: pair set-up + 60 chained frames to the counting writer
  chained_4k    the same at 3840 x 2160 on a context of its own (not among the default --rows)
  chained_frame one context, the 60 chained frames of a resident pair to the counting writer (what the extra launch costs a chained frame)
  d2h_ceiling   pinned device-to-host copies of one frame's bytes, back to back on one stream (BGR, I420 and PAL8 sizes at 1080p and 4K)
and, at the end, the conversion kernels' own times in timing mode 1 at 1080p and 4K (I420: frame_format; PAL8: pal8_hist, pal8_build, frame_format = the index plane;
PAL8_SEQ: pal8_seq_hist per frame, pal8_seq_build per sequence, frame_format = the index plane; GIF: PAL8's three, then gif_lzw and gif_pack; JPEG: I420's frame_format, then
jpeg_code and jpeg_pack; JPEG444: frame_format = the I444 conversion, then the same two; PNG, PNG_RUNS and PNG_OPT: png_filter, png_cost, png_scan, png_pack, png_crc, png_finish — under PNG_RUNS png_cost and png_pack are the run-aware kernels, under PNG_OPT the ones that build and use the segments' own tables), and for the coded formats the median length of the 60 chained frames of the synthetic, of a textured and of a photograph pair (the golden 720 x 405 photographs, tiled; coded_bytes_median, with the coders' times on those frames; JPEG at --jpeg-quality).  Under PAL8_SEQ a pair's (a call's) frames are handed over after its last
frame.

    python tools/frame_format_timing.py [--runs 3 --steps 8 --steps-4k 3 --contexts 6 --formats bgr,i420,pal8,pal8_seq,gif,jpeg,jpeg444,png,png_runs,jpeg_opt,jpeg444_opt,png_opt --scales 1,2 --kernel-scales 2,4
                                         --size 1280x720 --size-4k 1920x1080]
--formats leaves formats out (a library older than GIF: bgr,i420,pal8,pal8_seq; older than JPEG: without jpeg; older than JPEG444: without jpeg444; older than PNG: without png; older than PNG_RUNS: without png_runs; older than PNG_OPT: without png_opt; older than JPEG_OPT: without jpeg_opt,jpeg444_opt — the formats on per-frame Huffman tables, whose marks are jpeg_count, jpeg_tables, jpeg_code, jpeg_pack).  --scales adds every format again per scale above 1 (poppy_hip_set_frame_scale: the
column "gif@2" is GIF at scale 2), alternated with the others in the same process; --kernel-scales adds k_bgr_downscale's own time (timing mode 1: frame_scale) under BGR
at 1080p and 4K for those factors.  --size OWxOH adds every format again at that size (poppy_hip_set_frame_size: the column "i420@1280x720"); the 4K rows of such a
column use --size-4k (default: --size), and its timing mode 1 entry has the resize kernel's time (frame_resize).  GIF's d2h_ceiling entry is its CAPACITY (poppy_frame_bytes); a frame's copy moves its own
length, which depends on the content.  jpeg_seq and jpeg444_seq (POPPY_FRAME_JPEG_SEQ, POPPY_FRAME_JPEG444_SEQ: one table set per sequence) and png_seq (POPPY_FRAME_PNG_SEQ: one ninth deflate
table per sequence; its marks are png_filter, png_seq_count, png_seq_table, png_seq_cost, png_scan, png_seq_pack, png_crc, png_finish) are columns only when --formats names them:
under them a row's call hands its writer nothing before its last frame is rendered, and job480 is one sequence of 480 frames.  One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poppy_amd import capi, synth  # noqa: E402

ALL_FMTS = (("bgr", capi.FRAME_BGR), ("i420", capi.FRAME_I420), ("pal8", capi.FRAME_PAL8), ("pal8_seq", capi.FRAME_PAL8_SEQ), ("gif", capi.FRAME_GIF), ("jpeg", capi.FRAME_JPEG),
            ("jpeg444", capi.FRAME_JPEG444), ("png", getattr(capi, "FRAME_PNG", 1024)), ("png_runs", getattr(capi, "FRAME_PNG_RUNS", 2048)),
            ("jpeg_opt", getattr(capi, "FRAME_JPEG_OPT", 4096)), ("jpeg444_opt", getattr(capi, "FRAME_JPEG444_OPT", 8192)), ("png_opt", getattr(capi, "FRAME_PNG_OPT", 16384)),
            ("jpeg_seq", getattr(capi, "FRAME_JPEG_SEQ", 32768)), ("jpeg444_seq", getattr(capi, "FRAME_JPEG444_SEQ", 65536)),
            ("png_seq", getattr(capi, "FRAME_PNG_SEQ", 131072)))      # (the sequence formats of JPEG and PNG are not among the default --formats)


PNG_MARKS = ("png_filter", "png_cost", "png_scan", "png_pack", "png_crc", "png_finish", "png_seq_count", "png_seq_table", "png_seq_cost", "png_seq_pack")
PHOTOS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "photo_pair_720x405.npz")


def pair_images(torch, dev, w, h, n):
    out = []
    for k in range(n):
        a = np.ascontiguousarray(synth.gen(w, h, 1234 + k, 0, 0)); b = np.ascontiguousarray(synth.gen(w, h, 1234 + k, w // 60 + k, h // 90))
        out.append((torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)))
    torch.cuda.synchronize()
    return out


def pool_row(pool, ptrs, w, h, steps, torch):
    pool.morph_pairs_device_counted(ptrs, w, h, -1.0)              # warm (and the first pairs of this format's buffers)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        pool.submit_pairs_device_counted(ptrs, w, h, -1.0)
    n = pool.wait()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def d2h(torch, dev, nbytes, reps=200):
    d = torch.empty(nbytes, dtype=torch.uint8, device=dev); d.fill_(7)
    hbuf = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    hbuf.copy_(d, non_blocking=True); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        hbuf.copy_(d, non_blocking=True)
    e1.record(); torch.cuda.synchronize()
    s = e0.elapsed_time(e1) / 1e3
    return {"GBps": round(nbytes * reps / s / 1e9, 2), "frames_per_s_cap": round(reps / s, 1)}


def summary(xs):
    return {"min": round(min(xs), 1), "median": round(statistics.median(xs), 1), "max": round(max(xs), 1), "runs": [round(x, 1) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--steps-4k", type=int, default=3)
    ap.add_argument("--contexts", type=int, default=6)
    ap.add_argument("--rows", default="pool_1080p,pool_4k,job480,chained,chained_frame,d2h_ceiling")
    ap.add_argument("--formats", default="bgr,i420,pal8,pal8_seq,gif,jpeg,jpeg444,png,png_runs,jpeg_opt,jpeg444_opt,png_opt")
    ap.add_argument("--jpeg-quality", type=int, default=capi.JPEG_QUALITY_DEFAULT)
    ap.add_argument("--scales", default="1")
    ap.add_argument("--kernel-scales", default="")
    ap.add_argument("--size", default="")
    ap.add_argument("--size-4k", default="")
    a = ap.parse_args()
    rows = a.rows.split(",")
    scales = [int(x) for x in a.scales.split(",")]
    # a column is a format at a scale; scale 1 keeps the format's plain name and never calls the scale setter
    # ... and a size column is a format at (the size of the 1080p rows, the size of the 4K rows): a tuple where the others have their scale
    size = tuple(int(x) for x in a.size.split("x")) if a.size else None
    size4k = tuple(int(x) for x in a.size_4k.split("x")) if a.size_4k else size
    FMTS = tuple((f if sc == 1 else f"{f}@{sc}" if isinstance(sc, int) else f"{f}@{a.size}", (v, sc)) for f, v in ALL_FMTS if f in a.formats.split(",")
                 for sc in scales + ([(size, size4k)] if size else []))

    def set_scaling(target, sc, four_k=False):
        sized = not isinstance(sc, int)
        if size and not sized:
            target.set_frame_size(0, 0)                            # size and scale are alternatives: the one off before the other goes on
        if scales != [1] or sized:
            target.set_frame_scale(1 if sized else sc)
        if sized:
            target.set_frame_size(*sc[1 if four_k else 0])

    def set_column(target, col, four_k=False):
        fmt, sc = col
        target.set_frame_format(fmt)
        set_scaling(target, sc, four_k)

    def writer_size(w, h, sc):
        return (-(-w // sc), -(-h // sc)) if isinstance(sc, int) else sc[1 if w > W else 0]
    import torch
    dev = torch.device("cuda", 0)
    res = {r: {f: [] for f, _ in FMTS} for r in rows if r != "d2h_ceiling"}
    W, H = 1920, 1080
    p1080 = pair_images(torch, dev, W, H, 6)
    ptrs = [(x.data_ptr(), y.data_ptr()) for x, y in p1080]
    pool = capi.Pool([0], contexts_per_device=a.contexts, number_of_frames=60) if "pool_1080p" in rows else None
    p4k = pair_images(torch, dev, 3840, 2160, 6) if "pool_4k" in rows or "chained_4k" in rows else None
    pool4 = capi.Pool([0], contexts_per_device=a.contexts, number_of_frames=60) if "pool_4k" in rows else None
    ctx4 = capi.Context(0, number_of_frames=60) if "chained_4k" in rows else None
    ctx = capi.Context(0, number_of_frames=60)
    if {"jpeg", "jpeg444", "jpeg_opt", "jpeg444_opt", "jpeg_seq", "jpeg444_seq"} & set(a.formats.split(",")):
        for target in (pool, pool4, ctx4, ctx):
            if target:
                target.set_jpeg_quality(a.jpeg_quality)
    ta, tb = p1080[0]
    ph480 = np.arange(480) / 480.0
    shapes = np.array([capi.lib().poppy_frame_ratio(j, 60, -1.0) for j in range(60)])
    for run in range(a.runs):
        for name, fmt in FMTS:
            if pool:
                set_column(pool, fmt)
                res["pool_1080p"][name].append(pool_row(pool, ptrs, W, H, a.steps, torch))
            if pool4:
                set_column(pool4, fmt, four_k=True)
                res["pool_4k"][name].append(pool_row(pool4, [(x.data_ptr(), y.data_ptr()) for x, y in p4k], 3840, 2160, a.steps_4k, torch))
            set_column(ctx, fmt)
            if "job480" in rows:
                ctx.pair_begin_device(ta.data_ptr(), tb.data_ptr(), W, H); ctx.render_phases(ph480, counted=True); ctx.sync()
                t0 = time.perf_counter()
                for _ in range(3):
                    ctx.pair_begin_device(ta.data_ptr(), tb.data_ptr(), W, H)
                    n = ctx.render_phases(ph480, counted=True)
                ctx.sync()
                res["job480"][name].append(3 * n / (time.perf_counter() - t0))
            if "chained" in rows:
                t0 = time.perf_counter(); n = 0
                for x, y in p1080:
                    ctx.pair_begin_device(x.data_ptr(), y.data_ptr(), W, H)
                    n += ctx.morph_frames_counted(-1.0)
                ctx.sync()
                res["chained"][name].append(n / (time.perf_counter() - t0))
            if ctx4:
                set_column(ctx4, fmt, four_k=True)
                t0 = time.perf_counter(); n = 0
                for x, y in p4k[:3]:
                    ctx4.pair_begin_device(x.data_ptr(), y.data_ptr(), 3840, 2160)
                    n += ctx4.morph_frames_counted(-1.0)
                ctx4.sync()
                res["chained_4k"][name].append(n / (time.perf_counter() - t0))
            if "chained_frame" in rows:
                ctx.pair_begin_device(ta.data_ptr(), tb.data_ptr(), W, H)
                ctx.reset(); ctx.render_many_counted(shapes, chain=True); ctx.sync()
                t0 = time.perf_counter()
                for _ in range(10):
                    ctx.reset(); ctx.render_many_counted(shapes, chain=True)
                ctx.sync()
                res["chained_frame"][name].append(600 / (time.perf_counter() - t0))
        print(f"run {run}: " + ", ".join(f"{r} {f} {v[f][-1]:.0f}" for r, v in res.items() for f in v), flush=True)
    out = {"unit": "frames/s", "rows": {r: {f: summary(v) for f, v in fv.items()} for r, fv in res.items()}}
    for r, fv in res.items():
        for f in (f for f, _ in FMTS if f != "bgr" and "bgr" in fv):
            out["rows"][r][f + "_over_bgr_median"] = round(statistics.median(fv[f]) / statistics.median(fv["bgr"]), 3)
    if "d2h_ceiling" in rows:
        out["d2h_ceiling"] = {f"{w}x{h}_{f}": d2h(torch, dev, capi.frame_bytes(fmt, *writer_size(w, h, sc))) for w, h in ((1920, 1080), (3840, 2160)) for f, (fmt, sc) in FMTS}
    # the conversion kernels in timing mode 1 (events around every kernel of a chained frame): time per launch
    out["timing_mode1_us"] = {}
    for (w, h), (x, y) in (((W, H), (ta, tb)),) + ((((3840, 2160), p4k[0]),) if p4k else ()):      # (the 1080p context takes the 4K pair here)
        kernel_cols = tuple((f"bgr@{k}", (capi.FRAME_BGR, int(k))) for k in a.kernel_scales.split(",") if k)
        for name, fmt in tuple(c for c in FMTS if c[1] != (capi.FRAME_BGR, 1)) + kernel_cols:
            ctx.set_frame_format(fmt[0])
            if size:
                ctx.set_frame_size(0, 0)                           # (the pair first: the size of the other geometry's rows may not be admissible for it)
            if fmt[1] != 1 or scales != [1]:
                ctx.set_frame_scale(fmt[1] if isinstance(fmt[1], int) else 1)
            ctx.pair_begin_device(x.data_ptr(), y.data_ptr(), w, h)
            if not isinstance(fmt[1], int):
                ctx.set_frame_size(*fmt[1][1 if w > W else 0])
            ctx.set_timing(1)
            ctx.reset(); ctx.render_many_counted(shapes, chain=True)
            t = {n: (ms, k) for n, ms, k in ctx.timing_summary()}
            ctx.set_timing(0)
            out["timing_mode1_us"][f"{w}x{h}_{name}"] = {n: round(ms / k * 1e3, 2) for n, (ms, k) in t.items() if n in ("unsharp", "frame_scale", "frame_resize", "frame_format", "pal8_hist", "pal8_build", "pal8_seq_hist", "pal8_seq_build", "gif_lzw", "gif_pack", "jpeg_count", "jpeg_tables", "jpeg_code", "jpeg_pack") + PNG_MARKS}
    # the coded formats' frame lengths: the 60 chained frames of the synthetic pair and of a textured pair, collected
    out["coded_bytes_median"] = {}
    coded = tuple(c for c in FMTS if c[1][0] in capi.FRAMES_CODED and c[1][1] == 1)
    for (w, h), (x, y) in ((((W, H), (ta, tb)),) + ((((3840, 2160), p4k[0]),) if p4k else ())) if coded else ():
        tex = [torch.from_numpy(np.ascontiguousarray(np.tile(synth.textured_bgr(960, 540, sd), (h // 540, w // 960, 1)))).to(dev) for sd in (41, 42)]
        for name, fmt in coded:
            set_column(ctx, fmt, four_k=w > W)
            pairs = [("synthetic", (x, y)), ("textured", tex)]
            if os.path.exists(PHOTOS):
                z = np.load(PHOTOS)
                pairs.append(("photo", [torch.from_numpy(np.ascontiguousarray(np.tile(z[k], (-(-h // 405), -(-w // 720), 1))[:h, :w])).to(dev) for k in ("a", "b")]))
            for pair, (u, v) in pairs:
                sizes = []
                ctx.pair_begin_device(u.data_ptr(), v.data_ptr(), w, h)
                ctx.set_timing(1)
                ctx.reset(); ctx.render_many(shapes, chain=True, write=lambda f: sizes.append(int(f.size)))
                t = {n: round(ms / k * 1e3, 2) for n, ms, k in ctx.timing_summary() if n in ("gif_lzw", "gif_pack", "jpeg_count", "jpeg_tables", "jpeg_code", "jpeg_pack") + PNG_MARKS}
                ctx.set_timing(0)
                out["coded_bytes_median"][f"{w}x{h}_{name}_{pair}"] = {"bytes": int(statistics.median(sizes)), "kernels_us": t}
    for p in (pool, pool4, ctx4):
        if p:
            p.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
