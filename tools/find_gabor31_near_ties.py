#!/usr/bin/env python3
"""Search two-dot 96 x 64 grey images for plane values of the 31 x 31 Gabor bank (ctx.orb_input) that lie within 1e-14 x amax of the
midpoint between two floats ("inside": the FFT form's doubt rule must catch them) or between 1.0 and 1.5 doubt bands from one
("outside": nothing catches them, the transform's accuracy alone keeps the two forms equal), amax = max(1, the largest |us| in the
tile's 64 x 64 patch), and write the rows into tests/gabor_ties_util.py (GABOR31_ROWS and the docstring's yield line).

The bank runs on us, the grey of the unsharp-masked image, so the values cannot be placed: they are found, with the oracle's double
planes (O.orb_unsharp_gray, O.gabor_planes) and the util's own classify and band31_map.  Deterministic: image n comes from seed n.
CPU only; about two minutes of CPU for the default 320 images.

    python tools/find_gabor31_near_ties.py [--images 320] [--keep 8] [--jobs 8] [--dry-run]"""
import argparse
import multiprocessing
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gabor_ties_util as U                                   # noqa: E402
import oracle_lib as O                                        # noqa: E402


def image(seed):
    """Two 3 x 3 dots (U.dots31): anywhere, borders included; half of the bytes 255 (us overshoots 1 around a white dot), the rest arbitrary."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, U.W31, 2); y = rng.integers(0, U.H31, 2)
    b = np.where(rng.integers(0, 2, 2) == 1, 255, rng.integers(1, 256, 2))
    return tuple(int(v) for v in (x[0], y[0], b[0], x[1], y[1], b[1]))


def search(seed):
    dots = image(seed)
    gf, _ = U.dots31(("", *dots, 0, 0, 0, 0.0))
    us = O.orb_unsharp_gray(gf)
    planes = O.gabor_planes(us, U.KS31, U.bank(U.KS31))       # (h, w, 16)
    band = U.band31_map(us)[..., None]
    c = U.classify(planes, band)
    live = (planes >= U.MIN_VALUE) & (planes < 1)
    dist = np.abs(c.mid)
    rows = []
    for kind, m in (("inside", live & (dist <= U.INSIDE * band / U.band_unit())), ("outside", live & (dist > band) & (dist <= 1.5 * band))):
        for ty, tx, o in zip(*np.nonzero(m)):
            if not U.visible(planes[ty, tx], o) or (kind == "outside" and c.doubt[ty, tx].any()):
                continue
            rows.append((kind, *dots, int(tx), int(ty), int(o), float(c.mid[ty, tx, o]), float(band[ty, tx, 0] / U.band_unit())))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=320)
    ap.add_argument("--keep", type=int, default=8, help="rows of each kind to keep")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    U.band_unit(); U.bank(U.KS31); O.lib()
    t0 = time.time()
    with multiprocessing.get_context("fork").Pool(a.jobs) as pool:
        found = [r for rows in pool.map(search, range(a.images), chunksize=8) for r in rows]
    wall = time.time() - t0
    kept, counts = [], {}
    for kind in ("inside", "outside"):
        rows = [r for r in found if r[0] == kind]
        counts[kind] = len(rows)
        # inside: the nearest first; outside: the nearest to the band's edge first; both sides of the midpoint and scaled bands (amax > 1) first in line
        key = (lambda r: abs(r[10]) / r[11]) if kind == "inside" else (lambda r: abs(r[10]) / r[11])
        rows.sort(key=key)
        pick = []
        for want in (lambda r: r[10] < 0 and r[11] > 1, lambda r: r[10] > 0 and r[11] > 1, lambda r: r[10] < 0, lambda r: r[10] > 0):
            pick += [r for r in rows if want(r) and r not in pick][:1]
        pick += [r for r in rows if r not in pick][:max(0, a.keep - len(pick))]
        kept += sorted(pick, key=key)
    inside = [r for r in found if r[0] == "inside"]
    smallest = min((abs(r[10]) / r[11] for r in inside), default=float("nan"))
    print(f"{a.images} images, {wall:.0f} s wall on {a.jobs} processes: {counts['inside']} inside, {counts['outside']} outside; smallest distance {smallest:.2e} x amax")
    if not counts["inside"] or not counts["outside"]:
        sys.exit("at least one inside and one outside row are required")
    table = "GABOR31_ROWS = [\n" + "".join(
        f"    ({r[0]!r}, {r[1]}, {r[2]}, {r[3]}, {r[4]}, {r[5]}, {r[6]}, {r[7]}, {r[8]}, {r[9]}, {r[10]!r}),\n" for r in kept) + "]\n"
    n_in, n_out = sum(r[0] == "inside" for r in kept), sum(r[0] == "outside" for r in kept)
    doc = (f"GABOR31_ROWS: {len(kept)} rows ({n_in} inside, {n_out} outside) kept of {counts['inside']} inside and {counts['outside']} outside found in\n"
           f"{a.images} two-dot images ({wall * a.jobs:.0f} s of CPU); the smallest distance found is {smallest:.1e} in units of the tile's\n"
           f"max(1, max |us|) (the first row).\"\"\"")
    if a.dry_run:
        print(table + doc)
        return
    path = os.path.join(ROOT, "tests", "gabor_ties_util.py")
    s = open(path).read()
    s, n1 = re.subn(r"(# BEGIN GABOR31_ROWS[^\n]*\n).*?(# END GABOR31_ROWS)", lambda m: m.group(1) + table + m.group(2), s, flags=re.S)
    s, n2 = re.subn(r'GABOR31_ROWS: \d+ rows.*?"""', lambda m: doc, s, count=1, flags=re.S)
    assert n1 == 1 and n2 == 1
    open(path, "w").write(s)


if __name__ == "__main__":
    main()
