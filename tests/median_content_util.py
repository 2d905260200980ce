"""Content families for the median kernels (k_median_cols, kernels_median_cols.hip; k_median_u8, kernels_prefilter.hip): images BUILT for the places
random content almost never reaches - a median on the smallest or largest present value, a cumulative count equal to half the window, one rank pair
across a whole window's columns, windows of ranks below and above the first one, a wave-uniform dword beside a mixed one.  Every family is a function
that returns {name: image}; test_oracle_median_content.py asserts on the CPU that the oracle's medians of these images sit where the family says,
test_gpu_median_content.py compares the kernels with the oracle on them.

One tile of k_median_cols is TILE_COLS columns by TILE_ROWS rows at every size used here (poppy_median_cols_geom; asserted by the CPU test).  A tile's
table of ranks is built from the values PRESENT in its footprint (the union of the 256-bit maps of the source tiles its windows touch), so an image
that wants a value at a given rank puts every value of its set into every tile: _plant does that."""
import numpy as np

TILE_COLS, TILE_ROWS = 128, 16
KSIZES = (3, 9, 25, 49, 65, 89)            # the family runs of the GPU test
DS = (2, 64, 65, 129, 130, 256)            # present values: one count per lane up to 64, two up to 129 (128 + the spare dword), windows of ranks beyond


def value_set(d, seed):
    """d different byte values, sorted; 0 and 255 among them from two values on (the first and the last bit of the presence map)"""
    if d >= 256:
        return np.arange(256, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    if d == 1:
        return np.array([rng.integers(0, 256)], np.uint8)
    inner = np.sort(rng.choice(np.arange(1, 255), d - 2, replace=False))
    return np.concatenate(([0], inner, [255])).astype(np.uint8)


def _plant(img, values, where, seed):
    """writes every one of `values` once into every tile of img, at cells of the boolean plane `where` (on at most a quarter of the tile's such cells: a cut tile
    at the right or bottom edge may hold fewer values - its footprint reaches a whole tile for every window of 3 and more); returns the cells written"""
    rng = np.random.default_rng(seed)
    h, w = img.shape
    done = np.zeros((h, w), bool)
    values = np.asarray(values, np.uint8)
    for y0 in range(0, h, TILE_ROWS):
        for x0 in range(0, w, TILE_COLS):
            ys, xs = np.nonzero(where[y0:y0 + TILE_ROWS, x0:x0 + TILE_COLS])
            n = min(len(ys) // 4, len(values))                          # thin: at most a quarter of the cells (a whole tile has room for 256 on either colour of a checkerboard)
            pick = rng.permutation(len(ys))[:n]
            img[y0 + ys[pick], x0 + xs[pick]] = values[:n]
            done[y0 + ys[pick], x0 + xs[pick]] = True
    return done


def checkerboard(w, h):
    """True where x + y is even"""
    return (np.add.outer(np.arange(h), np.arange(w)) & 1) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def ties_one(d, n_below, between=False, w=300, h=100, seed=0):
    """A period-1 checkerboard of two values a (x + y even) and b > a among d present values: every window that is not clamped holds (k * k + 1) / 2 cells
    of the colour of its centre and (k * k - 1) / 2 of the other, so the count of values <= a is half + 1 at an even pixel and half at an odd one:
    the decision C <= half flips at every pixel, and the median is a, b, a, b ...  The other d - 2 values keep that count where it is: values below a
    are planted on a's cells only, values above b on b's cells only, once per tile (thin: at most 254 of a tile's 2048 cells).  a has rank n_below, b rank n_below + 1.
    between=True: a is the smallest and b the largest value and the other d - 2 lie BETWEEN them, on a's cells: then the count that ties is that of
    the largest of them (`tie`), and the median alternates between a value <= tie (the largest one the window holds) and b.
    Returns (image, a, b, tie)."""
    vals = value_set(d, 1000 * d + n_below + seed)
    even = checkerboard(w, h)
    if between:
        a, b, tie = vals[0], vals[-1], (vals[-2] if d > 2 else vals[0])
        img = np.where(even, a, b).astype(np.uint8)
        _plant(img, vals[1:-1], even, seed + 1)
        return img, int(a), int(b), int(tie)
    a, b = vals[n_below], vals[n_below + 1]
    img = np.where(even, a, b).astype(np.uint8)
    _plant(img, vals[:n_below], even, seed + 1)
    _plant(img, vals[n_below + 2:], ~even, seed + 2)
    return img, int(a), int(b), int(a)


# (d, rank of a): (a, b) at ranks (0, 1), (62, 63), (63, 64), (64, 65), (127, 128), (128, 129) and (d - 2, d - 1) of every d
TIES_CASES = ((2, 0), (64, 0), (64, 62), (65, 0), (65, 62), (65, 63), (129, 0), (129, 63), (129, 64), (129, 127), (130, 0), (130, 64), (130, 127), (130, 128),
              (256, 0), (256, 62), (256, 63), (256, 64), (256, 127), (256, 128), (256, 254))
TIES_BETWEEN = (64, 65, 129, 130, 256)


def ties_meta():
    """{name: (image, a, b, tie)}"""
    out = {f"ties_d{d}_r{nb}": ties_one(d, nb) for d, nb in TIES_CASES}
    out.update({f"ties_d{d}_between": ties_one(d, 0, between=True) for d in TIES_BETWEEN})
    return out


def ties():
    return {k: v[0] for k, v in ties_meta().items()}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def extremes_one(d, top, w=300, h=100, seed=0):
    """A majority of the largest (top=True) or smallest of d present values with the other d - 1 sprinkled over 35 % of the cells, every one of them at
    least once in every tile: most medians are the value of rank d - 1 (rank 0) - the last lane of the one-count form at d = 64, answer 128 of the
    129-value tile (the spare dword of inv8), the first window's exact answers 128 / 0 beyond.  Returns (image, the extreme value)."""
    vals = value_set(d, 2000 * d + seed)
    rng = np.random.default_rng(3000 * d + top + seed)
    ext = vals[-1] if top else vals[0]
    others = vals[:-1] if top else vals[1:]
    img = np.full((h, w), ext, np.uint8)
    if len(others):
        planted = _plant(img, others, np.ones((h, w), bool), seed + 5)
        speck = (rng.random((h, w)) < max(0.35 - len(others) / (TILE_COLS * TILE_ROWS), 0.05)) & ~planted
        img[speck] = others[rng.integers(0, len(others), int(speck.sum()))]
    return img, int(ext)


def extremes_meta():
    return {f"extremes_d{d}_{'top' if top else 'bottom'}": extremes_one(d, top) + (d,) for d in DS for top in (True, False)}


def extremes():
    return {k: v[0] for k, v in extremes_meta().items()}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def three_windows_one(w, h, high_minor=False, seed=0, lo=30, hi=225, spread=22, edge=50):
    """Every tile holds all 256 values; the columns x with (x + 44) % 256 < 94 have medians low in the ranks (around `lo`), the other 162 of every 256
    high (around `hi`) - both parts wider than the largest window, their edges (x = 50, 212) inside tiles: no window of 128 ranks holds such a tile's
    medians.  The kernel lays the first window around the median of a sample of the tile (four rows, all 128 columns): that sits in the part that
    holds most of the tile's columns, the high one, and the low part needs the pass below; high_minor=True swaps the two levels: the pass above."""
    rng = np.random.default_rng(seed + high_minor)
    minor = ((np.arange(w) + 44) % 256) < 44 + edge
    base = np.where(minor != high_minor, lo, hi)
    img = np.clip(base[None, :] + rng.integers(-spread, spread + 1, (h, w)), 0, 255).astype(np.uint8)
    far = rng.random((h, w)) < 0.04
    img[far] = rng.integers(0, 256, int(far.sum()), dtype=np.uint8)
    _plant(img, np.arange(256), np.ones((h, w), bool), seed + 9)
    return img


def three_windows():
    """the two forms, and the first one at 150 x 300 transposed (rows 0 .. 55 are the low part: the tiles of rows 48 .. 63 straddle the edge in their
    middle; at ksize 89 their rows 48 .. 51 still have low medians and their sample rows 50, 54, 58 and 62 lie on either side)"""
    a, b = three_windows_one(300, 150), three_windows_one(300, 150, True)
    t = np.ascontiguousarray(three_windows_one(150, 300, seed=1, edge=56).T)
    _plant(t, np.arange(256), np.ones(t.shape, bool), 11)
    return {"three_windows_low_minor": a, "three_windows_high_minor": b, "three_windows_transposed": t}


def three_windows_tiled(w, h, seed=0):
    """the same content across a large image (natural rows != 16): the split moves from tile row to tile row so that the sample rows meet both sides"""
    rng = np.random.default_rng(seed)
    x, y = np.arange(w), np.arange(h)
    low = ((x[None, :] + 3 * (y[:, None] // 8)) % TILE_COLS) < 48
    img = np.clip(np.where(low, 30, 225) + rng.integers(-22, 23, (h, w)), 0, 255).astype(np.uint8)
    far = rng.random((h, w)) < 0.04
    img[far] = rng.integers(0, 256, int(far.sum()), dtype=np.uint8)
    return img


# ---------------------------------------------------------------------------------------------------------------------------------------------------
STRIPE_WIDTHS = (1, 2, 63, 64, 65, 89)


def _stripe_index(w, widths, start=0):
    edges = [0] if start == 0 else [0, start]
    k = 0
    while edges[-1] < w:
        edges.append(edges[-1] + widths[k % len(widths)]); k += 1
    return np.searchsorted(np.array(edges[1:]), np.arange(w), side="right")


def runs():
    """rows_*: a function of y alone - every column of every window enters and leaves the same pair of ranks at a row step, so a chain's 2r + 1 changes
    are ONE run (two from lane 64 on): one atomic adds the run's length, up to 64 + 25 = 89, to a biased byte.  few: 40 values (one count per lane),
    all: every row another value (two counts per lane from 65 rows in a footprint on; forms 5 to 7 take it by windows of ranks); rows_two: two values alternating row by row (the byte swings by the full 2r + 1 every step).
    cols_*: a function of x alone - no row step changes anything.
    stripes_*: vertical stripes of widths 1, 2, 63, 64, 65, 89 (mixed), and of width 64 beginning at column 4, 8 and 12 (a tile's chain w of ksize
    2r + 1 begins at column X0 - r + 16 w, so these put a stripe on lanes 0 .. 63 of a chain of ksize 89, 81 and 73: a run that ends at lane 63 with the
    second batch of lanes beginning a new one), every stripe a new value in every row.
    plateaus: two values with edges that move one column per row (runs of one column that walk through the lanes), left and right leaning."""
    w, h = 300, 100
    out = {}
    for name, d in (("few", 40), ("all", 256)):
        vals = value_set(d, 40 + d)
        rng = np.random.default_rng(d)
        col = vals[rng.integers(0, d, h)] if d <= 64 else vals[rng.permutation(d)[:h]]      # all: every row another value (100 different ones)
        out[f"rows_{name}"] = np.repeat(col[:, None], w, 1)
        row = vals[rng.integers(0, d, w)]
        out[f"cols_{name}"] = np.repeat(row[None, :], h, 0)
    out["rows_two"] = np.repeat(np.where(np.arange(h) & 1, 200, 17).astype(np.uint8)[:, None], w, 1)
    for name, idx in (("mixed", _stripe_index(w, STRIPE_WIDTHS)), ("64_at4", _stripe_index(w, (64,), 4)), ("64_at8", _stripe_index(w, (64,), 8)),
                      ("64_at12", _stripe_index(w, (64,), 12))):
        rng = np.random.default_rng(len(name) + int(idx.sum()))
        vals = value_set(48, 7)                                     # few values: the run test needs equal rank pairs in neighbouring columns only within a stripe
        per = vals[rng.integers(0, len(vals), (h, int(idx.max()) + 1))]
        for s in range(per.shape[1]):                               # neighbouring stripes never share a value in a row, nor a stripe with itself one row up
            for y in range(h):
                while (s and per[y, s] == per[y, s - 1]) or (y and per[y, s] == per[y - 1, s]):
                    per[y, s] = vals[rng.integers(0, len(vals))]
        out[f"stripes_{name}"] = np.ascontiguousarray(per[:, idx])
    x, y = np.arange(w), np.arange(h)
    out["plateaus"] = np.where(((x[None, :] + y[:, None]) // 37) & 1, 180, 60).astype(np.uint8)
    out["plateaus_back"] = np.where(((x[None, :] - y[:, None] + 200) // 23) % 3, 5, 250).astype(np.uint8)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def uniform_dwords_one(w, h, seed=0):
    """flat blocks at least 64 + 89 columns wide beside noise, block edges inside a wave's 64 columns and at every byte of a dword (they move by
    one column every few rows), flat rows between noisy ones: k_median_u8's four-equal-bytes shortcut holds for some dwords of a window row and
    not for others, in the warm-up and in the steps"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    flat_w = min(64 + 89, w - 20)
    for y in range(h):
        x0 = 13 + (y // 3) % 9
        img[y, x0:x0 + flat_w] = 77 if (y // 10) % 2 == 0 else 201
    img[h // 2: h // 2 + 3, :] = 140                                 # whole flat rows
    img[h // 2 + 5, :] = rng.integers(0, 256, w, dtype=np.uint8)     # and a noisy one through the block
    return img


def uniform_dwords():
    return {"uniform_blocks": uniform_dwords_one(300, 100), "uniform_blocks_small": uniform_dwords_one(200, 40, 1),
            "flat_255": np.full((100, 300), 255, np.uint8), "flat_0": np.zeros((100, 300), np.uint8)}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
THIN_SIZES = ((1, 1), (1, 150), (300, 1), (2, 2), (43, 43), (45, 45), (129, 17), (257, 33))      # (w, h)
THIN_KSIZES = (3, 45, 87, 89)


def thin():
    """sizes at which the clamped rows and columns are folded many times; noise and a few-valued image of each"""
    out = {}
    for w, h in THIN_SIZES:
        rng = np.random.default_rng(w * 1000 + h)
        out[f"thin_{w}x{h}_noise"] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        vals = value_set(5, w + h)
        out[f"thin_{w}x{h}_few"] = vals[rng.integers(0, 5, (h, w))]
    return out


def noise(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


FAMILIES = dict(ties=ties, extremes=extremes, three_windows=three_windows, runs=runs, uniform_dwords=uniform_dwords, thin=thin)


def family_ksizes(family):
    return THIN_KSIZES if family == "thin" else KSIZES


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# what the kernel's tables of ranks look like for an image, restated from its description: which values each tile's footprint holds
def tile_presence(img, rows=TILE_ROWS, cols=TILE_COLS):
    """bool [tiles_y, tiles_x, 256]: the values each tile holds"""
    h, w = img.shape
    ty, tx = -(-h // rows), -(-w // cols)
    p = np.zeros((ty, tx, 256), bool)
    for j in range(ty):
        for i in range(tx):
            p[j, i, np.unique(img[j * rows:(j + 1) * rows, i * cols:(i + 1) * cols])] = True
    return p


def footprint_presence(img, ksize, rows=TILE_ROWS, cols=TILE_COLS):
    """bool [tiles_y, tiles_x, 256]: the values of the tiles that a tile's windows of `ksize` touch (clamped to the image)"""
    h, w = img.shape
    r = ksize // 2
    p = tile_presence(img, rows, cols)
    f = np.zeros_like(p)
    for j in range(p.shape[0]):
        y0, y1 = min(max(j * rows - r, 0), h - 1) // rows, min(max(j * rows + rows - 1 + r, 0), h - 1) // rows
        for i in range(p.shape[1]):
            x0, x1 = min(max(i * cols - r, 0), w - 1) // cols, min(max(i * cols + cols - 1 + r, 0), w - 1) // cols
            f[j, i] = p[y0:y1 + 1, x0:x1 + 1].any(axis=(0, 1))
    return f


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Images for Extractor::foreground's chain of medians at 1024 x 128: 8 x 8 tiles of 128 x 16, and the host sample's 32 blocks of 128 x 32 tile the image
# (two tiles each).  B = G = R, so the grey image (and the green channel the host samples) is the plane built here.
CHAIN_W, CHAIN_H = 1024, 128


def two_tone(w=CHAIN_W, h=CHAIN_H, lo=60, hi=190):
    """two values in large shapes (discs and a diagonal band) whose edges the medians round off link by link"""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    shape = ((x - 300) ** 2 + (y - 70) ** 2 < 45 ** 2) | ((x - 700) ** 2 + (y - 40) ** 2 < 30 ** 2) | (((x + 2 * y) // 90) % 4 == 0)
    return np.where(shape, hi, lo).astype(np.uint8)


def _patch_values(kind, ph, pw, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (ph, pw), dtype=np.uint8)
    if kind == "ramp":                                               # a steep ramp under noise: the medians keep the ramp, so many values per tile survive link after link
        ramp = (np.arange(pw) % 64) * 4
        return np.clip(ramp[None, :] + rng.integers(-30, 31, (ph, pw)), 0, 255).astype(np.uint8)
    n = int(kind)                                                    # exactly n values, the two tones (60, 190) among them, every one in every tile of the patch
    pool = np.setdiff1d(np.arange(256), (60, 190))
    vals = np.sort(np.concatenate((rng.choice(pool, n - 2, replace=False), (60, 190)))).astype(np.uint8)
    p = vals[rng.integers(0, n, (ph, pw))]
    _plant(p, vals, np.ones((ph, pw), bool), seed + 1)
    return p


CHAIN_IMAGES = {           # name: (kind of patch, x0, y0, width, height) - at most three of the host's sample blocks
    "noise_patch": ("noise", 0, 0, 384, 32), "ramp_patch": ("ramp", 0, 0, 384, 32),
    "left_edge": ("ramp", 0, 32, 128, 96), "right_edge": ("noise", 896, 0, 128, 96),
    "values_64": ("64", 256, 32, 384, 32), "values_65": ("65", 256, 32, 384, 32), "values_129": ("129", 256, 64, 384, 32), "values_130": ("130", 256, 64, 384, 32),
}


def chain_plane(name):
    kind, x0, y0, pw, ph = CHAIN_IMAGES[name]
    img = two_tone()
    img[y0:y0 + ph, x0:x0 + pw] = _patch_values(kind, ph, pw, sum(map(ord, name)))
    return img


def bgr_of(plane):
    return np.ascontiguousarray(np.repeat(plane[:, :, None], 3, 2))


def tiles_plane(values_per_tile, seed=0, w=CHAIN_W, h=CHAIN_H):
    """an image whose tile k (row-major, 128 x 16) holds exactly values_per_tile[k] different values: two tones in shapes, and the other values of the tile
    in a block of noise inside it"""
    img = two_tone(w, h)
    rng = np.random.default_rng(seed)
    tx = w // TILE_COLS
    for k, n in enumerate(values_per_tile):
        y0, x0 = (k // tx) * TILE_ROWS, (k % tx) * TILE_COLS
        t = img[y0:y0 + TILE_ROWS, x0:x0 + TILE_COLS].ravel()         # (a copy: written back below)
        have = np.unique(t)
        extra = rng.choice(np.setdiff1d(np.arange(256), have), n - len(have), replace=False).astype(np.uint8)
        if len(extra):
            cells = rng.permutation(TILE_COLS * TILE_ROWS)[:max(len(extra), 300)]
            fill = np.concatenate((extra, extra[rng.integers(0, len(extra), len(cells) - len(extra))]))
            keep = [np.flatnonzero(t == v)[0] for v in have]          # a cell of each tone stays
            cells = cells[~np.isin(cells, keep)]
            t[cells] = fill[:len(cells)]
            img[y0:y0 + TILE_ROWS, x0:x0 + TILE_COLS] = t.reshape(TILE_ROWS, TILE_COLS)
    return img
