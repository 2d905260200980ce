"""The content families of median_content_util.py on the CPU: (a) the oracle's median against an independent numpy restatement (edge-padded
sliding windows + np.partition) on every family, and (b) that each family's images put the oracle's medians where the family says - on a count
equal to half the window, on the smallest / largest present value, below and above the first window of ranks, on one rank pair per row step.
(b) are conditions of the INPUTS, computed from the oracle's output and the tile geometry (poppy_median_cols_geom): they hold by construction and
are asserted so that test_gpu_median_content.py, which compares the kernels with the oracle on these images, cannot pass beside the code it names."""
import numpy as np
import pytest

import median_content_util as M
import oracle_lib as O
from poppy_amd import capi


def restated_median(img, ksize):
    """cv::medianBlur's definition: the middle one of the ksize * ksize values around a pixel, the border replicated"""
    r = ksize // 2
    p = np.pad(img, r, mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(p, (ksize, ksize))
    out = np.empty_like(img)
    half = (ksize * ksize) // 2
    for y in range(img.shape[0]):                                   # row by row: a row's windows are w * ksize * ksize bytes
        out[y] = np.partition(win[y].reshape(img.shape[1], -1), half, axis=1)[:, half]
    return out


@pytest.fixture(scope="module")
def medians():
    """the oracle's medians, computed once per (image name, ksize) and shared"""
    cache = {}

    def get(name, img, ksize):
        if (name, ksize) not in cache:
            cache[name, ksize] = O.median_blur_u8(img, ksize)
        return cache[name, ksize]
    return get


def test_tile_geometry_the_families_are_built_for():
    assert capi.median_cols_geom(300, 100) == (3, 7, M.TILE_ROWS, M.TILE_COLS) and capi.median_cols_geom(300, 150) == (3, 10, 16, 128)
    assert capi.median_cols_geom(1024, 128) == (8, 8, 16, 128) and capi.median_cols_geom(200, 40) == (2, 3, 16, 128)
    # the default geometry away from 16 rows: 1080p, 4K, and the two sizes of the GPU test's natural-rows cases
    assert capi.median_cols_geom(1920, 1080)[2] == 22 and capi.median_cols_geom(3840, 2160)[2] == 87
    assert capi.median_cols_geom(3840, 540) == (30, 25, 22, 128) and capi.median_cols_geom(5120, 700) == (40, 19, 37, 128)
    assert capi.median_cols_geom(1, 1) == (1, 1, 1, 128) and capi.median_cols_geom(129, 7) == (2, 1, 7, 128)       # rows never exceed the image
    with pytest.raises(ValueError):
        capi.median_cols_geom(0, 5)


def test_host_hint_export():
    """poppy_median_cols_hint: 0 under 256 x 64 whatever the content; 29 of the 32 sample blocks with at most 24 values decide"""
    flat = np.full((128, 1024, 3), 9, np.uint8)
    assert capi.median_cols_hint(flat) == 1 and capi.median_cols_hint(flat[:63]) == 0 and capi.median_cols_hint(flat[:, :255]) == 0
    noisy = np.random.default_rng(0).integers(0, 256, flat.shape, dtype=np.uint8)
    assert capi.median_cols_hint(noisy) == 0
    # the sample blocks of a 1024 x 128 image are disjoint (8 x 4 of 128 x 32): noise in three of them leaves 29 easy ones, in four 28
    for blocks, want in ((3, 1), (4, 0)):
        img = flat.copy()
        img[:32, :128 * blocks] = noisy[:32, :128 * blocks]
        assert capi.median_cols_hint(img) == want
    # only the green channel is sampled
    img = flat.copy(); img[..., 0] = noisy[..., 0]; img[..., 2] = noisy[..., 2]
    assert capi.median_cols_hint(img) == 1
    assert capi.lib().poppy_median_cols_hint(None, 3072, 1024, 128) < 0


# ---- (a) the oracle against the restatement ------------------------------------------------------------------------------------------------------
def _cut(img):
    return np.ascontiguousarray(img[:70, :160])


@pytest.mark.parametrize("family", sorted(M.FAMILIES))
def test_oracle_median_is_the_restated_median(family):
    imgs = M.FAMILIES[family]()
    names = sorted(imgs)
    if family == "thin":                                            # every size, at every ksize of the family (the images are small)
        for name in names:
            for ksize in M.THIN_KSIZES:
                if imgs[name].size * ksize * ksize > 40e6:
                    continue
                assert np.array_equal(O.median_blur_u8(imgs[name], ksize), restated_median(imgs[name], ksize)), (name, ksize)
        return
    step = max(len(names) // 3, 1)
    for k, name in enumerate(names[::step][:3]):                    # three images spread over the family, cut to 160 x 70
        img = _cut(imgs[name])
        for ksize in (3, 9, 25, 89) if k < 2 else (3, 9, 25):
            assert np.array_equal(O.median_blur_u8(img, ksize), restated_median(img, ksize)), (name, ksize)


# ---- (b) each family reaches its branch -----------------------------------------------------------------------------------------------------------
def window_counts(mask, ksize):
    """the number of True cells in every pixel's window (replicated border), by an integral image"""
    r = ksize // 2
    p = np.pad(mask.astype(np.int64), r, mode="edge")
    s = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    s[1:, 1:] = p.cumsum(0).cumsum(1)
    return s[ksize:, ksize:] - s[:-ksize, ksize:] - s[ksize:, :-ksize] + s[:-ksize, :-ksize]


def interior(img, ksize):
    r = ksize // 2
    m = np.zeros(img.shape, bool)
    m[r:img.shape[0] - r, r:img.shape[1] - r] = True
    return m


def ranks_in_footprints(img, ksize):
    """(number of present values, value -> rank table) of every tile's footprint"""
    f = M.footprint_presence(img, ksize)
    return f.sum(-1), np.cumsum(f, -1) - f


@pytest.mark.parametrize("name", sorted(M.ties_meta()))
def test_ties_sit_on_half_and_flip_at_every_pixel(name, medians):
    """The fraction of ALL pixels whose window holds exactly half or half + 1 values <= the tie value is bounded by the share of windows that are not
    clamped ((w - 2r)(h - 2r) / (w h): 0.90 at ksize 9, 0.28 at ksize 65 on 300 x 100 - a clamped window repeats a row or column of the board and
    leaves the tie), so the 80 % are asserted of all pixels up to ksize 9 and of the pixels with an unclamped window up to 65, where the construction
    gives every single one."""
    img, a, b, tie = M.ties_meta()[name]
    d = int(name.split("_")[1][1:])
    for ksize in M.KSIZES:
        half = ksize * ksize // 2
        n, rank = ranks_in_footprints(img, ksize)
        assert (n == d).all(), f"{name} ksize {ksize}: a footprint holds {n.min()}..{n.max()} values"
        if "between" not in name:
            want_rank = int(name.split("_r")[1])
            assert (rank[..., a] == want_rank).all() and (rank[..., b] == want_rank + 1).all()
        inner = interior(img, ksize)
        if ksize <= 65:
            c = window_counts(img <= tie, ksize)
            tied = (c == half) | (c == half + 1)
            assert tied[inner].mean() >= 0.8 and tied[inner].all(), f"{name} ksize {ksize}: {tied[inner].mean():.3f} of the unclamped windows tie"
            if ksize <= 9:
                assert tied.mean() >= 0.8, f"{name} ksize {ksize}: {tied.mean():.3f} of all windows tie"
        med = medians(name, img, ksize)
        low = med <= tie
        pairs = inner[:, :-1] & inner[:, 1:]
        flips = (low[:, :-1] != low[:, 1:])[pairs]
        assert flips.size and flips.mean() >= 0.8, f"{name} ksize {ksize}: medians alternate on {flips.mean():.3f} of the interior pairs"
        if "between" not in name:
            assert np.isin(med[inner], (a, b)).mean() >= 0.99          # (a window of 3 whose every b is planted over has another median)
        else:
            assert (med[inner & ~low] == b).all()
            if ksize >= 25:                                         # (a window of 3 or 9 rarely holds one) the low median is one of the values between
                assert (med[inner & low] > a).mean() >= 0.8


@pytest.mark.parametrize("name", sorted(M.extremes_meta()))
def test_extremes_put_the_median_on_the_first_or_last_rank(name, medians):
    img, ext, d = M.extremes_meta()[name]
    for ksize in M.KSIZES:
        n, rank = ranks_in_footprints(img, ksize)
        assert (n == d).all(), f"{name} ksize {ksize}: a footprint holds {n.min()}..{n.max()} values"
        assert (rank[..., ext] == (d - 1 if name.endswith("top") else 0)).all()
        med = medians(name, img, ksize)
        assert (med == ext).mean() >= 0.5, f"{name} ksize {ksize}: {(med == ext).mean():.3f} of the medians are the extreme value"


def first_window_bases(img, ksize):
    """the base rank of every tile's first window as kernels_median_cols.hip describes it: 512 samples of the tile (all 128 columns of four rows),
    counted by rank in groups of four; the window of 128 ranks is laid 64 below the sample's median, within 0 .. distinct - 129"""
    h, w = img.shape
    tx, ty, rows, cols = capi.median_cols_geom(w, h)
    n, rank = ranks_in_footprints(img, ksize)
    base = np.zeros((ty, tx), int)
    for j in range(ty):
        for i in range(tx):
            tid = np.arange(512)
            sx = np.minimum(i * cols + (tid & 127), w - 1)
            sy = np.minimum(j * rows + ((tid >> 7) * rows >> 2) + (rows >> 3), h - 1)
            four = np.bincount(rank[j, i][img[sy, sx]] >> 2, minlength=64)
            ms = 4 * int((np.cumsum(four) <= 256).sum()) + 2
            base[j, i] = min(max(ms - 64, 0), max(int(n[j, i]) - 129, 0))
    return base, n, rank


@pytest.mark.parametrize("ksize", M.KSIZES)
def test_three_windows_need_the_passes_below_and_above(ksize, medians):
    imgs = M.three_windows()
    seen = {}
    for name, img in imgs.items():
        h, w = img.shape
        tx, ty, rows, cols = capi.median_cols_geom(w, h)
        base, n, rank = first_window_bases(img, ksize)
        assert (n == 256).all()
        med = medians(name, img, ksize).astype(int)                 # all 256 values present: a value is its rank
        span = below = above = 0
        for j in range(ty):
            for i in range(tx):
                t = med[j * rows:(j + 1) * rows, i * cols:(i + 1) * cols]
                span = max(span, int(t.max() - t.min()))
                below += int(((t <= base[j, i]) & (base[j, i] > 0)).sum())                # answer 0 of a window that does not begin at rank 0
                above += int(((t >= base[j, i] + 128) & (base[j, i] < 127)).sum())        # answer 128 of one that does not reach the last rank
        seen[name] = (span, below, above)
        assert span > 128, f"{name} ksize {ksize}: the widest tile spans {span} ranks"
    assert seen["three_windows_low_minor"][1] > 500 and seen["three_windows_high_minor"][2] > 500, seen
    assert sum(seen["three_windows_transposed"][1:]) > 500, seen


def test_runs_are_what_their_docstring_says():
    imgs = M.runs()
    for name, img in imgs.items():
        h, w = img.shape
        if name.startswith("rows_"):
            assert (img == img[:, :1]).all()                        # a function of y alone: one rank pair across the 2r + 1 columns of any window
            for ksize in M.KSIZES:
                r = ksize // 2
                y = np.arange(h - 1)
                changes = img[np.minimum(y + r + 1, h - 1), 0] != img[np.maximum(y - r, 0), 0]
                assert changes.sum() >= (h - 1 - 2 * r) * 0.9 - 2, (name, ksize, int(changes.sum()))
        if name.startswith("cols_"):
            assert (img == img[:1]).all()                           # no row step changes anything
        if name == "rows_two":
            assert set(np.unique(img)) == {17, 200} and (img[1:, 0] != img[:-1, 0]).all()
    assert len(np.unique(imgs["rows_few"])) <= 64 < len(np.unique(imgs["rows_all"])) == imgs["rows_all"].shape[0]
    # stripes: the widths are there, and every stripe changes in every row
    mixed = imgs["stripes_mixed"]
    edges = np.flatnonzero(np.r_[True, (mixed[:, 1:] != mixed[:, :-1]).any(0), True])
    assert list(np.diff(edges)[:6]) == list(M.STRIPE_WIDTHS)
    assert (mixed[1:] != mixed[:-1]).all()
    # a stripe of 64 columns on lanes 0 .. 63 of a chain (its window begins at column X0 - r + 16 wave), the next one from lane 64 on: the first batch of
    # lanes is one run that ends at lane 63 and the second batch (ksize 73 and up) begins a new one, at row steps where both stripes change
    for start, ksize in ((4, 89), (8, 81), (12, 73)):
        img = imgs[f"stripes_64_at{start}"]
        h, w = img.shape
        r = ksize // 2
        hits = 0
        for X0 in range(0, w, M.TILE_COLS):
            for wave in range(8):
                c0 = X0 - r + 16 * wave
                if c0 < 0 or c0 + 2 * r >= w:
                    continue
                whole = (img[:, c0:c0 + 64] == img[:, c0:c0 + 1]).all() and (img[:, c0 + 64:c0 + 2 * r + 1] == img[:, c0 + 64:c0 + 65]).all()
                if whole and (img[:, c0 + 63] != img[:, c0 + 64]).all() and (c0 == 0 or (img[:, c0 - 1] != img[:, c0]).all()):
                    y = np.arange(r, h - r - 1)
                    both = (img[y + r + 1, c0] != img[y - r, c0]) & (img[y + r + 1, c0 + 64] != img[y - r, c0 + 64])
                    hits += int(both.sum())
        assert hits > 0, f"stripes_64_at{start}: no chain of ksize {ksize} has a run on lanes 0 .. 63"
    # plateaus: the edges move by one column per row
    for name in ("plateaus", "plateaus_back"):
        img = imgs[name]
        e0, e1 = np.flatnonzero(img[10, 1:] != img[10, :-1]), np.flatnonzero(img[11, 1:] != img[11, :-1])
        assert len(e0) >= 3 and any(abs(int(a) - int(b)) == 1 for a in e0 for b in e1)


def test_uniform_dwords_hold_flat_blocks_beside_noise():
    for name, img in M.uniform_dwords().items():
        if name.startswith("flat"):
            assert len(np.unique(img)) == 1 and int(img[0, 0]) in (0, 255)
            continue
        eq = img[:, 1:] == img[:, :-1]
        longest = max(max(len(run) for run in "".join("1" if e else "0" for e in row).split("0")) for row in eq)
        assert longest >= min(64 + 89, img.shape[1] - 20) - 1
        noisy_rows = sum(1 for row in eq if 0.3 * len(row) < row.sum() < 0.9 * len(row))
        assert noisy_rows > img.shape[0] // 2                       # most rows hold both a flat block and noise


def test_thin_sizes_straddle_the_largest_radius():
    sizes = {im.shape[::-1] for im in M.thin().values()}
    assert sizes == set(M.THIN_SIZES) and (43, 43) in sizes and (45, 45) in sizes and 89 // 2 == 44
