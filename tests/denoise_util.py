"""The non-local-means denoise (include/poppy_hip.h: poppy_bgr_denoise) restated in numpy, independently of the C++: per-offset squared-difference images
and their integrals, exp from Python's math.  Also the image families the host and GPU tests share, and what the restatement saw on the way (the largest
estimate, the table indices reached, the residues of the final division), so that a test can assert that a family still reaches its branch."""
import functools
import math

import numpy as np

MAX_DIST = 3 * 255 * 255


@functools.lru_cache(maxsize=None)
def weights(hs, tw, sw):
    """dict(table int64 [n], n, L, fpm, shift, near_half = entries where fpm * wd lies within 1e-6 of a half)"""
    fpm = min((2 ** 32 - 1) // (sw * sw * 255), 2 ** 31 - 1)
    shift = 0
    while (1 << shift) < tw * tw:
        shift += 1
    mult = float(1 << shift) / float(tw * tw)
    n = int(MAX_DIST / mult) + 1
    den = float(np.float32(np.float32(hs) * np.float32(hs)) * np.float32(3))      # float, then widened
    floor_w = 0.001 * fpm
    table = np.zeros(n, np.int64)
    near_half = []
    last = 0
    for a in range(n):
        v = fpm * math.exp(-(a * mult) / den)
        if abs((v - math.floor(v)) - 0.5) < 1e-6:
            near_half.append(a)
        r = round(v)                                  # Python rounds halves to even
        if r < floor_w:
            r = 0
        table[a] = r
        if r:
            last = a + 1
    assert (np.diff(table) <= 0).all()
    return dict(table=table, n=n, L=last, fpm=fpm, shift=shift, near_half=near_half)


def fold101(i, n):
    """reflect-101 of an index array, folded as often as needed"""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def denoise(img, hs, tw=7, sw=21, info=None):
    """The rule on an HxWx3 uint8 image.  info (a dict): max_est, hit (the set of table indices a = D >> shift seen among L - 1, L), residues = the
    (est + ws // 2) % ws of every pixel and channel, ws."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    W = weights(float(hs), int(tw), int(sw))
    t, L, shift = W["table"], W["L"], W["shift"]
    th, sh = tw // 2, sw // 2
    b = th + sh
    e = img[fold101(np.arange(-b, h + b), h)][:, fold101(np.arange(-b, w + b), w)].astype(np.int64)
    est = np.zeros((h, w, 3), np.int64)
    ws = np.zeros((h, w), np.int64)
    p = e[sh:sh + h + 2 * th, sh:sh + w + 2 * th]
    at_last = at_cut = 0
    for dy in range(-sh, sh + 1):
        for dx in range(-sh, sh + 1):
            q = e[sh + dy:sh + dy + h + 2 * th, sh + dx:sh + dx + w + 2 * th]
            sq = ((p - q) ** 2).sum(axis=2)
            integral = np.zeros((h + 2 * th + 1, w + 2 * th + 1), np.int64)
            integral[1:, 1:] = sq.cumsum(axis=0).cumsum(axis=1)
            D = integral[tw:, tw:] - integral[:-tw, tw:] - integral[tw:, :-tw] + integral[:-tw, :-tw]
            a = D >> shift
            at_last += int((a == L - 1).sum())
            at_cut += int((a == L).sum())
            wgt = np.where(a < L, t[np.minimum(a, L - 1)], 0)
            est += wgt[:, :, None] * e[b + dy:b + dy + h, b + dx:b + dx + w]
            ws += wgt
    assert est.max() < 2 ** 32 and ws.min() >= W["fpm"]            # unsigned 32 bits hold every sum but the rounding one
    full = est + (ws // 2)[:, :, None]
    if info is not None:
        info.update(max_est=int(est.max()), at_last=at_last, at_cut=at_cut, residues=full % ws[:, :, None], ws=ws)
    return (full // ws[:, :, None]).astype(np.uint8)


# ---- image families ---------------------------------------------------------------------------------------------------------------------------------

def flat(w, h, v):
    return np.full((h, w, 3), v, np.uint8)


def saturated_noise(w, h, seed=1):
    """every sample 0 or 255: at moderate strengths only the centre offset has weight, and the image comes back unchanged"""
    return (np.random.RandomState(seed).randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def gaussian_noise(w, h, seed=2, sigma=6.0):
    """sigma 6 around 128: many distinct non-zero weights"""
    return np.clip(np.rint(128 + sigma * np.random.RandomState(seed).randn(h, w, 3)), 0, 255).astype(np.uint8)


def gradient(w, h):
    """smooth ramps of a different slope per channel: small distances, the dense head of the table"""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(2 * x + y) % 256, (255 - x - 2 * y) % 256, (x + y) // 2 % 256], axis=2).astype(np.uint8)


def corner_pixel(w, h):
    """flat but for one corner pixel: the reflected border carries it"""
    a = flat(w, h, 100)
    a[0, 0] = (255, 0, 180)
    return a


def three_squares(lo, hi):
    """(d0, d1, d2), each 0 .. 255, with lo <= d0^2 + d1^2 + d2^2 < hi"""
    for d0 in range(min(255, math.isqrt(max(hi - 1, 0))), -1, -1):
        for d1 in range(0, d0 + 1):
            rest = lo - d0 * d0 - d1 * d1
            c = 0 if rest <= 0 else math.isqrt(rest - 1) + 1           # the smallest c with c^2 >= rest
            if c <= 255 and lo <= d0 * d0 + d1 * d1 + c * c < hi:
                return d0, d1, c
    raise AssertionError(f"no three squares in [{lo}, {hi})")


def cutoff(w, h, hs, tw=7, sw=21):
    """A flat field of 0 with two planted clusters.  A template that holds a whole cluster is at distance D = the cluster's energy from every flat template;
    the first cluster's energy has D >> shift = L - 1, the second's L: one on each side of the table's cut-off.  A cluster is a block of at most tw x tw
    pixels: full pixels of 255 in all channels, and one pixel tuned by three squares."""
    W = weights(float(hs), int(tw), int(sw))
    L, shift = W["L"], W["shift"]
    assert L < W["n"], "the whole table is non-zero: no cut-off to sit on"
    a = flat(w, h, 0)
    b = tw // 2 + sw // 2
    spots = [(w // 4, h // 2), (3 * w // 4, h // 2)] if sw > 3 else [(w // 4, h // 3), (3 * w // 4, 2 * h // 3)]
    for (cx, cy), target in zip(spots, (L - 1, L)):
        lo = target << shift
        k = lo // MAX_DIST                                  # full pixels
        side = 1
        while side * side < k + 1:
            side += 1
        assert side <= tw and b >= 0
        d = three_squares(lo - k * MAX_DIST, lo - k * MAX_DIST + (1 << shift))
        cells = [(cx - side // 2 + i % side, cy - side // 2 + i // side) for i in range(k + 1)]
        for i, (x, y) in enumerate(cells):
            a[y, x] = (255, 255, 255) if i < k else d
    return a


def half_ties(w, h, hs=10.0, tw=7, sw=21, seed=5):
    """High-contrast noise in which every block of sw // 2 columns is followed by its copy, so that a pixel well inside a block has exactly two offsets of
    non-zero weight: itself and its twin sw // 2 columns away (every other template differs by far more than the cut-off).  The copies are perturbed at
    designed places (half_tie_designs): at a pair of twins with weights fpm and t, values v and v + d and ws = fpm + t, the final sum is
    congruent to t d + ws // 2 modulo ws.  d = 1 with t = fpm is an exact half (the sum is a multiple of ws); other (t, d) leave it one short."""
    W = weights(float(hs), int(tw), int(sw))
    P = sw // 2
    assert P >= tw, "a block holds a whole template"
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (h, w, 3)).astype(np.int64)
    for x0 in range(0, w - 2 * P + 1, 2 * P):
        a[:, x0 + P:x0 + 2 * P] = a[:, x0:x0 + P]
    designs = half_tie_designs(float(hs), int(tw), int(sw))
    th = tw // 2
    spots = [(x0, y) for y in range(th, h - th, tw) for x0 in range(0, w - 2 * P + 1, 2 * P)]          # templates of two spots never overlap
    assert len(spots) >= len(designs), "the frame is too small for every design"
    for (x0, y), (d, extra) in zip(spots, designs):
        x = x0 + th                                          # the leftmost column whose template lies inside the block
        a[y, x] = a[y, x + P] = (128, 128, 128)
        a[y, x + P, 0] += d
        a[y, x + 1] = a[y, x + 1 + P] = (0, 0, 0)
        a[y, x + 1 + P] = extra
    return a.astype(np.uint8)


PARAMS = [(3.0, 7, 21), (10.0, 7, 21), (10.0, 5, 9), (10.0, 3, 3), (40.0, 7, 21), (100.0, 7, 21)]      # the last: the whole table is non-zero
DEFAULT = (10.0, 7, 21)


def bound_strengths(table_length, bound, tw=7, sw=21):
    """(hs_below, hs_above): neighbouring strengths on a 1 / 64 grid whose non-zero prefix L is <= bound and > bound.  table_length(hs, tw, sw) -> L."""
    lo, hi = 64, 64 * 100                                     # hs = 1 .. 100 in 64ths; L grows with hs
    assert table_length(lo / 64, tw, sw) <= bound < table_length(hi / 64, tw, sw)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if table_length(mid / 64, tw, sw) <= bound:
            lo = mid
        else:
            hi = mid
    return lo / 64, hi / 64


def cases(tile, strengths_at_bound):
    """[(name, image, (hs, tw, sw))]: every family of the host and GPU tests.  tile: the kernel's output tile (poppy_denoise_tile); strengths_at_bound:
    bound_strengths of the kernel's LDS table bound."""
    tile_w, tile_h = tile
    out = []
    for w, h in [(1, 1), (1, 40), (40, 1), (2, 2), (5, 3), (13, 13), (26, 27), (27, 26)]:          # every index folds, several times below 13
        out.append((f"size_{w}x{h}", gaussian_noise(w, h, seed=w * 100 + h), DEFAULT))
    for d in (-1, 0, 1):                                      # the tile's width and height, one axis at a time
        out.append((f"tile_w{d:+d}", gaussian_noise(tile_w + d, 20, seed=10 + d), DEFAULT))
        out.append((f"tile_h{d:+d}", gaussian_noise(20, tile_h + d, seed=20 + d), DEFAULT))
    big = (3 * tile_w + 7, 2 * tile_h + 5)                    # 3 x 2 tiles and a ragged edge
    for p in PARAMS:
        out.append((f"tiles_3x2_hs{p[0]:g}_{p[1]}_{p[2]}", gaussian_noise(*big, seed=31), p))
    for hs, side in zip(strengths_at_bound, ("below", "above")):
        out.append((f"table_bound_{side}", gaussian_noise(tile_w + 9, 24, seed=41, sigma=20.0), (hs, 7, 21)))
    w, h = tile_w + 12, 40                                    # two tiles across
    for v in (0, 255, 128):
        out.append((f"flat_{v}", flat(w, h, v), DEFAULT))
    out.append(("flat_255_hs100", flat(w, h, 255), PARAMS[-1]))
    out.append(("saturated_noise_hs3", saturated_noise(w, h), PARAMS[0]))
    out.append(("saturated_noise_hs10", saturated_noise(w, h), DEFAULT))
    out.append(("gaussian_noise", gaussian_noise(w, h), DEFAULT))
    for p in PARAMS[:-1]:
        out.append((f"cutoff_hs{p[0]:g}_{p[1]}_{p[2]}", cutoff(96, 48, *p), p))
    out.append(("half_ties", half_ties(80, 40), DEFAULT))
    out.append(("gradient", gradient(w, h), DEFAULT))
    out.append(("gradient_hs100", gradient(w, h), PARAMS[-1]))
    out.append(("corner_pixel_small", corner_pixel(9, 7), DEFAULT))
    out.append(("corner_pixel", corner_pixel(w, h), DEFAULT))
    return out


@functools.lru_cache(maxsize=None)
def half_tie_designs(hs, tw, sw):
    """[(d, (e0, e1, e2))]: the twin's centre differs by d in channel 0 and its right neighbour by e, so that the two templates are D = d^2 + |e|^2 apart
    and the twin's weight is t[D >> shift].  First the exact half (d = 1, e = 0: D = 1, weight fpm), then every solution of
    t d + ws // 2 = -1 (mod ws), ws = fpm + t, |d| <= 127, found by search over the table."""
    W = weights(hs, tw, sw)
    t, L, shift, fpm = W["table"], W["L"], W["shift"], W["fpm"]
    out = [(1, (0, 0, 0))]
    for a in range(L):
        ws = fpm + int(t[a])
        for d in range(-127, 128):
            if d * d >= (a + 1) << shift or (int(t[a]) * d + ws // 2) % ws != ws - 1:
                continue
            try:
                e = three_squares(max((a << shift) - d * d, 0), ((a + 1) << shift) - d * d)
            except AssertionError:
                continue
            out.append((d, e))
            if len(out) >= 4:
                return out
    return out
