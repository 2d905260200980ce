"""Images built so that plane values of the Gabor banks land exactly on, just beside, or just outside the doubt band around the
midpoint between two floats — the places where the FFT form of the banks (k_gabor_fft<13>, k_gabor_fft<31>, k_gabor_redo in
poppy_amd/csrc/kernels_gabor_fft.hip) equals the direct double sums only through its doubt rule (rounding_in_doubt, gabor_doubt.h) and
the hand-over to k_gabor_redo, or, just outside the band, only through the transform's accuracy.  On textures such values turn up
about once in 1e8; here every target pixel holds one.

The 13 x 13 x 3 bank (ctx.gabor_field) runs on bytes / 255 and byte 255 is exactly 1.0f, so a window with two white pixels on black
has the exact plane value K[i] + K[j]: 9 979 (orientation, tap pair) combinations of the 14 196 tap pairs are exact midpoints in
(0, 1), and for 1 227 of them the other rounding changes the output float after the clamp, the float sum over 16 orientations and
/ 16 (tie_rows).  Two pixels of arbitrary byte values give K[i] p + K[j] q rounded once to double: a seeded search over those finds
values within 1e-14 of a midpoint and values between 1.0 and 1.5 bands from one (near_tie_rows).  The 31 x 31 bank (ctx.orb_input)
runs on the unsharp-masked grey image, which cannot be placed exactly: tools/find_gabor31_near_ties.py searches two-dot images with
the oracle's planes and writes what it finds into GABOR31_ROWS below.

classify is written from IEEE arithmetic (np.frexp), not from the kernel's code; the band per tile follows the kernel's geometry
(block side 52 / 34, a 64 x 64 reflect-101 patch) and takes its unit from the library (capi.gabor_band_unit), so no copy of the
number lives here.  tests/test_oracle_gabor_ties.py asserts from the oracle alone that every builder reaches what it is built for;
tests/test_gpu_gabor_ties.py compares the kernels with the oracle and with the library's direct form on them.

A builder returns (image, [Target]).  Target: x, y, ch the pixel and channel, o the orientation whose plane holds the value, up
whether the float nearest to the value (ties to even) lies above it, mult the largest number of taps of the window that read one of
the two placed pixels (1: no mirror, 2: mirrored once, 4: mirrored in x and in y), dist the value's signed distance to the midpoint
the builder computed.

GABOR31_ROWS: 14 rows (6 inside, 8 outside) kept of 6 inside and 45 outside found in
320 two-dot images (116 s of CPU); the smallest distance found is 2.2e-15 in units of the tile's
max(1, max |us|) (the first row)."""
import collections
import functools

import numpy as np

import oracle_lib as O

KS13, KS31 = 13, 31
BLOCK13, BLOCK31 = 64 - KS13 + 1, 64 - KS31 + 1           # 52, 34: the output pixels a tile of the FFT form owns, per side
PATCH = 64
REDO_TRIP = 512 * 16                                      # entries one trip of k_gabor_redo's 512 workgroups takes
INSIDE = 1e-14                                            # "inside" near-ties lie at most this far from a midpoint
MIN_VALUE = 2.0 ** -13                                    # near-tie targets are at least this large: the floats there are 2^-36 = 1.5e-11 apart, 145 bands
W31, H31 = 96, 64                                         # the two-dot images of the 31-tap rows

Target = collections.namedtuple("Target", "x y ch o up mult dist")
Classes = collections.namedtuple("Classes", "mid zero doubt")


@functools.lru_cache(maxsize=None)
def band_unit():
    from poppy_amd import capi
    return capi.gabor_band_unit()


@functools.lru_cache(maxsize=None)
def bank(ks):
    """(16, ks, ks) float32: tap (dy, dx) multiplies the pixel at (x + dx - ks // 2, y + dy - ks // 2)."""
    b = O.gabor_bank(ks, 5, 10 if ks == KS13 else 2)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def byte_floats():
    """The 256 floats byte / 255 as the 13-tap bank sees them."""
    t = O.u8_to_f32(np.arange(256, dtype=np.uint8).reshape(1, 256))[0].astype(np.float64)
    assert t[255] == 1.0 and t[0] == 0.0
    return t


def reflect101(p, n):
    """borderInterpolate(p, n, BORDER_REFLECT_101), any distance outside (ints or integer arrays)."""
    if n == 1:
        return p * 0
    q = np.mod(p, 2 * (n - 1))
    return np.where(q < n, q, 2 * (n - 1) - q) if isinstance(q, np.ndarray) else (q if q < n else 2 * (n - 1) - q)


# ---- IEEE: where a double lies between the floats ------------------------------------------------------------------------------------
def classify(planes, band):
    """Per plane value (float64, any shape; band broadcasts against it):
    mid    the signed distance v - m to the nearest midpoint m between two neighbouring floats.  In [2^e, 2^(e + 1)) the floats are
           2^(e - 23) apart; just above a power of two the nearest midpoint can be the one below it, where the floats are half as far
           apart.  (Below 2^-126 the spacing is that of the subnormals.)
    zero   |v|
    doubt  0 / 1 / 2 as the FFT form's rule states it: nothing outside [-band, 1 + band] (clamped either way), 1 below band (near
           zero), 2 within band of a midpoint."""
    v = np.asarray(planes, np.float64)
    a = np.abs(v)
    _, e = np.frexp(a)                                    # a = m 2^e, m in [0.5, 1): a in [2^(e - 1), 2^e)
    e = np.maximum(e, -125)
    sp = np.ldexp(1.0, e - 24)                            # the spacing of the floats in a's binade
    u = a / sp                                            # exact (a power of two), < 2^24
    k = np.floor(u)
    fr = u - k                                            # exact: the position between float k and float k + 1
    mid = (fr - 0.5) * sp
    below = (k == 2.0 ** 23) & (fr < 0.125)               # nearer to the midpoint below the power of two: a quarter spacing below it
    mid = np.where(below, (fr + 0.25) * sp, mid)
    mid = np.where(v < 0, -mid, mid)
    band = np.broadcast_to(np.asarray(band, np.float64), v.shape)
    doubt = np.where((v < -band) | (v > 1.0 + band), 0, np.where(v < band, 1, np.where(np.abs(mid) < band, 2, 0)))
    return Classes(mid, a, doubt.astype(np.int8))


def other_float(v):
    """The float on the other side of v from the one nearest to it."""
    v = np.asarray(v, np.float64)
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))).astype(np.float32)


def rounds_up(v):
    v = np.asarray(v, np.float64)
    return v.astype(np.float32).astype(np.float64) > v


def field_of(plane_floats):
    """gabor_filter's output of the 16 float planes (..., 16): clamp to [0, 1], sum in float in orientation order, / 16."""
    c = np.clip(np.asarray(plane_floats, np.float32), np.float32(0), np.float32(1))
    acc = np.zeros(c.shape[:-1], np.float32)
    for a in range(16):
        acc = acc + c[..., a]
    return acc * np.float32(0.0625)


def visible(planes16, o):
    """Does rounding plane o of the pixel(s) (..., 16 doubles) to the other neighbour change the output float?"""
    p = np.asarray(planes16, np.float64)
    f = p.astype(np.float32)
    g = f.copy()
    idx = np.asarray(o)
    alt = other_float(np.take_along_axis(p, idx[..., None], -1)[..., 0])
    np.put_along_axis(g, idx[..., None], alt[..., None], -1)
    return field_of(f) != field_of(g)


# ---- the kernel's band per tile -------------------------------------------------------------------------------------------------------
def band13():
    """Fixed for the 13-tap bank: its input is bytes / 255, at most 1."""
    return band_unit()


def band31(us, x, y):
    """unit x max(1, max |us|) over the 64 x 64 reflect-101 patch of the tile that owns pixel (x, y)."""
    h, w = us.shape
    bx, by = x // BLOCK31 * BLOCK31, y // BLOCK31 * BLOCK31
    r = KS31 // 2
    ys = reflect101(np.arange(by - r, by - r + PATCH), h)
    xs = reflect101(np.arange(bx - r, bx - r + PATCH), w)
    amax = np.float32(np.abs(us[np.ix_(ys, xs)]).max())
    return band_unit() * float(max(np.float32(1), amax))


def band31_map(us):
    """band31 for every pixel."""
    h, w = us.shape
    out = np.empty((h, w), np.float64)
    for by in range(0, h, BLOCK31):
        for bx in range(0, w, BLOCK31):
            out[by:by + BLOCK31, bx:bx + BLOCK31] = band31(us, bx, by)
    return out


# ---- exact ties of the 13-tap bank ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_rows():
    """Every (orientation o, tap pair i < j) whose K[o, i] + K[o, j] is exactly the midpoint of two floats in (0, 1) and whose other
    rounding shows in the output float: arrays i, j, o, up, sorted."""
    K = bank(KS13).astype(np.float64).reshape(16, -1)
    i, j = np.triu_indices(KS13 * KS13, 1)
    s = (K[:, i] + K[:, j]).T                             # (pairs, 16), every sum exact in double
    c = classify(s, 0.0)
    tie = (c.mid == 0) & (s > 0) & (s < 1)
    p, o = np.nonzero(tie)
    vis = visible(s[p], o)
    p, o = p[vis], o[vis]
    return i[p], j[p], o, rounds_up(s[p, o])


def _pick_tie(t):
    """The t-th choice: orientation t % 16, direction (t // 16) % 2, then through that group's rows."""
    i, j, o, up = tie_rows()
    sel = np.nonzero((o == t % 16) & (up == bool((t // 16) % 2)))[0]
    assert len(sel), (t % 16, (t // 16) % 2)
    k = sel[(t // 32 * 7 + t) % len(sel)]
    return int(i[k]), int(j[k]), int(o[k]), bool(up[k])


def _put(img, x, y, ch, tap, value):
    img[y + tap // KS13 - KS13 // 2, x + tap % KS13 - KS13 // 2, ch] = value


def _disjoint(positions):
    for a in range(len(positions)):
        for b in range(a):
            if abs(positions[a][0] - positions[b][0]) < KS13 and abs(positions[a][1] - positions[b][1]) < KS13:
                return False
    return True


# targets at block coordinates 51 and 0 in x (51, 52, 103, 104) and in y (51, 52), one in a tile's interior, some in the ragged last blocks
# (x >= 104, y >= 52), the rest filled in; every window lies inside the image and no two windows share a pixel
_BLACK_FIRST = [(51, 25), (52, 38), (25, 51), (38, 52), (51, 51), (103, 12), (104, 25), (90, 51), (104, 38), (12, 12), (110, 60), (70, 63)]


@functools.lru_cache(maxsize=None)
def _black_positions(w, h):
    pos = [p for p in _BLACK_FIRST if p[0] < w - 6 and p[1] < h - 6]
    for y in range(6, h - 6):
        for x in range(6, w - 6):
            if all(abs(x - px) >= KS13 or abs(y - py) >= KS13 for px, py in pos):
                pos.append((x, y))
    assert _disjoint(pos)
    return tuple(pos)


def _place_on_black(w, h, rows):
    """One target per position and channel; rows(t) -> (tap i, byte, tap j, byte, o, up, dist)."""
    img = np.zeros((h, w, 3), np.uint8)
    targets = []
    for n, (x, y) in enumerate(_black_positions(w, h)):
        for ch in range(3):
            i, bi, j, bj, o, up, dist = rows(3 * n + ch)
            _put(img, x, y, ch, i, bi); _put(img, x, y, ch, j, bj)
            targets.append(Target(x, y, ch, o, up, 1, dist))
    return img, targets


def _tie_row(t):
    i, j, o, up = _pick_tie(t)
    return i, 255, j, 255, o, up, 0.0


def ties_on_black(w=120, h=70):
    """White pixel pairs on black, one pair per target pixel and channel, each an exact tie whose other rounding is visible."""
    return _place_on_black(w, h, _tie_row)


def saturated_noise(w, h, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def _place_in_noise(w, h, rows, seed):
    """0 / 255 noise in all channels; 13 x 13 black squares at pitch 16, each the window of its centre pixel, one target per square and channel."""
    img = saturated_noise(w, h, seed)
    targets = []
    t = 0
    for sy in range(h // 16):
        for sx in range(w // 16):
            x, y = 16 * sx + 1 + KS13 // 2, 16 * sy + 1 + KS13 // 2
            img[y - 6:y + 7, x - 6:x + 7, :] = 0
            for ch in range(3):
                i, bi, j, bj, o, up, dist = rows(t)
                _put(img, x, y, ch, i, bi); _put(img, x, y, ch, j, bj)
                targets.append(Target(x, y, ch, o, up, 1, dist))
                t += 1
    return img, targets


def ties_in_noise(w=256, h=192):
    """Exact ties (still K[i] + K[j]) inside patches of close to the largest norm a byte image can have."""
    return _place_in_noise(w, h, _tie_row, 31)


def many_listed():
    """ties_in_noise at 1024 x 768: 3 072 squares x 3 channels, more entries than one trip of k_gabor_redo takes."""
    return ties_in_noise(1024, 768)


# ---- exact ties through mirrored windows ---------------------------------------------------------------------------------------------
def _window_hits(x, y, w, h):
    """(13, 13) arrays of the image row and column each tap of pixel (x, y)'s window reads."""
    iy = reflect101(np.arange(y - 6, y + 7), h)
    ix = reflect101(np.arange(x - 6, x + 7), w)
    return np.repeat(iy[:, None], KS13, 1), np.repeat(ix[None, :], KS13, 0)


def _ordered_planes(IY, IX, p, q):
    """The 16 sums of a window whose image pixels p and q (y, x) are white, added tap by tap in the oracle's order."""
    K = bank(KS13).astype(np.float64).reshape(16, -1)
    hit = np.nonzero((((IY == p[0]) & (IX == p[1])) | ((IY == q[0]) & (IX == q[1]))).ravel())[0]
    acc = np.zeros(16)
    for k in hit:
        acc = acc + K[:, k]
    return acc


def _border_tie(x, y, w, h, want_mult, skip):
    """Search the pairs of image pixels in pixel (x, y)'s window, at least one of them read by want_mult taps, for an exact tie in (0, 1)
    whose other rounding is visible; the skip-th hit in search order.  -> (p, q, o, up, mult)."""
    IY, IX = _window_hits(x, y, w, h)
    K = bank(KS13).astype(np.float64)
    ys, xs = np.unique(IY), np.unique(IX)
    eff = np.zeros((16, h, w))
    np.add.at(eff, (slice(None), IY, IX), K)
    mult = np.zeros((h, w), np.int64)
    np.add.at(mult, (IY, IX), 1)
    py, px = [g.ravel() for g in np.meshgrid(ys, xs, indexing="ij")]
    a, b = np.triu_indices(len(py), 1)
    m = np.maximum(mult[py[a], px[a]], mult[py[b], px[b]])
    keep = m >= want_mult
    a, b, m = a[keep], b[keep], m[keep]
    s = (eff[:, py[a], px[a]] + eff[:, py[b], px[b]]).T   # (pairs, 16): a first look; the order of the additions is settled below
    c = classify(s, 0.0)
    cand, co = np.nonzero((c.mid == 0) & (s > 0) & (s < 1))
    for n, o in zip(cand, co):
        p, q = (int(py[a[n]]), int(px[a[n]])), (int(py[b[n]]), int(px[b[n]]))
        planes = _ordered_planes(IY, IX, p, q)
        if classify(planes[o], 0.0).mid != 0 or not 0 < planes[o] < 1 or not visible(planes, np.int64(o)):
            continue
        if skip == 0:
            return p, q, int(o), bool(rounds_up(planes[o])), int(m[n])
        skip -= 1
    raise AssertionError(f"no visible tie with a pixel read {want_mult} times in the window of ({x}, {y}) of a {w} x {h} image")


# (x, y, the largest number of taps that must read one placed pixel): along every border mirrored once, in every corner twice
_BORDER_POS = {
    (120, 70): [(0, 0, 4), (117, 2, 4), (3, 66, 4), (119, 69, 4), (0, 20, 2), (3, 40, 2), (119, 20, 2), (115, 45, 2),
                (30, 0, 2), (60, 4, 2), (90, 2, 2), (30, 69, 2), (60, 65, 2), (90, 67, 2)],
    (20, 12): [(3, 5, 4), (16, 2, 4)],
}


@functools.lru_cache(maxsize=None)
def _border_rows(w, h):
    pos = _BORDER_POS[(w, h)]
    assert _disjoint([(x, y) for x, y, _ in pos])
    return tuple((x, y, ch, _border_tie(x, y, w, h, mult, 3 * ch)) for x, y, mult in pos for ch in range(3))


def ties_at_borders(w=120, h=70):
    """White pixel pairs within 6 px of every border and corner (also on 20 x 12): reflect-101 mirrors a white pixel into the window a
    second (fourth) time, so the exact value is a sum of three to eight taps.  The ties are found by search, one per position and channel."""
    img = np.zeros((h, w, 3), np.uint8)
    targets = []
    for x, y, ch, (p, q, o, up, mult) in _border_rows(w, h):
        img[p[0], p[1], ch] = 255; img[q[0], q[1], ch] = 255
        targets.append(Target(x, y, ch, o, up, mult, 0.0))
    return img, targets


# ---- near-ties of the 13-tap bank -----------------------------------------------------------------------------------------------------
NEAR_QUOTA = {"inside": 6, "outside": 24}                 # rows per kind and side (the inside ones are the rare ones)
NEAR_DRAWS = 64                                           # (orientation, tap pair) draws per batch: 64 x 65 536 values
NEAR_BATCHES = 40


@functools.lru_cache(maxsize=None)
def near_tie_rows():
    """Seeded search over two pixels of arbitrary byte values p, q under taps i < j: the plane value K[o, i] p + K[o, j] q (exact
    products, one rounding to double, as the oracle and the direct kernel form it).  -> {"inside": rows, "outside": rows}, a row being
    (i, byte, j, byte, o, up, dist): inside 0 < |dist| <= 1e-14, outside band < |dist| <= 1.5 band with no plane of the pixel in doubt;
    both sides of the midpoint in equal numbers, the other rounding visible in the output."""
    K = bank(KS13).astype(np.float64).reshape(16, -1)
    P = byte_floats()
    band = band13()
    rng = np.random.default_rng(20240607)
    rows = {("inside", False): [], ("inside", True): [], ("outside", False): [], ("outside", True): []}
    for _ in range(NEAR_BATCHES):
        o = rng.integers(0, 16, NEAR_DRAWS)
        i = rng.integers(0, KS13 * KS13 - 1, NEAR_DRAWS)
        j = rng.integers(i + 1, KS13 * KS13)
        v = (K[o, i][:, None] * P[None, :])[:, :, None] + (K[o, j][:, None] * P[None, :])[:, None, :]     # (draw, byte of i, byte of j)
        f = v.astype(np.float32)                            # classify's distance, lean (the search is most of this module's time): v = f + r, the
        r = v - f                                           # midpoints half a spacing from f; every kept row is checked against classify below
        d = r - np.copysign(0.5 * np.spacing(np.abs(f)).astype(np.float64), r)
        for n, bi, bj in zip(*np.nonzero(np.abs(d) <= 1.5 * band)):
            dist, val = abs(d[n, bi, bj]), v[n, bi, bj]
            kind = "inside" if 0 < dist <= INSIDE else "outside" if dist > band else None
            if kind and MIN_VALUE <= val < 1:
                side = bool(d[n, bi, bj] > 0)
                if len(rows[(kind, side)]) >= NEAR_QUOTA[kind]:
                    continue
                planes = K[:, i[n]] * P[bi] + K[:, j[n]] * P[bj]
                assert planes[o[n]] == v[n, bi, bj] and classify(planes[o[n]], band).mid == d[n, bi, bj]
                if not visible(planes, o[n]) or (kind == "outside" and classify(planes, band).doubt.any()):
                    continue
                rows[(kind, side)].append((int(i[n]), int(bi), int(j[n]), int(bj), int(o[n]), bool(rounds_up(planes[o[n]])), float(d[n, bi, bj])))
        if all(len(r) >= NEAR_QUOTA[k[0]] for k, r in rows.items()):
            break
    out = {}
    for kind in ("inside", "outside"):
        a, b = rows[(kind, False)], rows[(kind, True)]
        assert len(a) == len(b) == NEAR_QUOTA[kind], (kind, len(a), len(b))
        out[kind] = tuple(r for pair in zip(a, b) for r in pair)          # alternating sides
    return out


def near_ties(kind, layout="black"):
    """Two pixels of arbitrary byte values per target: kind "inside" (within 1e-14 of a midpoint: in doubt) or "outside" (between 1.0 and
    1.5 bands from one: not in doubt, the equality of the forms rests on the transform's accuracy); layout "black" (as ties_on_black) or
    "noise" (as ties_in_noise)."""
    rows = near_tie_rows()[kind]
    pick = lambda t: rows[t % len(rows)]
    return _place_on_black(120, 70, pick) if layout == "black" else _place_in_noise(256, 192, pick, 32)


# ---- the 31-tap bank: two-dot grey images found by tools/find_gabor31_near_ties.py ----------------------------------------------------
def dots31(row):
    """The 96 x 64 grey image of a GABOR31_ROWS row — two 3 x 3 dots, top left corners and bytes from the row (a single pixel comes out of the
    unsharp mask as itself; around a 3 x 3 white dot us reaches 5.4 and -0.7) — and its Target."""
    kind, x1, y1, b1, x2, y2, b2, tx, ty, o, dist = row
    gf = np.zeros((H31, W31), np.uint8)
    gf[y1:y1 + 3, x1:x1 + 3] = b1; gf[y2:y2 + 3, x2:x2 + 3] = b2
    return gf, Target(tx, ty, 0, o, None, 1, dist)


# (kind, x1, y1, byte1, x2, y2, byte2, target x, target y, orientation, signed distance to the midpoint)
# BEGIN GABOR31_ROWS (written by tools/find_gabor31_near_ties.py)
GABOR31_ROWS = [
    ('inside', 53, 1, 8, 70, 44, 255, 69, 17, 0, -1.1581013925621164e-14),
    ('inside', 29, 16, 58, 72, 47, 255, 40, 24, 2, -1.2878587085651816e-14),
    ('inside', 62, 20, 8, 36, 46, 247, 20, 47, 5, -1.7763568394002505e-14),
    ('inside', 3, 27, 155, 66, 41, 29, 77, 49, 2, -6.439293542825908e-15),
    ('inside', 94, 38, 66, 44, 46, 67, 33, 35, 6, -9.992007221626409e-15),
    ('inside', 43, 19, 245, 76, 28, 77, 66, 17, 9, 4.474198789239381e-14),
    ('outside', 51, 44, 12, 82, 24, 255, 56, 51, 12, -5.366054822708577e-13),
    ('outside', 90, 5, 11, 89, 44, 255, 81, 20, 11, -5.373028411082004e-13),
    ('outside', 76, 45, 113, 9, 48, 255, 66, 33, 7, 2.3925306180672123e-13),
    ('outside', 48, 36, 255, 29, 56, 54, 18, 44, 5, 5.42343947529389e-13),
    ('outside', 79, 32, 23, 51, 16, 255, 91, 26, 14, 5.439815264907111e-13),
    ('outside', 23, 36, 239, 55, 42, 255, 41, 20, 8, 5.647982082024328e-13),
    ('outside', 21, 25, 253, 70, 23, 255, 29, 43, 14, -5.706546346573305e-13),
    ('outside', 29, 15, 255, 41, 49, 75, 55, 35, 4, -1.7214007996813052e-13),
]
# END GABOR31_ROWS
