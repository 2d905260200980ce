"""Integer-defined synthetic inputs for the morph hot path.

Everything here is plain integer arithmetic so that the same bytes can be
produced on any box without OpenCV: the golden generator (container only),
the parity tests and bench.py all draw their inputs from these functions.

gen_pair(w, h)            -> (imgA, imgB)  8UC3 BGR, flat discs/squares on grey
textured_gray(w, h, seed) -> 8UC1 image with block + pixel noise (many FAST corners)
unit_field(w, h, seed)    -> f32x3 field in [0,1] (stand-in for gabor2 in B-stage tests)
point_pairs(w, h, n, seed)-> two float32 point sets (n x 2) with a smooth displacement
"""
import numpy as np

_M64 = (1 << 64) - 1


class XorShift64Star:
    """xorshift64* (Vigna); uniform(lo, hi) = lo + (next() >> 33) % (hi - lo)."""

    def __init__(self, seed):
        self.x = (seed & _M64) or 0x9E3779B97F4A7C15

    def next(self):
        x = self.x
        x ^= x >> 12
        x ^= (x << 25) & _M64
        x ^= x >> 27
        self.x = x
        return (x * 0x2545F4914F6CDD1D) & _M64

    def uniform(self, lo, hi):
        return lo + (self.next() >> 33) % (hi - lo)


def gen(w, h, seed, dx=0, dy=0):
    """40 filled shapes on a (30,30,30) background; odd i = disc, even i = square."""
    img = np.full((h, w, 3), 30, dtype=np.uint8)
    rng = XorShift64Star(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    for i in range(40):
        cx = rng.uniform(w // 8, 7 * w // 8) + dx
        cy = rng.uniform(h // 8, 7 * h // 8) + dy
        r = rng.uniform(max(h // 40, 1), max(h // 10, 2))
        col = [rng.uniform(40, 255) for _ in range(3)]
        if i & 1:
            m = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
        else:
            m = (np.abs(xx - cx) <= r) & (np.abs(yy - cy) <= r)
        img[m] = col
    return img


def gen_pair(w, h, seed=1234):
    return gen(w, h, seed, 0, 0), gen(w, h, seed, w // 50, w // 100)


def _hash32(x, y, seed):
    h = (x.astype(np.uint64) * np.uint64(73856093)) ^ (y.astype(np.uint64) * np.uint64(19349663)) \
        ^ np.uint64((seed * 83492791) & 0xFFFFFFFF)
    h &= np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(0x5BD1E995)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    return h


def textured_gray(w, h, seed=7):
    """Grey version of gen() plus 4x4-block noise (+-40) and pixel noise (+-6)."""
    base = gen(w, h, seed).astype(np.int64)
    g = (base[..., 0] * 29 + base[..., 1] * 150 + base[..., 2] * 77) >> 8
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    nb = (_hash32(xx >> 2, yy >> 2, seed).astype(np.int64) % 81) - 40
    npx = (_hash32(xx, yy, seed + 1).astype(np.int64) % 13) - 6
    return np.clip(g + nb + npx, 0, 255).astype(np.uint8)


def textured_bgr(w, h, seed=7):
    """Colour image with per-channel texture (remap / blend tests)."""
    base = gen(w, h, seed).astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    out = np.empty((h, w, 3), dtype=np.uint8)
    for c in range(3):
        nb = (_hash32(xx >> 3, yy >> 3, seed + 10 * c).astype(np.int64) % 61) - 30
        npx = (_hash32(xx, yy, seed + 10 * c + 1).astype(np.int64) % 17) - 8
        out[..., c] = np.clip(base[..., c] + nb + npx, 0, 255)
    return out


def unit_field(w, h, seed=11):
    """f32x3 field in [0,1]: k/1024 with k from 16x16-block noise + pixel noise."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    out = np.empty((h, w, 3), dtype=np.float32)
    for c in range(3):
        k = (_hash32(xx >> 4, yy >> 4, seed + c).astype(np.int64) % 769) \
            + (_hash32(xx, yy, seed + 3 + c).astype(np.int64) % 256)
        out[..., c] = (k.astype(np.float64) / 1024.0).astype(np.float32)
    return out


def point_pairs(w, h, n, seed=5, dup=2, oob=2):
    """n correspondences: p1 on quarter-pixel lattice, p2 = p1 + smooth shift.

    `dup` exact duplicates and `oob` slightly out-of-range points are appended to
    exercise clip_points / make_uniq (reference src/util.cpp:453-460, 541-548).
    The 4 image corners are appended last, as Matcher::prepare does.
    """
    rng = XorShift64Star(seed)
    p1 = np.empty((n, 2), dtype=np.float32)
    p2 = np.empty((n, 2), dtype=np.float32)
    for i in range(n):
        x = rng.uniform(4 * 2, 4 * (w - 2)) / 4.0
        y = rng.uniform(4 * 2, 4 * (h - 2)) / 4.0
        sx = (w / 50.0) * (0.5 + y / h) + (rng.uniform(0, 17) - 8) / 4.0
        sy = (w / 100.0) * (0.5 + x / w) + (rng.uniform(0, 17) - 8) / 4.0
        p1[i] = (x, y)
        p2[i] = (min(max(x + sx, 0.0), w - 1.0), min(max(y + sy, 0.0), h - 1.0))
    extra1, extra2 = [], []
    for k in range(dup):
        j = rng.uniform(0, n)
        extra1.append(p1[j].copy())
        extra2.append(p2[j].copy())
    for k in range(oob):
        extra1.append(np.array([w + 3.5, h / 2.0 + k], dtype=np.float32))
        extra2.append(np.array([w / 2.0 + k, -2.25], dtype=np.float32))
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], dtype=np.float32)
    a = np.vstack([p1] + [e[None] for e in extra1] + [corners]).astype(np.float32)
    b = np.vstack([p2] + [e[None] for e in extra2] + [corners]).astype(np.float32)
    return a, b


def upscale_bgr(img, w, h):
    """Integer bilinear resize of a u8 image to w x h (16.16 fixed-point source coordinates, pixel centres aligned, result rounded to nearest):
    defined here, in integers, so that every box makes the same pixels from the committed photo fixture (tests/golden/photo_pair_720x405.npz)."""
    sh, sw = img.shape[:2]
    def axis(n_out, n_in):
        c = ((2 * np.arange(n_out, dtype=np.int64) + 1) * n_in * 32768) // n_out - 32768       # source coordinate of the pixel centre, 16.16
        c = np.clip(c, 0, (n_in - 1) << 16)
        i0 = (c >> 16).astype(np.int64)
        return i0, np.minimum(i0 + 1, n_in - 1), (c & 0xffff).astype(np.int64)
    y0, y1, fy = axis(h, sh)
    x0, x1, fx = axis(w, sw)
    a = img.astype(np.int64)
    top = a[y0][:, x0] * (65536 - fx)[None, :, None] + a[y0][:, x1] * fx[None, :, None]
    bot = a[y1][:, x0] * (65536 - fx)[None, :, None] + a[y1][:, x1] * fx[None, :, None]
    out = (top * (65536 - fy)[:, None, None] + bot * fy[:, None, None] + (1 << 31)) >> 32
    return np.ascontiguousarray(out.astype(np.uint8))            # (the fancy indexing above leaves a transposed memory order)


def photo_pair(w, h):
    """The reference's own sample photographs (images/amir1.jpg, amir2.jpg; committed as pixels: tests/golden/photo_pair_720x405.npz) at w x h."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "photo_pair_720x405.npz"))
    return upscale_bgr(z["a"], w, h), upscale_bgr(z["b"], w, h)


def demo_pair(name):
    """One of the reference's own demo pairs of a width that is no multiple of 4 (committed as pixels: tests/golden/demo_pairs.npz, tools/make_demo_fixture.py):
    "numbers" = images/1st.png + 2nd.png (639 x 480), "cars" = images/kindpng1s.png + kindpng2s.png (749 x 480)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "demo_pairs.npz"))
    return np.ascontiguousarray(z[name + "_a"]), np.ascontiguousarray(z[name + "_b"])


def fnv1a64(buf):
    """FNV-1a over the raw bytes of an array (used by the golden manifests)."""
    data = np.ascontiguousarray(buf).view(np.uint8).ravel()
    # vectorised FNV is awkward; process in Python ints on chunks via polynomial trick is
    # overkill here, fixtures are small. Use a simple loop over bytes in blocks.
    hsh = 1469598103934665603
    prime = 1099511628211
    for b in data.tobytes():
        hsh = ((hsh ^ b) * prime) & _M64
    return hsh


# ---- content that reaches the set-up's content-dependent branches on purpose (flat, saturated, two-tone, tie-heavy) ------------------
def as_bgr(gray):
    """A grey image as BGR with three equal channels: cvtColor(BGR2GRAY) gives the grey image back (the weights sum to 1 << 14)."""
    return np.ascontiguousarray(np.repeat(np.asarray(gray, np.uint8)[..., None], 3, axis=2))


def flat_bgr(w, h, value):
    """One colour everywhere: value is a grey level or a (b, g, r) triple.  Foreground and dft_detail2 of it are constant / 0."""
    img = np.empty((h, w, 3), np.uint8)
    img[...] = value
    return img


def checker(w, h, period, lo=0, hi=255, phase=0):
    """Checkerboard of square cells `period` pixels wide, shifted by `phase` pixels along both axes; cell (0, 0) is lo.  Its FAST corners
    come in families of exactly equal scores (the ties retainBest keeps, OCV/features2d/src/keypoint.cpp:69-90)."""
    c = max(int(period), 1)
    yy, xx = np.mgrid[0:h, 0:w]
    odd = (((xx + phase) // c) + ((yy + phase) // c)) & 1
    return np.where(odd == 1, hi, lo).astype(np.uint8)


def checker_bgr(w, h, period, lo=0, hi=255, phase=0):
    return as_bgr(checker(w, h, period, lo, hi, phase))


def plateau(w, h, base, contrast):
    """Flat `base` with four axis-aligned rectangles of exactly base + contrast (clipped to 0..255): every FAST ring difference is 0 or
    +-contrast, so the corner test sits on its threshold (20, strict > in fast.cpp's threshold table) when contrast is 20 or 21."""
    img = np.full((h, w), base, np.uint8)
    v = int(np.clip(base + contrast, 0, 255))
    for fx0, fy0, fx1, fy1 in ((0.2, 0.25, 0.4, 0.5), (0.55, 0.2, 0.8, 0.45), (0.25, 0.6, 0.45, 0.8), (0.6, 0.58, 0.75, 0.82)):
        img[int(fy0 * h):int(fy1 * h), int(fx0 * w):int(fx1 * w)] = v
    return img


def dot_positions(w, h):
    """Positions 0..16 px from each border (0, 1, 6 and 15: the 13 and 31 tap Gabor banks' radii and their window edges; 16 one further)
    plus a few inside, all distinct."""
    out = []
    for d in (0, 1, 6, 15, 16):
        out += [(d, h // 2), (w - 1 - d, h // 3), (w // 3, d), (2 * w // 3, h - 1 - d)]
    out += [(w // 2, h // 2), (w // 4, h // 4), (3 * w // 4, 3 * h // 4)]
    return sorted(set(out))


def dots(w, h, positions=None, value=255, size=1):
    """Black image with single pixels (size 1) or size x size squares (centred; clipped at the border) of `value` at `positions`."""
    img = np.zeros((h, w), np.uint8)
    r = size // 2
    for x, y in (dot_positions(w, h) if positions is None else positions):
        img[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = value
    return img


def rings(w, h, radii=(6, 12, 20, 30, 44), lo=0, hi=255):
    """Concentric bands about the image centre, symmetric about both image axes: the intensity-centroid moments (ICAngles,
    OCV/features2d/src/orb.cpp:181-215) of every point on an axis vanish.  Band k is hi for even k, lo for odd k; r is measured in half pixels."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    r2 = (2 * xx - (w - 1)) ** 2 + (2 * yy - (h - 1)) ** 2           # (2 r)^2: exact for even and odd sizes
    band = np.zeros((h, w), np.int64)
    for rr in radii:
        band += r2 > (2 * rr) ** 2
    return np.where(band % 2 == 0, hi, lo).astype(np.uint8)


def near_flat(w, h, value=77, x=None, y=None, delta=1):
    """Flat `value` with one pixel off by `delta` (at the centre unless given)."""
    img = np.full((h, w), value, np.uint8)
    x = w // 2 if x is None else x
    y = h // 2 if y is None else y
    img[y, x] = np.uint8(int(np.clip(value + delta, 0, 255)))
    return img


def uniform_noise(w, h, seed=3, channels=1):
    """Independent uniform bytes from the hash (no block structure): FAST fires nearly everywhere."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    planes = [(_hash32(xx, yy, seed + 7 * c) & np.uint64(0xFF)).astype(np.uint8) for c in range(channels)]
    return planes[0] if channels == 1 else np.ascontiguousarray(np.stack(planes, axis=2))


def channel_stripes(w, h, period=6):
    """Vertical stripes of pure blue, green and red (255 in one channel, 0 in the others) between black ones, each period // 2 wide:
    the grey conversion's rounding on single-channel input."""
    img = np.zeros((h, w, 3), np.uint8)
    c = max(period // 2, 1)
    k = np.arange(w) // c
    for ch in range(3):
        img[:, k % 6 == 2 * ch, ch] = 255
    return img
