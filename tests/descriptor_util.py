"""Inputs built to reach the branches of the descriptor path (k_orb_blur, k_orb_describe, k_hamming, k_hamming_knn2 in
poppy_amd/csrc/kernels_orb.hip; OrbDetector::describe / hamming / hamming_knn2; poppy_hip_pair_begin_descriptors) that keypoints
from the detector on fixture images never reach, and plain numpy restatements of what those kernels compute: ORB::compute at
octave 0, the Hamming 1-NN and 2-NN, the ratio and symmetry rule.  Everything is deterministic from seeds.  NaN and infinite angles
and coordinates are not pinned (cvRound of NaN indexes out of the atlas in the oracle).  tests/test_oracle_descriptors.py asserts
from numpy and the oracle alone that every family reaches what it is built for; tests/test_gpu_descriptors.py compares the kernels
with the oracle and the numpy references on them.

A describe family is a list of (label, image, kps7); the kps7 columns are x, y, size, angle, response, octave, class id."""
import ctypes as C
import ctypes.util
import functools
import os

import numpy as np

import oracle_lib as O
from poppy_amd import synth

W, H = 64, 48
SMALL_W, SMALL_H = 20, 16
LEVELS = 8                                          # kOrbLevels
BORDER = 32                                         # kOrbBorder: the reflect-101 ring around every level
# OrbDetector::describe takes a keypoint whose rounded level position lies in [23 - kOrbBorder, L.w + kOrbBorder - 23) on x and the
# same with L.h on y, and refuses the rest: a steered pattern point lies at most sqrt(13^2 + 13^2) < 19 px from the centre
REACH = 23
ACCEPT_LO = REACH - BORDER                          # -9
ACCEPT_PAST = BORDER - REACH                        # L.w + 9 is the first refused coordinate, L.w + 8 the last accepted one
KP_CAP = 1 << 16                                    # OrbDetector's first keypoint buffers; more makes describe call grow_keypoints

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = _libm.sinf.restype = C.c_float
_libm.cosf.argtypes = _libm.sinf.argtypes = [C.c_float]


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


@functools.lru_cache(maxsize=None)
def pattern():
    """The 256 rBRIEF test pairs as (512, 2) float32 (x, y): points 2 i and 2 i + 1 are compared for bit i."""
    path = os.path.join(O.ORACLE_DIR, "orb_pattern.inc")
    with open(path) as f:
        text = "".join(line for line in f if not line.lstrip().startswith("//"))
    v = np.array([int(t) for t in text.replace("\n", "").split(",") if t.strip()], np.float32)
    assert v.size == 1024
    v = v.reshape(512, 2)
    v.setflags(write=False)
    return v


# ---- level geometry (orb.cpp:1033-1060: scale 1.2f stored as a double, sizes cvRound(size / scale)) ----------------------------------
@functools.lru_cache(maxsize=None)
def levels(w, h):
    """[(level width, level height, scale f32, 1 / scale f32)] of the 8 levels."""
    out = []
    for l in range(LEVELS):
        scale = np.float32(np.float64(np.float32(1.2)) ** l)
        inv = np.float32(1) / scale
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv)), scale, inv))
    return out


def level_position(kps7, w, h):
    """Rounded level positions (cx, cy) of kps7 rows: cvRound(pt * (1 / scale)), half to even."""
    k = _f32(kps7).reshape(-1, 7)
    inv = np.array([levels(w, h)[int(o)][3] for o in k[:, 5]], np.float32)
    return np.rint(k[:, 0] * inv).astype(np.int64), np.rint(k[:, 1] * inv).astype(np.int64)


def image_position(target, octave, w, h):
    """An image coordinate (float32) that rounds to level coordinate `target` at `octave`."""
    _, _, scale, inv = levels(w, h)[octave]
    x = np.float32(np.float32(target) * scale)
    assert int(np.rint(x * inv)) == target, (target, octave)
    return x


# ---- the steered pattern --------------------------------------------------------------------------------------------------------------
def cos_sin(angle):
    """(cos, sin) of a keypoint angle in degrees as orb.cpp:236 computes them: angle *= (float)(CV_PI / 180), then the float cosine and
    sine of the C library (the calls the oracle and the library make; numpy's own float32 routines are SIMD code that need not round alike)."""
    rad = np.float32(angle) * np.float32(np.pi / np.float64(np.float32(180)))
    return np.float32(_libm.cosf(float(rad))), np.float32(_libm.sinf(float(rad)))


def steered(angle, contract=0):
    """(x, y) float32 arrays of the 512 rotated pattern points before rounding: x = px a - py b, y = px b + py a, every product and sum
    rounded to float32.  contract = 1 keeps the first product of each expression exact as fma(px, a, -(py b)) / fma(px, b, py a) do,
    contract = 2 the second one (fma(-py, b, px a) / fma(py, a, px b)); a pattern coordinate has 4 bits, so the exact product of it and
    a float32, and its sum with a float32 of similar size, are exact in float64."""
    a, b = cos_sin(angle)
    px, py = pattern()[:, 0], pattern()[:, 1]
    if contract == 0:
        return px * a - py * b, px * b + py * a
    d = np.float64
    if contract == 1:
        return _f32(px.astype(d) * d(a) - (py * b).astype(d)), _f32(px.astype(d) * d(b) + (py * a).astype(d))
    return _f32((px * a).astype(d) - py.astype(d) * d(b)), _f32((px * b).astype(d) + py.astype(d) * d(a))


def _round(v, rounding):
    if rounding == "half_even":
        return np.rint(v).astype(np.int64)
    assert rounding == "half_up"
    return np.floor(v.astype(np.float64) + 0.5).astype(np.int64)


def offsets(angle, rounding="half_even", contract=0):
    """Integer (dx, dy) of the 512 pattern points around the keypoint."""
    x, y = steered(angle, contract)
    return _round(x, rounding), _round(y, rounding)


def half_tie_count(angle):
    """How many of the 1024 steered coordinates are exactly k + 0.5, and how many of those round-half-up moves (k even)."""
    v = np.concatenate(steered(angle)).astype(np.float64)
    tie = v - np.floor(v) == 0.5
    return int(tie.sum()), int((tie & (np.floor(v) % 2 == 0)).sum())


def patch_reads(kps7, w, h):
    """Level coordinates every keypoint reads, any octave: (X, Y) of shape (n, 512), and the keypoints' (level w, level h)."""
    k = _f32(kps7).reshape(-1, 7)
    cx, cy = level_position(k, w, h)
    X = np.empty((len(k), 512), np.int64); Y = np.empty((len(k), 512), np.int64)
    for i in range(len(k)):
        dx, dy = offsets(k[i, 3])
        X[i] = cx[i] + dx; Y[i] = cy[i] + dy
    size = np.array([levels(w, h)[int(o)][:2] for o in k[:, 5]], np.int64).reshape(-1, 2)
    return X, Y, size[:, 0], size[:, 1]


# ---- ORB::compute at octave 0 in numpy ------------------------------------------------------------------------------------------------
GAUSS7 = np.array([float.fromhex(t) for t in ("0x1.1f5f62p-4", "0x1.0c70fcp-3", "0x1.869472p-3", "0x1.ba95c0p-3",
                                              "0x1.869472p-3", "0x1.0c70fcp-3", "0x1.1f5f62p-4")], np.float32)


def reflect101(p, n):
    """borderInterpolate(BORDER_REFLECT_101), as often as it takes."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n - 2)
    return np.where(q >= n, 2 * n - 2 - q, q)


def padded(img):
    """The level inside its reflect-101 ring of 32."""
    g = np.asarray(img, np.uint8)
    h, w = g.shape
    return g[reflect101(np.arange(-BORDER, h + BORDER), h)][:, reflect101(np.arange(-BORDER, w + BORDER), w)]


def blurred_level0(img):
    """GaussianBlur(7 x 7, sigma 2) of the level in place inside the padded atlas: float32 row pass acc = k0 s0; acc += kj sj, column pass
    acc = k3 c + 0; acc += kj (c[+j] + c[-j]), round half to even, clamp to 8 bits; the ring keeps the unblurred pixels."""
    h, w = np.asarray(img).shape
    P = padded(img)
    F = P.astype(np.float32)
    B = BORDER
    rows = F[B - 3:B + h + 3]                                                       # the rows the column pass reads
    acc = GAUSS7[0] * rows[:, B - 3:B - 3 + w]
    for j in range(1, 7):
        acc = acc + GAUSS7[j] * rows[:, B - 3 + j:B - 3 + j + w]
    r = acc                                                                         # (h + 6, w)
    col = GAUSS7[3] * r[3:3 + h] + np.float32(0)
    for j in range(1, 4):
        col = col + GAUSS7[3 + j] * (r[3 + j:3 + j + h] + r[3 - j:3 - j + h])
    assert col.dtype == np.float32
    out = P.copy()
    out[B:B + h, B:B + w] = np.clip(np.rint(col), 0, 255).astype(np.uint8)
    return out


def describe_level0(img, kps7, rounding="half_even", contract=0, strict=True):
    """ORB::compute (WTA_K 2) of octave-0 keypoints: (n, 32) uint8.  The three switches restate the kernel errors the families are built
    to detect: rounding="half_up" instead of cvRound's half to even, contract=1|2 with one product of the rotation fused, strict=False
    with <= in place of <."""
    k = _f32(kps7).reshape(-1, 7)
    assert (k[:, 5] == 0).all()
    blur = blurred_level0(img).astype(np.int64)
    cx = np.rint(k[:, 0]).astype(np.int64); cy = np.rint(k[:, 1]).astype(np.int64)          # 1 / scale is 1
    out = np.zeros((len(k), 32), np.uint8)
    for i in range(len(k)):
        dx, dy = offsets(k[i, 3], rounding, contract)
        v = blur[cy[i] + BORDER + dy, cx[i] + BORDER + dx]
        bits = (v[0::2] < v[1::2]) if strict else (v[0::2] <= v[1::2])
        out[i] = np.packbits(bits.astype(np.uint8), bitorder="little")
    return out


def level0_rows(kps7):
    return np.flatnonzero(_f32(kps7).reshape(-1, 7)[:, 5] == 0)


# ---- describe families ----------------------------------------------------------------------------------------------------------------
def kp_row(x, y, angle, octave=0):
    return [x, y, 31.0, angle, 1.0, octave, -1.0]


def _kps(rows):
    return _f32(rows).reshape(-1, 7)


@functools.lru_cache(maxsize=None)
def noise(w=W, h=H, seed=41):
    g = synth.uniform_noise(w, h, seed)
    g.setflags(write=False)
    return g


def level_centre(octave, w, h):
    lw, lh, _, _ = levels(w, h)[octave]
    return image_position(lw // 2, octave, w, h), image_position(lh // 2, octave, w, h)


# angle: (steered coordinates that are exactly k + 0.5, those of them that round-half-up moves).  sinf gives exactly 0.5 at 30 degrees and
# at the next float32 above it.  60 and 210 degrees look like candidates and have none: the C library's correctly rounded cosf and sinf
# give 0.49999997 and -0.49999997 there (a routine that is one ulp off and returns 0.5 would count 2 and 4), and neither do the other
# multiples of 30 or 45 degrees.  They stay in the family as contrast.
TIE_ANGLES = {30.0: (24, 11), 30.000001907348633: (24, 11)}
CONTRAST_ANGLES = [60.0, 210.0, 0.0, 45.0, 90.0, 180.0, 270.0]
INTERIOR = [(32.0, 24.0), (33.0, 19.0), (41.0, 20.0)]           # where the 11 moved coordinates flip at least one bit on the noise image


def half_ties():
    rows = []
    for a in list(TIE_ANGLES) + CONTRAST_ANGLES:
        rows += [kp_row(x, y, a) for x, y in INTERIOR]
        rows += [kp_row(*level_centre(o, W, H), a, o) for o in range(1, LEVELS)]
    return [("half_ties", noise(), _kps(rows))]


# Angles at which a rounded pattern coordinate differs when one product of the rotation is fused (found by solving r cos(t + phi) =
# k + 0.5 for a pattern point and scanning the neighbouring float32 angles), with the position on the 64 x 48 noise image at which the
# descriptor differs too.  (angle, x, y, the fused forms it detects).  tests/test_oracle_descriptors.py re-derives that they qualify.
CONTRACTION_ROWS = [
    (2.396374464035034, 32.0, 24.0, (2,)),
    (2.5387227535247803, 32.0, 24.0, (1,)),
    (6.777388095855713, 32.0, 24.0, (1,)),
    (8.703092575073242, 32.0, 24.0, (2,)),
    (13.836954116821289, 25.0, 20.0, (1,)),
    (14.105984687805176, 32.0, 24.0, (2,)),
    (15.054841995239258, 3.0, 44.0, (2,)),
    (20.83083152770996, 60.0, 5.0, (1, 2)),
    (23.094751358032227, -5.0, 30.0, (2,)),
    (23.17375946044922, 60.0, 5.0, (2,)),
    (26.61220932006836, 3.0, 44.0, (1,)),
    (42.10489273071289, 3.0, 44.0, (2,)),
    (61.52827835083008, 3.0, 44.0, (1,)),
    (64.08735656738281, 25.0, 20.0, (2,)),
    (70.8103256225586, 25.0, 20.0, (1,)),
    (76.11328887939453, 32.0, 24.0, (2,)),
    (77.8758316040039, 3.0, 44.0, (1,)),
    (101.38594055175781, 32.0, 24.0, (2,)),
    (112.0206527709961, 25.0, 20.0, (2,)),
    (133.67236328125, 3.0, 44.0, (1,)),
    (161.79443359375, 40.0, 27.0, (2,)),
    (166.00531005859375, 3.0, 44.0, (1, 2)),
    (173.61814880371094, 32.0, 24.0, (1,)),
    (192.334228515625, 3.0, 44.0, (2,)),
    (199.5727996826172, 32.0, 24.0, (1, 2)),
    (218.86981201171875, 32.0, 24.0, (1,)),
    (243.38778686523438, 3.0, 44.0, (1,)),
    (267.06634521484375, 40.0, 27.0, (2,)),
    (291.3045349121094, 3.0, 44.0, (1, 2)),
    (314.0532531738281, 32.0, 24.0, (2,)),
    (346.97918701171875, 32.0, 24.0, (2,)),
]


def contraction():
    return [("contraction", noise(), _kps([kp_row(x, y, np.float32(a)) for a, x, y, _ in CONTRACTION_ROWS]))]


FLAT_ANGLES = [0.0, 30.0, 77.7, 192.334228515625, 301.0]
FLAT_POSITIONS = [(32.0, 24.0), (0.0, 0.0), (63.0, 47.0), (-9.0, 56.0)]


def step_edge(w=W, h=H):
    g = np.zeros((h, w), np.uint8)
    g[:, w // 2:] = 255
    return g


def flat_and_two_valued():
    """[(label, image, kps7)]: labels flat* and two_valued*."""
    rows = _kps([kp_row(x, y, a) for a in FLAT_ANGLES for x, y in FLAT_POSITIONS] +
                [kp_row(*level_centre(o, W, H), 30.0 + 40 * o, o) for o in (1, 4, 7)])
    out = [(f"flat{v}", np.full((H, W), v, np.uint8), rows) for v in (0, 77, 255)]
    out.append(("two_valued_checker", synth.checker(W, H, 1), rows))
    edge_rows = _kps([kp_row(x, y, a) for a in FLAT_ANGLES for x, y in ((32.0, 24.0), (30.0, 20.0), (36.0, 3.0), (20.0, 40.0))] +
                     [kp_row(*level_centre(o, W, H), 30.0 + 40 * o, o) for o in (1, 4, 7)])
    out.append(("two_valued_edge", step_edge(), edge_rows))
    return out


BORDER_ANGLES = [0.0, 30.0, 123.4, 192.334228515625, 210.0, 271.0, 45.0, 333.3]


def reads_past_one_reflection(kps7, w, h):
    """Per keypoint: the number of pattern points that lie more than one reflection outside the level (|offset| beyond size - 1)."""
    X, Y, lw, lh = patch_reads(kps7, w, h)
    lw, lh = lw[:, None], lh[:, None]
    return ((X < -(lw - 1)) | (X > 2 * (lw - 1)) | (Y < -(lh - 1)) | (Y > 2 * (lh - 1))).sum(1)


def reads_ring(kps7, w, h):
    """Per keypoint: the number of pattern points that lie in the unblurred ring around the level."""
    X, Y, lw, lh = patch_reads(kps7, w, h)
    lw, lh = lw[:, None], lh[:, None]
    return ((X < 0) | (X >= lw) | (Y < 0) | (Y >= lh)).sum(1)


def border_rows(w, h):
    """(kps7, labels): 'corner' = every octave at the four image corners, 'edge' = the first and last accepted level coordinate on each
    axis at every octave, 'half' = octave-0 positions k + 0.5 on both axes for even and odd k.  The angles cycle through BORDER_ANGLES; a
    corner row skips ahead to the first angle at which it reads past one reflection of the level, where there is one."""
    rows, labels = [], []

    def add(label, x, y, octave):
        n = len(rows)
        cycle = [BORDER_ANGLES[(n + i) % len(BORDER_ANGLES)] for i in range(len(BORDER_ANGLES))]
        far = [a for a in cycle if label == "corner" and reads_past_one_reflection([kp_row(x, y, a, octave)], w, h)[0]]
        rows.append(kp_row(x, y, (far or cycle)[0], octave)); labels.append(label)

    for o in range(LEVELS):
        for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
            add("corner", float(x), float(y), o)
    for o in range(LEVELS):
        lw, lh, _, _ = levels(w, h)[o]
        mx, my = image_position(lw // 2, o, w, h), image_position(lh // 2, o, w, h)
        add("edge", image_position(ACCEPT_LO, o, w, h), my, o)
        add("edge", image_position(lw + ACCEPT_PAST - 1, o, w, h), my, o)
        add("edge", mx, image_position(ACCEPT_LO, o, w, h), o)
        add("edge", mx, image_position(lh + ACCEPT_PAST - 1, o, w, h), o)
    add("edge", image_position(ACCEPT_LO, 0, w, h), image_position(ACCEPT_LO, 0, w, h), 0)             # (-9, -9)
    add("edge", float(w + ACCEPT_PAST - 1), float(h + ACCEPT_PAST - 1), 0)                            # (w + 8, h + 8)
    for x, y in ((10.5, 6.5), (11.5, 7.5), (10.5, 7.5), (11.5, 6.5), (2.5, 3.5), (-8.5, -7.5), (w + 7.5, h + 6.5), (w - 0.5, 0.5)):
        add("half", x, y, 0)
    return _kps(rows), labels


def border():
    return [("border", noise(), border_rows(W, H)[0]), ("border_small", noise(SMALL_W, SMALL_H, 43), border_rows(SMALL_W, SMALL_H)[0])]


COUNTS = [0, 1, 7, 8, 9, 255, 256, 257, KP_CAP, KP_CAP + 1]


@functools.lru_cache(maxsize=None)
def random_keypoints(n, w=W, h=H, seed=7):
    """n keypoints at random positions (up to 8 px outside the image at octave 0), angles and octaves; the first one is at octave 0, so
    that the numpy restatement has a row to check in every set."""
    rng = np.random.default_rng(seed + n)
    k = np.zeros((n, 7), np.float32)
    k[:, 0] = rng.uniform(-8, w + 8, n); k[:, 1] = rng.uniform(-8, h + 8, n)
    k[:, 2] = 31; k[:, 3] = rng.uniform(0, 360, n); k[:, 4] = 1; k[:, 5] = rng.integers(0, LEVELS, n); k[:, 6] = -1
    k[:1, 5] = 0
    k.setflags(write=False)
    return k


def counts(n):
    return [(f"counts{n}", noise(), random_keypoints(n))]


def level_subsets():
    """Three calls for ONE context, in this order: image A with all octaves, image B with octave 0 only (the other levels of the atlas
    stay A's), image B with octave 7 only."""
    a, b = noise(W, H, 44), noise(W, H, 45)
    k = random_keypoints(300, seed=9)
    return [("levels_all", a, k.copy()), ("levels_octave0", b, k[k[:, 5] == 0].copy()), ("levels_octave7", b, k[k[:, 5] == 7].copy())]


def describe_cases():
    """[(label, builder)] of every describe family but level_subsets; builder() -> [(label, image, kps7)]."""
    out = [("half_ties", half_ties), ("contraction", contraction), ("flat_and_two_valued", flat_and_two_valued), ("border", border)]
    out += [(f"counts{n}", functools.partial(counts, n)) for n in COUNTS]
    return out


@functools.lru_cache(maxsize=None)
def oracle_describe(family):
    """{label: oracle descriptors} of one describe family (or 'level_subsets'), computed once per session."""
    build = level_subsets if family == "level_subsets" else dict(describe_cases())[family]
    out = {}
    for label, img, kps in build():
        d = O.orb_describe(img, kps)
        d.setflags(write=False)
        out[label] = d
    return out


def accepted(kps7, w, h):
    """The range test of OrbDetector::describe."""
    k = _f32(kps7).reshape(-1, 7)
    cx, cy = level_position(k, w, h)
    size = np.array([levels(w, h)[int(o)][:2] for o in k[:, 5]], np.int64).reshape(-1, 2)
    return (cx >= ACCEPT_LO) & (cx < size[:, 0] + ACCEPT_PAST) & (cy >= ACCEPT_LO) & (cy < size[:, 1] + ACCEPT_PAST)


def refused_rows(w=W, h=H):
    """[(what, kps7 row)]: one level coordinate past each end of the accepted range on each axis, at octaves 0 and 3, and octaves -1, 8."""
    out = []
    for o in (0, 3):
        lw, lh, _, _ = levels(w, h)[o]
        mx, my = image_position(lw // 2, o, w, h), image_position(lh // 2, o, w, h)
        out += [(f"x below, octave {o}", kp_row(image_position(ACCEPT_LO - 1, o, w, h), my, 10.0, o)),
                (f"x above, octave {o}", kp_row(image_position(lw + ACCEPT_PAST, o, w, h), my, 10.0, o)),
                (f"y below, octave {o}", kp_row(mx, image_position(ACCEPT_LO - 1, o, w, h), 10.0, o)),
                (f"y above, octave {o}", kp_row(mx, image_position(lh + ACCEPT_PAST, o, w, h), 10.0, o))]
    out += [("x = -9.5 rounds to -10", kp_row(-9.5, 20.0, 10.0, 0)), ("octave -1", kp_row(30.0, 20.0, 10.0, -1)),
            ("octave 8", kp_row(30.0, 20.0, 10.0, LEVELS))]
    return out


# ---- Hamming references ---------------------------------------------------------------------------------------------------------------
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _d32(a):
    return np.ascontiguousarray(a, np.uint8).reshape(-1, 32)


def hamming_distances(q, t):
    """(nq, nt) popcounts of the xor over the 32 bytes."""
    q, t = _d32(q), _d32(t)
    return _POP8[q[:, None, :] ^ t[None, :, :]].sum(2)


def hamming_match_ref(q, t):
    """Rows (query, train, distance): the first minimum; no rows without train descriptors."""
    d = hamming_distances(q, t)
    if d.shape[1] == 0:
        return np.zeros((0, 3), np.int32)
    j = d.argmin(1)                                     # the first of equal minima
    return np.stack([np.arange(len(d)), j, d[np.arange(len(d)), j]], 1).astype(np.int32)


def hamming_knn2_ref(q, t):
    """Rows (train0, distance0, train1, distance1): the first two of a stable sort by distance, -1 where there is none."""
    d = hamming_distances(q, t)
    out = np.full((len(d), 4), -1, np.int32)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    for k in range(order.shape[1]):
        out[:, 2 * k] = order[:, k]
        out[:, 2 * k + 1] = d[np.arange(len(d)), order[:, k]]
    return out


def ratio_symmetry_ref(knn12, knn21, ratio):
    """include/poppy_hip.h: a query survives the ratio test with two neighbours unless distance0 / distance1 > ratio (float division of the
    float-converted distances; 0 / 0 is NaN, not greater, and stays; d / 0 is +inf and goes); then, for every surviving 1 -> 2 match in
    query order, the first surviving 2 -> 1 match that points back.  Rows (query, train, distance)."""
    knn12 = np.asarray(knn12, np.int32).reshape(-1, 4); knn21 = np.asarray(knn21, np.int32).reshape(-1, 4)

    def keep(k):
        with np.errstate(divide="ignore", invalid="ignore"):
            return (k[:, 0] >= 0) & (k[:, 2] >= 0) & ~(k[:, 1].astype(np.float32) / k[:, 3].astype(np.float32) > np.float32(ratio))

    k1, k2 = keep(knn12), keep(knn21)
    out = []
    for i in np.flatnonzero(k1):
        for j in np.flatnonzero(k2):
            if knn21[j, 0] == i and knn12[i, 0] == j:
                out.append((i, j, knn12[i, 1]))
                break
    return k1.astype(np.int32), k2.astype(np.int32), np.array(out, np.int32).reshape(-1, 3)


# ---- Hamming families: [(label, query, train)] ------------------------------------------------------------------------------------------
def flip_bits(row, bits):
    out = np.array(row, np.uint8).copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def random_descriptors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


NQ = [1, 2, 3, 4, 5, 9]
NT = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1537]


def lengths(nq, nt):
    """Train rows and the further queries are the first query with 0 to 2 (queries: 0 to 3) random bits flipped, so ties abound."""
    rng = np.random.default_rng(5000 + 17 * nt + nq)
    q0 = random_descriptors(rng, 1)[0]
    q = np.stack([q0] + [flip_bits(q0, rng.choice(256, rng.integers(0, 4), replace=False)) for _ in range(nq - 1)])
    t = np.stack([flip_bits(q0, rng.choice(256, rng.integers(0, 3), replace=False)) for _ in range(nt)]) if nt else np.zeros((0, 32), np.uint8)
    return q, t


ALL_EQUAL_NT = [64, 513, 1537]


def all_equal(nt, nq=5):
    row = random_descriptors(np.random.default_rng(61), 1)[0]
    return np.tile(row, (nq, 1)), np.tile(row, (nt, 1))


def complement(nt, nq=5):
    q, t = all_equal(nt, nq)
    return q, ~t


PLANT_NT = [1537, 1088]                             # three full tiles and one descriptor; two full tiles and 64 (the last one in lane 63)
PLANT_SINGLE = [("first", lambda nt: 0), ("last", lambda nt: nt - 1), ("i63", lambda nt: 63), ("i511", lambda nt: 511), ("i512", lambda nt: 512)]
# pairs: the same lane of one tile (j and j + 64), neighbouring lanes, different tiles, the later tile first, the last and the first
PLANT_PAIRS = [("same_lane", lambda nt: (5, 69)), ("lanes", lambda nt: (5, 6)), ("tiles", lambda nt: (5, 517)),
               ("tiles_back", lambda nt: (1024, 3)), ("last_first", lambda nt: (nt - 1, 0))]
PLANT_DISTANCES = [(3, 3), (3, 4), (4, 3)]          # equal; the first listed index nearer; the second listed index nearer
PLANT_NQ = 5


def planted_cases():
    """[(label, nt, planted query, [(train index, distance)])]"""
    out, n = [], 0
    for nt in PLANT_NT:
        for name, where in PLANT_SINGLE:
            for d in (0, 5):
                out.append((f"nt{nt}_{name}_d{d}", nt, n % PLANT_NQ, [(where(nt), d)])); n += 1
        for name, where in PLANT_PAIRS:
            for da, db in PLANT_DISTANCES:
                a, b = where(nt)
                out.append((f"nt{nt}_{name}_d{da}_{db}", nt, n % PLANT_NQ, [(a, da), (b, db)])); n += 1
    return out


def planted(label):
    """Random train rows, all at distance >= 64 from every query, with the one or two nearest of one query planted."""
    cases = planted_cases()
    at = next(i for i, c in enumerate(cases) if c[0] == label)
    _, nt, qi, plants = cases[at]
    rng = np.random.default_rng(7000 + at)
    q = random_descriptors(rng, PLANT_NQ)
    t = random_descriptors(rng, nt)
    far = hamming_distances(q, t).min(0) >= 64
    while not far.all():
        t[~far] = random_descriptors(rng, int((~far).sum()))
        far = hamming_distances(q, t).min(0) >= 64
    for idx, d in plants:
        t[idx] = flip_bits(q[qi], rng.choice(256, d, replace=False))
    return q, t


def planted_expectation(label):
    """(query, expected match row, expected knn2 row) of the planted query; a single plant's second neighbour is not stated (None)."""
    _, nt, qi, plants = next(c for c in planted_cases() if c[0] == label)
    order = sorted(plants, key=lambda p: (p[1], p[0]))
    match = (qi, order[0][0], order[0][1])
    knn = (order[0][0], order[0][1], order[1][0], order[1][1]) if len(order) == 2 else None
    return qi, match, knn


def hamming_cases():
    """[(family, label, builder)]: builder() -> (query, train), both (n, 32) uint8."""
    out = [("lengths", f"nq{nq}_nt{nt}", functools.partial(lengths, nq, nt)) for nq in NQ for nt in NT]
    out += [("all_equal", f"nt{nt}", functools.partial(all_equal, nt)) for nt in ALL_EQUAL_NT]
    out += [("complement", f"nt{nt}", functools.partial(complement, nt)) for nt in ALL_EQUAL_NT]
    out += [("planted", c[0], functools.partial(planted, c[0])) for c in planted_cases()]
    out += [("empty", "nq0", lambda: (np.zeros((0, 32), np.uint8), random_descriptors(np.random.default_rng(62), 70))),
            ("empty", "nt0", lambda: (random_descriptors(np.random.default_rng(63), 5), np.zeros((0, 32), np.uint8)))]
    return out


@functools.lru_cache(maxsize=None)
def hamming_reference(family, label):
    """(query, train, match rows, knn2 rows) of one Hamming case from the numpy references, computed once per session."""
    build = next(b for f, l, b in hamming_cases() if (f, l) == (family, label))
    q, t = build()
    m, k = hamming_match_ref(q, t), hamming_knn2_ref(q, t)
    for a in (q, t, m, k):
        a.setflags(write=False)
    return q, t, m, k
