"""Scenes and numpy restatements for the RANSAC fundamental-matrix filter (include/poppy_hip.h: poppy_ransac_fundamental), shared by
tests/test_host_ransac.py and tests/test_gpu_ransac.py.  Everything comes from seeded numpy.random.RandomState; nothing here calls the library."""
import numpy as np

W, H, FOCAL = 1280, 960, 800.0
K = np.array([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]], np.float64)
_ANGLE = np.deg2rad(10.0)
R = np.array([[np.cos(_ANGLE), 0, np.sin(_ANGLE)], [0, 1, 0], [-np.sin(_ANGLE), 0, np.cos(_ANGLE)]], np.float64)      # the second camera, turned about y
C2 = np.array([1.0, 0.1, 0.2])                                                                                       # ... and moved
_T = -R @ C2
F_TRUE = np.linalg.inv(K).T @ np.array([[0, -_T[2], _T[1]], [_T[2], 0, -_T[0]], [-_T[1], _T[0], 0]]) @ R @ np.linalg.inv(K)     # x2^T F x1 = 0


def _line_distance(F, a, b):
    """distance of b (n x 2) from the epipolar lines F (a, 1) (n x 2 points a)"""
    l = np.concatenate([a, np.ones((len(a), 1))], 1) @ F.T
    return np.abs((l[:, :2] * b).sum(1) + l[:, 2]) / np.hypot(l[:, 0], l[:, 1])


def two_view(n_in, n_out, noise=0.0, seed=0):
    """(points1, points2, planted) — n_in projections of 3-D points at depth 4 .. 12 into two pinhole cameras (f = 800, 1280 x 960), each coordinate
    moved by a uniform +-noise, and n_out pairs of unrelated points at least 20 px from the true epipolar line in BOTH images, shuffled; float32;
    planted[i] is True for the projections."""
    rs = np.random.RandomState(seed)
    a, b = np.zeros((0, 2)), np.zeros((0, 2))
    while len(a) < n_in:
        m = 2 * (n_in - len(a)) + 8
        z = rs.uniform(4, 12, m)
        x1 = np.stack([rs.uniform(0, W - 1, m), rs.uniform(0, H - 1, m)], 1)
        X = (np.linalg.inv(K) @ np.concatenate([x1, np.ones((m, 1))], 1).T).T * z[:, None]
        q = (K @ (R @ (X - C2).T)).T
        x2 = q[:, :2] / q[:, 2:3]
        ok = (q[:, 2] > 0) & (x2[:, 0] >= 0) & (x2[:, 0] <= W - 1) & (x2[:, 1] >= 0) & (x2[:, 1] <= H - 1)
        a, b = np.concatenate([a, x1[ok]])[:n_in], np.concatenate([b, x2[ok]])[:n_in]
    if noise:
        a = a + rs.uniform(-noise, noise, a.shape); b = b + rs.uniform(-noise, noise, b.shape)
    oa, ob = np.zeros((0, 2)), np.zeros((0, 2))
    while len(oa) < n_out:
        m = 2 * (n_out - len(oa)) + 8
        x1 = np.stack([rs.uniform(0, W - 1, m), rs.uniform(0, H - 1, m)], 1)
        x2 = np.stack([rs.uniform(0, W - 1, m), rs.uniform(0, H - 1, m)], 1)
        ok = (_line_distance(F_TRUE, x1, x2) >= 20) & (_line_distance(F_TRUE.T, x2, x1) >= 20)
        oa, ob = np.concatenate([oa, x1[ok]])[:n_out], np.concatenate([ob, x2[ok]])[:n_out]
    p1, p2 = np.concatenate([a, oa]), np.concatenate([b, ob])
    planted = np.arange(n_in + n_out) < n_in
    order = rs.permutation(n_in + n_out)
    return np.ascontiguousarray(p1[order], np.float32), np.ascontiguousarray(p2[order], np.float32), planted[order]


def degenerate():
    """name -> (points1, points2): identical pairs, a pure shift by (5, 3), collinear points, 64 copies of one pair"""
    rs = np.random.RandomState(77)
    p = np.stack([rs.uniform(0, W - 1, 64), rs.uniform(0, H - 1, 64)], 1).astype(np.float32)
    t = rs.uniform(0, 400, 64)
    line1 = np.stack([100 + t, 50 + 2 * t], 1).astype(np.float32)
    line2 = np.stack([900 - 1.5 * t, 120 + t], 1).astype(np.float32)
    one = np.array([[321.5, 123.25]], np.float32).repeat(64, 0)
    return {"identical": (p, p.copy()), "shift": (p, p + np.array([5, 3], np.float32)), "collinear": (line1, line2),
            "copies": (one, (one + np.float32(7)).astype(np.float32))}


def sizes():
    return [8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16385]


def quarter_outliers(n, seed):
    """a two_view scene of n pairs, a quarter of them planted outliers, half a pixel of noise"""
    return two_view(n - n // 4, n // 4, 0.5, seed)


# ---- numpy restatements ---------------------------------------------------------------------------------------------------------------------
def mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def samples(n, hypotheses=2048):
    """[hypotheses, 8] indices of the rule's sampler among n points, in draw order"""
    h = np.arange(hypotheses, dtype=np.uint32)
    out = np.zeros((hypotheses, 8), np.int64)
    with np.errstate(over="ignore"):
        for k in range(8):
            r = (mix32(np.uint32(0x9E3779B9) * (np.uint32(8) * h + np.uint32(k + 1))) % np.uint32(n - k)).astype(np.int64)
            earlier = np.sort(out[:, :k], axis=1)
            for j in range(k):
                r += r >= earlier[:, j]
            out[:, k] = r
    return out


def inlier_matrix(models, p1, p2, distance):
    """[hypotheses, n] bool: pair i is an inlier of model h by the rule's two inequalities, in the rule's operation order (float64, no fused products)"""
    F = np.asarray(models, np.float64).reshape(-1, 3, 3)[:, :, :, None]
    x1, y1 = p1[:, 0].astype(np.float64)[None, :], p1[:, 1].astype(np.float64)[None, :]
    x2, y2 = p2[:, 0].astype(np.float64)[None, :], p2[:, 1].astype(np.float64)[None, :]
    a = (F[:, 0, 0] * x1 + F[:, 0, 1] * y1) + F[:, 0, 2]
    b = (F[:, 1, 0] * x1 + F[:, 1, 1] * y1) + F[:, 1, 2]
    c = (F[:, 2, 0] * x1 + F[:, 2, 1] * y1) + F[:, 2, 2]
    e = (a * x2 + b * y2) + c
    a2 = (F[:, 0, 0] * x2 + F[:, 1, 0] * y2) + F[:, 2, 0]
    b2 = (F[:, 0, 1] * x2 + F[:, 1, 1] * y2) + F[:, 2, 1]
    ee = e * e
    d2 = np.float64(distance) * np.float64(distance)
    return (ee <= d2 * (a * a + b * b)) & (ee <= d2 * (a2 * a2 + b2 * b2))


def recount(models, p1, p2, distance):
    """inlier counts [hypotheses] of models [hypotheses, 3, 3]"""
    return inlier_matrix(models, p1, p2, distance).sum(1)


def unrelated(n, seed):
    """n pairs of unrelated points: no geometry fits more than the 8 pairs it was solved from, but for an accident"""
    rs = np.random.RandomState(seed)
    return (np.stack([rs.uniform(0, W - 1, n), rs.uniform(0, H - 1, n)], 1).astype(np.float32),
            np.stack([rs.uniform(0, W - 1, n), rs.uniform(0, H - 1, n)], 1).astype(np.float32))


def _normalise(p):
    m = p.mean(0)
    s = np.sqrt(2.0) / np.hypot(*(p - m).T).mean()
    T = np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1]])
    return (p - m) * s, T


def eight_point(p1, p2):
    """normalised 8-point fit in float64 numpy: rank 2, Frobenius norm 1, largest-magnitude entry positive"""
    a, T1 = _normalise(np.asarray(p1, np.float64)); b, T2 = _normalise(np.asarray(p2, np.float64))
    A = np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1], a[:, 0], a[:, 1], np.ones(len(a))], 1)
    f = np.linalg.svd(A)[2][-1].reshape(3, 3)
    u, s, vt = np.linalg.svd(f)
    F = T2.T @ (u @ np.diag([s[0], s[1], 0]) @ vt) @ T1
    F = F / np.linalg.norm(F)
    return F if F.flat[np.abs(F).argmax()] > 0 else -F
