"""The definition of the resize-then-Gaussian anomaly map (csrc/resize_gaussian.hip, ops.resize_gaussian, tools.upsample(method=
'resize_blur')) in float64, stated on its own: nothing here imports the package.

out = A_y M A_x^T with A = G R per axis.  R [T][extent] is F.interpolate(mode='bilinear', align_corners=False) as a matrix; G [T][T]
is the Gaussian of scipy.ndimage.gaussian_filter (radius int(4 sigma + 0.5), taps exp(-0.5 (d / sigma)^2) normalised) with the
indices outside [0, T) folded back: 'symmetric' b a | a b (scipy's mode='reflect'), 'reflect' c b | a b c (torch's padding).
tests/test_resize_gaussian_host.py pins this against scipy and torch themselves."""
import math

import numpy as np

# (h, w, T, sigma) of the issue's CPU check, square maps
SHAPES = [(32, 256, 4.0), (29, 256, 4.0), (5, 40, 4.0), (7, 17, 4.0), (3, 18, 4.0), (128, 512, 4.0), (32, 64, 1.5)]
U = 2.0 ** -24


def bilinear_matrix(extent, T):
    R = np.zeros((T, extent), np.float64)
    for d in range(T):
        src = max((d + 0.5) * extent / T - 0.5, 0.0)
        i0 = min(int(math.floor(src)), extent - 1)
        i1 = min(i0 + 1, extent - 1)
        lam = src - i0
        R[d, i0] += 1.0 - lam
        R[d, i1] += lam
    return R


def fold(j, T, border):
    if j < 0:
        return -j - 1 if border == "symmetric" else -j
    if j >= T:
        return 2 * T - 1 - j if border == "symmetric" else 2 * T - 2 - j
    return j


def gaussian_matrix(T, sigma, border):
    assert border in ("symmetric", "reflect")
    r = int(4.0 * sigma + 0.5)
    assert r < T
    taps = np.array([math.exp(-0.5 * (d / sigma) ** 2) for d in range(-r, r + 1)], np.float64)
    taps = taps / taps.sum()
    G = np.zeros((T, T), np.float64)
    for y in range(T):
        for i, d in enumerate(range(-r, r + 1)):
            G[y, fold(y + d, T, border)] += taps[i]
    return G


_CACHE = {}


def operator(extent, T, sigma, border):
    """A = G R, float64 [T][extent] (cached; treat as read-only)."""
    key = (extent, T, float(sigma), border)
    if key not in _CACHE:
        A = gaussian_matrix(T, sigma, border) @ bilinear_matrix(extent, T)
        A.setflags(write=False)
        _CACHE[key] = A
    return _CACHE[key]


def pack(A):
    """Band form of A: (first int32 [T], weights float32 [T][K], K).  Row d is weights[d] over columns first[d] .. first[d] + K - 1,
    K the longest run of non-zeros of any row; shorter runs are zero-padded and pushed left where they would pass the last column."""
    T, extent = A.shape
    runs = []
    for d in range(T):
        cols = np.flatnonzero(A[d])
        runs.append((int(cols[0]), int(cols[-1])))
    K = max(b - a + 1 for a, b in runs)
    first = np.zeros(T, np.int32)
    weights = np.zeros((T, K), np.float32)
    for d, (a, _) in enumerate(runs):
        a = min(a, extent - K)
        first[d] = a
        weights[d] = A[d, a:a + K].astype(np.float32)
    return first, weights, K


def unpack(first, weights, extent):
    """The [T][extent] matrix a band form stands for, float64 of the stored fp32 weights."""
    T, K = weights.shape
    A = np.zeros((T, extent), np.float64)
    for d in range(T):
        A[d, first[d]:first[d] + K] = weights[d].astype(np.float64)
    return A


def reference(M, T, sigma=4.0, border="symmetric"):
    """M [..., h, w] -> [..., T, T] float64."""
    M = np.asarray(M, np.float64)
    Ay, Ax = operator(M.shape[-2], T, sigma, border), operator(M.shape[-1], T, sigma, border)
    return Ay @ M @ Ax.T


def bar(M, T, sigma=4.0, border="symmetric"):
    """Per-pixel bound on |fp32 kernel - reference|: (K_y + K_x + 4) 2^-24 (A_y |M| A_x^T).  Each chain of K FMAs over weights rounded
    once is within (K + 1) u of its exact sum to first order (one u for the weight, at most K for the partial sums a term passes
    through), the two chains compose to (K_y + K_x + 2) u, and 2 u cover the second-order terms; K counts the zero-padded taps, which
    round like any other.  For square maps this is the (2 K + 4) u of the design note."""
    M = np.asarray(M, np.float64)
    Ay, Ax = operator(M.shape[-2], T, sigma, border), operator(M.shape[-1], T, sigma, border)
    Ky, Kx = pack(Ay)[2], pack(Ax)[2]
    return (Ky + Kx + 4) * U * (np.abs(Ay) @ np.abs(M) @ np.abs(Ax).T)


def maps(kind, n, h, w, seed):
    """The test maps, float32: 'nonneg' (distances, up to ~10), 'mixed' (signs), 'constant', 'impulse' (one cell)."""
    rng = np.random.default_rng(seed)
    if kind == "nonneg":
        return (10.0 * rng.random((n, h, w))).astype(np.float32)
    if kind == "mixed":
        return rng.standard_normal((n, h, w)).astype(np.float32) * 3.0
    if kind == "constant":
        return np.full((n, h, w), 2.7182817, np.float32)
    if kind == "impulse":
        m = np.zeros((n, h, w), np.float32)
        for i in range(n):
            m[i, (h - 1 + i) % h, (w // 2 + i) % w] = 5.0
        return m
    raise KeyError(kind)
