"""numpy yardsticks of the Euclidean kNN on an 8-bit scalar-quantised bank (csrc/knn_l2_int8.hip), shared by the knn-l2-int8 tests.
The definition, restated from the kernel file's header: one affine code (lo, s) for the whole bank, s = (hi - lo) / 255 (1 when hi ==
lo), inv_s = 1 / s and s2 = s s, each computed in float64 and rounded once to fp32 (inv_s and s2 from the rounded s).  The code of an
fp32 element x, in fp32 operations in this order, is
    c(x) = rint(min(max((x - lo) * inv_s, 0), 255)) - 128       (rint to nearest even; max(NaN, 0) = 0, so NaN -> -128),
an int8 that stands for lo + s (c + 128).  D2(q, b) = sum_j (c(q_j) - c(b_j))^2 in int64; excess(q) = sum_j (q_j - min(max(q_j, lo),
hi_q))^2 with hi_q = fl32(lo + 255 s), the value of code 127; the neighbours of a query are a stable ascending argsort of (D2, row);
d(q, b) = sqrt(s2 D2 + excess(q)) in float64."""
import numpy as np
import torch

F = np.float32
U = 2.0 ** -24          # unit roundoff of fp32


def _np(v):
    return (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(F)


def quantiser(lo, hi):
    """(lo, s, inv_s, s2) as np.float32 from the bank's smallest / largest element."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("the range must be finite")
    s = F((hi - lo) / 255.0) if hi != lo else F(1.0)
    return F(lo), s, F(1.0 / float(s)), F(float(s) * float(s))


def quantiser_of(bank):
    b = _np(bank)
    return quantiser(b.min(), b.max())


def codes(x, lo, inv_s):
    """int8 codes of the fp32 rows x by the expression above (every step an fp32 operation)."""
    x = _np(x)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x - F(lo)) * F(inv_s)
        assert v.dtype == F
        v = np.fmin(np.fmax(v, F(0)), F(255))           # fmax / fmin return the other operand for a NaN
        return (np.rint(v).astype(np.int32) - 128).astype(np.int8)


def hi_q(lo, s):
    """fl32(lo + 255 s): 255 s is exact in float64, and so is the sum unless the exponents of lo and s lie 2^21 apart."""
    return F(float(lo) + 255.0 * float(s))


def over(x, lo, s):
    """x - clamp(x, lo, hi_q) in fp32 (exact unless x is many binades above the range: then one rounding)."""
    x = _np(x)
    with np.errstate(invalid="ignore", over="ignore"):
        return x - np.fmin(np.fmax(x, F(lo)), hi_q(lo, s))


def excess64(x, lo, s):
    return (over(x, lo, s).astype(np.float64) ** 2).sum(1)


def sq64(c):
    return (c.astype(np.int64) ** 2).sum(1)


def d2_int(xc, bc):
    """[N][R] int64 sums of squared code differences, by differences (not the expanded form)."""
    xc, bc = xc.astype(np.int64), bc.astype(np.int64)
    out = np.empty((xc.shape[0], bc.shape[0]), dtype=np.int64)
    for i in range(0, xc.shape[0], 16):
        diff = xc[i:i + 16, None, :] - bc[None, :, :]
        out[i:i + 16] = (diff * diff).sum(2)
    return out


def d2_expanded(xc, bc):
    """qsq + bsq - 2 dot in int64: what the kernel evaluates."""
    xc, bc = xc.astype(np.int64), bc.astype(np.int64)
    return sq64(xc)[:, None] + sq64(bc)[None, :] - 2 * (xc @ bc.T)


def d2_blas(xc, bc):
    """d2_expanded with the dot products as a float64 matrix product: every partial sum is an integer below 2^53, so it is exact
    (tests/test_knn_l2_int8_host.py holds it to d2_int); the form the GPU tests can afford at their largest shapes."""
    xf, bf = xc.astype(np.float64), bc.astype(np.float64)
    return sq64(xc)[:, None] + sq64(bc)[None, :] - 2 * (xf @ bf.T).astype(np.int64)


def kneighbors(d2, k):
    """(D2 [N][k] int64, rows [N][k] int64): the first k of a stable ascending argsort -- equal D2 to the smaller row."""
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d2, order, 1), order


def dist64(d2, s2, excess):
    """sqrt(s2 D2 + excess) in float64; s2 the fp32 value, excess [N] (float64 values)."""
    return np.sqrt(float(s2) * d2.astype(np.float64) + np.asarray(excess, dtype=np.float64)[:, None])


def decode(c, lo, s):
    """float64 values the codes stand for."""
    return float(lo) + float(s) * (c.astype(np.float64) + 128.0)


def exact64(x, bank):
    """[N][R] float64 Euclidean distances between the unquantised rows."""
    x, bank = _np(x).astype(np.float64), _np(bank).astype(np.float64)
    out = np.empty((x.shape[0], bank.shape[0]))
    for i in range(0, x.shape[0], 16):
        out[i:i + 16] = np.sqrt(((x[i:i + 16, None, :] - bank[None, :, :]) ** 2).sum(2))
    return out


def ulps32(got, want64):
    """|got - want| in units of the fp32 spacing at want (got: float32 array, want: float64)."""
    want64 = np.asarray(want64, dtype=np.float64)
    spacing = np.spacing(np.maximum(np.abs(want64), np.finfo(F).tiny).astype(F)).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want64) / spacing


def mean_of(dist, k):
    """(d0 [+ d1] [+ d2]) / k, added smallest first, in IEEE fp32 on the host -- the kernel's epilogue."""
    d = _np(dist)
    s = d[:, 0].copy()
    for j in range(1, k):
        s = s + d[:, j]
    return s / F(k)
