"""float64 numpy yardsticks of the Euclidean kNN with half-precision operands (csrc/knn_l2_half.hip), shared by the knn-l2-half tests.
The definition: h(v) rounds an fp32 value to fp16 -- round to nearest even, saturating at +-65504 instead of overflowing, results of
magnitude below 2^-14 (the subnormal halves) becoming signed zero -- so no half holds inf, NaN or a subnormal; the distance is that of
tests/knn_l2_ref.py BETWEEN THE ROUNDED ROWS, d(q, b) = sqrt(max(|h(q)|^2 + |h(b)|^2 - 2 <h(q), h(b)>, 0)), in float64, with its order
(lexicographic on (d2, row)) and its patch score (the mean of the k = 3 smallest d)."""
import numpy as np
import torch

import knn_l2_ref as ref

EPS = ref.EPS
HALF_MAX = 65504.0
HALF_MIN_NORMAL = 2.0 ** -14
U_HALF = 2.0 ** -11         # relative rounding error of h on in-range values


def h(v):
    """fp32 array (or tensor) -> numpy float16 array by the definition above."""
    v = (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float32)
    r = np.clip(v, np.float32(-HALF_MAX), np.float32(HALF_MAX)).astype(np.float16)       # numpy rounds to nearest even
    small = np.abs(r.astype(np.float32)) < np.float32(HALF_MIN_NORMAL)
    return np.where(small, np.copysign(np.float16(0), r), r).astype(np.float16)


def rounded(v):
    """h(v) as a float32 torch tensor: the rows the float64 functions of knn_l2_ref take."""
    return torch.from_numpy(h(v).astype(np.float32))


def sqnorms64(x):
    return ref.sqnorms64(rounded(x))


def d2_64(x, bank):
    return ref.d2_64(rounded(x), rounded(bank))


def scale_a(x, bank):
    """A~ = |h(q)|^2 + |h(b)|^2 + 2 sum |h(q)_i| |h(b)_i|: the bar on a squared distance is tau 2^-24 A~."""
    return ref.scale_a(rounded(x), rounded(bank))


def kneighbors64(x, bank, m):
    return ref.kneighbors64(rounded(x), rounded(bank), m)


def patch_scores64(x, bank, k=3):
    return ref.patch_scores64(rounded(x), rounded(bank), k)
