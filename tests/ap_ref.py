"""The float64 reference of average precision and the precision-recall curve: the definition of include/ssad.h restated in numpy, with
np.unique grouping, independent of scikit-learn and of the code under test.  Shared by tests/test_ap_host.py and tests/test_hip_ap.py.

A threshold is a distinct score value (np.unique groups by ==: -0.0 with +0.0, inf with inf).  For the j-th distinct value in DESCENDING
order TP_j / N_j = positives / elements with a score at least it (exact int64), P = TP_m, positive = non-zero target:
    precision_j = TP_j / N_j      recall_j = TP_j / P (1.0 when P = 0)      AP = sum_j (TP_j - TP_{j-1}) / P * TP_j / N_j   (0.0 when P = 0)
A group of zeros reports -0.0 when it holds one, +0.0 otherwise (the smallest member in the total order of the bit patterns)."""
import collections

import numpy as np

Curve = collections.namedtuple("Curve", "thresholds tp n P m precision recall ap")


def pr_counts(scores, targets):
    """-> thresholds float32 [m] descending, TP int64 [m], N int64 [m], P."""
    s = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    y = np.asarray(targets).reshape(-1) != 0
    assert s.size and s.size == y.size and not np.isnan(s).any()
    values, inv = np.unique(s, return_inverse=True)               # ascending distinct values
    inv = inv.reshape(-1)
    m = values.size
    pos = np.bincount(inv[y], minlength=m).astype(np.int64)[::-1]
    cnt = np.bincount(inv, minlength=m).astype(np.int64)[::-1]
    thresholds = values[::-1].astype(np.float32).copy()
    zero = thresholds == 0
    if zero.any():
        thresholds[zero] = np.float32(-0.0) if (s.view(np.uint32) == 0x80000000).any() else np.float32(0.0)
    tp, n = np.cumsum(pos), np.cumsum(cnt)
    return thresholds, tp, n, int(tp[-1])


def ap_ref(scores, targets):
    """-> Curve: the counts, precision and recall per threshold (descending) and AP, in float64."""
    thresholds, tp, n, P = pr_counts(scores, targets)
    precision = tp / n
    recall = tp / P if P else np.ones(tp.size)
    d = np.diff(tp, prepend=0)
    ap = float(np.sum(d / P * precision)) if P else 0.0
    return Curve(thresholds, tp, n, P, tp.size, precision, recall, ap)


def ulps(got, want):
    """|got - want| in units of the last place of `want` (float64 arrays)."""
    return np.abs(got - want) / np.spacing(np.abs(want))
