"""float64 yardsticks of the refined search (csrc/knn_refine.hip), shared by the knn-refine tests.

The re-rank: for every query gather its listed bank rows, d2 = sum (x - b)^2 by direct differences in float64, and sort the valid
entries (0 <= row < R) ascending and stably by (d2, row, place in the list); missing places are (+inf, -1).  A row listed twice
appears twice.

The int8 top-k: the exact integer D2 of tests/knn_l2_int8_ref.py (imported, not restated) and a stable argsort of (D2, row).

The bar of a direct fp32 d2 against float64, BAR_UNITS(D) units of 2^-24 of d2: every difference is rounded once (relative 2^-24 of
the difference, so 2 x 2^-24 of its square, to first order), lane l's chain of n = ceil(D / 64) fused multiply-adds rounds each
partial sum once (n x 2^-24 of a sum of non-negative terms, each partial at most the final one), and the six butterfly additions round
once each (6 x 2^-24, all terms non-negative): (n + 8) 2^-24 d2 to first order.  Exactly, the m = n + 8 roundings compound to at
most (1 + u)^m - 1 <= m u / (1 - m u), u = 2^-24: the remainder beyond m u is below (m u)^2 / (1 - m u) < m^2 2^-48, that is under
m 2^-24 of ONE unit (2^-14 of a unit at D = 65 536); the float64 reference's own error, about D 2^-53 d2, is smaller still.  The bar
is therefore m (1 + 2^-12) units: the first-order constant, widened by less than a thousandth of a unit for what it leaves out."""
import numpy as np
import torch

import knn_l2_int8_ref as qref

F = np.float32
U = 2.0 ** -24


def bar_units(d):
    return (-(-int(d) // 64) + 8) * (1.0 + 2.0 ** -12)


def _np64(v):
    return (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float64)


def gathered_d2(x, bank, cand):
    """[N][r] float64 direct squared distances of every query to its listed rows; NaN where the entry is outside 0 .. R - 1."""
    x, bank = _np64(x), _np64(bank)
    cand = np.asarray(cand.cpu() if torch.is_tensor(cand) else cand).astype(np.int64)
    ok = (cand >= 0) & (cand < bank.shape[0])
    rows = bank[np.where(ok, cand, 0)]                          # [N][r][D]
    d2 = ((x[:, None, :] - rows) ** 2).sum(2)
    return np.where(ok, d2, np.nan), ok


def rerank(x, bank, cand, k):
    """(dist [N][k] float64, idx [N][k] int64, d2 sorted [N][k] float64): the definition above."""
    d2, ok = gathered_d2(x, bank, cand)
    cand = np.asarray(cand.cpu() if torch.is_tensor(cand) else cand).astype(np.int64)
    n, r = cand.shape
    dist = np.full((n, k), np.inf)
    idx = np.full((n, k), -1, dtype=np.int64)
    for i in range(n):
        order = sorted((j for j in range(r) if ok[i, j]), key=lambda j: (d2[i, j], cand[i, j], j))[:k]
        dist[i, :len(order)] = np.sqrt(d2[i, order])
        idx[i, :len(order)] = cand[i, order]
    return dist, idx


def near_ties(x, bank, cand, units):
    """[N] bool: the query has two valid listed entries, adjacent in the float64 order, whose d2 differ by less than twice the bar
    (`units` x 2^-24 of the larger) -- fp32 may order them either way, so the index comparison leaves the query out."""
    d2, ok = gathered_d2(x, bank, cand)
    d2 = np.sort(np.where(ok, d2, np.inf), axis=1)
    gap = d2[:, 1:] - d2[:, :-1]
    with np.errstate(invalid="ignore"):
        close = np.isfinite(d2[:, 1:]) & (gap < 2.0 * units * U * d2[:, 1:])
    return close.any(1), close.sum(), np.isfinite(d2[:, 1:]).sum()


def mean_of(dist, k):
    """(d0 + d1 + ... + d_{k-1}) / k in IEEE fp32 on the host, added smallest first: the kernel's epilogue."""
    d = np.asarray(dist.cpu() if torch.is_tensor(dist) else dist).astype(F)
    s = d[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for j in range(1, k):
            s = s + d[:, j]
        return s / F(k)


def int8_topk(xc, bc, k):
    """(D2 [N][k] int64, rows [N][k] int64) of the codes xc / bc: knn_l2_int8_ref's exact D2 and its stable argsort."""
    return qref.kneighbors(qref.d2_blas(xc, bc), k)


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


# the seeded Gaussian case of the index comparison (tests/test_hip_knn_refine.py) and of the host test that bounds what it leaves out
GAUSS_CASE = dict(n=257, r=16, d=96, rows=300)
LEFT_OUT_CAP = 0.02


def gauss_case():
    c = GAUSS_CASE
    x, bank = gauss(c["n"], c["d"], 4100), gauss(c["rows"], c["d"], 4101)
    rng = np.random.RandomState(4102)          # distinct rows per list: a row listed twice is a tie by construction (tested apart)
    cand = np.stack([rng.permutation(c["rows"])[:c["r"]] for _ in range(c["n"])]).astype(np.int32)
    return x, bank, torch.from_numpy(cand)
