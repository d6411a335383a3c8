"""Yardsticks of the k = 4..32 Euclidean search (csrc/knn_topk.hip) beyond those of tests/knn_l2_ref.py / knn_l2_half_ref.py:
integer rows whose squared distances are exact in fp32 and fp16, and the comparison of a (dist, idx) result with float64 for any k."""
import numpy as np
import torch

import knn_l2_ref as ref

EPS = ref.EPS


def integer_rows(n, r, d, seed):
    """(x [n][d], bank [r][d]) float32 with entries uniform in {-2..2}: every product and partial sum is a small integer, exact in
    fp32 and in fp16, so the kernels' d2 equals float64's.  The bank repeats about r / 3 distinct rows (massive ties, duplicated
    rows); the first queries copy bank rows (d2 = 0 several times)."""
    g = np.random.default_rng(seed)
    distinct = g.integers(-2, 3, size=(max(1, r // 3), d))
    bank = distinct[g.integers(0, distinct.shape[0], size=r)]
    x = g.integers(-2, 3, size=(n, d))
    c = min(n, max(1, n // 4))
    x[:c] = bank[g.integers(0, r, size=c)]
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(bank.astype(np.float32))


def sequential_mean(dist, k):
    """(d0 + d1 + ... + d_{k-1}) / k added one after the other in IEEE fp32 on the host: the mean form's epilogue."""
    d = dist.cpu().numpy()
    assert d.dtype == np.float32
    s = d[:, 0].copy()
    for j in range(1, k):
        s = s + d[:, j]
    assert s.dtype == np.float32
    return torch.from_numpy(s / np.float32(k))


def check_topk_against_float64(dist, idx, k, d2_all, a_all, t, max_loose=0.03):
    """dist / idx [N][k] (host tensors) against the float64 squared distances d2_all [N][R] with the scale a_all and the bar t units
    of 2^-24 A.  (1) every returned dist^2 within the bar of the float64 d2 of the returned row; (2) the returned row is one of the
    float64 rows within the bar of that rank; (3) idx equals the stable float64 order wherever the float64 gaps to both sorted
    neighbours exceed twice the bar -- at most `max_loose` of the positions may be left out.  Returns (worst ratio, share left out)."""
    n, r = d2_all.shape
    want_d2, want_i = ref.smallest_stable(d2_all, min(k + 1, r))
    dist64, idx = dist.double().numpy(), idx.numpy().astype(np.int64)
    assert dist64.shape == (n, k) and idx.shape == (n, k)
    assert np.isfinite(dist64).all() and (dist64 >= 0).all()
    assert idx.min() >= 0 and idx.max() < r
    assert all(len(set(row)) == k for row in idx)
    d2_row = np.take_along_axis(d2_all, idx, 1)
    a_row = np.take_along_axis(a_all, idx, 1)
    err = np.abs(dist64 ** 2 - d2_row)
    ratio = float((err / (EPS * a_row)).max())
    print(f"   worst |d^2 - d2_ref| / (2^-24 A) = {ratio:.3f}")
    assert (err <= t * EPS * a_row + 2 * EPS * d2_row).all(), ratio
    a_ref = np.take_along_axis(a_all, want_i[:, :k], 1)
    bar2 = 2 * t * EPS * np.maximum(a_row, a_ref)
    assert (np.abs(d2_row - want_d2[:, :k]) <= bar2).all()
    strict = np.ones((n, k), dtype=bool)
    for j in range(k):
        if j > 0:
            strict[:, j] &= want_d2[:, j] - want_d2[:, j - 1] > bar2[:, j]
        if j + 1 < want_d2.shape[1]:
            strict[:, j] &= want_d2[:, j + 1] - want_d2[:, j] > bar2[:, j]
    loose = 1.0 - strict.mean()
    print(f"   positions left out of the index comparison: {100 * loose:.2f} %")
    assert loose <= max_loose, loose
    assert np.array_equal(idx[strict], want_i[:, :k][strict])
    return ratio, loose


def scores_tol(rows, bank, k, t, mod=ref):
    """Per-row bound on |k-NN mean score - float64| from the bar t (the selection may swap rows within it):
    |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b)) per root, plus the k roundings of the sequential sum."""
    d2, idx = mod.kneighbors64(rows, bank, k)
    a = np.concatenate([np.take_along_axis(mod.scale_a(rows[i:i + 512], bank), idx[i:i + 512], 1) for i in range(0, rows.shape[0], 512)])
    e = 2 * t * EPS * a + 2 * EPS * d2
    dref = np.sqrt(d2)
    return np.minimum(np.sqrt(e), e / np.maximum(dref, 1e-300)).mean(1) + (k + 3) * EPS * dref.mean(1)
