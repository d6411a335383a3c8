"""Float64 reference of the per-position Gaussian detector (PaDiM, Defard et al., ICPR 2020, as anomalib implements it), numpy /
scipy only: gather the selected columns, per position the mean, ``np.cov(rowvar=False) + eps I``, ``np.linalg.inv`` and
``scipy.spatial.distance.mahalanobis``.  Shared by tests/test_padim_host.py and tests/test_hip_padim.py.

Rows are [n_img * P][D] with row n P + p = position p of image n."""
import numpy as np
from scipy.spatial.distance import mahalanobis


def gather(rows, sel, P):
    """rows [n * P][D] -> float64 [n][P][d]: the selected columns, image by image."""
    r = np.asarray(rows, dtype=np.float64)
    return r.reshape(r.shape[0] // P, P, r.shape[1])[:, :, np.asarray(sel, dtype=np.int64)]


def stats(g):
    """g [n][P][d] -> (mean [P][d], scatter [P][d][d], bar_mean, bar_scatter): the centred statistics and the magnitudes the
    project's 1e-10 bars of tests/test_hip_gde.py scale with (mean |x| and |c|^T |c|)."""
    mean = g.mean(0)
    c = g - mean
    ac = np.abs(c)
    return mean, np.einsum("npa,npb->pab", c, c), np.abs(g).mean(0), np.einsum("npa,npb->pab", ac, ac)


def fit(rows, sel, P, eps=0.01):
    """(mean [P][d], cov [P][d][d], inverse covariance [P][d][d]) of the fit rows, position by position with numpy's own cov."""
    g = gather(rows, sel, P)
    d = g.shape[2]
    mean = g.mean(0)
    cov = np.stack([np.cov(g[:, p, :], rowvar=False) + eps * np.eye(d) for p in range(P)])
    return mean, cov, np.stack([np.linalg.inv(c) for c in cov])


def scores(rows, sel, P, mean, vi):
    """[n * P] Mahalanobis distances of the query rows, vectorised; a few of them are checked against scipy's loop form."""
    g = gather(rows, sel, P)
    c = g - mean
    fast = np.sqrt(np.einsum("npa,pab,npb->np", c, vi, c))
    n = g.shape[0]
    for i, p in {(0, 0), (n // 2, P // 2), (n - 1, P - 1)}:
        assert abs(fast[i, p] - mahalanobis(g[i, p], mean[p], vi[p])) <= 1e-9 * fast[i, p]
    return fast.reshape(-1)


def scores_from_factor(rows, sel, P, mu_hi, mu_lo, w):
    """float64 ||W_p (x_sel - (mu_hi + mu_lo))|| on the fp32 mean pair and the lower triangle of the fp32 W the kernel is given: the
    bar then judges the kernel's arithmetic only (test_hip_gde.py's _maha_ref)."""
    mu = np.asarray(mu_hi, dtype=np.float64) + np.asarray(mu_lo, dtype=np.float64)
    wl = np.tril(np.nan_to_num(np.asarray(w, dtype=np.float64)))
    y = np.einsum("pab,npb->npa", wl, gather(rows, sel, P) - mu)
    return np.linalg.norm(y, axis=2).reshape(-1)


def synthetic_rows(n_img, P, D, seed, draw=0, spread=1.0):
    """x[n][p] = m_p + spread * A (s_p * z) as float32 rows [n_img * P][D]: a mean m_p and scales s_p in [0.5, 1.5] per position,
    one mixing matrix A = (I + G / sqrt(D)) / 2 for all -- covariances A diag(s_p^2) A^T with condition numbers of a few tens.
    `seed` fixes the distribution, `draw` the sample (fit rows and query rows share the seed and differ in the draw)."""
    rng = np.random.RandomState(seed)
    m = rng.randn(P, D) * 2.0
    s = rng.uniform(0.5, 1.5, (P, D))
    a = 0.5 * np.eye(D) + 0.5 * rng.randn(D, D) / np.sqrt(D)
    z = np.random.RandomState(seed * 1009 + draw + 1).randn(n_img, P, D)
    return (m + spread * ((z * s) @ a.T)).reshape(n_img * P, D).astype(np.float32)
