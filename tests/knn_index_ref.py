"""float64 numpy yardsticks of the index-returning kNN (csrc/knn.hip ssad_cosine_knn_index), the row selection and the image scores
(csrc/image_score.hip), shared by the knn-index tests.  Everything is a brute force on the same fp32 inputs: normalise, 1 - X B^T,
clip to [0, 2], stable argsort -- which is the lexicographic (distance, index) order."""
import numpy as np
import torch


def _np64(a):
    return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)


def unit_rows64(x):
    x = _np64(x)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def distances64(x, bank_n):
    """[N][R] float64 cosine distances clip(1 - <x / ||x||, B_r>, 0, 2) of raw rows x to the (already normalised) bank rows."""
    return np.clip(1.0 - unit_rows64(x) @ _np64(bank_n).T, 0.0, 2.0)


def smallest_stable(d, m):
    """First min(m, R) columns of np.argsort(d, axis=1, kind='stable') and their values, without sorting whole rows: the candidates
    of a row are all columns not above its (m + 1)-th smallest value, ordered by (value, column)."""
    n, r = d.shape
    m = min(int(m), r)
    if r <= 4 * m + 8:
        idx = np.argsort(d, axis=1, kind="stable")[:, :m]
        return np.take_along_axis(d, idx, 1), idx
    thr = np.partition(d, m - 1, axis=1)[:, m - 1]
    idx = np.empty((n, m), dtype=np.int64)
    for i in range(n):
        cand = np.flatnonzero(d[i] <= thr[i])                       # ascending columns
        idx[i] = cand[np.argsort(d[i, cand], kind="stable")[:m]]
    return np.take_along_axis(d, idx, 1), idx


def kneighbors64(x, bank_n, m, chunk=512):
    """(dist [N][m'], idx [N][m'], m' = min(m, R)): the m' nearest bank rows of every query in float64, lexicographic on (distance,
    row), query chunks of `chunk` rows."""
    b = _np64(bank_n)
    q = unit_rows64(x)
    m = min(int(m), b.shape[0])
    dist = np.empty((q.shape[0], m))
    idx = np.empty((q.shape[0], m), dtype=np.int64)
    for i in range(0, q.shape[0], chunk):
        d = np.clip(1.0 - q[i:i + chunk] @ b.T, 0.0, 2.0)
        dist[i:i + chunk], idx[i:i + chunk] = smallest_stable(d, m)
    return dist, idx


def strict_positions(dist_sorted, k, gap=1e-5):
    """mask [N][k]: position j of a query is compared index for index when the float64 gaps to its sorted neighbours j - 1 and j + 1
    (where they exist) both exceed `gap`.  dist_sorted holds at least min(k + 1, R) sorted distances per query."""
    n, m = dist_sorted.shape
    ok = np.ones((n, k), dtype=bool)
    for j in range(k):
        if j > 0:
            ok[:, j] &= dist_sorted[:, j] - dist_sorted[:, j - 1] > gap
        if j + 1 < m:
            ok[:, j] &= dist_sorted[:, j + 1] - dist_sorted[:, j] > gap
    return ok


def image_scores64(x, bank_n, n_patches, neighbours=None, k=3, gap=1e-5):
    """float64 image scores of x [n_img * P][D] against the normalised bank.  Returns a dict: s_max [n_img], p_star [n_img] and, with
    `neighbours` = b, also w [n_img], score [n_img] = w s_max, and `fragile` [n_img]: the top two patch scores, the first / second
    nearest rows of x_{p*} or the b-th / (b + 1)-th neighbours of B_{m*} lie closer than `gap`."""
    b64 = _np64(bank_n)
    r = b64.shape[0]
    dk, _ = kneighbors64(x, bank_n, k)
    s = dk[:, :k].mean(1).reshape(-1, n_patches)
    p_star = s.argmax(1)                                            # first maximum: the smallest p on ties
    s_max = s[np.arange(s.shape[0]), p_star]
    out = {"s_max": s_max, "p_star": p_star, "patch_scores": s}
    if neighbours is None:
        return out
    top2 = np.sort(s, axis=1)[:, -2:]
    fragile = (top2[:, 1] - top2[:, 0] <= gap) if n_patches > 1 else np.zeros(s.shape[0], dtype=bool)
    xs = _np64(x)[np.arange(s.shape[0]) * n_patches + p_star]
    d = distances64(xs, bank_n)                                     # [n_img][R]
    d2, i2 = smallest_stable(d, 2)
    m_star = i2[:, 0]
    if r > 1:
        fragile |= d2[:, 1] - d2[:, 0] <= gap
    bp = min(int(neighbours), r)
    dc = np.clip(1.0 - b64[m_star] @ b64.T, 0.0, 2.0)              # distances of B_{m*} to the bank
    dn, nbr = smallest_stable(dc, bp + 1)
    if r > bp:
        fragile |= dn[:, bp] - dn[:, bp - 1] <= gap
    nbr = nbr[:, :bp]
    num = np.exp(d[np.arange(d.shape[0]), m_star])
    den = np.exp(np.take_along_axis(d, nbr, 1)).sum(1)
    w = 1.0 - num / den
    out.update(w=w, score=w * s_max, fragile=fragile, m_star=m_star, nbr=nbr)
    return out


def auroc64(labels, scores):
    """Area under the ROC curve by the rank statistic (ties count half), float64."""
    y = np.asarray(labels).astype(bool)
    s = np.asarray(scores, dtype=np.float64)
    pos, neg = s[y], s[~y]
    gt = (pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()
    return float(gt) / (pos.size * neg.size)
