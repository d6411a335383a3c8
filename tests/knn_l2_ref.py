"""float64 numpy yardsticks of the Euclidean kNN (csrc/knn_l2.hip), shared by the knn-l2 tests.  The definition: on the raw fp32
rows, d2(q, b) = max(|q|^2 + |b|^2 - 2 <q, b>, 0) and d = sqrt(d2) -- the expanded form torch.cdist evaluates -- in float64, the
order a stable argsort of d2: lexicographic on (d2, row).  The patch score is the mean of the k = 3 smallest d."""
import numpy as np
import torch

from knn_index_ref import auroc64, smallest_stable, strict_positions  # noqa: F401  (re-exported: one selection for both metrics)

EPS = 2.0 ** -24


def _np64(a):
    return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)


def sqnorms64(x):
    x = _np64(x)
    return (x * x).sum(1)


def d2_64(x, bank):
    """[N][R] float64 squared distances max(|x|^2 + |b|^2 - 2 <x, b>, 0)."""
    x, b = _np64(x), _np64(bank)
    return np.maximum((x * x).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (x @ b.T), 0.0)


def scale_a(x, bank):
    """[N][R] A = |q|^2 + |b|^2 + 2 sum_i |q_i| |b_i|: what the rounding errors of the fp32 evaluation scale with (every product of
    the three sums enters with its magnitude); the bar on a squared distance is tau 2^-24 A."""
    x, b = np.abs(_np64(x)), np.abs(_np64(bank))
    return (x * x).sum(1)[:, None] + (b * b).sum(1)[None, :] + 2.0 * (x @ b.T)


def kneighbors64(x, bank, m, chunk=512):
    """(d2 [N][m'], idx [N][m'], m' = min(m, R)): the m' nearest bank rows of every query, lexicographic on (d2, row)."""
    m = min(int(m), bank.shape[0])
    n = x.shape[0]
    d2 = np.empty((n, m))
    idx = np.empty((n, m), dtype=np.int64)
    for i in range(0, n, chunk):
        d2[i:i + chunk], idx[i:i + chunk] = smallest_stable(d2_64(x[i:i + chunk], bank), m)
    return d2, idx


def patch_scores64(x, bank, k=3):
    d2, _ = kneighbors64(x, bank, k)
    return np.sqrt(d2[:, :k]).mean(1)


def image_scores64(x, bank, n_patches, neighbours=None, k=3, gap=1e-5):
    """float64 image scores (PatchCore eq. 6-7 on Euclidean distances) of x [n_img * P][D].  Returns s_max, p_star, patch_scores and,
    with `neighbours` = b: w, score = w s_max, m_star, nbr and `fragile` [n_img] -- the top two patch scores, the two nearest rows of
    x_{p*} (in d2) or the b-th / (b + 1)-th neighbours of B_{m*} (in d2) lie closer than `gap` relative to the values' scale."""
    b64 = _np64(bank)
    r = b64.shape[0]
    s = patch_scores64(x, bank, k).reshape(-1, n_patches)
    p_star = s.argmax(1)
    s_max = s[np.arange(s.shape[0]), p_star]
    out = {"s_max": s_max, "p_star": p_star, "patch_scores": s}
    if neighbours is None:
        return out
    top2 = np.sort(s, axis=1)[:, -2:]
    fragile = (top2[:, 1] - top2[:, 0] <= gap * top2[:, 1]) if n_patches > 1 else np.zeros(s.shape[0], dtype=bool)
    xs = _np64(x)[np.arange(s.shape[0]) * n_patches + p_star]
    d2 = d2_64(xs, b64)
    a = scale_a(xs, b64)
    v2, i2 = smallest_stable(d2, 2)
    m_star = i2[:, 0]
    if r > 1:
        fragile |= v2[:, 1] - v2[:, 0] <= gap * a[np.arange(a.shape[0]), m_star]
    bp = min(int(neighbours), r)
    dc = d2_64(b64[m_star], b64)
    ac = scale_a(b64[m_star], b64)
    dn, nbr = smallest_stable(dc, bp + 1)
    if r > bp:
        fragile |= dn[:, bp] - dn[:, bp - 1] <= gap * np.take_along_axis(ac, nbr[:, bp - 1:bp], 1)[:, 0]
    nbr = nbr[:, :bp]
    # direct differences for the weight's distances, as the kernel takes them
    d_m = np.sqrt(((xs - b64[m_star]) ** 2).sum(1))
    d_n = np.sqrt(((xs[:, None, :] - b64[nbr]) ** 2).sum(2))
    dmax = d_n.max(1)
    w = 1.0 - np.exp(d_m - dmax) / np.exp(d_n - dmax[:, None]).sum(1)
    out.update(w=w, score=w * s_max, fragile=fragile, m_star=m_star, nbr=nbr)
    return out
