"""float64 numpy yardsticks of SPADE's image-conditioned gallery (csrc/knn_gallery.hip), shared by the knn-gallery tests.  On the raw
fp32 rows, x [Q P][D] and bank [T P][D] holding P rows per image, image after image:
  descriptor      the mean of an image's P rows, rounded once to fp32 (the descriptor IS that fp32 row; descriptors64 gives the
                  unrounded mean, descriptors32 the descriptor);
  stage 1         d2 = sum (desc_q - desc_t)^2 by direct differences of the descriptors; the gallery of a query image = the first K' = min(K, T)
                  columns of a stable ascending argsort (equal distances to the smaller image);
  stage 2         per query row, the k nearest rows among the gallery images' blocks by knn_l2_ref's expanded d2, lexicographic on
                  (d2, GLOBAL bank row);
  scores          patch: the mean of the k roots; retrieval (SPADE's image score): the mean of the K' stage-1 roots."""
import numpy as np

from knn_l2_ref import EPS, _np64, d2_64, scale_a, smallest_stable  # noqa: F401


def descriptors64(x, p):
    x = _np64(x)
    return x.reshape(-1, int(p), x.shape[1]).mean(1)


def descriptors32(x, p):
    """The descriptors as defined: the float64 mean rounded once to fp32 (returned as float64 values)."""
    return descriptors64(x, p).astype(np.float32).astype(np.float64)


def direct_d2_64(q, b):
    """[Q][T] float64 sum (q - b)^2 by direct differences."""
    q, b = _np64(q), _np64(b)
    return ((q[:, None, :] - b[None, :, :]) ** 2).sum(2)


def gallery64(x, bank, p, kk):
    """(gallery int64 [Q][K'], d2 [Q][K'], all d2 [Q][T]) of stage 1."""
    d2 = direct_d2_64(descriptors32(x, p), descriptors32(bank, p))
    order = np.argsort(d2, axis=1, kind="stable")[:, :min(int(kk), d2.shape[1])]
    return order, np.take_along_axis(d2, order, 1), d2


def gallery_rows(gallery_row, p, t=None):
    """Global bank rows of one query image's gallery, in gallery order; entries outside 0..t-1 are left out."""
    ids = [int(g) for g in gallery_row if t is None or 0 <= int(g) < t]
    if not ids:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.arange(g * p, (g + 1) * p, dtype=np.int64) for g in ids])


def restricted_knn64(x, bank, gallery, p, k, t=None):
    """(d2 [Q P][k], rows [Q P][k] int64 global bank rows, A [Q P][k]): the k nearest gallery rows of every query row, lexicographic
    on (d2, global row); slots a gallery cannot fill hold (inf, -1, nan).  A: knn_l2_ref.scale_a of the pair."""
    x64 = _np64(x)
    n = x64.shape[0]
    d2o, io, ao = np.full((n, k), np.inf), np.full((n, k), -1, dtype=np.int64), np.full((n, k), np.nan)
    for q in range(n // p):
        rows = np.sort(gallery_rows(gallery[q], p, t))          # ascending global rows: a stable argsort is then lexicographic
        if rows.size == 0:
            continue
        xs = x64[q * p:(q + 1) * p]
        d2, a = d2_64(xs, _np64(bank)[rows]), scale_a(xs, _np64(bank)[rows])
        m = min(k, rows.size)
        order = np.argsort(d2, axis=1, kind="stable")[:, :m]
        d2o[q * p:(q + 1) * p, :m] = np.take_along_axis(d2, order, 1)
        io[q * p:(q + 1) * p, :m] = rows[order]
        ao[q * p:(q + 1) * p, :m] = np.take_along_axis(a, order, 1)
    return d2o, io, ao


def next_gap64(x, bank, gallery, p, k, t=None):
    """d2 [Q P][k + 1] of the k + 1 nearest gallery rows (inf where there are fewer): the gaps the strict index comparison needs."""
    return restricted_knn64(x, bank, gallery, p, k + 1, t)[0]


def patch_scores64(x, bank, gallery, p, k=3, t=None):
    d2, _, _ = restricted_knn64(x, bank, gallery, p, k, t)
    return np.sqrt(d2).mean(1)


def retrieval_scores64(x, bank, p, kk):
    _, d2, _ = gallery64(x, bank, p, kk)
    return np.sqrt(d2).mean(1)
