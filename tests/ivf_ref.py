"""float64 numpy yardsticks of the inverted-file index of the Euclidean kNN (csrc/knn_ivf.hip), shared by the knn-ivf tests.  The
definition, on the raw fp32 rows and with knn_l2_ref's expanded d2 = max(|x|^2 + |b|^2 - 2 <x, b>, 0):
  fit       Lloyd's k-means from given initial rows: every row goes to its nearest centroid, lexicographic on (d2, cell); a centroid
            becomes the mean of its rows, summed in row order and rounded once to fp32; a cell without rows keeps its centroid;
  probes    the nprobe cells of a query: the first columns of a stable ascending argsort of d2 to the centroids -- (d2, cell);
  search    per query the k smallest (d2, ORIGINAL bank row) pairs among the rows of the probed cells; an entry outside 0..nlist-1
            is skipped; slots the cells cannot fill hold (inf, -1).
The bar on a squared distance is the one tests/knn_l2_ref.py states, TAU = 64 units of 2^-24 A, A = |q|^2 + |b|^2 + 2 sum |q_i| |b_i|."""
import numpy as np

from knn_l2_ref import EPS, _np64, d2_64, scale_a  # noqa: F401

TAU = 64.0


def segment_means64(x, order, offsets, prev):
    """[nlist][D] float64: the mean of x[order[offsets[g]:offsets[g + 1]]] added in that sequence; an empty segment keeps prev[g]."""
    x, out = _np64(x), _np64(prev).copy()
    for g in range(len(offsets) - 1):
        rows = np.asarray(order[offsets[g]:offsets[g + 1]], dtype=np.int64)
        if rows.size:
            out[g] = np.cumsum(x[rows], axis=0)[-1] / rows.size      # cumsum: strictly in sequence
    return out


def assign64(x, centroids, check_bar=True):
    """(assign [N] int64, d2 of the assignment [N]); with check_bar asserts that the nearest and the second nearest centroid of every
    row differ by more than the bar of either: nothing the fp32 kernels may decide differently."""
    d2 = d2_64(x, centroids)
    order = np.argsort(d2, axis=1, kind="stable")
    a = order[:, 0]
    rows = np.arange(d2.shape[0])
    if check_bar and d2.shape[1] > 1:
        b = order[:, 1]
        bar = TAU * EPS * scale_a(x, centroids)
        assert (d2[rows, b] - d2[rows, a] > bar[rows, a] + bar[rows, b]).all(), "the blobs are not separated by the bar"
    return a, d2[rows, a]


def lloyd64(x, init_rows, iters, check_bar=True):
    """Lloyd from the rows x[init_rows] -> (centroids [nlist][D] float64 holding fp32 values, assign [N] to the final centroids,
    objectives [iters + 1]: the sum of d2 to the assigned centroid before every update and at the end)."""
    x64 = _np64(x)
    cent = x64[np.asarray(init_rows, dtype=np.int64)].copy()
    nlist = cent.shape[0]
    objs = []
    for _ in range(int(iters)):
        a, d2 = assign64(x64, cent, check_bar)
        objs.append(d2.sum())
        order = np.argsort(a, kind="stable")
        offsets = np.searchsorted(a[order], np.arange(nlist + 1))
        cent = segment_means64(x64, order, offsets, cent).astype(np.float32).astype(np.float64)
    a, d2 = assign64(x64, cent, check_bar)
    objs.append(d2.sum())
    return cent, a, np.array(objs)


def objective64(x, centroids):
    return d2_64(x, centroids).min(1).sum()


def probes64(x, centroids, nprobe):
    """int64 [N][nprobe]: the nearest cells by (d2, cell)."""
    return np.argsort(d2_64(x, centroids), axis=1, kind="stable")[:, :int(nprobe)]


def restricted_knn64(x, bank, cell_of_row, probes, nlist, k):
    """bank [R][D] in the ORIGINAL row order, cell_of_row [R] the cell of every original row, probes [N][nprobe] -> (d2 [N][k],
    rows [N][k] int64 original rows, A [N][k]): the k smallest (d2, original row) among the rows of the probed cells; missing slots
    (inf, -1, nan)."""
    probes = np.asarray(probes, dtype=np.int64)
    cell_of_row = np.asarray(cell_of_row, dtype=np.int64)
    n, r = x.shape[0], bank.shape[0]
    valid = (probes >= 0) & (probes < nlist)
    hit = np.zeros((n, nlist + 1), dtype=bool)
    hit[np.arange(n)[:, None], np.where(valid, probes, nlist)] = True
    hit[:, nlist] = False
    mask = hit[:, cell_of_row]                                       # [N][R]
    d2 = np.where(mask, d2_64(x, bank), np.inf)
    a = scale_a(x, bank)
    m = min(int(k), r)
    order = np.argsort(d2, axis=1, kind="stable")[:, :m]            # original rows ascend: stable = lexicographic (d2, row)
    d2o, io, ao = np.full((n, k), np.inf), np.full((n, k), -1, dtype=np.int64), np.full((n, k), np.nan)
    d2o[:, :m] = np.take_along_axis(d2, order, 1)
    io[:, :m] = np.where(np.isfinite(d2o[:, :m]), order, -1)
    ao[:, :m] = np.where(np.isfinite(d2o[:, :m]), np.take_along_axis(a, order, 1), np.nan)
    return d2o, io, ao


def reference_case(x, bank, cell_of_row, probes, nlist, k, cap=0.01):
    """What the comparison with the kernels needs that the reference alone gives: the k + 1 nearest probed rows, the bar of every
    pick and where the row comparison is strict (the gaps to both neighbours in the order exceed the bars of both); asserts, on the
    reference alone, that at most `cap` of the (query, slot) pairs are left out."""
    d2, rows, a = restricted_knn64(x, bank, cell_of_row, probes, nlist, k + 1)
    bar = TAU * EPS * np.nan_to_num(a)
    strict = np.isfinite(d2[:, :k])
    with np.errstate(invalid="ignore"):                             # inf - inf: both slots are missing
        for j in range(k):
            if j > 0:
                strict[:, j] &= ~(d2[:, j] - d2[:, j - 1] <= bar[:, j] + bar[:, j - 1])
            strict[:, j] &= ~(d2[:, j + 1] - d2[:, j] <= bar[:, j] + bar[:, j + 1])
    present = np.isfinite(d2[:, :k])
    loose = float((present & ~strict).sum()) / max(1, present.size)
    assert loose <= cap, f"{loose:.4f} of the (query, slot) pairs are near-ties: choose other seeds"
    return d2[:, :k], rows[:, :k], a[:, :k], strict, loose
