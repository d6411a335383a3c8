"""The definition of the defect-region calls (csrc/regions.hip, ops.label_regions / region_stats / region_filter / pro_weights,
tools.defect_regions) in library calls -- scipy.ndimage and numpy, nothing of the project's -- and the mask zoo that the host
and the GPU tests share.  Everything is integers: the tests compare with exact equality."""
import numpy as np
from scipy import ndimage

STRUCTURES = {8: np.ones((3, 3), dtype=int), 4: ndimage.generate_binary_structure(2, 1)}


def label(mask, connectivity=8):
    """(labels int32 [H][W], count): ndimage.label numbers the components in raster order of their first pixel."""
    lab, k = ndimage.label(np.asarray(mask) != 0, STRUCTURES[connectivity])
    return lab.astype(np.int32), int(k)


def label_batch(masks, connectivity=8):
    labs, counts = zip(*(label(m, connectivity) for m in masks))
    counts = np.asarray(counts, dtype=np.int32)
    return np.stack(labs), counts, np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def stats(lab, k, scores=None):
    """area [k], bbox [k][4] = x0, y0, x1, y1 (maxima inclusive), coord_sum [k][2] = sum x, sum y, peak [k], peak_pos [k]."""
    h, w = lab.shape
    area = np.bincount(lab.ravel(), minlength=k + 1)[1:].astype(np.int32)
    bbox = np.zeros((k, 4), dtype=np.int32)
    csum = np.zeros((k, 2), dtype=np.int64)
    peak = np.zeros(k, dtype=np.float32)
    pos = np.zeros(k, dtype=np.int32)
    ys, xs = np.mgrid[0:h, 0:w]
    for r, sl in enumerate(ndimage.find_objects(lab, max_label=k)):
        m = lab == r + 1
        bbox[r] = (sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1)
        csum[r] = (xs[m].sum(dtype=np.int64), ys[m].sum(dtype=np.int64))
        if scores is not None:
            masked = np.where(m, scores, -np.inf).ravel()
            peak[r] = masked.max()
            pos[r] = np.flatnonzero(m.ravel())[np.argmax(scores.ravel()[m.ravel()])]      # first index attaining the peak
    return area, bbox, csum, (peak if scores is not None else None), (pos if scores is not None else None)


def stats_batch(labs, counts, scores=None):
    parts = [stats(l, int(k), None if scores is None else scores[i]) for i, (l, k) in enumerate(zip(labs, counts))]
    cat = lambda j: np.concatenate([p[j] for p in parts]) if scores is not None or j < 3 else None
    return tuple(cat(j) for j in range(5))


def filter_labels(lab, k, keep):
    """keep bool [k] -> (mask uint8, labels renumbered 1 .. in the same order, new count)."""
    new = np.concatenate(([0], np.where(keep, np.cumsum(keep), 0))).astype(np.int32)
    out = new[lab]
    return (out != 0).astype(np.uint8), out, int(np.count_nonzero(keep))


def pro_weights(labs, counts):
    """The planes metrics.compute_pro_gpu builds on the host."""
    fp_w = (labs == 0).astype(np.uint8)
    pro_w = np.zeros(labs.shape, dtype=np.float64)
    for i, (lab, k) in enumerate(zip(labs, counts)):
        if k:
            sizes = np.bincount(lab.ravel())[1:]
            pro_w[i] = np.concatenate([[0.0], 1.0 / sizes])[lab]
    return fp_w.reshape(-1), pro_w.reshape(-1)


def defect_regions(maps, threshold, min_area=1, connectivity=8):
    """tools.defect_regions on the host: (pred_masks uint8 [n][H][W], labels int32, per image a list of dicts)."""
    maps = np.asarray(maps, dtype=np.float32)
    masks, labs, regions = [], [], []
    for s in maps:
        lab, k = label(np.greater_equal(s, np.float32(threshold)), connectivity)
        area = np.bincount(lab.ravel(), minlength=k + 1)[1:]
        m, lab2, k2 = filter_labels(lab, k, area >= min_area)
        a, bb, cs, pk, pp = stats(lab2, k2, s)
        w = s.shape[1]
        regions.append([dict(box=tuple(int(v) for v in bb[r]), area=int(a[r]), centroid=(cs[r, 0] / a[r], cs[r, 1] / a[r]),
                             score=float(pk[r]), peak=(int(pp[r] % w), int(pp[r] // w))) for r in range(k2)])
        masks.append(m)
        labs.append(lab2)
    return np.stack(masks), np.stack(labs), regions


# ---- the mask zoo: the smallest shapes at which a tiled union-find labeller goes wrong ----
def spiral(side, gap=1, start=0):
    """A one-pixel-wide square spiral walked inwards from (start, start), `gap` background pixels between its turns: one
    component under both connectivities whose path runs through the whole image."""
    m = np.zeros((side, side), dtype=np.uint8)
    inside = lambda x, y: start <= x < side - start and start <= y < side - start
    x = y = start
    dx, dy = 1, 0
    m[y, x] = 1
    turns = 0
    while turns < 2:
        nx, ny, ax, ay = x + dx, y + dy, x + (gap + 1) * dx, y + (gap + 1) * dy
        if inside(nx, ny) and not m[ny, nx] and not (inside(ax, ay) and m[ay, ax]):
            x, y, turns = nx, ny, 0
            m[y, x] = 1
        else:
            dx, dy, turns = -dy, dx, turns + 1
    return m


def two_spirals(side):
    """Two interleaved spirals, one background pixel apart: two components whose paths wind through each other."""
    return spiral(side, gap=3) | spiral(side, gap=3, start=2)


def diagonal_spirals(k):
    """two_spirals(k) turned by 45 degrees into a (2k - 1)-sided image: edge neighbours become diagonal neighbours, so under 8
    there are the two spirals, joined by diagonal steps only, and under 4 every pixel is a component of its own."""
    src = two_spirals(k)
    out = np.zeros((2 * k - 1, 2 * k - 1), dtype=np.uint8)
    ys, xs = np.nonzero(src)
    out[xs - ys + k - 1, xs + ys] = 1
    return out


def diagonal_touch():
    """Two 4-connected L shapes that touch at one corner only: one component under 8, two under 4."""
    return np.array([[1, 1, 0, 0],
                     [1, 0, 0, 0],
                     [0, 1, 1, 1],
                     [0, 0, 0, 1]], np.uint8)


def interleaved_diagonals(h, w):
    """Diagonal lines of both directions that cross: joined by diagonal steps only."""
    ys, xs = np.mgrid[0:h, 0:w]
    return (((xs - ys) % 6 == 0) | ((xs + ys) % 6 == 3)).astype(np.uint8)


def comb(h, w):
    """Vertical teeth on every other column, joined only by the last row."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[:, ::2] = 1
    m[-1, :] = 1
    return m


def nested_u(side):
    """Nested U shapes, open at the top, that do not touch each other."""
    m = np.zeros((side, side), dtype=np.uint8)
    for o in range(0, side // 2, 2):
        m[o:side - o, o] = 1
        m[o:side - o, side - 1 - o] = 1
        m[side - 1 - o, o:side - o] = 1
    return m


def checkerboard(h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    return ((xs + ys) % 2 == 0).astype(np.uint8)


def stripes(h, w, period=4):
    ys, xs = np.mgrid[0:h, 0:w]
    return ((xs + ys) % period == 0).astype(np.uint8)


def rings(side):
    ys, xs = np.mgrid[0:side, 0:side]
    d = np.maximum(np.abs(xs - side // 2), np.abs(ys - side // 2))
    return (d % 3 == 0).astype(np.uint8)


def random_mask(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def blobs(n, side, seed, threshold=0.5):
    """Smooth random fields like upsampled anomaly maps: float32 [n][side][side] with a few blobs above `threshold`."""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((n, side, side)), (0, side / 24, side / 24))
    f = f / np.abs(f).max(axis=(1, 2), keepdims=True)
    return (0.5 + f).astype(np.float32)


def zoo(T):
    """name -> uint8 mask; T: the labelling kernel's tile side (ops.REGION_TILE)."""
    s = 2 * T + 1
    z = {
        "1x1_fg": np.ones((1, 1), np.uint8), "1x1_bg": np.zeros((1, 1), np.uint8),
        "1x7": np.array([[1, 1, 0, 1, 0, 1, 1]], np.uint8), "7x1": np.array([[1, 1, 0, 1, 0, 1, 1]], np.uint8).T.copy(),
        "all_bg": np.zeros((T + 1, T + 1), np.uint8), "all_fg": np.ones((T + 1, s), np.uint8),
        "spiral": spiral(s), "two_spirals": two_spirals(s), "diagonal_spirals": diagonal_spirals(T + 1), "diagonal_touch": diagonal_touch(),
        "diagonals": interleaved_diagonals(s, s),
        "comb": comb(s, s), "nested_u": nested_u(s), "checkerboard": checkerboard(s, s), "checkerboard_3xs": checkerboard(3, s),
        "stripes": stripes(s, T + 1), "rings": rings(s),
    }
    for side in (T - 1, T, T + 1, s):
        z[f"random_{side}"] = random_mask(side, side, 0.5, 100 + side)
    z[f"random_3x{s}"] = random_mask(3, s, 0.5, 7)
    for d in (0.1, 0.4, 0.6, 0.9):
        z[f"density_{d}"] = random_mask(s, s, d, int(d * 100))
    return z
