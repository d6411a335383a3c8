"""Cut-paste primitives on PIL images (host side of the synthetic-defect generator).

Mirrors src/self_supervised/dataset_generator.py:15-275 of the reference: same function names, arguments and --
because results are compared against vectors produced by the reference under a fixed ``random.seed`` -- the same
order of draws from Python's ``random``.  The batched GPU version of the pixel work (polygon rasterise, masked
paste, rotated scars, poly-lines, jitter, normalise) is csrc/augment.hip, driven by augment.py.
"""
import random
from typing import Tuple

import numpy as np
from PIL import Image, ImageDraw
from scipy import ndimage


class Container:
    """Centred square region defects are clamped into (dataset_generator.py:15-24)."""

    def __init__(self, imsize: tuple, scaling_factor: float) -> None:
        half = int(imsize[0] / 2)
        reach = half / scaling_factor
        self.center = half
        self.dim = int(imsize[0] / scaling_factor)
        self.left = self.top = int(half - reach)
        self.right = self.bottom = int(half + reach)
        self.width = self.right - self.left
        self.height = self.bottom - self.top


# ---- object mask: Canny -> dilate -> close -> fill -> erode -> largest component (dataset_generator.py:27-39) ----
def _canny(gray, sigma, low, high):
    """skimage.feature.canny(gray_uint8, sigma, low_threshold=low, high_threshold=high) -- THIRD-PARTY RESTATEMENT (scikit-image is
    not a dependency of this package), pinned: identical edge maps to scikit-image 0.18.3 on tests/golden/skimage.npz, where the
    REFERENCE's own obj_mask built on it is reproduced exactly too.  Its documented pipeline, step for step -- the image scaled to [0, 1] (thresholds divided
    by 255 accordingly), Gaussian smoothing with zero ('constant') borders renormalised by the smoothed all-ones mask, Sobel
    derivatives, non-maximum suppression by bilinear interpolation of the magnitude along the gradient direction on the
    border-eroded mask, double threshold and hysteresis over 8-connected components."""
    out = _canny_thinned(gray, sigma, low)
    if out is None:
        return np.zeros(gray.shape, bool)
    high = high / 255.0
    low_mask = out > 0
    lab, n = ndimage.label(low_mask, structure=np.ones((3, 3), int))
    if n == 0:
        return low_mask
    high_mask = low_mask & (out >= high)
    sums = ndimage.sum_labels(high_mask, lab, np.arange(n + 1))
    good = sums > 0
    good[0] = False
    return good[lab]


def _canny_thinned(gray, sigma, low):
    """The first half of _canny: the gradient magnitude after non-maximum suppression and the low threshold (0 elsewhere), the plane
    hysteresis runs on; None for an image with a side below 3 (no interior pixel: no edges)."""
    img = gray.astype(np.float64) / 255.0
    low = low / 255.0
    bleed = ndimage.gaussian_filter(np.ones_like(img), sigma, mode="constant", cval=0.0) + np.finfo(np.float64).eps
    sm = ndimage.gaussian_filter(img, sigma, mode="constant", cval=0.0) / bleed
    js = ndimage.sobel(sm, axis=1)
    is_ = ndimage.sobel(sm, axis=0)
    mag = np.hypot(is_, js)
    h, w = mag.shape
    out = np.zeros_like(mag)
    if h < 3 or w < 3:
        return None
    c = (slice(1, -1), slice(1, -1))

    def sh(dx, dy):                                  # magnitude at (row + dx, col + dy) for the interior pixels
        return mag[1 + dx:h - 1 + dx, 1 + dy:w - 1 + dy]
    i, j, m = is_[c], js[c], mag[c]
    ai, aj = np.abs(i), np.abs(j)
    ok = m >= low                                    # the eroded mask only removes the one-pixel border, i.e. the interior
    up, down, left, right = i >= 0, i <= 0, j <= 0, j >= 0
    c1 = (up & right) | (down & left)
    c2 = ~c1 & ((down & right) | (up & left))
    with np.errstate(divide="ignore", invalid="ignore"):
        w_ji, w_ij = np.where(ai > 0, aj / ai, 0.0), np.where(aj > 0, ai / aj, 0.0)
    keep = np.zeros(m.shape, bool)

    def test(sel, wgt, n11, n12, n21, n22):
        plus = (n12 * wgt + n11 * (1.0 - wgt)) <= m
        minus = (n22 * wgt + n21 * (1.0 - wgt)) <= m
        keep[sel & plus & minus] = True
    a = c1 & (ai > aj)
    test(a, w_ji, sh(1, 0), sh(1, 1), sh(-1, 0), sh(-1, -1))
    test(c1 & ~a, w_ij, sh(0, 1), sh(1, 1), sh(0, -1), sh(-1, -1))
    b = c2 & (ai < aj)
    test(b, w_ij, sh(0, 1), sh(-1, 1), sh(0, -1), sh(1, -1))
    test(c2 & ~b, w_ji, sh(-1, 0), sh(-1, 1), sh(1, 0), sh(1, -1))
    out[c] = np.where(keep & ok, m, 0.0)
    return out


def obj_mask(image: Image.Image) -> Image.Image:
    gray = np.array(image.convert('L'))
    edges = _canny(gray, sigma=1.5, low=5, high=15)
    sq3, sq4 = np.ones((3, 3), int), np.ones((4, 4), int)
    m = ndimage.binary_dilation(edges, sq3)
    m = ndimage.binary_closing(m, sq3)
    m = ndimage.binary_fill_holes(m, sq3)
    m = ndimage.binary_erosion(m, sq4)
    lab, _ = ndimage.label(m, structure=np.ones((3, 3), int))      # skimage.morphology.label: full (8-) connectivity by default
    # no component at all: bincount = [0], argmax 0, `labels == 0` is everywhere true -- the reference's white mask
    sizes = np.bincount(lab.ravel(), weights=m.ravel().astype(np.float64))
    return Image.fromarray(lab == int(np.argmax(sizes))).convert('RGB')


# ---- polygon mask (dataset_generator.py:42-101) ----
def _side_points(side: int, w: int, h: int):
    """One or two points on a side of the w x h rectangle, drawn in the reference's order."""
    two = random.randint(1, 2) == 2
    hw, hh = int(w / 2), int(h / 2)
    if side == 0:      # left, walking upwards
        return [(0, random.randint(hh + 1, h)), (0, random.randint(1, hh))] if two else [(0, random.randint(1, h))]
    if side == 1:      # top, walking right
        return [(random.randint(1, hw), 0), (random.randint(hw + 1, w), 0)] if two else [(random.randint(1, w), 0)]
    if side == 2:      # right, walking down
        return [(w, random.randint(1, hh)), (w, random.randint(hh + 1, h))] if two else [(w, random.randint(1, h))]
    return [(random.randint(hw + 1, w), h), (random.randint(1, hw), h)] if two else [(random.randint(1, w), h)]


def polygon_points(size: Tuple[int, int], sides=4):
    """Vertex list of the irregular polygon inscribed in a ``size`` rectangle (4 or up to 8 vertices)."""
    w, h = size
    if sides == 4:
        return [(0, random.randint(1, h)), (random.randint(1, w), 0), (w, random.randint(1, h)), (random.randint(1, w), h)]
    pts = []
    for side in range(4):
        pts += _side_points(side, w, h)
    return pts


def rect2poly(patch: Image.Image, regular: bool = False, sides: list = 4):
    """RGBA mask (white polygon on transparent) of the patch's size."""
    w, h = patch.size
    mask = Image.new('RGBA', patch.size, color=(0, 0, 0, 0))
    draw = ImageDraw.Draw(mask)
    if regular:
        draw.regular_polygon(bounding_circle=((int(w / 2), int(h / 2)), int(min(w, h) / 2)),
                             n_sides=random.choice(sides), fill='white')
    else:
        draw.polygon(polygon_points((w, h), sides), fill='white')
    return mask


# ---- placement (dataset_generator.py:104-144) ----
def check_valid_coordinates_by_container(imsize: tuple, patchsize: tuple, current_coords: tuple = None,
                                         container_scaling_factor: int = 1):
    """Top-left paste corner for a patch centred at ``current_coords`` (random centre when None), pulled back
    inside the container on each side in the order right, bottom, left, top."""
    pw, ph = patchsize
    box = Container(imsize, scaling_factor=container_scaling_factor)
    if current_coords is None:
        cx, cy = random.randint(box.left, box.right), random.randint(box.top, box.bottom)
    else:
        cx, cy = current_coords[0], current_coords[1]
    left, top = cx - int(pw / 2), cy - int(ph / 2)
    right, bottom = cx + int(pw / 2), cy + int(ph / 2)
    if right > box.right:
        left = box.right - pw
    if bottom > box.bottom:
        top = box.bottom - ph
    if left < box.left:
        left = box.left
    if top < box.top:
        top = box.top
    return (left, top)


def check_color_similarity(patch: Image.Image, defect: Image.Image) -> float:
    """Cosine similarity of the two mean RGB colours (dataset_generator.py:147-159)."""
    a = np.array(patch).mean(axis=(0, 1))[:3] / 255.0
    b = np.array(defect).mean(axis=(0, 1))[:3] / 255.0
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


# ---- patch sampling (dataset_generator.py:164-210) ----
def sample_patch_box(imsize: Tuple[int, int], area_ratio, aspect_ratio):
    """(left, top, w, h) of the random rectangle: area ~ U(area_ratio) * image area, aspect from one of two ranges."""
    iw, ih = imsize
    area = random.uniform(area_ratio[0], area_ratio[1]) * (iw * ih)
    aspect = random.choice([random.uniform(*aspect_ratio[0]), random.uniform(*aspect_ratio[1])])
    pw, ph = max(int(np.sqrt(area * aspect)), 2), max(int(np.sqrt(area / aspect)), 2)
    left, top = random.randint(0, max(iw - pw, 1)), random.randint(0, max(ih - ph, 1))
    return left, top, pw, ph


def generate_patch(image: Image.Image, area_ratio: tuple = (0.02, 0.15), aspect_ratio: tuple = ((0.3, 1), (1, 3.3)),
                   augs=None, colorized: bool = False, color_type: str = 'random') -> Image.Image:
    left, top, pw, ph = sample_patch_box(image.size, area_ratio, aspect_ratio)
    box = (left, top, left + pw, top + ph)
    if not colorized:
        return image.crop(box)
    if color_type == 'random':
        rgb = (random.randint(0, 255), random.randint(0, 255), random.randint(0, 255))
    elif color_type == 'sample':
        rgb = random.choice(['black', 'white', 'silver', 'gray'])
    else:                                                  # 'average'
        mean = np.array(image.crop(box)).mean(axis=(0, 1))
        rgb = (int(mean[0]), int(mean[1]), int(mean[2]))
    return Image.new('RGB', (pw, ph), color=rgb)


def get_random_coordinate(xy_coords) -> Tuple[int, int]:
    if len(xy_coords) == 0:
        return None
    if len(xy_coords) < 2:
        return xy_coords[0]
    return xy_coords[random.randint(0, len(xy_coords) - 1)]


def paste_patch(image: Image.Image, patch: Image.Image, coords: tuple, mask: Image.Image = None):
    out = image.copy()
    out.paste(patch, (coords[0], coords[1]), mask=mask)
    return out


# ---- 'cable' pre-segmentation: SLIC super-pixels + per-segment mean colour (datasets.py:201-206) ----
# THIRD-PARTY RESTATEMENT, pinned: the reference calls skimage.segmentation.slic(image, n_segments=5, sigma=2,
# convert2lab=True) and skimage.color.label2rgb(segments, image, kind='avg'); scikit-image is not a dependency of this
# package, so its algorithm (Achanta et al., "SLIC Superpixels": Gaussian pre-smoothing, CIELAB, k-means in (L, a, b, y, x)
# restricted to 2S x 2S windows with compactness 10, 10 iterations, connectivity enforcement with min / max size factors
# 0.5 / 3) is written out here and reproduces scikit-image 0.18.3's label image bit for bit (tests/golden/skimage.npz,
# test_skimage_restatements_match_the_library).
def _rgb2lab(x):
    """skimage.color.rgb2lab of float RGB in [0, 1] (sRGB -> XYZ -> CIE-Lab, D65 / 2 degree observer) -- third-party, restated;
    pinned against scikit-image 0.18.3 (tests/golden/skimage.npz)."""
    x = np.asarray(x, dtype=np.float64)
    lin = x.copy()
    hi = x > 0.04045
    lin[hi] = np.power((x[hi] + 0.055) / 1.055, 2.4)
    lin[~hi] /= 12.92
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    xyz = lin @ m.T.copy()
    xyz = xyz / np.array([0.95047, 1.0, 1.08883])
    hi = xyz > 0.008856
    f = xyz.copy()
    f[hi] = np.cbrt(xyz[hi])
    f[~hi] = 7.787 * xyz[~hi] + 16.0 / 116.0
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    return np.concatenate([x_[..., np.newaxis] for x_ in [(116.0 * fy) - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)]], axis=-1)


def _regular_grid(shape, n_points):
    """skimage.util.regular_grid: (start, step) per axis of a grid of ~n_points points, as cubically spaced as the shape allows."""
    ar = np.asanyarray(shape)
    ndim = len(ar)
    unsort = np.argsort(np.argsort(ar))
    sd = np.sort(ar)
    space = float(np.prod(ar))
    if space <= n_points:
        return [(0, 1)] * ndim
    st = np.full(ndim, (space / n_points) ** (1.0 / ndim), dtype="float64")
    if (sd < st).any():
        for dim in range(ndim):
            st[dim] = sd[dim]
            space = float(np.prod(sd[dim + 1:]))
            st[dim + 1:] = (space / n_points) ** (1.0 / (ndim - dim - 1))
            if (sd >= st).all():
                break
    starts = (st // 2).astype(int)
    steps = np.round(st).astype(int)
    return [(int(starts[i]), int(steps[i])) for i in unsort]


def _slic_kmeans(image, segments, step, max_iter):
    """The k-means core of scikit-image's SLIC (_slic_cython, unit spacing, no mask) on a (H, W, C) float64 image whose
    colours are already divided by the compactness; `segments` = rows [y, x, c...].  Every centroid searches a window of
    +-2 grid steps -- the grid of the ACTUAL number of centroids, not of the requested one -- a pixel goes to the centroid
    with the smallest colour^2 + xy^2 / step^2 (strict improvement, centroids in order), centroids become the means of their
    pixels, until nothing changes or max_iter.  Returns labels from 0.  Bit-identical to the compiled function of 0.18.3."""
    h, w, nc = image.shape
    seg = np.array(segments, dtype=np.float64)
    n = seg.shape[0]
    spatial_weight = 1.0 / (step ** 2)
    (_, _), (_, wy), (_, wx) = _regular_grid((1, h, w), n)
    nearest = np.zeros((h, w), np.intp)
    ys = np.arange(h, dtype=np.float64)[:, None]
    xs = np.arange(w, dtype=np.float64)[None, :]
    yy, xx = np.mgrid[0:h, 0:w]
    fy, fx = yy.ravel().astype(np.float64), xx.ravel().astype(np.float64)
    for _ in range(max_iter):
        change = False
        dist = np.full((h, w), np.finfo(np.float64).max)
        for k in range(n):
            cy, cx = seg[k, 0], seg[k, 1]
            y0, y1 = int(max(cy - 2 * wy, 0)), int(min(cy + 2 * wy + 1, h))
            x0, x1 = int(max(cx - 2 * wx, 0)), int(min(cx + 2 * wx + 1, w))
            d = (0.0 + (cy - ys[y0:y1]) ** 2 + (cx - xs[:, x0:x1]) ** 2) * spatial_weight
            dc = np.zeros((y1 - y0, x1 - x0))
            for c in range(nc):
                dc = dc + (image[y0:y1, x0:x1, c] - seg[k, 2 + c]) ** 2
            d = d + dc
            sub = dist[y0:y1, x0:x1]
            better = sub > d
            if better.any():
                change = True
                sub[better] = d[better]
                nearest[y0:y1, x0:x1][better] = k
        if not change:
            break
        flat = nearest.ravel()
        cnt = np.bincount(flat, minlength=n).astype(np.float64)
        new = np.zeros_like(seg)
        new[:, 0] = np.bincount(flat, weights=fy, minlength=n)
        new[:, 1] = np.bincount(flat, weights=fx, minlength=n)
        for c in range(nc):
            new[:, 2 + c] = np.bincount(flat, weights=image[:, :, c].ravel(), minlength=n)
        with np.errstate(divide="ignore", invalid="ignore"):
            seg = new / cnt[:, None]
    return nearest


def _slic_connectivity(labels, min_size, max_size):
    """scikit-image's _enforce_label_connectivity_cython (2-D, labels from 0 -> from 1): components are found in raster order by
    a breadth-first search over the 4-neighbourhood (capped at max_size pixels); one smaller than min_size takes the label of
    the last already-relabelled neighbour the search met, every other one the next new label."""
    h, w = labels.shape
    out = np.zeros((h, w), dtype=np.intp)              # 0 = not yet relabelled
    cur = 1
    nbr = ((0, 1), (0, -1), (1, 0), (-1, 0))
    coord = np.empty((max(max_size, 1), 2), np.intp)
    for y in range(h):
        for x in range(w):
            if out[y, x] > 0:
                continue
            adjacent = 0
            lab = labels[y, x]
            out[y, x] = cur
            size, visited = 1, 0
            coord[0] = (y, x)
            while visited < size < max_size:
                for dy, dx in nbr:
                    yy, xx = coord[visited, 0] + dy, coord[visited, 1] + dx
                    if 0 <= xx < w and 0 <= yy < h:
                        if labels[yy, xx] == lab and out[yy, xx] == 0:
                            out[yy, xx] = cur
                            coord[size] = (yy, xx)
                            size += 1
                            if size >= max_size:
                                break
                        elif out[yy, xx] > 0 and out[yy, xx] != cur:
                            adjacent = out[yy, xx]
                visited += 1
            if size < min_size:
                for i in range(size):
                    out[coord[i, 0], coord[i, 1]] = adjacent
            else:
                cur += 1
    return out


def slic_superpixels(image_array, n_segments=5, sigma=2, compactness=10.0, max_num_iter=10, rescale=True):
    """skimage.segmentation.slic(image, n_segments, sigma=sigma, convert2lab=True) for an H x W x 3 uint8 array: labels from 1.
    THIRD-PARTY RESTATEMENT (scikit-image is not a dependency of this package).  Pinned: Lab conversion, Gaussian pre-filter, grid
    seeding, the k-means core and the connectivity pass reproduce scikit-image 0.18.3 bit for bit (tests/golden/skimage.npz,
    generated with the real library by tests/golden/make_skimage_fixtures.py).  `rescale` selects the wrapper's pre-processing:
    True (default) = releases >= 0.19, which stretch the float image to [0, 1] by its min / max before the Lab conversion and
    number labels from 1 -- the releases the reference must have run (datasets.py:204-205 hands label2rgb's result to
    Image.fromarray, which only the dtype-preserving label2rgb of 0.19+ survives); False = 0.18 (uint8 / 255 only)."""
    h, w = image_array.shape[:2]
    img = np.asarray(image_array, dtype=np.float64) / 255.0
    if rescale:
        imin, imax = img.min(), img.max()
        img = img - imin
        if imax != imin:
            img = img / (imax - imin)
    lab = _rgb2lab(img)[np.newaxis]                                       # (1, H, W, 3), as the library lays it out
    (z0, zs), (y0, ystep), (x0, xstep) = _regular_grid((1, h, w), n_segments)
    gy, gx = np.arange(y0, h, ystep), np.arange(x0, w, xstep)
    cy, cx = [a.ravel() for a in np.meshgrid(gy, gx, indexing="ij")]
    lab = ndimage.gaussian_filter(lab, [sigma, sigma, sigma, 0])          # 'reflect' borders, 4 sigma
    segments = np.concatenate([cy[:, None], cx[:, None], np.zeros((len(cy), 3))], axis=-1).astype(np.float64)
    step = float(max(zs, ystep, xstep))
    lab = np.ascontiguousarray(lab[0] * (1.0 / compactness))
    labels = _slic_kmeans(lab, segments, step, max_num_iter)
    segment_size = h * w / float(len(cy))
    return _slic_connectivity(labels, int(0.5 * segment_size), int(3 * segment_size))


def label_mean_rgb(segments, image_array):
    """skimage.color.label2rgb(segments, image, kind='avg') of releases >= 0.19: every pixel takes the mean colour of its
    segment, written into an array of the IMAGE's dtype (float64 mean -> uint8 by truncation); label 0 would be background."""
    out = np.zeros_like(image_array)
    for s in np.unique(segments):
        if s == 0:
            continue
        msk = (segments == s).nonzero()
        out[msk] = image_array[msk].mean(axis=0)
    return out


_SLIC_MEMO = {}


def slic_superpixels_cached(image_array, n_segments=5, sigma=2, **kw):
    """slic_superpixels with a memo: the labels of an image are a pure function of its pixels and the parameters, and the one caller
    (the 'cable' pre-segmentation, datasets.py:201-206 of the reference) asks for the same first training image at every dataset
    construction -- train, validation and every later run.  In-process dictionary, then a file under SSAD_CACHE_DIR (default
    ~/.cache/ssad; SSAD_CACHE_DIR="" switches the files off) named by the SHA-1 of the pixels, the shape and the parameters: the
    host k-means (0.1-0.3 s) then runs once per image ever, not once per construction."""
    import hashlib
    import os
    arr = np.ascontiguousarray(image_array)
    key = hashlib.sha1(arr.tobytes() + repr((arr.shape, str(arr.dtype), n_segments, sigma, sorted(kw.items()))).encode()).hexdigest()
    if key in _SLIC_MEMO:
        return _SLIC_MEMO[key].copy()
    root = os.environ.get("SSAD_CACHE_DIR", os.path.join(os.path.expanduser("~"), ".cache", "ssad"))
    path = os.path.join(root, f"slic_{key}.npy") if root else None
    labels = None
    if path and os.path.exists(path):
        try:
            labels = np.load(path)
            if labels.shape != arr.shape[:2]:
                labels = None
        except Exception:          # noqa: BLE001  (a truncated cache file is recomputed, never trusted)
            labels = None
    if labels is None:
        labels = slic_superpixels(arr, n_segments=n_segments, sigma=sigma, **kw)
        if path:
            try:
                os.makedirs(root, exist_ok=True)
                tmp = f"{path}.{os.getpid()}.tmp"
                with open(tmp, "wb") as f:
                    np.save(f, labels)
                os.replace(tmp, path)          # atomic: concurrent ranks either see the whole file or none
            except OSError:
                pass
    _SLIC_MEMO[key] = labels
    return labels.copy()
