"""Gaussian density estimator (GDE) anomaly scorer of CutPaste (Li et al., CVPR 2021, §3.3), on HIP kernels.

A Gaussian with Ledoit-Wolf shrinkage is fitted to the normal embeddings; the anomaly score is the Mahalanobis distance to it.
The reference repository has no such scorer (it only has the cosine 3-NN of ``AnomalyDetector``), so there is no reference
vector: the yardstick is sklearn.covariance.LedoitWolf(assume_centered=False) + scipy.spatial.distance.mahalanobis in float64.

Split of the work: the O(N D^2) statistics (mean, centred scatter matrix, sum of ||x - mean||^4) and the O(N D^2) scoring run on
the GPU (csrc/gde.hip); the one-off D x D shrinkage, Cholesky factor and its triangular inverse run here in float64.

``normalize=True`` (the default) scores L2-normalised embeddings: the view of the embedding the cosine detector has, and what the
common PyTorch re-implementations of CutPaste feed their GDE.  The rows are normalised on the GPU bit-identically to
``ops.l2_normalize_rows``.

``PositionGaussianDetector`` (below) is the per-position form for dense localisation (PaDiM): one Gaussian per map position over a
random choice of columns, fitted over the training images (csrc/padim.hip); its yardstick is numpy.cov + eps I and scipy's
mahalanobis in float64.
"""
import numpy as np
import torch
from scipy.linalg import solve_triangular
from torch import Tensor

from . import ops
from .detectors import Detector


def ledoit_wolf_covariance(mean, scatter, m4, n):
    """Ledoit-Wolf shrunk covariance from centred sufficient statistics: (shrunk [p][p] float64, shrinkage).

    Restates sklearn/covariance/_shrunk_covariance.py (scikit-learn 1.x): ``ledoit_wolf_shrinkage(X - X.mean(0),
    assume_centered=True)`` and ``_ledoit_wolf`` as used by ``LedoitWolf(assume_centered=False).fit``, with its sums over X
    replaced by the statistics of ``ops.gaussian_fit_stats``:
      emp_cov = scatter / n;  mu = trace(emp_cov) / p
      delta_  = sum(scatter ** 2) / n^2                 (sum of the squared coefficients of X^T X, / n^2)
      beta_   = m4                                      (sum(X2.T @ X2) = sum_i ||x_i||^4 of the centred rows)
      beta    = (beta_ / n - delta_) / (p n);  delta = (delta_ - 2 mu trace(emp_cov) + p mu^2) / p
      shrinkage = min(beta, delta) / delta  (0 when min(beta, delta) == 0)
      shrunk  = (1 - shrinkage) emp_cov + shrinkage mu I"""
    mean = np.asarray(mean, dtype=np.float64)
    scatter = np.asarray(scatter, dtype=np.float64)
    n = int(n)
    p = mean.shape[0]
    if n < 2:
        raise ValueError(f"a Gaussian fit needs at least 2 rows, got {n}")
    emp_cov = scatter / n
    trace = np.trace(emp_cov)
    mu = trace / p
    delta_ = np.sum(scatter ** 2) / n ** 2
    beta = 1.0 / (p * n) * (float(m4) / n - delta_)
    delta = (delta_ - 2.0 * mu * trace + p * mu ** 2) / p
    beta = min(beta, delta)
    shrinkage = 0.0 if beta == 0 else beta / delta
    shrunk = (1.0 - shrinkage) * emp_cov
    shrunk.flat[:: p + 1] += shrinkage * mu
    return shrunk, float(shrinkage)


def ledoit_wolf_factor(mean, scatter, m4, n):
    """The Ledoit-Wolf Gaussian of ``ledoit_wolf_covariance`` in the form the scoring kernel takes.

    C = cholesky(shrunk) (lower) and W = C^-1 (triangular solve), so that W^T W = shrunk^-1 and ||W (x - mean)|| is the
    Mahalanobis distance.  Returns (mu_hi, mu_lo, W, shrinkage): the mean as a pair of float32 vectors (mu_hi = fp32(mean),
    mu_lo = fp32(mean - mu_hi)), W as float32 [p][p] lower triangular, the shrinkage as a float.

    ValueError when the shrunk covariance is singular: always at n = 2 (sklearn's beta is then exactly 0 -- the two centred rows
    are c and -c -- so the shrinkage is 0 and the estimate has rank 1), and when every fit row is the same."""
    shrunk, shrinkage = ledoit_wolf_covariance(mean, scatter, m4, n)
    try:
        c = np.linalg.cholesky(shrunk)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"the Ledoit-Wolf covariance of {int(n)} rows is singular (shrinkage {shrinkage:g}): no Mahalanobis "
                         "distance exists; fit on more (and distinct) rows") from e
    mean = np.asarray(mean, dtype=np.float64)
    p = mean.shape[0]
    w = solve_triangular(c, np.eye(p), lower=True)
    mu_hi = mean.astype(np.float32)
    mu_lo = (mean - mu_hi.astype(np.float64)).astype(np.float32)
    return mu_hi, mu_lo, np.ascontiguousarray(w, dtype=np.float32), shrinkage


class GaussianDensityDetector(Detector):
    """Opt-in second scorer with the call surface of ``models.AnomalyDetector``: a Ledoit-Wolf Gaussian fitted to the normal
    embeddings, the Mahalanobis distance to it as the score (CutPaste's GDE).

    ``fit`` takes the same 70/30 split as ``AnomalyDetector.fit`` (detectors.split_indices: the same draws from the global numpy RNG,
    quirk Q5), fits on the train part and sets ``threshold`` to the largest score of the held-out part.  Fitting needs at least
    2 rows: the image-level bank of ``tools.inference`` is ONE embedding (quirk Q3), so image-level GDE raises ValueError."""

    def __init__(self, patch_level: bool = False, batch: int = None, num_patches: int = None, normalize: bool = True) -> None:
        super().__init__(patch_level, batch, num_patches)
        self.normalize = bool(normalize)
        self.mu_hi = self.mu_lo = self.w = None
        self.shrinkage = None

    @staticmethod
    def fit_rows(n: int, split: bool = True) -> int:
        """Rows a fit on n embeddings uses (the train part of the 70/30 split); ValueError when fewer than 2."""
        m = n - int(np.ceil(0.3 * n)) if split else n
        if m < 2:
            raise ValueError(f"GaussianDensityDetector needs at least 2 fit rows, got {m} (from {n} embeddings"
                             f"{', 70/30 split' if split else ''}); the image-level bank of tools.inference is one embedding")
        return m

    def check_fit_size(self, rows: int, n_images, width: int) -> None:
        if n_images is not None:        # the rows of the images the 70/30 split keeps
            rows = (n_images - int(np.ceil(0.3 * n_images))) * (rows // max(1, n_images))
        self.fit_rows(rows, split=n_images is None)

    def _check_fit(self, emb, split, groups):
        if groups is None:
            self.fit_rows(int(emb.shape[0]), split)
        return groups

    def fit_bank(self, bank: Tensor) -> None:
        n = int(torch.as_tensor(bank).shape[0])
        self.fit_rows(n, split=False)
        x = self._dev(bank)
        mean, scatter, m4 = ops.gaussian_fit_stats(x, self.normalize)
        mu_hi, mu_lo, w, self.shrinkage = ledoit_wolf_factor(mean.cpu().numpy(), scatter.cpu().numpy(), m4.item(), n)
        self.mu_hi, self.mu_lo, self.w = (torch.from_numpy(a).to(x.device) for a in (mu_hi, mu_lo, w))

    def _scores(self, x):
        return ops.mahalanobis_fused(x, self.mu_hi, self.mu_lo, self.w, self.normalize)

    def state(self) -> dict:
        return {"mu_hi": self.mu_hi.cpu(), "mu_lo": self.mu_lo.cpu(), "w": self.w.cpu(), "shrinkage": self.shrinkage,
                "normalize": self.normalize}

    def load_state(self, state: dict) -> None:
        self.mu_hi, self.mu_lo, self.w = (self._dev(state[k]) for k in ("mu_hi", "mu_lo", "w"))
        self.shrinkage, self.normalize = state["shrinkage"], state["normalize"]

    @classmethod
    def from_state(cls, state: dict, patch_level: bool = False, batch: int = None, num_patches: int = None):
        det = cls(patch_level=patch_level, batch=batch, num_patches=num_patches, normalize=state["normalize"])
        det.load_state(state)
        return det


# ------------------------------------------------------------------------------------------------ per-position Gaussian (PaDiM)

def position_channels(D: int, d: int, seed: int = 0):
    """The `d` of `D` columns the per-position Gaussian keeps (PaDiM's random dimension reduction): ``randperm(D)[:d]`` on a CPU
    torch.Generator of its own seeded with `seed`, sorted ascending, int64; d == D = every column, no draw.  Never draws from the
    global torch, numpy or `random` generators (as models.coreset_projection).  ValueError unless d % 32 == 0 and 32 <= d <= D."""
    if isinstance(d, (bool, np.bool_)) or not isinstance(d, (int, np.integer)) or d % 32 or not 32 <= d <= D:
        raise ValueError(f"channels must be a multiple of 32 in 32..{int(D)} (the rows' width), got {d!r}")
    if d == D:
        return torch.arange(D, dtype=torch.int64)
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randperm(int(D), generator=g)[:int(d)].sort().values


def position_gaussian_factor(mean, scatter, n, eps=0.01, chunk=64, dtype=np.float32):
    """The per-position Gaussians in the form the scoring kernel takes, from the statistics of ``ops.position_gaussian_fit_stats``:
    Sigma_p = scatter_p / (n - 1) + eps I (numpy.cov plus PaDiM's regulariser), C_p = cholesky(Sigma_p) (lower), W_p = C_p^-1
    (batched triangular solve), all in float64 on the host, `chunk` positions at a time.  Returns (mu_hi [P][d], mu_lo [P][d],
    W [P][d][d]) float32: the mean as the pair fp32(mean), fp32(mean - mu_hi) of ``ledoit_wolf_factor``, W lower triangular with
    exact zeros above the diagonal (dtype=np.float64: W before that rounding, for checks).  ValueError for n < 2 or eps <= 0 (with eps > 0 every Sigma_p is positive definite)."""
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    scatter = np.ascontiguousarray(scatter, dtype=np.float64)
    n = int(n)
    if n < 2:
        raise ValueError(f"a per-position Gaussian needs at least 2 fit images, got {n}")
    if not eps > 0:
        raise ValueError(f"eps must be positive (it keeps every covariance positive definite), got {eps!r}")
    P, d = mean.shape
    if scatter.shape != (P, d, d):
        raise ValueError(f"scatter is {scatter.shape}, expected {(P, d, d)}")
    w = np.empty((P, d, d), dtype=dtype)
    eye = torch.eye(d, dtype=torch.float64)
    for a in range(0, P, chunk):
        sigma = scatter[a:a + chunk] / (n - 1)
        sigma[:, np.arange(d), np.arange(d)] += eps
        try:
            c = np.linalg.cholesky(sigma)
        except np.linalg.LinAlgError as e:      # (not reachable with finite statistics and eps > 0)
            raise ValueError(f"a covariance of positions {a}..{min(P, a + chunk) - 1} is not positive definite") from e
        wc = torch.linalg.solve_triangular(torch.from_numpy(c), eye.expand(c.shape[0], d, d), upper=False)
        w[a:a + chunk] = np.tril(wc.numpy())
    mu_hi = mean.astype(np.float32)
    mu_lo = (mean - mu_hi.astype(np.float64)).astype(np.float32)
    return mu_hi, mu_lo, w


class PositionGaussianDetector(Detector):
    """Opt-in third scorer (PaDiM, Defard et al., ICPR 2020, as anomalib implements it) with ``GaussianDensityDetector``'s call
    surface, for rows that are whole images of `num_patches` positions in (image, position) order (the dense rows of
    ``PeraNet.enable_dense_mode``): one Gaussian per position over `channels` randomly chosen columns (``position_channels``),
    fitted over the images, the Mahalanobis distance to it as the pixel score.  Rows are not L2-normalised.

    ``fit`` draws the 70/30 split over images (detectors.split_rows; `groups` given or implied by the row order), fits on the 70 % and
    sets ``threshold`` to the largest score of the held-out images.  Patch level only, at least 2 fit images.

    ``factor``: where the P covariances are factored.  'host' (the default): ``position_gaussian_factor`` on copies of the statistics;
    'device': ``ops.position_gaussian_factor``, a batched fp64 Cholesky + triangular inverse kernel on the statistics where they are
    (channels <= 512) -- the fit never leaves the device.

    ``preselected=True``: the rows already hold the chosen columns and nothing else (the stage pyramid of
    ``PeraNet.enable_dense_mode(features='pyramid', columns=position_channels(width, channels, seed))`` writes only those): their
    width must equal `channels`, the kernels get the identity selection and read contiguous rows.  ``width`` (required then) is the
    number of columns the selection was drawn from; ``sel`` in ``state()`` still records ``position_channels(width, channels, seed)``,
    so a saved fit says which columns of the full rows it means."""

    FACTORS = ('host', 'device')

    def __init__(self, patch_level: bool = True, batch: int = None, num_patches: int = None, channels: int = 96, eps: float = 0.01,
                 seed: int = 0, factor: str = 'host', preselected: bool = False, width: int = None) -> None:
        if not patch_level or not num_patches:
            raise ValueError("PositionGaussianDetector is a patch-level detector: patch_level=True and num_patches (positions per "
                             "image) are required")
        if isinstance(channels, (bool, np.bool_)) or not isinstance(channels, (int, np.integer)) or channels % 32 or channels < 32:
            raise ValueError(f"channels must be a multiple of 32, at least 32, got {channels!r}")
        if not eps > 0:
            raise ValueError(f"eps must be positive, got {eps!r}")
        if not isinstance(factor, str) or factor not in self.FACTORS:
            raise ValueError(f"factor must be one of {self.FACTORS}, got {factor!r}")
        if factor == 'device' and channels > 512:
            raise ValueError(f"factor='device' takes at most 512 channels, got {channels}")
        if not isinstance(preselected, (bool, np.bool_)):
            raise ValueError(f"preselected must be a bool, got {preselected!r}")
        if preselected:
            if isinstance(width, (bool, np.bool_)) or not isinstance(width, (int, np.integer)):
                raise ValueError(f"preselected=True needs width, the number of columns the selection was drawn from, got {width!r}")
            position_channels(int(width), channels, seed)       # channels <= width
        elif width is not None:
            raise ValueError("width belongs to preselected=True (otherwise the rows' own width is the one the selection is drawn from)")
        super().__init__(True, batch, num_patches)
        self.factor = factor
        self.preselected, self.width = bool(preselected), None if width is None else int(width)
        self.num_patches = int(num_patches)
        self.channels, self.eps, self.seed = int(channels), float(eps), int(seed)
        self.sel = self.mu_hi = self.mu_lo = self.w = None
        self._sel_dev = None

    @staticmethod
    def fit_images(n_img: int, split: bool = True) -> int:
        """Images a fit on n_img images uses (the train part of the 70/30 split); ValueError when fewer than 2."""
        m = n_img - int(np.ceil(0.3 * n_img)) if split else n_img
        if m < 2:
            raise ValueError(f"PositionGaussianDetector needs at least 2 fit images, got {m} (from {n_img} images"
                             f"{', 70/30 split' if split else ''}): one image gives no covariance")
        return m

    def _images(self, rows: int) -> int:
        if rows == 0 or rows % self.num_patches:
            raise ValueError(f"{rows} rows are not whole images of {self.num_patches} positions")
        return rows // self.num_patches

    def check_fit_size(self, rows: int, n_images, width: int) -> None:
        self.fit_images(self._images(rows) if n_images is None else n_images)      # the images the 70/30 split keeps
        self._check_width(width)
        if self.channels > width:
            raise ValueError(f"channels must be a multiple of 32 in 32..{width} (the rows' width), got {self.channels}")

    def _check_width(self, width: int) -> None:
        if self.preselected and int(width) != self.channels:
            raise ValueError(f"preselected=True: the rows must hold the {self.channels} chosen columns and nothing else, got {int(width)} "
                             f"columns")

    def _selection(self, width: int):
        """(sel recorded in the state, sel the kernels index the rows with)."""
        if self.preselected:
            self._check_width(width)
            return position_channels(self.width, self.channels, self.seed), torch.arange(self.channels, dtype=torch.int64)
        sel = position_channels(int(width), self.channels, self.seed)
        return sel, sel

    def _check_fit(self, emb, split, groups):
        """groups: image index per row (default: implied by the row order, `num_patches` rows per image)."""
        n_img = self._images(int(emb.shape[0]))
        self._selection(int(emb.shape[1]))
        self.fit_images(n_img, split)
        if not split:
            return groups
        if groups is None:
            return torch.arange(n_img).repeat_interleave(self.num_patches)
        g = torch.as_tensor(groups).cpu().reshape(-1).long()
        if g.numel() != emb.shape[0] or not torch.equal(torch.bincount(g, minlength=n_img), torch.full((n_img,), self.num_patches)):
            raise ValueError(f"groups must give every one of the {n_img} images {self.num_patches} rows")
        return groups

    def fit_bank(self, bank: Tensor) -> None:
        bank = torch.as_tensor(bank)
        n_img = self._images(int(bank.shape[0]))
        sel, ksel = self._selection(int(bank.shape[1]))
        self.fit_images(n_img, split=False)
        x = self._dev(bank)
        sel_dev = ops.position_sel(ksel, x.shape[1], x.device)
        mean, scatter = ops.position_gaussian_fit_stats(x, ksel, n_img, self.num_patches, sel_dev=sel_dev)
        if self.factor == 'device':
            fitted = ops.position_gaussian_factor(mean, scatter, n_img, self.eps)       # consumes scatter; nothing visits the host
        else:
            fitted = position_gaussian_factor(mean.cpu().numpy(), scatter.cpu().numpy(), n_img, self.eps)
            fitted = [torch.from_numpy(a).to(x.device) for a in fitted]
        self.sel, self._sel_dev = sel, sel_dev
        self.mu_hi, self.mu_lo, self.w = fitted

    def _scores(self, x):
        if self.w is None:
            raise ValueError("PositionGaussianDetector: not fitted (fit or fit_bank first)")
        n_img = self._images(int(x.shape[0]))
        self._check_width(int(x.shape[1]))
        if not self.preselected and int(self.sel.max()) >= x.shape[1]:
            raise ValueError(f"the rows have {x.shape[1]} columns, the fitted selection reaches column {int(self.sel.max())}")
        return ops.position_mahalanobis(x, self.sel, self.mu_hi, self.mu_lo, self.w, n_img, self.num_patches, sel_dev=self._sel_dev)

    def _check_image_scores(self, mode, neighbours) -> None:
        if mode != 'max':               # (`neighbours` belongs to 'reweighted': accepted for AnomalyDetector's call surface only)
            raise ValueError(f"PositionGaussianDetector.image_scores: mode must be 'max' (a Gaussian patch score has no nearest bank "
                             f"row to reweight with), got {mode!r}")

    def _image_patches(self, rows: int) -> int:
        return self._images(rows) and self.num_patches

    def state(self) -> dict:
        return {"sel": self.sel.cpu(), "mu_hi": self.mu_hi.cpu(), "mu_lo": self.mu_lo.cpu(), "w": self.w.cpu(), "eps": self.eps,
                "channels": self.channels, "seed": self.seed, "factor": self.factor, "preselected": self.preselected,
                "width": self.width}

    def load_state(self, state: dict) -> None:
        self.mu_hi, self.mu_lo, self.w = (self._dev(state[k]) for k in ("mu_hi", "mu_lo", "w"))
        self.sel = torch.as_tensor(state["sel"]).cpu().long()
        self.preselected, self.width = bool(state.get("preselected", False)), state.get("width")
        ksel = torch.arange(self.sel.numel(), dtype=torch.int64) if self.preselected else self.sel
        self._sel_dev = ops.position_sel(ksel, int(ksel.max()) + 1, self.mu_hi.device)

    @classmethod
    def from_state(cls, state: dict, patch_level: bool = True, batch: int = None, num_patches: int = None):
        det = cls(patch_level=patch_level, batch=batch, num_patches=num_patches, channels=state["channels"], eps=state["eps"],
                  seed=state.get("seed", 0), factor=state.get("factor", "host"), preselected=state.get("preselected", False),
                  width=state.get("width"))
        det.load_state(state)
        return det
