"""Gaussian density estimator (GDE) anomaly scorer of CutPaste (Li et al., CVPR 2021, §3.3), on HIP kernels.

A Gaussian with Ledoit-Wolf shrinkage is fitted to the normal embeddings; the anomaly score is the Mahalanobis distance to it.
The reference repository has no such scorer (it only has the cosine 3-NN of ``AnomalyDetector``), so there is no reference
vector: the yardstick is sklearn.covariance.LedoitWolf(assume_centered=False) + scipy.spatial.distance.mahalanobis in float64.

Split of the work: the O(N D^2) statistics (mean, centred scatter matrix, sum of ||x - mean||^4) and the O(N D^2) scoring run on
the GPU (csrc/gde.hip); the one-off D x D shrinkage, Cholesky factor and its triangular inverse run here in float64.

``normalize=True`` (the default) scores L2-normalised embeddings: the view of the embedding the cosine detector has, and what the
common PyTorch re-implementations of CutPaste feed their GDE.  The rows are normalised on the GPU bit-identically to
``ops.l2_normalize_rows``.
"""
import numpy as np
import torch
from scipy.linalg import solve_triangular
from torch import Tensor

from . import ops


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


class GaussianDensityDetector:
    """Opt-in second scorer with the call surface of ``models.AnomalyDetector``: a Ledoit-Wolf Gaussian fitted to the normal
    embeddings, the Mahalanobis distance to it as the score (CutPaste's GDE).

    ``fit`` takes the same 70/30 split as ``AnomalyDetector.fit`` (models.split_indices: the same draws from the global numpy RNG,
    quirk Q5), fits on the train part and sets ``threshold`` to the largest score of the held-out part.  Fitting needs at least
    2 rows: the image-level bank of ``tools.inference`` is ONE embedding (quirk Q3), so image-level GDE raises ValueError."""

    def __init__(self, patch_level: bool = False, batch: int = None, num_patches: int = None, normalize: bool = True) -> None:
        self.patch_level = patch_level
        self.batch = batch
        self.dim = int(np.sqrt(num_patches)) if num_patches else None
        self.normalize = bool(normalize)
        self.mu_hi = self.mu_lo = self.w = None
        self.shrinkage = None
        self.threshold = None

    @staticmethod
    def _dev(t):
        t = torch.as_tensor(t, dtype=torch.float32)
        if not t.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("GaussianDensityDetector needs the MI355X HIP kernels (no CPU fallback)")
            t = t.cuda()
        return t.contiguous()

    @staticmethod
    def fit_rows(n: int, split: bool = True) -> int:
        """Rows a fit on n embeddings uses (the train part of the 70/30 split); ValueError when fewer than 2."""
        m = n - int(np.ceil(0.3 * n)) if split else n
        if m < 2:
            raise ValueError(f"GaussianDensityDetector needs at least 2 fit rows, got {m} (from {n} embeddings"
                             f"{', 70/30 split' if split else ''}); the image-level bank of tools.inference is one embedding")
        return m

    def fit(self, embeddings: Tensor, split: bool = True, groups=None) -> None:
        """groups: image index per row -- the 70/30 split is then drawn over images (models.split_rows)."""
        from .models import _take, split_rows
        emb = torch.as_tensor(embeddings)
        n = emb.shape[0]
        if groups is None:
            self.fit_rows(n, split)
        if split:
            train_idx, val_idx = split_rows(n, groups, 0.3)
            train, val = _take(emb, train_idx), _take(emb, val_idx)
        else:
            train, val = emb, emb
        self.fit_bank(train)
        self.threshold = torch.max(self._scores(self._dev(val))).item()

    def fit_bank(self, bank: Tensor) -> None:
        n = int(torch.as_tensor(bank).shape[0])
        self.fit_rows(n, split=False)
        x = self._dev(bank)
        mean, scatter, m4 = ops.gaussian_fit_stats(x, self.normalize)
        mu_hi, mu_lo, w, self.shrinkage = ledoit_wolf_factor(mean.cpu().numpy(), scatter.cpu().numpy(), m4.item(), n)
        self.mu_hi, self.mu_lo, self.w = (torch.from_numpy(a).to(x.device) for a in (mu_hi, mu_lo, w))

    def _scores(self, x):
        return ops.mahalanobis_fused(x, self.mu_hi, self.mu_lo, self.w, self.normalize)

    def predict(self, x: Tensor) -> Tensor:
        anomaly_scores = self._scores(self._dev(x))
        if self.patch_level:
            anomaly_scores = torch.reshape(anomaly_scores, (self.batch, 1, self.dim, self.dim))
        return anomaly_scores

    def state(self) -> dict:
        """What another rank needs to score (host tensors, picklable); the threshold travels beside it."""
        return {"mu_hi": self.mu_hi.cpu(), "mu_lo": self.mu_lo.cpu(), "w": self.w.cpu(), "shrinkage": self.shrinkage,
                "normalize": self.normalize}

    @classmethod
    def from_state(cls, state: dict, patch_level: bool = False, batch: int = None, num_patches: int = None):
        det = cls(patch_level=patch_level, batch=batch, num_patches=num_patches, normalize=state["normalize"])
        det.mu_hi, det.mu_lo, det.w = (cls._dev(state[k]) for k in ("mu_hi", "mu_lo", "w"))
        det.shrinkage = state["shrinkage"]
        return det
