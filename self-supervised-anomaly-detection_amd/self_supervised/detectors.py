"""What the anomaly detectors share: the 70/30 split, and the base classes of ``models.AnomalyDetector`` (cosine / Euclidean kNN),
``density.GaussianDensityDetector`` (GDE) and ``density.PositionGaussianDetector`` (PaDiM).  ``models.DETECTORS`` names the three."""
import numpy as np
import torch
from torch import Tensor

from . import ops


def split_indices(n, test_size=0.3):
    """Index form of sklearn.model_selection.train_test_split(test_size=..., random_state=None, shuffle=True):
    n_test = ceil(test_size*n); one permutation from the global numpy RNG; test = its first n_test entries,
    train = the rest (quirk Q5: unseeded in the reference)."""
    n_test = int(np.ceil(test_size * n))
    perm = np.random.permutation(n)
    return perm[n_test:], perm[:n_test]


def split_rows(n, groups=None, test_size=0.3):
    """(train, held-out) row indices of the detectors' 70/30 split.  groups=None: split_indices(n) over the rows.  groups [n] (the
    image index 0..G-1 of every row): the split is drawn over the IMAGES -- split_indices(G), one permutation from the global numpy
    RNG -- and every row goes with its image, images in the permutation's order, rows ascending within an image.  (A row split would
    put overlapping patches of one image on both sides and drive the threshold towards 0.)"""
    if groups is None:
        return split_indices(n, test_size)
    g = np.asarray(torch.as_tensor(groups).cpu()).reshape(-1).astype(np.int64)
    if g.shape[0] != n:
        raise ValueError(f"groups has {g.shape[0]} entries for {n} rows")
    order = np.argsort(g, kind="stable")
    n_groups = int(g.max()) + 1 if n else 0
    bounds = np.searchsorted(g[order], np.arange(n_groups + 1))
    tr, va = split_indices(n_groups, test_size)
    take = lambda ids: (np.concatenate([order[bounds[i]:bounds[i + 1]] for i in ids]) if len(ids) else np.zeros(0, np.int64))
    return take(tr), take(va)


def _take(t, idx):
    return t[torch.as_tensor(idx, dtype=torch.int64, device=t.device)]


class Detector:
    """What tools.inference calls, whichever detector it built.  A subclass supplies ``fit_bank(bank)``, ``_scores(x)`` (x on the device)
    and ``state()`` / ``load_state(state)``: a picklable dict that carries everything scoring reads, so that a detector of the same
    constructor arguments that loads it returns the fitted one's bits (the threshold travels beside it)."""

    def __init__(self, patch_level: bool = False, batch: int = None, num_patches: int = None) -> None:
        self.patch_level = patch_level
        self.batch = batch
        self.dim = int(np.sqrt(num_patches)) if num_patches else None      # the side of a map
        self.threshold = None

    @classmethod
    def _dev(cls, t):
        t = torch.as_tensor(t, dtype=torch.float32)
        if not t.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError(f"{cls.__name__} needs the MI355X HIP kernels (no CPU fallback)")
            t = t.cuda()
        return t.contiguous()

    def check_fit_size(self, rows: int, n_images, width: int) -> None:
        """ValueError when a fit on `rows` x `width` embeddings (of `n_images` images, None for a row split) cannot work; sizes alone."""

    def _check_fit(self, emb, split, groups):
        """``fit``'s refusals, before the split is drawn; returns the groups it is drawn over."""
        return groups

    def _after_bank(self, train) -> None:
        """Between ``fit_bank`` and the threshold.  train: the rows ``fit_bank`` was given."""

    def fit(self, embeddings: Tensor, split: bool = True, groups=None) -> None:
        """Fits on 70 % of the rows, `threshold` = the largest score of the other 30 % (split=False: both on every row).  groups: image
        index per row -- the split is then drawn over images (split_rows): one draw from numpy's global generator, after ``_check_fit``."""
        train = val = emb = torch.as_tensor(embeddings)
        groups = self._check_fit(emb, split, groups)
        if split:
            train_idx, val_idx = split_rows(int(emb.shape[0]), groups, 0.3)
            train, val = _take(emb, train_idx), _take(emb, val_idx)
        self.fit_bank(train)
        self._after_bank(train)
        self.threshold = torch.max(self._scores(self._dev(val))).item()

    def predict(self, x: Tensor) -> Tensor:
        anomaly_scores = self._scores(self._dev(x))
        if self.patch_level:            # (batch=None: PaDiM counts the images itself)
            batch = self._images(anomaly_scores.shape[0]) if self.batch is None else self.batch
            anomaly_scores = torch.reshape(anomaly_scores, (batch, 1, self.dim, self.dim))
        return anomaly_scores

    def describe_fit(self):
        """A line about the last ``fit`` for the log, or None."""

    def image_scores(self, x: Tensor, mode: str = 'max', neighbours: int = 9, scores: Tensor = None) -> Tensor:
        """One score per image, for the detectors with ``_check_image_scores`` and ``_image_patches`` (kNN, PaDiM).  x [batch * P][D],
        image after image; `scores`: the map predict returned, when the caller has it; p* = the largest patch score's index, the smallest
        on ties.  'max': s_{p*}; any other mode the subclass accepts: its ``_reweight`` of s_{p*}.  Returns [batch]."""
        self._check_image_scores(mode, neighbours)
        x = self._dev(x)
        p = self._image_patches(int(x.shape[0]))
        s = self._scores(x) if scores is None else self._dev(scores)
        smax, flat = ops.rows_argmax(s.reshape(x.shape[0] // p, p))
        if mode == 'max':
            return smax
        return self._reweight(x.index_select(0, flat), smax, neighbours)           # x_{p*} of every image
