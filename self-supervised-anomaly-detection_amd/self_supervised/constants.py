"""Containers and category lists (mirrors src/self_supervised/constants.py:7-118 of the reference)."""
from __future__ import annotations

import torch
from torch import Tensor

_FIELDS = ("original_data", "tensor_data", "y_true_binary_labels", "raw_predictions", "y_hat",
           "y_true_multiclass_labels", "ground_truths", "anomaly_maps", "embedding_vectors")
_OPTIONAL_IN_CAT = ("ground_truths", "anomaly_maps")
# carried beside the reference's nine fields, one row per image: tools.inference(image_scores=...) fills it, None otherwise
_PER_IMAGE_EXTRA = ("image_scores",)


class ModelOutputsContainer:
    """The 9 tensor fields ``predict_step`` / ``tools.inference`` hand around (constants.py:7-53)."""

    def __init__(self) -> None:
        for f in _FIELDS + _PER_IMAGE_EXTRA:
            setattr(self, f, None)

    def to_cpu(self):
        for f in _FIELDS + _PER_IMAGE_EXTRA:
            v = getattr(self, f)
            setattr(self, f, v.to('cpu') if torch.is_tensor(v) else None)

    def from_list(self, predictions: list[ModelOutputsContainer]):
        cols = {f: [] for f in _FIELDS}
        for p in predictions:
            p.to_cpu()
            for f in _FIELDS:
                v = getattr(p, f)
                if f in _OPTIONAL_IN_CAT and not torch.is_tensor(v):
                    continue
                cols[f].append(v)
        for f in _FIELDS:
            setattr(self, f, torch.cat(cols[f]) if len(cols[f]) else None)
        for f in _PER_IMAGE_EXTRA:
            vals = [getattr(p, f, None) for p in predictions]
            setattr(self, f, torch.cat(vals) if vals and all(torch.is_tensor(v) for v in vals) else None)

    def split(self, n_images: int) -> list:
        """One container per image: the inverse of ``from_list`` for a container that holds ``n_images`` images
        (patch-level fields carry num_patches rows per image, image-level fields one)."""
        parts = []
        for i in range(n_images):
            c = ModelOutputsContainer()
            for f in _FIELDS:
                v = getattr(self, f)
                if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] and v.shape[0] % n_images == 0:
                    k = v.shape[0] // n_images
                    setattr(c, f, v[i * k:(i + 1) * k].clone())
                else:
                    setattr(c, f, v)
            for f in _PER_IMAGE_EXTRA:
                v = getattr(self, f, None)
                if torch.is_tensor(v):
                    setattr(c, f, v[i:i + 1].clone())
            parts.append(c)
        return parts


class RegionsOutput:
    """What ``tools.defect_regions`` hands back: ``pred_masks`` uint8 [n][1][H][W] and ``labels`` int32 [n][1][H][W] on the device
    (regions below ``min_area`` removed, the rest numbered 1 .. per image), and ``regions``: per image a list of dicts of host
    values -- ``box`` (x0, y0, x1, y1, maxima inclusive), ``area``, ``centroid`` (x, y), ``score`` (the region's peak, anomalib's
    ``box_scores``) and ``peak`` (x, y)."""

    def __init__(self, pred_masks=None, labels=None, regions=None, threshold=None) -> None:
        self.pred_masks = pred_masks
        self.labels = labels
        self.regions = regions if regions is not None else []
        self.threshold = threshold

    @property
    def pred_boxes(self) -> list:
        return [[r['box'] for r in img] for img in self.regions]

    @property
    def box_scores(self) -> list:
        return [[r['score'] for r in img] for img in self.regions]


class EvaluationOutputContainer:
    def __init__(self) -> None:
        self.auroc = None
        self.f1_score = None
        self.aupro = None
        self.iou = None

    def to_string(self) -> str:
        r = lambda v: round(v, 2) if v else None
        return ("scores: [\n    auroc: {0},\n    f1-score: {1},\n    aupro: {2},\n    iou: {3}\n]"
                .format(r(self.auroc), r(self.f1_score), r(self.aupro), r(self.iou)))


def METRICS() -> list:
    return ['auroc', 'f1-score', 'aupro', 'iou']


def TEXTURES() -> list:
    return ['carpet', 'grid', 'leather', 'tile', 'wood']


def OBJECTS() -> list:
    return ['bottle', 'cable', 'capsule', 'hazelnut', 'metal_nut', 'pill', 'screw', 'tile', 'toothbrush',
            'transistor', 'zipper']


def OBJECTS_SET_ONE() -> list:
    return ['bottle', 'cable', 'capsule', 'hazelnut', 'metal_nut']


def OBJECTS_SET_TWO() -> list:
    return ['pill', 'screw', 'toothbrush', 'transistor', 'zipper']


def NON_FIXED_OBJECTS() -> list:
    return ['hazelnut', 'screw', 'metal_nut']
