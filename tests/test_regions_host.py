"""Defect regions without a GPU: the reference (tests/regions_ref.py) on hand-drawn cases whose answers are written out here, the
mask zoo's own properties, and the argument errors of the public calls on host tensors."""
import numpy as np
import pytest
import torch

import regions_ref as ref
from self_supervised import metrics, ops, tools
from self_supervised.constants import RegionsOutput

T = ops.REGION_TILE


def test_ops_surface():
    for name in ("label_regions", "region_stats", "region_filter", "pro_weights"):
        assert callable(getattr(ops, name))
    assert T == 32 and isinstance(RegionsOutput().regions, list)


def test_diagonal_joins_under_8_not_under_4():
    m = np.array([[1, 0, 0],
                  [0, 1, 0],
                  [0, 0, 0],
                  [1, 1, 0]], np.uint8)                      # 4 rows x 3 columns
    lab8, k8 = ref.label(m, 8)
    lab4, k4 = ref.label(m, 4)
    assert k8 == 2 and k4 == 3
    assert lab8.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 0], [2, 2, 0]]
    assert lab4.tolist() == [[1, 0, 0], [0, 2, 0], [0, 0, 0], [3, 3, 0]]
    area, bbox, csum, _, _ = ref.stats(lab8, k8)
    assert area.tolist() == [2, 2]
    assert bbox.tolist() == [[0, 0, 1, 1], [0, 3, 1, 3]]       # x0, y0, x1, y1 with inclusive maxima
    assert csum.tolist() == [[1, 1], [1, 6]]


def test_ring_around_a_dot():
    m = np.array([[1, 1, 1, 1, 1],
                  [1, 0, 0, 0, 1],
                  [1, 0, 1, 0, 1],
                  [1, 0, 0, 0, 1],
                  [1, 1, 1, 1, 1]], np.uint8)
    scores = np.zeros((5, 5), np.float32)
    scores[4, 1] = scores[0, 3] = 7.0                           # a tie for the ring's peak: the first in raster order wins
    scores[2, 2] = -1.0
    for c in (8, 4):
        lab, k = ref.label(m, c)
        assert k == 2 and lab[0, 0] == 1 and lab[2, 2] == 2     # numbered by first pixel in raster order
        area, bbox, csum, peak, pos = ref.stats(lab, k, scores)
        assert area.tolist() == [16, 1]
        assert bbox.tolist() == [[0, 0, 4, 4], [2, 2, 2, 2]]
        assert csum.tolist() == [[32, 32], [2, 2]]
        assert peak.tolist() == [7.0, -1.0] and pos.tolist() == [3, 12]
        mask, lab2, k2 = ref.filter_labels(lab, k, area >= 2)
        assert k2 == 1 and lab2[2, 2] == 0 and mask.sum() == 16 and lab2[0, 0] == 1
        mask, lab2, k2 = ref.filter_labels(lab, k, area < 2)
        assert k2 == 1 and lab2[2, 2] == 1 and mask.sum() == 1      # renumbered from 1
        mask, lab2, k2 = ref.filter_labels(lab, k, area > 99)
        assert k2 == 0 and not mask.any() and not lab2.any()


def test_reference_defect_regions_on_the_ring():
    s = np.zeros((1, 5, 5), np.float32)
    s[0, 0, :] = s[0, 4, :] = s[0, :, 0] = s[0, :, 4] = 1.0
    s[0, 2, 2] = 3.0
    s[0, 3, 4] = 2.0
    masks, labs, regions = ref.defect_regions(s, 1.0, min_area=2)
    assert masks.sum() == 16 and labs.max() == 1
    (r,), = regions
    assert r == dict(box=(0, 0, 4, 4), area=16, centroid=(2.0, 2.0), score=2.0, peak=(4, 3))
    assert ref.defect_regions(s, np.inf)[2] == [[]]
    nan = s.copy(); nan[0, 0, 0] = np.nan                        # NaN >= threshold is False: background
    assert ref.defect_regions(nan, 1.0, min_area=2)[2][0][0]["area"] == 15


def test_pro_weight_planes_of_the_reference():
    m = np.array([[[1, 1, 0], [0, 0, 0], [0, 0, 1]], [[0, 0, 0]] * 3], np.uint8)
    labs, counts, offsets = ref.label_batch(m, 8)
    assert counts.tolist() == [2, 0] and offsets.tolist() == [0, 2, 2]
    fp_w, pro_w = ref.pro_weights(labs, counts)
    assert fp_w.tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0] + [1] * 9
    assert pro_w.tolist() == [0.5, 0.5, 0, 0, 0, 0, 0, 0, 1.0] + [0.0] * 9


def test_zoo_properties():
    z = ref.zoo(T)
    s = 2 * T + 1
    assert {m.shape for m in z.values()} >= {(1, 1), (1, 7), (7, 1), (T - 1, T - 1), (T, T), (T + 1, T + 1), (s, s), (3, s)}
    for c in (8, 4):
        assert ref.label(z["spiral"], c)[1] == 1                # one component through every tile
        assert ref.label(z["two_spirals"], c)[1] == 2
        assert ref.label(z["comb"], c)[1] == 1
        assert ref.label(z["nested_u"], c)[1] == T // 2
        assert ref.label(z["all_fg"], c)[1] == 1 and ref.label(z["all_bg"], c)[1] == 0
        assert ref.label(z["rings"], c)[1] == T // 3 + 1
    assert z["spiral"].shape == (s, s) and z["spiral"][:, 0].sum() >= s - 2 and z["spiral"][s // 2, s // 2] == 1
    # touching tiles: the spiral has pixels in each of the nine tiles of its image
    assert all(z["spiral"][y:y + T, x:x + T].any() for y in range(0, s, T) for x in range(0, s, T))
    assert ref.label(z["checkerboard"], 8)[1] == 1
    assert ref.label(z["checkerboard"], 4)[1] == (s * s + 1) // 2     # the most components an image can hold
    assert ref.label(z["diagonal_spirals"], 8)[1] == 2
    assert ref.label(z["diagonal_spirals"], 4)[1] == int(z["diagonal_spirals"].sum())
    assert ref.label(z["diagonal_touch"], 8)[1] == 1 and ref.label(z["diagonal_touch"], 4)[1] == 2
    assert ref.label(z["diagonals"], 8)[1] == 1 < ref.label(z["diagonals"], 4)[1]
    for d in (0.1, 0.4, 0.6, 0.9):
        assert abs(z[f"density_{d}"].mean() - d) < 0.03
    again = ref.zoo(T)
    assert all(np.array_equal(z[k], again[k]) for k in z)         # seeds fixed


def test_numbering_is_raster_order_of_first_pixels():
    for name, m in ref.zoo(T).items():
        for c in (8, 4):
            lab, k = ref.label(m, c)
            first = [int(np.flatnonzero(lab.ravel() == r)[0]) for r in range(1, k + 1)]
            assert first == sorted(first), (name, c)


@pytest.mark.parametrize("kwargs", [dict(connectivity=6), dict(min_area=0), dict(min_area=1.5), dict(threshold=float("nan"))])
def test_defect_regions_argument_errors(kwargs):
    args = dict(threshold=0.5)
    args.update(kwargs)
    with pytest.raises(ValueError):
        tools.defect_regions(torch.zeros(2, 1, 8, 8), **args)


@pytest.mark.parametrize("shape", [(8, 8), (2, 3, 8, 8), (2, 1, 1, 8, 8), (0, 1, 8, 8)])
def test_defect_regions_shape_errors(shape):
    with pytest.raises(ValueError):
        tools.defect_regions(torch.zeros(shape), 0.5)


def test_host_tensors_are_refused():
    with pytest.raises(RuntimeError):
        tools.defect_regions(torch.zeros(2, 1, 8, 8), 0.5)
    with pytest.raises(RuntimeError):
        ops.label_regions(torch.zeros(1, 4, 4), 0.5)
    lab, off = torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.region_stats(lab, off)
    with pytest.raises(RuntimeError):
        ops.region_filter(lab, off, torch.zeros(0, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ops.pro_weights(lab, off, torch.zeros(0, dtype=torch.int32))


def test_compute_pro_gpu_labelling_argument():
    maps, gts = torch.zeros(1, 4, 4), torch.zeros(1, 4, 4)
    with pytest.raises(ValueError):
        metrics.compute_pro_gpu(maps, gts, labelling="gpu")
    for how in ("host", "device"):
        with pytest.raises(RuntimeError):                          # host maps: compute_pro is the host call
            metrics.compute_pro_gpu(maps, gts, labelling=how)
    with pytest.raises(ValueError):
        tools.Evaluator(["aupro"], pro_labelling="gpu")
    assert tools.Evaluator(["aupro"]).pro_labelling == "host"
    assert tools.Evaluator(["aupro"], pro_labelling="device").pro_labelling == "device"
