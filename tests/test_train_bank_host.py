"""CPU: the host side of scoring against the whole training set -- tools' `bank` argument, the image-wise 70/30 split
(models.split_rows), the split-count rule of the bank-split kNN and its C ABI declaration."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kw,match", [({"bank": "all"}, "bank must be one of"),
                                      ({"bank": "train", "mvtec_inference": False}, "mvtec_inference=True")])
def test_bank_checked_before_any_file_is_read(tmp_path, kw, match):
    from self_supervised import tools
    missing = str(tmp_path / "nothing_here")
    with pytest.raises(ValueError, match=match):
        tools.inference(missing + "/model.ckpt", missing + "/", "bottle", **kw)
    with pytest.raises(ValueError, match="bank must be one of"):
        tools.sweep(missing + "/", missing + "/", ["bottle"], bank="bogus")


def test_groups_split_is_split_indices_over_images():
    from self_supervised.models import split_indices, split_rows
    sizes = [5, 1, 3, 4, 2, 6, 3]
    groups = torch.arange(len(sizes)).repeat_interleave(torch.tensor(sizes))
    starts = np.r_[0, np.cumsum(sizes)]
    for seed in range(5):
        np.random.seed(seed)
        tr_img, va_img = split_indices(len(sizes), 0.3)
        after = np.random.get_state()
        np.random.seed(seed)
        tr, va = split_rows(int(groups.numel()), groups)
        assert all(np.array_equal(a, b) for a, b in zip(after, np.random.get_state()))      # one permutation, nothing else drawn
        assert np.array_equal(tr, np.concatenate([np.arange(starts[i], starts[i + 1]) for i in tr_img]))
        assert np.array_equal(va, np.concatenate([np.arange(starts[i], starts[i + 1]) for i in va_img]))
    # no groups: the row split of the reference, unchanged
    np.random.seed(1)
    a = split_indices(20, 0.3)
    np.random.seed(1)
    b = split_rows(20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # rows of one image need not be contiguous
    g = torch.tensor([1, 0, 1, 2, 0, 2, 1])
    np.random.seed(2)
    tr_img, va_img = split_indices(3, 0.3)
    np.random.seed(2)
    tr, va = split_rows(7, g)
    assert sorted(set(g[tr].tolist())) == sorted(tr_img.tolist()) and set(g[va].tolist()) == set(va_img.tolist())
    assert len(tr) + len(va) == 7 and not set(tr) & set(va)


def test_knn_split_rule(monkeypatch):
    from self_supervised import ops
    assert ops.knn_splits(841, 588) == 1                 # the reference bank: today's one-launch kernel
    assert ops.knn_splits(4 * 10 ** 6, 123000) == 1      # WideResNet-50 scales
    assert ops.knn_splits(215296, 588) == 1              # the reference bank at the ResNet-18 scoring size
    assert ops.knn_splits(128 * ops.KNN_SPLIT_TARGET_WG, 123000) == 1
    assert ops.knn_splits(841, 3000) == 1                # splits would be too small
    s = ops.knn_splits(13456, 123000)
    assert s > 1 and 123000 / s >= ops.KNN_SPLIT_MIN_ROWS
    assert ops.knn_splits(841, 123000) > 1
    monkeypatch.setenv("SSAD_KNN_SPLIT", "0")
    assert ops.knn_splits(841, 123000) == 1


def test_split_entry_point_declared_and_bound():
    from self_supervised import _hip
    head = open(os.path.join(ROOT, "include", "ssad.h")).read()
    m = re.search(r"int ssad_cosine_knn_split\(([^)]*)\);", head)
    assert m, "ssad_cosine_knn_split not declared in include/ssad.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(_hip.SIGNATURES["ssad_cosine_knn_split"]) == 10
    kinds = {ctypes.c_void_p: ("*",), ctypes.c_int64: ("int64_t",), ctypes.c_int: ("int ",)}
    for p, t in zip(params, _hip.SIGNATURES["ssad_cosine_knn_split"]):
        assert any(k in p for k in kinds[t]), (p, t)
