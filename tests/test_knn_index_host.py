"""CPU-only checks of the index-returning kNN and the image scores: argument checks that need no GPU, the float64 helper of the GPU
tests against sklearn, and the container's extra per-image field."""
import inspect

import numpy as np
import pytest
import torch

import knn_index_ref as ref


@pytest.mark.parametrize("kw,match", [
    ({"image_scores": "max"}, "patch_localization=True"),
    ({"image_scores": "reweighted", "patch_localization": True, "detector": "gde"}, "detector='knn'"),
    ({"image_scores": "reweighted", "patch_localization": True, "neighbours": 1}, "neighbours must be an int in 2..32"),
    ({"image_scores": "reweighted", "patch_localization": True, "neighbours": 33}, "neighbours must be an int in 2..32"),
    ({"image_scores": "reweighted", "patch_localization": True, "neighbours": 9.0}, "neighbours must be an int in 2..32"),
    ({"image_scores": "mean", "patch_localization": True}, "image_scores must be one of")])
def test_image_scores_checked_before_any_file_is_read(tmp_path, kw, match):
    from self_supervised import tools
    missing = str(tmp_path / "nothing_here")
    with pytest.raises(ValueError, match=match):
        tools.inference(missing + "/model.ckpt", missing + "/", "bottle", **kw)
    sweep_kw = {k: v for k, v in kw.items() if k != "patch_localization"}
    sweep_kw["patch_localization"] = kw.get("patch_localization", False)
    with pytest.raises(ValueError, match=match):
        tools.sweep(missing + "/", missing + "/", ["bottle"], **sweep_kw)


def test_defaults_are_off():
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector
    for fn in (tools.inference, tools.sweep):
        sig = inspect.signature(fn).parameters
        assert sig["image_scores"].default is None and sig["neighbours"].default == 9
    sig = inspect.signature(AnomalyDetector.image_scores).parameters
    assert sig["mode"].default == 'max' and sig["neighbours"].default == 9
    assert inspect.signature(AnomalyDetector.kneighbors).parameters["k"].default is None
    # 'max' ignores neighbours; 'reweighted' checks it
    from self_supervised.models import check_image_scores
    assert check_image_scores('max', 1) == 'max' and check_image_scores(None, 0) is None
    assert check_image_scores('reweighted', 2) == 'reweighted' and check_image_scores('reweighted', 32) == 'reweighted'


def test_detector_argument_errors_without_a_gpu():
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector
    with pytest.raises(ValueError, match="patch-level"):
        AnomalyDetector().image_scores(torch.zeros(4, 64))
    with pytest.raises(ValueError, match="image_scores must be one of"):
        AnomalyDetector(patch_level=True, batch=1, num_patches=4).image_scores(torch.zeros(4, 64), mode='top')
    with pytest.raises(ValueError, match="neighbours"):
        AnomalyDetector(patch_level=True, batch=1, num_patches=4).image_scores(torch.zeros(4, 64), 'reweighted', 1)
    with pytest.raises(ValueError, match="no bank"):
        AnomalyDetector(patch_level=True, batch=1, num_patches=4).image_scores(torch.zeros(4, 64))
    with pytest.raises(ValueError, match="no bank"):
        AnomalyDetector().kneighbors(torch.zeros(4, 64))
    with pytest.raises(ValueError, match="k must be 1, 2 or 3"):
        ops.cosine_knn_index(torch.zeros(4, 64), torch.zeros(9, 64), k=4)
    with pytest.raises(ValueError, match="fewer than k"):
        ops.cosine_knn_index(torch.zeros(4, 64), torch.zeros(2, 64), k=3)
    with pytest.raises(ValueError, match="splits must be >= 1"):
        ops.cosine_knn_index(torch.zeros(4, 64), torch.zeros(9, 64), k=3, splits=0)
    with pytest.raises(ValueError, match="b must lie in 1..32"):
        ops.rows_smallest_index(torch.zeros(4, 64), 33)
    with pytest.raises(ValueError, match="wgs must lie in"):
        ops.rows_smallest_index(torch.zeros(4, 64), 32, wgs=129)


def test_float64_helper_against_sklearn():
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.RandomState(0)
    bank = rng.randn(700, 64)
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    x = 3.0 * rng.randn(90, 64)
    want_d, want_i = NearestNeighbors(n_neighbors=3, metric='cosine', algorithm='brute').fit(bank).kneighbors(x)
    got_d, got_i = ref.kneighbors64(x, bank, 3, chunk=32)
    assert np.array_equal(got_i, want_i)                            # a tie-free set: Gaussian rows
    assert np.abs(got_d - want_d).max() <= 1e-12


def test_smallest_stable_is_the_stable_argsort_with_duplicates():
    rng = np.random.RandomState(1)
    for r in (1, 5, 40, 3000):
        d = rng.randint(0, 7, size=(13, r)).astype(np.float64)
        for m in (1, 3, 9, 33):
            vals, idx = ref.smallest_stable(d, m)
            want = np.argsort(d, axis=1, kind="stable")[:, :min(m, r)]
            assert np.array_equal(idx, want) and np.array_equal(vals, np.take_along_axis(d, want, 1))


def test_strict_positions():
    d = np.array([[0.1, 0.2, 0.2 + 5e-6, 0.4]])
    assert ref.strict_positions(d, 3, 1e-5).tolist() == [[True, False, False]]
    assert ref.strict_positions(d[:, :1], 1, 1e-5).tolist() == [[True]]


def test_image_scores64_by_hand():
    """Two images of two patches against a bank of three rows, the formula of the issue written out."""
    bank = np.eye(3)
    x = np.array([[1.0, 0.0, 0.0], [2.0, 2.0, 0.0], [0.0, 0.0, 5.0], [0.0, 3.0, 4.0]])
    out = ref.image_scores64(x, bank, 2, neighbours=2, k=1)
    d = 1.0 - np.array([[1, 0, 0], [np.sqrt(.5), np.sqrt(.5), 0], [0, 0, 1], [0, .6, .8]])
    assert np.allclose(out["patch_scores"], d.min(1).reshape(2, 2))
    assert out["p_star"].tolist() == [1, 1]
    # image 0: x_{p*} = (1, 1, 0) / sqrt 2, m* = row 0 (tie with row 1: the smaller row), N = rows {0, 1} (0 itself, then 1 < 2 at distance 1)
    w0 = 1.0 - np.exp(d[1, 0]) / (np.exp(d[1, 0]) + np.exp(d[1, 1]))
    # image 1: x_{p*} = (0, .6, .8), m* = row 2, N = rows {2, 0}
    w1 = 1.0 - np.exp(d[3, 2]) / (np.exp(d[3, 2]) + np.exp(d[3, 0]))
    assert np.allclose(out["w"], [w0, w1]) and np.allclose(out["score"], [w0 * d[1, 0], w1 * d[3, 2]])
    # image 0: first / second nearest rows tie; image 1: rows 0 and 1 tie as 2nd / 3rd neighbours of row 2
    assert out["fragile"].tolist() == [True, True]
    assert not ref.image_scores64(x[2:], np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0.6, 0.8]]), 2, neighbours=2, k=1)["fragile"][0]
    assert ref.auroc64([0, 1, 1, 0], [0.1, 0.4, 0.35, 0.35]) == 0.875


def test_container_carries_image_scores_per_image():
    from self_supervised import constants
    from self_supervised.constants import ModelOutputsContainer
    assert len(constants._FIELDS) == 9 and "image_scores" not in constants._FIELDS
    c = ModelOutputsContainer()
    assert c.image_scores is None
    for f in constants._FIELDS:
        setattr(c, f, torch.arange(3.).reshape(3, 1))
    c.embedding_vectors = torch.arange(12.).reshape(6, 2)           # two patches per image
    parts = c.split(3)
    assert all(p.image_scores is None for p in parts)
    back = ModelOutputsContainer()
    back.from_list(parts)
    assert back.image_scores is None and torch.equal(back.embedding_vectors, c.embedding_vectors)
    c.image_scores = torch.tensor([.5, .25, .75])
    parts = c.split(3)
    assert [p.image_scores.tolist() for p in parts] == [[.5], [.25], [.75]]
    back = ModelOutputsContainer()
    back.from_list([parts[2], parts[0], parts[1]])
    assert back.image_scores.tolist() == [.75, .5, .25]
    assert torch.equal(back.embedding_vectors, c.embedding_vectors[[4, 5, 0, 1, 2, 3]])


def test_image_auroc_on_host_scores():
    from self_supervised import tools
    from self_supervised.constants import ModelOutputsContainer
    c = ModelOutputsContainer()
    c.y_true_binary_labels = torch.tensor([0, 1, 1, 0])
    with pytest.raises(ValueError, match="no image_scores"):
        tools.image_auroc(c)
    c.image_scores = torch.tensor([0.1, 0.4, 0.35, 0.35])
    assert abs(tools.image_auroc(c) - 0.875) <= 1e-12
