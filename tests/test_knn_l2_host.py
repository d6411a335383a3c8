"""Host-only tests of the Euclidean metric of the kNN detector (no GPU): the argument errors of tools.inference / tools.sweep /
AnomalyDetector, the float64 yardstick of tests/knn_l2_ref.py against scipy, and the generator states across a Euclidean fit with a
coreset."""
import random

import numpy as np
import pytest
import torch

import knn_l2_ref as ref


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


def test_metric_argument_errors_come_before_any_file_is_read(tmp_path):
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector, check_metric
    missing = str(tmp_path / "nothing_here")
    for kw, match in (({"metric": "euclidean", "detector": "gde"}, "detector='knn' only"),
                      ({"metric": "euclidean", "detector": "padim", "patch_localization": True, "localization": "dense",
                        "bank": "train"}, "detector='knn' only"),
                      ({"metric": "l2"}, "metric must be one of"),
                      ({"metric": None}, "metric must be one of"),
                      ({"metric": "euclidean", "coreset": 0.0}, "coreset"),
                      ({"metric": "euclidean", "image_scores": "max"}, "patch_localization=True")):
        with pytest.raises(ValueError, match=match):
            tools.inference(missing + "/model.ckpt", missing + "/", "bottle", **kw)
        with pytest.raises(ValueError, match=match):
            tools.sweep(missing + "/", missing + "/out/", ["bottle"], **{"patch_localization": False, **kw})
    with pytest.raises(ValueError, match="metric must be one of"):
        AnomalyDetector(metric="manhattan")
    with pytest.raises(ValueError, match="multiple of 32"):
        AnomalyDetector(metric="euclidean").fit_bank(gauss(10, 48, 0))        # raised from the shape, before the device is touched
    assert check_metric("cosine") == "cosine" and AnomalyDetector().metric == "cosine"
    det = AnomalyDetector(metric="euclidean", coreset=0.5)
    assert det.metric == "euclidean" and det.bank_sq is None


def test_reference_matches_scipy_cdist():
    cdist = pytest.importorskip("scipy.spatial.distance").cdist
    for d, mean in ((32, 0.0), (384, 0.0), (384, 10.0)):
        x, b = gauss(57, d, 1, mean), gauss(131, d, 2, mean)
        x[5] = b[7]                                                  # an exact copy: 0 by the clamp, finite
        want = cdist(x.double().numpy(), b.double().numpy())         # direct differences in float64
        d2 = ref.d2_64(x, b)
        a = ref.scale_a(x, b)
        assert (d2 >= 0).all() and np.isfinite(d2).all()
        assert (np.abs(d2 - want ** 2) <= 8 * (d + 8) * 2.0 ** -53 * a).all()    # the expanded form in float64: its own rounding
        dd, idx = ref.kneighbors64(x, b, 3)
        assert idx[5, 0] == 7 and dd[5, 0] <= 8 * (d + 8) * 2.0 ** -53 * a[5, 7]
        order = np.argsort(d2, axis=1, kind="stable")[:, :3]
        assert np.array_equal(idx, order) and np.array_equal(dd, np.take_along_axis(d2, order, 1))
        keep = np.arange(57) != 5                                    # (the copy's root magnifies the float64 cancellation error)
        assert np.allclose(ref.patch_scores64(x, b)[keep], np.sort(want, axis=1)[keep, :3].mean(1), rtol=0, atol=1e-9)


def test_fp32_evaluation_of_the_formula_is_within_a_few_units():
    """Orientation for the bar of the GPU tests: numpy's fp32 evaluation of the same formula against float64, in units of 2^-24 A."""
    for d in (32, 384, 1536):
        x, b = gauss(64, d, 3), gauss(200, d, 4)
        xn, bn = x.numpy(), b.numpy()
        d2 = np.maximum(((xn * xn).sum(1)[:, None] + (bn * bn).sum(1)[None, :]) - np.float32(2) * (xn @ bn.T), np.float32(0))
        assert d2.dtype == np.float32
        ratio = np.abs(d2.astype(np.float64) - ref.d2_64(x, b)) / (ref.EPS * ref.scale_a(x, b))
        assert ratio.max() <= d + 8, (d, ratio.max())


def test_generator_states_are_unmoved_by_a_euclidean_fit_with_a_coreset(monkeypatch):
    """The Python path of fit(split=False) with metric='euclidean' and a coreset draws nothing from the global torch, numpy or
    `random` generators (the coreset projection has its own).  The device ops are replaced by torch CPU stand-ins: what is under test
    is the host code around them."""
    from self_supervised import models, ops
    from self_supervised.models import AnomalyDetector

    def greedy(p, m, start=0, wgs=None):
        mind = ((p - p[start]) ** 2).sum(1)
        sel = [start]
        for _ in range(1, m):
            sel.append(int(mind.argmax()))
            mind = torch.minimum(mind, ((p - p[sel[-1]]) ** 2).sum(1))
        return torch.tensor(sel), torch.zeros(len(sel))

    def knn(x, bank, bsq, k=3, splits=None):
        return torch.cdist(x, bank).topk(k, largest=False).values.mean(1)
    monkeypatch.setattr(AnomalyDetector, "_dev", staticmethod(lambda t: torch.as_tensor(t, dtype=torch.float32).contiguous()))
    monkeypatch.setattr(ops, "row_sqnorms", lambda x: (x * x).sum(1))
    monkeypatch.setattr(ops, "linear_fwd", lambda x, w: x @ w.t())
    monkeypatch.setattr(ops, "coreset_greedy", greedy)
    monkeypatch.setattr(ops, "l2_knn_fused", knn)
    monkeypatch.setattr(models, "_CORESET_OMEGA", {})                 # the projection is drawn inside this test
    emb = gauss(200, 64, 1)
    before = (torch.get_rng_state().clone(), np.random.get_state(), random.getstate())
    det = AnomalyDetector(coreset=0.25, coreset_dim=32, metric='euclidean')
    det.fit(emb, split=False)
    assert det.bank.shape == (50, 64) and det.bank_sq.shape == (50,) and det.coreset_counts == (50, 200)
    assert torch.equal(det.bank, emb[det.coreset_rows[0]])            # raw rows: nothing is normalised
    assert torch.equal(det.bank_sq, (det.bank * det.bank).sum(1))
    assert np.isfinite(det.threshold)
    assert torch.equal(torch.get_rng_state(), before[0])
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), before[1]))
    assert random.getstate() == before[2]
