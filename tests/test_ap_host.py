"""CPU tests of average precision and the precision-recall curve: the float64 reference (tests/ap_ref.py) and the host functions
metrics.compute_average_precision / compute_pr_curve against scikit-learn, the conventions scikit-learn leaves to the caller (no
positive label -> 0.0, NaN and empty inputs -> ValueError), the Evaluator with and without 'ap', and the header / _hip.SIGNATURES
agreement for the four entry points.

Bars (u = 2^-53).  Our side forms every term (TP_j - TP_{j-1}) / P * TP_j / N_j with three roundings and sums m non-negative terms,
within (m - 1) u of the exact sum: (m + 2) u AP in all.  sklearn sums (recall_j - recall_{j-1}) * precision_j: the two recalls are
rounded quotients, so their difference is off by up to u (recall_j + recall_{j-1}) <= 2 u recall_j in ABSOLUTE terms (cancellation),
then two more roundings and the sum: (m + 2) u AP + 2 u sum_j precision_j recall_j.  Together
    |ours - sklearn| <= 2^-52 ((m + 4) AP + sum_j precision_j recall_j).
precision / recall: one correctly rounded division of the same integers on every side (0 ulp expected; 2 allowed)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import ap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssad_average_precision_workspace", "ssad_average_precision", "ssad_pr_curve_workspace", "ssad_pr_curve")


def _cases():
    rng = np.random.RandomState(11)
    out = {}
    s = rng.rand(1000).astype(np.float32)
    out["distinct"] = (s, rng.rand(1000) < 0.3)
    out["quantised"] = ((np.floor(rng.rand(5000) * 8) / 8).astype(np.float32), rng.rand(5000) < 0.02)
    out["equal"] = (np.full(257, 0.625, np.float32), rng.rand(257) < 0.4)
    out["two_values"] = (np.where(rng.rand(300) < 0.5, -1.5, 2.0).astype(np.float32), rng.rand(300) < 0.5)
    s = rng.randn(4097).astype(np.float32)
    out["correlated"] = (s, rng.rand(4097) < 1 / (1 + np.exp(-2 * s)))
    out["negative"] = (-rng.rand(500).astype(np.float32) - 1, rng.rand(500) < 0.1)
    out["single_positive"] = (rng.rand(100).astype(np.float32), np.arange(100) == 37)
    out["all_positive"] = ((np.floor(rng.rand(64) * 5)).astype(np.float32), np.ones(64, bool))
    out["labels_not_01"] = (rng.rand(200).astype(np.float32), rng.randint(0, 4, 200).astype(np.uint8) * 85)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_and_host_function_match_sklearn(name):
    from sklearn.metrics import average_precision_score, precision_recall_curve
    from self_supervised import metrics as m
    s, y = CASES[name]
    yb = np.asarray(y) != 0
    want = average_precision_score(yb, s)
    p, r, t = precision_recall_curve(yb, s)
    ref = ap_ref.ap_ref(s, y)
    bar = 2.0 ** -52 * ((ref.m + 4) * want + float(np.sum(ref.precision * ref.recall)))
    got = m.compute_average_precision(y, s)
    assert abs(ref.ap - want) <= bar, (ref.ap, want)
    assert abs(got - want) <= bar, (got, want)
    assert abs(m.compute_average_precision(torch.from_numpy(np.asarray(y)), torch.from_numpy(s)) - want) <= bar
    # the reference's curve against sklearn's, in sklearn's layout
    assert np.array_equal(ref.thresholds[::-1], t)
    assert float(ap_ref.ulps(ref.precision[::-1], p[:-1]).max()) <= 2 and float(ap_ref.ulps(ref.recall[::-1], r[:-1]).max()) <= 2
    gp, gr, gt = m.compute_pr_curve(y, s)
    assert gp.shape == p.shape and gr.shape == r.shape and gt.shape == t.shape and gt.dtype == np.float32
    assert np.array_equal(gt, t)
    assert float(ap_ref.ulps(gp, p).max()) <= 2 and float(ap_ref.ulps(gr, r).max()) <= 2
    assert (gp[-1], gr[-1]) == (1.0, 0.0)


def test_zero_signs_are_one_threshold():
    from self_supervised import metrics as m
    s = np.array([0.0, -0.0, 0.5, -0.0, 0.0, -1.0], np.float32)
    y = np.array([1, 0, 0, 1, 0, 1])
    ref = ap_ref.ap_ref(s, y)
    assert ref.m == 3 and ref.tp.tolist() == [0, 2, 3] and ref.n.tolist() == [1, 5, 6]
    assert np.signbit(ref.thresholds[1]) and ref.thresholds[1] == 0
    _, _, t = m.compute_pr_curve(y, s)
    assert np.array_equal(t.view(np.uint32), ref.thresholds[::-1].view(np.uint32))
    assert m.compute_average_precision(y, s) == ref.ap
    assert not np.signbit(ap_ref.ap_ref(np.abs(s), y).thresholds[1])


def test_no_positive_gives_zero_as_sklearn_arithmetic_does():
    import warnings
    from sklearn.metrics import average_precision_score
    from self_supervised import metrics as m
    s = np.array([0.3, 0.1, 0.3, 0.9], np.float32)
    y = np.zeros(4, np.uint8)
    assert m.compute_average_precision(y, s) == 0.0 and ap_ref.ap_ref(s, y).ap == 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert average_precision_score(y, s) == 0.0
    p, r, t = m.compute_pr_curve(y, s)
    assert r.tolist() == [1.0, 1.0, 1.0, 0.0] and p.tolist() == [0.0, 0.0, 0.0, 1.0] and t.tolist() == [np.float32(0.1), np.float32(0.3), np.float32(0.9)]


def test_nan_and_empty_inputs_raise():
    from self_supervised import metrics as m
    for fn in (m.compute_average_precision, m.compute_pr_curve):
        with pytest.raises(ValueError, match="NaN"):
            fn(np.array([1, 0, 1]), np.array([0.5, np.nan, 0.1], np.float32))
        with pytest.raises(ValueError):
            fn(np.zeros(0, np.uint8), np.zeros(0, np.float32))
        with pytest.raises(ValueError):
            fn(torch.zeros(0), torch.zeros(0))


def test_gpu_functions_refuse_host_tensors():
    from self_supervised import metrics as m
    for fn in (m.average_precision_gpu, m.pr_curve_gpu):
        with pytest.raises(RuntimeError, match="GPU tensors"):
            fn(torch.tensor([1, 0]), torch.tensor([0.5, 0.25]))


def _container():
    from self_supervised.constants import ModelOutputsContainer
    g = torch.Generator().manual_seed(5)
    out = ModelOutputsContainer()
    gts = torch.zeros(4, 1, 32, 32)
    gts[1, 0, 4:12, 6:20] = 1
    gts[3, 0, 20:30, 2:9] = 1
    out.ground_truths = gts
    out.anomaly_maps = torch.rand(4, 1, 32, 32, generator=g) + 0.6 * gts * torch.rand(4, 1, 32, 32, generator=g)
    out.y_true_binary_labels = torch.tensor([0, 1, 0, 1])
    return out


def test_evaluator_without_ap_is_unchanged_and_with_ap_gains_the_column(tmp_path):
    """Without 'ap' the scores, the frame built from them and the json file are those of the functions the parent called, with the
    parent's keys; with 'ap' one more attribute / column, AP, holds compute_average_precision of the same maps."""
    from self_supervised import metrics as m, tools
    out = _container()
    targets, scores = torch.flatten(out.ground_truths, 0, -1), torch.flatten(out.anomaly_maps, 0, -1)
    thr = m.best_f1_threshold(scores, targets)
    fprs, pros = m.compute_pro(out.anomaly_maps.squeeze(1).numpy(), out.ground_truths.squeeze(1).numpy())
    want = {"auroc": m.compute_auc(*m.compute_roc(targets, scores)[:2]), "f1_score": None, "aupro": m.compute_aupro(fprs, pros, 0.3),
            "iou": m.compute_iou(scores, targets, thr)}
    frames = {}
    for name, names in (("plain", ['auroc', 'aupro', 'iou']), ("ap", ['auroc', 'aupro', 'iou', 'ap'])):
        ev = tools.Evaluator(evaluation_metrics=names)
        ev.evaluate(out, "bottle", str(tmp_path / name) + "/", patch_level=True)
        got = dict(vars(ev.scores))
        ap = got.pop("AP", None)
        assert list(got) == list(want) and got == want
        stored = json.load(open(tmp_path / name / "bottle_pixel_scores.json"))
        frames[name] = m.metrics_to_dataframe({k: [v] for k, v in vars(ev.scores).items() if v is not None}, ["bottle"])
        if name == "plain":
            assert ap is None and list(stored) == list(want)
            assert frames[name].equals(m.metrics_to_dataframe({k: [v] for k, v in want.items() if v is not None}, ["bottle"]))
        else:
            assert ap == m.compute_average_precision(targets, scores) and 0 < ap < 1
            assert list(stored) == list(want) + ["AP"] and stored["AP"] == ap
            assert list(frames[name].columns) == list(frames["plain"].columns) + ["AP"]
            assert frames[name].drop(columns="AP").equals(frames["plain"])
    # image level: 'ap' is valid there as 'auroc' is; an unknown name is refused with the message it always had
    img = _container()
    img.anomaly_maps = torch.tensor([0.1, 0.7, 0.4, 0.3])
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'ap'])
    ev.evaluate(img, "bottle", "", patch_level=False)
    assert ev.scores.AP == m.compute_average_precision(img.y_true_binary_labels, img.anomaly_maps)
    with pytest.raises(ValueError, match=re.escape("correct metrics list: ['auroc', 'f1-score', 'aupro', 'iou']")):
        tools.Evaluator(evaluation_metrics=['auroc', 'AP']).evaluate(img, "bottle", "", patch_level=False)


def test_image_ap_on_host_scores():
    from self_supervised import metrics as m, tools
    out = _container()
    with pytest.raises(ValueError, match="image_scores"):
        tools.image_ap(out)
    out.image_scores = torch.tensor([0.2, 0.9, 0.5, 0.4])
    assert tools.image_ap(out) == m.compute_average_precision(out.y_true_binary_labels, out.image_scores)


def test_sweep_refuses_average_precision_at_image_level_before_touching_anything(tmp_path):
    from self_supervised import tools
    missing = str(tmp_path / "nowhere") + "/"
    with pytest.raises(ValueError, match="average_precision"):
        tools.sweep(missing, missing, ["bottle"], patch_localization=False, average_precision=True)
    assert not os.path.exists(missing)


def test_header_and_signatures_agree_on_the_new_entry_points():
    from self_supervised import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssad.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/ssad.h"
        assert name in _hip.SIGNATURES, name
        assert len(_hip.SIGNATURES[name]) == len(m.group(2).split(",")), name
        assert (_hip.RESTYPES.get(name) is _hip._c_l) == (m.group(1) == "int64_t"), name
    src = open(os.path.join(ROOT, "self-supervised-anomaly-detection_amd", "csrc", "auroc.hip")).read()
    for name in NEW:
        assert re.search(r'extern "C" (int|int64_t) ' + name + r"\(", src), name
