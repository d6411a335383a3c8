"""The evaluation-metric table without a GPU (tests/metrics_table.py): every case the table exists for is reached by a row (from n and
the generated inputs alone); the references agree with the reference stack they restate (sklearn's roc_auc_score, metrics.compute_pro,
metrics.best_f1_threshold); the exact F1 tie is a tie; and the workspace functions of csrc/auroc.hip (plain host code) return what the
entries carve."""
import numpy as np
import pytest
import torch

import metrics_table as T


def _lib():
    from self_supervised import _hip
    return _hip.lib()


def _rows(entry):
    return [r for r in T.ROWS if r.entry == entry]


def test_row_ids_unique_and_listed_sizes_present():
    ids = [r.id for r in T.ROWS]
    assert len(ids) == len(set(ids))
    listed = {1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 3 * 4096 + 5, 20463, 262144 + 4097}
    for entry in ("auroc", "pro", "f1"):
        assert {r.n for r in _rows(entry)} >= listed, entry
    assert {r.n for r in _rows("conf")} == {257, 262144 + 4097}
    assert max(r.n for r in T.ROWS) == 262144 + 4097
    for tag in ("auroc_allpos_300", "auroc_allneg_300", "pro_no_fp_300", "pro_no_region_300", "pro_general_20463", "f1_no_positive_300",
                "f1_only_positives_300", "f1_exact_tie_80", "f1_late_full_recall_12288", "conf_bits_257"):
        assert tag in ids


@pytest.mark.parametrize("case", list(T.CASES))
def test_every_case_is_reached(case):
    hit = [r.id for r in T.ROWS if T.CASES[case](r, T.make_case(r))]
    assert hit, f"no row reaches: {case}"


@pytest.mark.parametrize("row", T.ROWS, ids=[r.id for r in T.ROWS])
def test_inputs(row):
    """What the references and the kernels leave out stays out, and the rows hold what their names say."""
    k = T.make_case(row)
    assert k.s.dtype == np.float32 and k.s.shape == (row.n,) and k.y.shape == (row.n,) and not np.isnan(k.s).any()
    if row.entry in ("pro", "f1"):
        assert np.isfinite(k.s).all(), "the host functions split a run of equal infinities"
    if row.n == 2:
        assert k.y.sum() == 1
    if row.family == "zeros":
        z = k.s == 0
        assert z.any() and (np.signbit(k.s[z]) == ~k.y[z]).all() and k.y[z].any() and not k.y[z].all()
    if row.entry == "pro":
        assert k.n_ok >= 1 and k.n_regions >= 1 and set(np.unique(k.fp_w)) <= {0, 1}
        if row.weights == "dyadic":
            assert set(np.unique(k.pro_w)) <= {0.0, 1.0, 2.0 ** -4, 2.0 ** -6, 2.0 ** -10}
        if row.id == "pro_no_fp_300":
            assert not k.fp_w.any() and k.n_ok == 1.0
        if row.id == "pro_no_region_300":
            assert not k.pro_w.any() and k.n_regions == 1.0
    if row.entry == "conf":
        t = k.thresholds
        assert (k.s == np.float32(t[0])).any() and t[1] == 0.0 and not np.signbit(t[1]) and (k.s.view(np.uint32) == T.NEG0).any()
        assert t[2:4] == [float("-inf"), float("inf")]
        lo, hi = k.s[k.pair_at]
        assert np.nextafter(lo, np.float32(1)) == hi and float(lo) < t[5] < float(hi) == t[4] and k.y[k.pair_at[0]] != k.y[k.pair_at[1]]


# ---- the references ----
def test_auroc_reference_on_hand_cases():
    s = np.array([0.1, 0.4, 0.35, 0.8], dtype=np.float32)
    assert T.ref_auroc(s, np.array([0, 0, 1, 1], dtype=bool)) == (0.75, 2)
    assert T.ref_auroc(np.array([-0.0, 0.0], dtype=np.float32), np.array([0, 1], dtype=bool)) == (0.5, 1)
    inf = np.array([np.inf, np.inf, -np.inf, 1.0], dtype=np.float32)
    assert T.ref_auroc(inf, np.array([1, 0, 0, 1], dtype=bool)) == (0.625, 2)          # (1.5 + 1) / 4
    v, p = T.ref_auroc(s, np.ones(4, dtype=bool))
    assert np.isnan(v) and p == 4
    k = T.make_case(next(r for r in T.ROWS if r.id == "auroc_equal_12293"))
    assert T.ref_auroc(k.s, k.y)[0] == 0.5


FINITE_AUROC = [r for r in _rows("auroc") if r.n > 1 and r.labels == "corr" and np.isfinite(T.make_case(r).s).all()]


@pytest.mark.parametrize("row", FINITE_AUROC, ids=lambda r: r.id)
def test_auroc_reference_against_sklearn(row):
    """On the rows without infinities (sklearn rejects those).  sklearn's trapezoid rounds once per curve point, the reference once in
    all: within 4 ulp (1 ulp seen at n = 20 463)."""
    from sklearn.metrics import roc_auc_score
    k = T.make_case(row)
    want, p = T.ref_auroc(k.s, k.y)
    assert p == int(k.y.sum())
    got = roc_auc_score(k.y, k.s)
    print(f"   {row.id}: reference {want!r}, sklearn {got!r}: {abs(got - want) / np.spacing(want):.1f} ulp")
    assert abs(got - want) <= 4 * np.spacing(want)


def test_pro_reference_against_compute_pro():
    """The restatement starts where metrics.compute_pro has its planes: on a map with labelled regions (touching at a corner, one
    image defect-free, heavy ties) both give the same curve."""
    from scipy import ndimage
    from self_supervised import metrics
    rng = np.random.RandomState(5)
    maps = (np.floor(rng.rand(4, 24, 24) * 41) / 41).astype(np.float32)
    gts = np.zeros((4, 24, 24), dtype=np.uint8)
    gts[0, 2:7, 3:9] = 1
    gts[0, 7:10, 9:12] = 1                      # touches the first block at a corner: one 8-connected region
    gts[1, 10:13, 10:11] = 1
    gts[1, 0:16, 20:24] = 1
    gts[3, 5:12, 5:12] = 1
    maps += np.float32(0.25) * gts
    fp_w, pro_w, n_regions = np.zeros(maps.shape, dtype=np.uint8), np.zeros(maps.shape), 0
    for i, gt in enumerate(gts):
        lab, n = ndimage.label(gt, np.ones((3, 3), dtype=int))
        n_regions += n
        fp_w[i] = lab == 0
        if n:
            pro_w[i] = np.concatenate([[0.0], 1.0 / np.bincount(lab.ravel())[1:]])[lab]
    assert n_regions == 4
    wf, wp = T.ref_pro(maps.ravel(), fp_w.ravel(), pro_w.ravel(), float(fp_w.sum()), float(n_regions))
    fprs, pros = metrics.compute_pro(maps, gts)
    assert wf.dtype == np.float32 and 1 < wf.size < maps.size
    assert np.array_equal(fprs[1:-1], wf.astype(np.float64)) and np.array_equal(pros[1:-1], wp)


@pytest.mark.parametrize("row", _rows("f1"), ids=lambda r: r.id)
def test_f1_reference_against_best_f1_threshold(row):
    from self_supervised import metrics
    k = T.make_case(row)
    ref = T.f1_ref_of(row)
    assert metrics.best_f1_threshold(torch.from_numpy(k.s.copy()), torch.from_numpy(k.y.astype(np.int64))) == ref.threshold
    assert ref.f1.dtype == np.float32
    if k.y.any():
        assert ref.f1 == np.nanmax(ref.curve) and 0.0 <= ref.f1 <= 1.0
    else:
        assert np.isnan(ref.f1) and ref.threshold == float(k.s.max())


def test_f1_exact_tie_is_a_tie():
    row = next(r for r in T.ROWS if r.id == "f1_exact_tie_80")
    ref = T.f1_ref_of(row)
    at = np.flatnonzero(ref.curve == ref.curve.max())
    assert at.size >= 2 and ref.threshold == 65.0
    # ascending thresholds 1 .. 80, cut at the first full-recall point (score 1 is the last positive: no cut)
    thr = np.arange(1, 81)[:ref.curve.size - 1]
    assert set(thr[at].tolist()) == {65, 77}


def test_confusion_reference():
    s = np.array([-0.0, 1.0, np.inf, -np.inf], dtype=np.float32)
    y = np.array([1, 0, 1, 0], dtype=bool)
    assert T.ref_confusion(s, y, 0.0) == (2, 1, 0, 1)
    assert T.ref_confusion(s, y, float("inf")) == (1, 0, 1, 2)
    assert T.ref_confusion(s, y, float("-inf")) == (2, 2, 0, 0)


# ---- the workspace functions: host code ----
def test_workspace_functions_return_what_the_entries_carve():
    lib = _lib()
    sizes = sorted({r.n for r in T.ROWS} | {4096 * 1024, 4096 * 1024 + 1, 83 * 65536})
    for entry, fn in T.WS_FN.items():
        f = getattr(lib, fn)
        for n in sizes:
            assert f(n) == T.ws_carved(entry, n) + T.WS_SLACK[entry], (entry, n)
            assert all(b > 0 for b in T.WS_SLICES(entry, n))
        assert f(0) == -1 and f(-5) == -1 and f(2 ** 31 - 1) == -1 and f(2 ** 31 - 2) > 0
