"""ssad_average_precision and ssad_pr_curve (csrc/auroc.hip) against the float64 reference of tests/ap_ref.py, and the Python layers
above them (metrics.average_precision_gpu / pr_curve_gpu, Evaluator 'ap', tools.image_ap, tools.sweep(average_precision=True)).

Rows.  n in 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 TILE + 3, 100 003 (TILE = SORT_T * SORT_ITEMS of the kernel
source: the span of one workgroup of the sort, the scans and the term sum), each with a score and a target pattern drawn in rotation,
then every score pattern and every target pattern once more at 2 TILE + 3, and 5 000 000 elements once (1221 workgroups: the
multi-block scans, int64 counts, more partials than the 256 threads of the last pass).
Score patterns: distinct | equal (one group of n) | two values | eight levels | straddle (groups of TILE centred on every workgroup
boundary of the sorted array) | zeros (-0.0 / +0.0 mixed among other values) | inf (+-inf present) | denormal | negative.
Target patterns: none | all | first / last (a single positive, first / last in sort order) | 1 % | bytes (values 0, 2, 85, 255).

How a row runs.  The C entry points are called directly on views between guards (inputs between 0x7f bytes: a huge finite score, a
positive label; outputs and the workspace between 0xff, pre-filled with 0xff), the workspace exactly ssad_*_workspace(n) bytes, each
entry twice into fresh buffers and once more on a permutation of the input: the same bits each time (the sort makes the result a
function of the multiset of (score, target) pairs), guards and inputs bit-unchanged, the curve arrays untouched past count.
Asserts.  out[1] == P, out[2] == m, count == m; thresholds bit-equal; TP_j = rint(recall_j P) and, where TP_j > 0, N_j = rint(TP_j /
precision_j) equal the reference's integers (TP_j = 0: precision_j == 0.0 exactly; N_j is then not implied by the curve); precision
and recall within 1 ulp (one division of exact integers each: 0.5 ulp if correctly rounded);
    |AP - AP_ref| <= (m + 4) 2^-52 AP_ref
(m non-negative terms in any order are within (m - 1) u of their sum, u = 2^-53, once for the kernel and once for the reference,
plus three roundings per term on either side; derived, not measured).

MEASURED (MI355X, 2026-10-20, `pytest -s -m gpu tests/test_hip_ap.py`; one run, one box; for the record, never asserted): worst
|AP - AP_ref| / bar = 0.142 (a row of 8 thresholds; 1.0e-6 on the 5 000 000 row, whose bar grows with m = 4 543 376); precision and
recall 0 ulp from the reference on every row (the correctly rounded quotients)."""
import os
import re

import numpy as np
import pytest
import torch

import ap_ref
from bn_table import Arena, twice, _lib, _p
from fake_mvtec import make_tree
from metrics_table import InArena, _poisoned

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "self-supervised-anomaly-detection_amd", "csrc", "auroc.hip")).read()
_M = re.search(r"constexpr int SORT_T = (\d+), SORT_ITEMS = (\d+), SORT_TILE = SORT_T \* SORT_ITEMS;", _SRC)
TILE = int(_M.group(1)) * int(_M.group(2))

MEASURED = {"AP err / bar": 0.142, "precision ulp": 0.0, "recall ulp": 0.0}
WORST = {"AP err / bar": 0.0, "precision ulp": 0.0, "recall ulp": 0.0}

SCORES = ("distinct", "equal", "two", "eight", "straddle", "zeros", "inf", "denormal", "negative")
TARGETS = ("none", "all", "first", "last", "percent", "bytes")
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 100003)
ROWS = [(n, SCORES[i % len(SCORES)], TARGETS[(i + 4) % len(TARGETS)]) for i, n in enumerate(SIZES)]
ROWS += [(2 * TILE + 3, sp, "percent" if i % 2 else "bytes") for i, sp in enumerate(SCORES)]
ROWS += [(2 * TILE + 3, "eight" if i % 2 else "distinct", tp) for i, tp in enumerate(TARGETS)]
ROWS += [(5000000, "distinct", "percent")]
ROWS = list(dict.fromkeys(ROWS))


def make_case(n, sp, tp):
    rng = np.random.RandomState((n * 31 + SCORES.index(sp) * 7 + TARGETS.index(tp)) % (1 << 31))
    if sp == "distinct":
        s = (rng.permutation(n).astype(np.float64) / n - 0.25).astype(np.float32)          # n <= 100 003: no two round together
    elif sp == "equal":
        s = np.full(n, 0.625, np.float32)
    elif sp == "two":
        s = np.where(rng.rand(n) < 0.5, -1.5, 2.0).astype(np.float32)
    elif sp == "eight":
        s = (np.floor(rng.rand(n) * 8) / 8).astype(np.float32)
    elif sp == "straddle":
        s = ((rng.permutation(n) + TILE // 2) // TILE).astype(np.float32)
    elif sp == "zeros":
        s = ((np.floor(rng.rand(n) * 5) - 2) / 2).astype(np.float32)
        z = s == 0
        s[z] = np.where(rng.rand(int(z.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    elif sp == "inf":
        s = rng.randn(n).astype(np.float32)
        s[rng.rand(n) < 0.1] = np.inf
        s[rng.rand(n) < 0.1] = -np.inf
    elif sp == "denormal":
        mag = rng.randint(0, 64, size=n).astype(np.uint32)
        s = (mag | np.where(rng.rand(n) < 0.5, np.uint32(0x80000000), np.uint32(0))).view(np.float32)
    else:
        s = (-1.0 - rng.rand(n) * 1e3).astype(np.float32)
    assert not np.isnan(s).any()
    order = np.lexsort((np.signbit(s), -s.astype(np.float64)))         # the sort's order: descending, +0.0 before -0.0
    y = np.zeros(n, np.uint8)
    if tp == "all":
        y[:] = 1
    elif tp == "first":
        y[order[0]] = 1
    elif tp == "last":
        y[order[-1]] = 1
    elif tp == "percent":
        rank = np.empty(n)
        rank[order] = np.arange(n) / n
        y[:] = rng.rand(n) < 0.03 * (1 - rank) ** 2                    # about 1 % positives, more of them at high scores
    elif tp == "bytes":
        y[:] = np.array([0, 0, 0, 2, 85, 255], np.uint8)[rng.randint(0, 6, size=n)]
    return np.ascontiguousarray(s), y


def _big_case(n):
    rng = np.random.RandomState(5)
    s = rng.rand(n).astype(np.float32)                                # 5 M draws of 2^24 values: ties of two and three as well
    y = (rng.rand(n) < 0.02 * (0.2 + s)).astype(np.uint8)
    return s, y


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    yield torch.device("cuda:0")
    for kind, v in sorted(WORST.items()):
        print(f"worst {kind}: {v:.3e}", flush=True)


def _launch_ap(rid, dev, sd, td, n):
    hip, lib, st = _lib()

    def launch():
        ar = Arena(dev)
        nbytes = lib.ssad_average_precision_workspace(n)
        ws = ar.out("workspace", (nbytes,), torch.uint8, all_written=False)
        out = ar.out("out", (3,), torch.float64, all_written=False)
        hip.check(lib.ssad_average_precision(_p(sd), _p(td), n, _p(ws), nbytes, _p(out), st))
        ar.check_outputs(rid)
        return {"out": out}
    return launch


def _launch_pr(rid, dev, sd, td, n):
    hip, lib, st = _lib()

    def launch():
        ar = Arena(dev)
        nbytes = lib.ssad_pr_curve_workspace(n)
        ws = ar.out("workspace", (nbytes,), torch.uint8, all_written=False)
        o = {"precision": ar.out("precision", (n,), torch.float64, all_written=False),
             "recall": ar.out("recall", (n,), torch.float64, all_written=False),
             "thresholds": ar.out("thresholds", (n,), torch.float32, all_written=False),
             "count": ar.out("count", (1,), torch.int64, all_written=False)}
        hip.check(lib.ssad_pr_curve(_p(sd), _p(td), n, _p(ws), nbytes, _p(o["precision"]), _p(o["recall"]), _p(o["thresholds"]),
                                    _p(o["count"]), st))
        ar.check_outputs(rid)
        return o
    return launch


def _same_bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def run_row(rid, s, y, dev):
    from self_supervised import metrics
    n = s.size
    ref = ap_ref.ap_ref(s, y)
    ia = InArena(dev)
    sd, td = ia.inp("scores", torch.from_numpy(s)), ia.inp("targets", torch.from_numpy(y))
    perm = np.random.RandomState(n % 1000 + 1).permutation(n)
    sp, tp = ia.inp("scores permuted", torch.from_numpy(s[perm])), ia.inp("targets permuted", torch.from_numpy(y[perm]))

    # ---- average precision ----
    out = twice(rid, _launch_ap(rid, dev, sd, td, n))["out"]
    assert not any(_poisoned(out[i:i + 1]) for i in range(3)), f"{rid}: an element of `out` left unwritten"
    assert _same_bits(out, _launch_ap(rid, dev, sp, tp, n)()["out"]), f"{rid}: the permuted input gives other bits"
    ap, P, m = out.cpu().tolist()
    bar = (ref.m + 4) * 2.0 ** -52 * ref.ap
    ratio = abs(ap - ref.ap) / bar if bar else (0.0 if ap == ref.ap else float("inf"))
    WORST["AP err / bar"] = max(WORST["AP err / bar"], ratio)
    print(f"   {rid}: AP {ap!r}, reference {ref.ap!r}, err / bar {ratio:.3e}; P {P}, m {m}", flush=True)
    assert P == ref.P and m == ref.m, f"{rid}: (P, m) = ({P}, {m}), reference ({ref.P}, {ref.m})"
    assert abs(ap - ref.ap) <= bar, f"{rid}: AP {ap!r} outside (m + 4) 2^-52 of {ref.ap!r} (ratio {ratio:.3f})"
    if ref.P == 0:
        assert ap == 0.0 and not np.signbit(ap), f"{rid}: no positive, AP {ap!r} is not 0.0"
    assert metrics.average_precision_gpu(td, sd) == ap, f"{rid}: metrics.average_precision_gpu differs from the direct call"

    # ---- precision-recall curve ----
    o = twice(rid, _launch_pr(rid, dev, sd, td, n))
    o2 = _launch_pr(rid, dev, sp, tp, n)()
    count = int(o["count"].item())
    assert count == ref.m, f"{rid}: count {count}, the reference has {ref.m} thresholds"
    for nm in ("precision", "recall", "thresholds"):
        assert _poisoned(o[nm][count:]), f"{rid}: `{nm}` written past count"
        assert _same_bits(o[nm][:count], o2[nm][:count]), f"{rid}: the permuted input gives other bits in `{nm}`"
    assert int(o2["count"].item()) == count
    gp, gr, gt = o["precision"][:count].cpu().numpy(), o["recall"][:count].cpu().numpy(), o["thresholds"][:count].cpu().numpy()
    assert np.array_equal(gt.view(np.uint32), ref.thresholds.view(np.uint32)), f"{rid}: thresholds differ at {int(np.argmax(gt.view(np.uint32) != ref.thresholds.view(np.uint32)))}"
    if ref.P:
        tp_implied = np.rint(gr * ref.P).astype(np.int64)
        assert np.array_equal(tp_implied, ref.tp), f"{rid}: TP_j implied by recall differ from the reference's"
    else:
        assert bool((gr == 1.0).all()), f"{rid}: no positive, recall is not 1 everywhere"
    has = ref.tp > 0
    assert bool((gp[~has] == 0.0).all()), f"{rid}: precision is not 0.0 where TP_j = 0"
    assert np.array_equal(np.rint(ref.tp[has] / gp[has]).astype(np.int64), ref.n[has]), f"{rid}: N_j implied by precision differ"
    up, ur = float(ap_ref.ulps(gp, ref.precision).max()), float(ap_ref.ulps(gr, ref.recall).max())
    WORST["precision ulp"], WORST["recall ulp"] = max(WORST["precision ulp"], up), max(WORST["recall ulp"], ur)
    print(f"   {rid}: {count} points; precision within {up:.2f} ulp, recall within {ur:.2f} ulp", flush=True)
    assert up <= 1 and ur <= 1, f"{rid}: precision / recall off by {up} / {ur} ulp"
    wp, wr, wt = metrics.pr_curve_gpu(td, sd)
    assert wp.is_cuda and wp.dtype == torch.float64 and wt.dtype == torch.float32 and wp.numel() == count + 1 and wt.numel() == count
    assert _same_bits(wp[:-1].flip(0), o["precision"][:count]) and _same_bits(wr[:-1].flip(0), o["recall"][:count])
    assert _same_bits(wt.flip(0), o["thresholds"][:count]) and (float(wp[-1]), float(wr[-1])) == (1.0, 0.0)
    ia.check_inputs(rid)


@pytest.mark.parametrize("n,sp,tp", ROWS, ids=[f"{n}_{sp}_{tp}" for n, sp, tp in ROWS])
def test_row_against_the_float64_reference(dev, n, sp, tp):
    s, y = _big_case(n) if n > (1 << 22) else make_case(n, sp, tp)
    run_row(f"{n}_{sp}_{tp}", s, y, dev)


def test_argument_errors_return_2_over_untouched_outputs(dev):
    hip, lib, st = _lib()
    n = 300
    ia = InArena(dev)
    sd, td = ia.inp("scores", torch.rand(n)), ia.inp("targets", (torch.rand(n) < 0.5).to(torch.uint8))
    need = {"ap": lib.ssad_average_precision_workspace(n), "pr": lib.ssad_pr_curve_workspace(n)}
    assert need["ap"] > need["pr"] > 0
    for bad in (0, -1, (1 << 31) - 1):
        assert lib.ssad_average_precision_workspace(bad) == -1 and lib.ssad_pr_curve_workspace(bad) == -1
    for entry in ("ap", "pr"):
        ar = Arena(dev)
        ws = ar.out("workspace", (need[entry] + 8,), torch.uint8, all_written=False)
        if entry == "ap":
            outs = [ar.out("out", (3,), torch.float64, all_written=False)]
            call = lambda s_, t_, n_, w_, b_, o_: lib.ssad_average_precision(s_, t_, n_, w_, b_, o_[0], st)
        else:
            outs = [ar.out("precision", (n,), torch.float64, all_written=False), ar.out("recall", (n,), torch.float64, all_written=False),
                    ar.out("thresholds", (n,), torch.float32, all_written=False), ar.out("count", (1,), torch.int64, all_written=False)]
            call = lambda s_, t_, n_, w_, b_, o_: lib.ssad_pr_curve(s_, t_, n_, w_, b_, *o_, st)
        good = [_p(sd), _p(td), n, _p(ws), need[entry], [_p(o) for o in outs]]
        cases = {"null scores": (0, None), "null targets": (1, None), "n = 0": (2, 0), "n < 0": (2, -5), "null workspace": (3, None),
                 "workspace one byte short": (4, need[entry] - 1), "workspace misaligned": (3, _p(ws) + 4)}
        for k in range(len(outs)):
            cases[f"null output {k}"] = (5, [None if j == k else p for j, p in enumerate(good[5])])
        for what, (at, value) in cases.items():
            args = list(good)
            args[at] = value
            rc = call(*args)
            msg = lib.ssad_last_error().decode()
            assert rc == 2, f"{entry}: {what}: return code {rc}"
            assert ("ssad_average_precision" if entry == "ap" else "ssad_pr_curve") in msg, f"{entry}: {what}: message {msg!r}"
            if "short" in what:
                assert "_workspace" in msg, msg
            ar.check_outputs(f"{entry}: {what}")
            assert all(_poisoned(o) for o in outs) and _poisoned(ws), f"{entry}: {what}: a refused call wrote"
    ia.check_inputs("argument errors")


def test_wrappers_refuse_nan_and_empty_inputs(dev):
    from self_supervised import metrics as m
    for fn in (m.average_precision_gpu, m.pr_curve_gpu):
        with pytest.raises(ValueError, match="NaN"):
            fn(torch.tensor([1, 0, 1], device=dev), torch.tensor([0.5, float("nan"), 0.1], device=dev))
        with pytest.raises(ValueError):
            fn(torch.zeros(0, device=dev), torch.zeros(0, device=dev))


# ---- the layers above: one inference + upsample run on the synthetic category ----
@pytest.fixture(scope="module")
def run(tmp_path_factory, seeded_sd, dev):
    from self_supervised import tools, datasets
    datasets._DataModule.num_workers = 0
    tmp = tmp_path_factory.mktemp("ap")
    root = make_tree(str(tmp / "data"), categories=("bottle",), n_train=3, n_test_good=2, n_test_bad=2, size=96)
    os.makedirs(tmp / "out" / "bottle")
    ck = str(tmp / "out" / "bottle" / "best_model.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    np.random.seed(3)
    torch.manual_seed(3)
    res = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, image_scores="max", neighbours=3)
    res.anomaly_maps = tools.upsample(res.anomaly_maps, int(res.ground_truths.shape[-1]), verbose=False)
    assert res.anomaly_maps.is_cuda
    return {"res": res, "root": root, "out": str(tmp / "out") + "/", "tmp": tmp}


def _sklearn_bar(s, y):
    ref = ap_ref.ap_ref(s, y)
    return 2.0 ** -52 * ((ref.m + 4) * ref.ap + float(np.sum(ref.precision * ref.recall)))       # derived in tests/test_ap_host.py


def test_average_precision_of_device_maps_equals_sklearn_and_the_evaluator_reports_it(run):
    from sklearn.metrics import average_precision_score
    from self_supervised import metrics as m, tools
    res = run["res"]
    s = res.anomaly_maps.reshape(-1).cpu().numpy()
    y = (res.ground_truths.reshape(-1).cpu().numpy() > 0)
    assert y.any() and not y.all()
    got = m.average_precision_gpu(res.ground_truths.reshape(-1), res.anomaly_maps.reshape(-1))
    want = average_precision_score(y, s)
    print(f"   pixel AP {got!r}, sklearn {want!r}", flush=True)
    assert abs(got - want) <= _sklearn_bar(s, y)
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou', 'ap'])
    ev.evaluate(res, "bottle", "", patch_level=True)
    assert ev.scores.AP == got
    frame = m.metrics_to_dataframe({k: [v] for k, v in vars(ev.scores).items() if v is not None}, ["bottle"])
    assert list(frame.columns) == ["auroc", "aupro", "iou", "AP"] and frame.loc["bottle", "AP"] == got
    plain = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou'])
    plain.evaluate(res, "bottle", "", patch_level=True)
    assert list(vars(plain.scores)) == ["auroc", "f1_score", "aupro", "iou"]
    assert {k: v for k, v in vars(ev.scores).items() if k != "AP"} == vars(plain.scores)
    # image level, beside image_auroc
    si, yi = res.image_scores.reshape(-1).cpu().numpy(), np.asarray(res.y_true_binary_labels.cpu()) > 0
    host = tools.image_ap(res)                                     # inference hands the image scores back on the host
    assert abs(host - average_precision_score(yi, si)) <= _sklearn_bar(si, yi)
    res.image_scores = res.image_scores.cuda()
    try:
        assert abs(tools.image_ap(res) - host) <= (len(si) + 4) * 2.0 ** -52 * host
    finally:
        res.image_scores = res.image_scores.cpu()


def test_sweep_writes_the_ap_table_and_leaves_the_others_alone(run):
    import pandas as pd
    from self_supervised import metrics as m, tools
    tables, frames = {}, {}
    for name, kw in (("plain", {}), ("ap", {"average_precision": True})):
        np.random.seed(3)
        torch.manual_seed(3)
        tables[name] = str(run["tmp"] / ("tables_" + name)) + "/"
        frames[name] = tools.sweep(run["root"], run["out"], ["bottle"], train=False, image_scores="max", neighbours=3,
                                   tables_output=tables[name], **kw)
    assert frames["plain"].equals(frames["ap"]) and "AP" not in frames["ap"].columns
    plain = sorted(os.listdir(tables["plain"] + "csv/"))
    assert sorted(os.listdir(tables["ap"] + "csv/")) == sorted(plain + ["patch_ap.csv"])
    for f in plain:
        assert open(tables["plain"] + "csv/" + f, "rb").read() == open(tables["ap"] + "csv/" + f, "rb").read(), f
    t = pd.read_csv(tables["ap"] + "csv/patch_ap.csv", index_col=0)
    assert list(t.index) == ["bottle", "average"] and list(t.columns) == ["pixel_ap", "image_ap"]
    res = run["res"]
    want = m.average_precision_gpu(res.ground_truths.reshape(-1), res.anomaly_maps.reshape(-1))
    assert abs(t.loc["bottle", "pixel_ap"] - want) <= 0.0051 and t.loc["average", "pixel_ap"] == t.loc["bottle", "pixel_ap"]     # two decimals
    assert abs(t.loc["bottle", "image_ap"] - tools.image_ap(res)) <= 0.0051
