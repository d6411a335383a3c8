"""CPU tests of the refined search (AnomalyDetector(bank_dtype='float16' | 'int8', refine=r); csrc/knn_refine.hip): check_refine's
accepted and refused combinations with their messages, the option's way from tools.inference / tools.sweep to the detector, a state
round trip with and without the option, knn_search.choose with four and five arguments, the ops' argument checks on host tensors, the
header / _hip.SIGNATURES agreement for the new entry points, and -- on the reference alone -- the share of the GPU test's seeded
Gaussian case that the index comparison leaves out."""
import os
import re

import numpy as np
import pytest
import torch

import knn_refine_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssad_rerank_l2_index", "ssad_rerank_l2", "ssad_topk_l2q_index")


def test_check_refine_accepts():
    from self_supervised.models import check_refine
    assert check_refine(None) is None and check_refine(None, 'float32', 32) is None and check_refine(None, 'int8', 3) is None
    for dt in ('float16', 'int8'):
        for r in (4, 5, 16, 32, np.int64(8)):
            for k in (1, 2, 3):
                got = check_refine(r, dt, k)
                assert got == int(r) and type(got) is int
    for k in (4, 16):
        assert check_refine(16, 'float16', k) == 16
    assert check_refine(32, 'float16', 32) == 32


REFUSED = [
    (dict(refine=3, bank_dtype='int8'), "refine must be None or an int in 4..32 (the length of the shortlist), got 3"),
    (dict(refine=33, bank_dtype='int8'), "refine must be None or an int in 4..32 (the length of the shortlist), got 33"),
    (dict(refine=0, bank_dtype='float16'), "refine must be None or an int in 4..32 (the length of the shortlist), got 0"),
    (dict(refine=True, bank_dtype='float16'), "refine must be None or an int in 4..32 (the length of the shortlist), got True"),
    (dict(refine=8.0, bank_dtype='float16'), "refine must be None or an int in 4..32 (the length of the shortlist), got 8.0"),
    (dict(refine='8', bank_dtype='float16'), "refine must be None or an int in 4..32 (the length of the shortlist), got '8'"),
    (dict(refine=8, bank_dtype='float32'),
     "refine=8 needs bank_dtype 'float16' or 'int8' (it ranks a compressed bank's shortlist again on the fp32 rows; the fp32 bank is "
     "searched exactly already), got bank_dtype='float32'"),
    (dict(refine=8, bank_dtype='float16', n_neighbors=9),
     "refine=8 must be at least n_neighbors=9: the k nearest are taken from the shortlist"),
]


@pytest.mark.parametrize("kw,msg", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_check_refine_refuses(kw, msg):
    from self_supervised.models import check_refine
    with pytest.raises(ValueError) as e:
        check_refine(**kw)
    assert str(e.value) == msg


def test_detector_option_and_the_refusals_that_stay():
    from self_supervised.models import AnomalyDetector
    det = AnomalyDetector(metric='euclidean', bank_dtype='int8', refine=8)
    assert det.refine == 8 and det.bank_f32 is None and det.quant is None
    assert AnomalyDetector(metric='euclidean', bank_dtype='float16', refine=16, n_neighbors=16).refine == 16
    plain = AnomalyDetector(metric='euclidean', bank_dtype='int8')
    assert plain.refine is None and "bank_f32" not in vars(plain) and "bank_f32" not in vars(AnomalyDetector())
    with pytest.raises(ValueError, match="needs bank_dtype 'float16' or 'int8'"):
        AnomalyDetector(metric='euclidean', refine=8)
    with pytest.raises(ValueError, match="needs bank_dtype 'float16' or 'int8'"):
        AnomalyDetector(refine=8)
    with pytest.raises(ValueError, match="must be at least n_neighbors=9"):
        AnomalyDetector(metric='euclidean', bank_dtype='float16', n_neighbors=9, refine=8)
    # what the compressed banks refuse stays refused, with the messages other tests pin
    with pytest.raises(ValueError, match="supports n_neighbors in 1..3"):
        AnomalyDetector(metric='euclidean', bank_dtype='int8', n_neighbors=4, refine=8)
    with pytest.raises(ValueError, match="bank_dtype='int8' needs index='flat'"):
        AnomalyDetector(metric='euclidean', index='ivf', bank_dtype='int8', refine=8)
    with pytest.raises(ValueError, match="bank_dtype='float16' needs metric='euclidean'"):
        AnomalyDetector(bank_dtype='float16', refine=8)
    det.patch_level, det.dim = True, 2
    det.bank = torch.zeros((4, 32), dtype=torch.int8)
    with pytest.raises(ValueError, match="takes image_scores None or 'max'"):
        det._check_image_scores('reweighted', 9)


def test_choose_with_four_and_five_arguments():
    from self_supervised import knn_search as ks
    assert type(ks.choose('euclidean', 'flat', None, 'int8')) is ks.FlatL2Int8
    assert type(ks.choose('euclidean', 'flat', None, 'float16')) is ks.FlatL2Half
    assert type(ks.choose('euclidean', 'flat', None, 'float16', None)) is ks.FlatL2Half
    assert type(ks.choose('euclidean', 'flat', None, 'float16', 8)) is ks.RefinedHalf
    assert type(ks.choose('euclidean', 'flat', None, 'int8', 32)) is ks.RefinedInt8
    assert isinstance(ks.choose('euclidean', 'flat', None, 'int8', 32), ks.FlatL2Int8)
    assert type(ks.choose('cosine', 'flat', None, 'float32')) is ks.Cosine and type(ks.choose('euclidean', 'ivf', None, 'float32')) is ks.IVF


def test_state_round_trip_with_and_without_the_option():
    from self_supervised.models import AnomalyDetector
    det = AnomalyDetector(metric='euclidean', bank_dtype='int8', refine=8)
    det.bank = torch.zeros((4, 32), dtype=torch.int8)
    det.bank_sq = torch.zeros(4, dtype=torch.int32)
    det.quant = (-1.0, 0.5)
    det.bank_f32 = torch.arange(128, dtype=torch.float32).reshape(4, 32)
    state = det.state()
    assert state["refine"] == 8 and torch.equal(state["bank_f32"], det.bank_f32) and state["bank_dtype"] == 'int8'
    assert set(state) == {"metric", "bank", "bank_dtype", "bank_sq", "lo", "s", "refine", "bank_f32"}
    plain = AnomalyDetector(metric='euclidean', bank_dtype='int8')
    plain.bank, plain.bank_sq, plain.quant = det.bank, det.bank_sq, det.quant
    assert set(plain.state()) == {"metric", "bank", "bank_dtype", "bank_sq", "lo", "s"}
    half = AnomalyDetector(metric='euclidean', bank_dtype='float16')
    half.bank = torch.zeros((4, 32), dtype=torch.float16)
    assert set(half.state()) == {"metric", "bank", "bank_dtype"}
    with pytest.raises(ValueError, match="fitted with refine=8, this detector has None"):
        plain.load_state(state)
    with pytest.raises(ValueError, match="fitted with refine=None, this detector has 8"):
        det.load_state(plain.state())
    with pytest.raises(ValueError, match="fitted with refine=8, this detector has 16"):
        AnomalyDetector(metric='euclidean', bank_dtype='int8', refine=16).load_state(state)
    other = AnomalyDetector(metric='euclidean', bank_dtype='int8', refine=8)
    if torch.cuda.is_available():
        other.load_state(state)
        assert torch.equal(other.bank_f32.cpu(), det.bank_f32) and torch.equal(other.bank.cpu(), det.bank) and other.quant == det.quant
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # past every check: only the device is missing
            other.load_state(state)


def test_tools_pass_the_option_through(tmp_path):
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector
    cls, kw = tools._check_options('knn', 'euclidean', 'dense', True, 'train', True, 0.5, 'max', 9, None, bank_dtype='int8', refine=8)
    assert cls is AnomalyDetector and kw == {"coreset": 0.5, "metric": 'euclidean', "bank_dtype": 'int8', "refine": 8}
    assert AnomalyDetector(**kw).refine == 8
    cls, kw = tools._check_options('knn', 'euclidean', 'patches', False, 'reference', False, None, None, 9, None, bank_dtype='float16',
                                   n_neighbors=5, refine=16)
    assert kw == {"metric": 'euclidean', "bank_dtype": 'float16', "n_neighbors": 5, "refine": 16}
    cls, kw = tools._check_options('knn', 'euclidean', 'patches', False, 'reference', False, None, None, 9, None, bank_dtype='int8')
    assert kw == {"metric": 'euclidean', "bank_dtype": 'int8'}                  # without the option nothing of it is passed
    missing = str(tmp_path / "nothing_here")
    for kw, match in [(dict(detector='gde', refine=8), "refine=8 applies to detector='knn' only, got detector='gde'"),
                      (dict(metric='euclidean', refine=8), "needs bank_dtype 'float16' or 'int8'"),
                      (dict(metric='euclidean', bank_dtype='int8', refine=2), "refine must be None or an int in 4..32"),
                      (dict(metric='euclidean', bank_dtype='float16', n_neighbors=12, refine=8), "must be at least n_neighbors=12")]:
        with pytest.raises(ValueError, match=match):
            tools.inference(missing + "/model.ckpt", missing + "/", "bottle", **kw)
        with pytest.raises(ValueError, match=match):
            tools.sweep(missing + "/", missing + "/out/", ["bottle"], **{"patch_localization": False, **kw})


def test_ops_argument_errors_come_before_any_launch_and_there_is_no_cpu_fallback():
    from self_supervised import _hip, ops
    x, bank = ref.gauss(5, 48, 1), ref.gauss(7, 48, 2)
    cand = torch.zeros((5, 8), dtype=torch.int32)
    for fn in (ops.l2_rerank_index, ops.l2_rerank_mean):
        with pytest.raises(ValueError, match="must be float32 of one width"):
            fn(x, bank[:, :32].contiguous(), cand, 3)
        with pytest.raises(ValueError, match="must be float32 of one width"):
            fn(x.half(), bank, cand, 3)
        with pytest.raises(ValueError, match=r"cand must be int32 \[5\]\[r\]"):
            fn(x, bank, cand.long(), 3)
        with pytest.raises(ValueError, match=r"cand must be int32 \[5\]\[r\]"):
            fn(x, bank, cand[:4], 3)
        with pytest.raises(ValueError, match="a shortlist holds 1..32 rows, got r = 33"):
            fn(x, bank, torch.zeros((5, 33), dtype=torch.int32), 3)
        with pytest.raises(ValueError, match="a shortlist holds 1..32 rows, got r = 0"):
            fn(x, bank, torch.zeros((5, 0), dtype=torch.int32), 1)
        for k in (0, 9):
            with pytest.raises(ValueError, match="k must lie in 1..r = 1..8"):
                fn(x, bank, cand, k)
        with pytest.raises(_hip.HipExtensionError):
            fn(x, bank, cand, 3)
    xq, bank_q, bsq = ref.gauss(5, 64, 1), torch.zeros((9, 64), dtype=torch.int8), torch.zeros(9, dtype=torch.int32)
    quant = (-1.0, 0.01)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.l2q_topk_index(xq[:, :48].contiguous(), bank_q[:, :48].contiguous(), bsq, quant, 4)
    with pytest.raises(ValueError, match="at most 32768"):
        ops.l2q_topk_index(torch.zeros((1, 32768 + 32)), torch.zeros((9, 32768 + 32), dtype=torch.int8), bsq, quant, 4)
    for k in (3, 33):
        with pytest.raises(ValueError, match="k must lie in 4..32"):
            ops.l2q_topk_index(xq, bank_q, bsq, quant, k)
    with pytest.raises(ValueError, match="fewer than k"):
        ops.l2q_topk_index(xq, bank_q, bsq, quant, 10)
    with pytest.raises(ValueError, match="int8 codes"):
        ops.l2q_topk_index(xq, bank_q.float(), bsq, quant, 4)
    with pytest.raises(ValueError, match="splits must be >= 1"):
        ops.l2q_topk_index(xq, bank_q, bsq, quant, 4, splits=0)
    with pytest.raises(ValueError, match="finite"):
        ops.l2q_topk_index(xq, bank_q, bsq, (float("inf"), 0.01), 4)
    with pytest.raises(ValueError, match="finite and positive"):
        ops.l2q_topk_index(xq, bank_q, bsq, (0.0, -1.0), 4)
    with pytest.raises(_hip.HipExtensionError):
        ops.l2q_topk_index(xq, bank_q, bsq, quant, 4)
    with pytest.raises(ValueError, match="k must be 1, 2 or 3"):            # the k <= 3 function keeps its check
        ops.l2q_knn_index(xq, bank_q, bsq, quant, k=4)


def test_header_signatures_and_sources_agree():
    from self_supervised import _hip
    header = open(os.path.join(ROOT, "include", "ssad.h")).read()
    src = open(os.path.join(ROOT, "self-supervised-anomaly-detection_amd", "csrc", "knn_refine.hip")).read()
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert len(_hip.SIGNATURES[name]) == len(args), name
        for a, ct in zip(args, _hip.SIGNATURES[name]):
            assert (ct is _hip._c_f) == a.startswith("float "), (name, a)
            assert (ct is _hip._c_l) == a.startswith("int64_t "), (name, a)
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
    assert "atomic" not in src.replace("No atomics", "")


def test_reference_rerank_on_a_case_done_by_hand():
    x = torch.tensor([[0.0, 0.0]])
    bank = torch.tensor([[3.0, 4.0], [1.0, 0.0], [1.0, 0.0], [0.0, 2.0]])
    cand = torch.tensor([[3, 7, 2, 0, -1, 1, 2]], dtype=torch.int32)
    dist, idx = ref.rerank(x, bank, cand, 6)
    assert idx.tolist() == [[1, 2, 2, 3, 0, -1]]            # equal d2: the smaller row, then the earlier place; skipped: 7 and -1
    assert dist.tolist() == [[1.0, 1.0, 1.0, 2.0, 5.0, np.inf]]
    assert ref.mean_of(dist[:, :5], 5).tolist() == [2.0]


def test_the_left_out_share_of_the_gaussian_case_is_small():
    """The GPU test compares the device's order with float64's on the queries that have no two listed rows closer than twice the
    bar; this is the share of adjacent pairs that are, and of queries dropped, on the reference alone."""
    x, bank, cand = ref.gauss_case()
    units = ref.bar_units(ref.GAUSS_CASE["d"])
    dropped, close, pairs = ref.near_ties(x, bank, cand, units)
    assert all(len(set(row)) == len(row) for row in cand.tolist())         # no list names a row twice
    share = close / pairs
    print(f"adjacent pairs under twice the bar ({units} units): {close} of {pairs}, share {share:.2e}; queries with such a pair "
          f"{int(dropped.sum())} of {len(dropped)}")
    assert pairs == ref.GAUSS_CASE["n"] * (ref.GAUSS_CASE["r"] - 1)
    assert share <= ref.LEFT_OUT_CAP and dropped.mean() <= ref.LEFT_OUT_CAP
