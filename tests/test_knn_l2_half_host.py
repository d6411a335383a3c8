"""CPU tests of the half-precision flat Euclidean search: the reference's rounding h (tests/knn_l2_half_ref.py) against torch's
.half() and on the special values, the operand-rounding model on the reference alone, every argument error of bank_dtype before any
path is touched, the header / _hip.SIGNATURES agreement for the new entry points, and the unchanged default detector."""
import os
import re

import numpy as np
import pytest
import torch

import knn_l2_half_ref as href
import knn_l2_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssad_rows_to_half", "ssad_l2h_knn_fused", "ssad_l2h_knn_index")


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


def bits(a):
    return np.asarray(a, dtype=np.float16).view(np.uint16)


def test_h_equals_torch_half_where_torch_neither_overflows_nor_denormalises():
    for scale in (1.0, 100.0, 1e-2):
        x = gauss(400, 96, seed=1) * scale
        want = x.half().numpy()
        keep = np.isfinite(want) & (np.abs(want.astype(np.float32)) >= 2.0 ** -14)
        assert keep.mean() > 0.9
        assert np.array_equal(bits(href.h(x))[keep], bits(want)[keep])
    small = gauss(400, 96, seed=2) * 1e-4                           # many results below 2^-14: torch keeps subnormals, h flushes
    got, want = href.h(small), small.half().numpy()
    sub = np.abs(want.astype(np.float32)) < 2.0 ** -14
    assert 0.05 < sub.mean() < 0.95
    assert np.array_equal(bits(got)[~sub], bits(want)[~sub])
    assert (got[sub] == 0).all() and np.array_equal(np.signbit(got[sub]), np.signbit(small.numpy()[sub]))


def test_h_saturates_flushes_and_rounds_ties_to_even():
    f = lambda *v: href.h(np.array(v, dtype=np.float32))
    big = f(65504.0, -65504.0, 1e6, -1e6, 65519.0, 65520.0, -65520.0, 3e38, -3e38)
    assert np.array_equal(bits(big), bits([65504.0, -65504.0] + [65504.0, -65504.0] + [65504.0, 65504.0, -65504.0, 65504.0, -65504.0]))
    assert np.isfinite(big.astype(np.float32)).all()
    tiny = f(2.0 ** -15, -2.0 ** -15, 6e-8, -6e-8, 0.0, -0.0, 2.0 ** -14, -2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12))
    assert np.array_equal(bits(tiny), np.array([0x0000, 0x8000, 0x0000, 0x8000, 0x0000, 0x8000, 0x0400, 0x8400, 0x0400], dtype=np.uint16))
    # ties: 1 + 2^-11 lies halfway between 1 and 1 + 2^-10 -> even (1); 1 + 3 2^-11 halfway between 1 + 2^-10 and 1 + 2^-9 -> even (1 + 2^-9)
    ties = f(1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2048.0 + 1.0, 2048.0 + 3.0, 1 + 2.0 ** -11 + 2.0 ** -20)
    assert np.array_equal(ties.astype(np.float64), [1.0, 1 + 2.0 ** -9, -1.0, 2048.0, 2052.0, 1 + 2.0 ** -10])
    assert not np.isnan(href.h(gauss(50, 32, 3) * 1e5).astype(np.float32)).any()


@pytest.mark.parametrize("d,mean", [(32, 0.0), (384, 0.0), (384, 10.0)])
def test_operand_rounding_model_on_the_reference(d, mean):
    """Each element carries a relative error of at most u = 2^-11 after h (in-range values), so each product q_i b_i -- and each
    square -- moves by at most (2 u + u^2) |q_i| |b_i|; summed over the three sums of the expanded form:
    |d2(h q, h b) - d2(q, b)| <= (2^-10 + 2^-22) A <= (2^-10 + 2^-20) A with A on the unrounded rows.  (max(., 0) is 1-Lipschitz.)"""
    x, bank = gauss(200, d, seed=5, mean=mean), gauss(300, d, seed=6, mean=mean)
    # in-range rows: the few elements of a Gaussian sample below 2^-13 (h would flush those below 2^-14) are set to 2^-10
    x = torch.where(x.abs() < 2.0 ** -13, torch.full_like(x, 2.0 ** -10), x)
    bank = torch.where(bank.abs() < 2.0 ** -13, torch.full_like(bank, 2.0 ** -10), bank)
    assert float(max(x.abs().max(), bank.abs().max())) < 65504
    a = ref.scale_a(x, bank)
    err = np.abs(href.d2_64(x, bank) - ref.d2_64(x, bank))
    ratio = (err / ((2.0 ** -10 + 2.0 ** -20) * a)).max()
    print(f"D={d} mean={mean}: worst |d2_half_ref - d2_ref| / ((2^-10 + 2^-20) A) = {ratio:.4f}")
    assert ratio <= 1.0


BAD = [({"bank_dtype": 'bfloat16', "metric": 'euclidean'}, "bank_dtype must be one of"),
       ({"bank_dtype": 'float16'}, "bank_dtype='float16' needs metric='euclidean'"),
       ({"bank_dtype": 'float16', "metric": 'euclidean', "detector": 'gde'}, "applies to detector='knn' only"),
       ({"bank_dtype": 'float16', "metric": 'euclidean', "index": 'ivf'}, "bank_dtype='float16' needs index='flat'"),
       ({"bank_dtype": 'float16', "metric": 'euclidean', "gallery": 2, "patch_localization": True, "bank": 'train'},
        "bank_dtype='float16' needs gallery=None"),
       ({"bank_dtype": 'float16', "metric": 'euclidean', "patch_localization": True, "image_scores": 'reweighted'},
        "takes image_scores None or 'max'")]


@pytest.mark.parametrize("kw,match", BAD, ids=[m[:24] for _, m in BAD])
def test_bank_dtype_argument_errors_come_before_any_file_is_read(tmp_path, kw, match):
    from self_supervised import tools
    missing = str(tmp_path / "nothing_here")
    with pytest.raises(ValueError, match=match):
        tools.inference(missing + "/model.ckpt", missing + "/", "bottle", **kw)
    with pytest.raises(ValueError, match=match):
        tools.sweep(missing + "/", missing + "/out/", ["bottle"], **{"patch_localization": False, **kw})


def test_detector_argument_errors_without_a_gpu():
    from self_supervised.models import AnomalyDetector, check_bank_dtype
    with pytest.raises(ValueError, match="bank_dtype must be one of"):
        AnomalyDetector(metric='euclidean', bank_dtype='half')
    with pytest.raises(ValueError, match="needs metric='euclidean'"):
        AnomalyDetector(bank_dtype='float16')
    with pytest.raises(ValueError, match="needs index='flat'"):
        AnomalyDetector(metric='euclidean', index='ivf', bank_dtype='float16')
    with pytest.raises(ValueError, match="needs gallery=None"):
        AnomalyDetector(patch_level=True, batch=1, num_patches=4, metric='euclidean', gallery=2, bank_dtype='float16')
    assert check_bank_dtype('float32', 'cosine', 'ivf', 3, 'reweighted') == 'float32'       # the default asks for nothing
    assert check_bank_dtype('float16', image_scores='max') == 'float16'
    det = AnomalyDetector(patch_level=True, batch=1, num_patches=4, metric='euclidean', bank_dtype='float16')
    det.bank = torch.zeros((4, 32), dtype=torch.float16)
    with pytest.raises(ValueError, match="takes image_scores None or 'max'"):
        det._check_image_scores('reweighted', 9)
    det._check_image_scores('max', 9)
    assert det.state()["bank_dtype"] == 'float16' and det.state()["bank"].dtype == torch.float16
    with pytest.raises(ValueError, match="fitted with bank_dtype='float16'"):
        AnomalyDetector(metric='euclidean').load_state(det.state())
    with pytest.raises(ValueError, match="fitted with bank_dtype='float32'"):
        det.load_state({"metric": 'euclidean', "bank": torch.zeros((4, 32))})


def test_ops_argument_errors_come_before_any_launch():
    """Host tensors: a launch would raise HipExtensionError, these must raise ValueError first."""
    from self_supervised import ops
    x, bank_h, bsq = gauss(5, 64, 1), gauss(4, 64, 2).half(), torch.zeros(4)
    for fn in (ops.l2h_knn_fused, ops.l2h_knn_index):
        with pytest.raises(ValueError, match="multiple of 32"):
            fn(x[:, :48].contiguous(), bank_h[:, :48].contiguous(), bsq)
        with pytest.raises(ValueError, match="k must be 1, 2 or 3"):
            fn(x, bank_h, bsq, k=4)
        with pytest.raises(ValueError, match="fewer than k"):
            fn(x, bank_h[:2], bsq[:2], k=3)
        with pytest.raises(ValueError, match="float16 rows"):
            fn(x, bank_h.float(), bsq)
        with pytest.raises(ValueError, match="splits must be >= 1"):
            fn(x, bank_h, bsq, splits=0)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.rows_to_half(x[:, :48].contiguous())


def test_header_and_signatures_agree_on_the_new_entry_points():
    from self_supervised import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssad.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/ssad.h"
        assert name in _hip.SIGNATURES, name
        assert len(_hip.SIGNATURES[name]) == len(m.group(1).split(",")), name
    src = open(os.path.join(ROOT, "self-supervised-anomaly-detection_amd", "csrc", "knn_l2_half.hip")).read()
    for name in NEW:
        assert re.search(r'extern "C" int ' + name + r"\(", src), name


TODAY = {"patch_level": False, "batch": None, "dim": None, "threshold": None, "k": 3, "bank": None, "bank_sq": None, "metric": 'cosine',
         "coreset": None, "coreset_dim": 128, "coreset_rows": None, "coreset_counts": None, "gallery": None, "bank_desc": None,
         "index": 'flat', "nlist": None, "nprobe": 8, "index_options": {}, "ivf": None}


def test_default_bank_dtype_leaves_the_detector_as_it_was():
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector
    for kw in ({}, {"metric": 'euclidean', "coreset": 0.5}, {"patch_level": True, "batch": 2, "num_patches": 25}):
        a, b = vars(AnomalyDetector(**kw)), vars(AnomalyDetector(bank_dtype='float32', **kw))
        assert a == b and a["bank_dtype"] == 'float32'
    plain = vars(AnomalyDetector())
    assert {k: plain[k] for k in TODAY} == TODAY and set(plain) - set(TODAY) == {"bank_dtype", "_search"}     # (_search: no data)
    cls, kw = tools._check_options('knn', 'euclidean', 'patches', True, 'train', True, None, None, 9, None)
    assert "bank_dtype" not in kw
    cls, kw = tools._check_options('knn', 'euclidean', 'dense', True, 'train', True, 0.1, 'max', 9, None, bank_dtype='float16')
    assert cls is AnomalyDetector and kw == {"coreset": 0.1, "metric": 'euclidean', "bank_dtype": 'float16'}
