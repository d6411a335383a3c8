"""CPU tests of the flat Euclidean search on an 8-bit scalar-quantised bank: the reference (tests/knn_l2_int8_ref.py) against itself
(the expanded integer form, the special values of the code), the error bound of the quantiser on the reference alone, every argument
error of bank_dtype='int8' before any path is touched, state() / load_state, the header / _hip.SIGNATURES agreement for the new entry
points, and the ops' refusal to run on host tensors."""
import os
import re

import numpy as np
import pytest
import torch

import knn_l2_int8_ref as qref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssad_rows_to_int8", "ssad_l2q_knn_fused", "ssad_l2q_knn_index")
F = np.float32


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


def test_reference_codes_on_the_special_values():
    lo, s, inv_s, s2 = qref.quantiser(-1.0, 1.55)           # s = 0.01 (rounded to fp32)
    assert s == F(2.55 / 255.0) and inv_s == F(1.0 / float(s)) and s2 == F(float(s) * float(s))
    x = np.array([[-1.0, 1.55, -5.0, 9.0, np.nan, np.inf, -np.inf, -1.0 + 0.5 * 0.01, 0.0]], dtype=F)
    c = qref.codes(x, lo, inv_s)[0]
    assert c.dtype == np.int8
    assert list(c[:7]) == [-128, 127, -128, 127, -128, 127, -128]
    assert c[8] == int(np.rint((F(0.0) - lo) * inv_s)) - 128
    # ties go to the even code: with lo = 0 and s = 1 the values k + 0.5 are exact
    lo, s, inv_s, _ = qref.quantiser(0.0, 255.0)
    assert s == 1 and inv_s == 1
    ties = np.array([[0.5, 1.5, 2.5, 253.5, 254.5, 255.5, 0.49999997, 1.5000001]], dtype=F)
    assert list(qref.codes(ties, lo, inv_s)[0].astype(int) + 128) == [0, 2, 2, 254, 254, 255, 0, 2]
    # hi == lo: s = 1, every bank element is code -128
    lo, s, inv_s, _ = qref.quantiser(3.25, 3.25)
    assert (s, inv_s) == (1, 1) and list(qref.codes(np.array([[3.25, 4.25, 2.0]], dtype=F), lo, inv_s)[0]) == [-128, -127, -128]
    with pytest.raises(ValueError):
        qref.quantiser(0.0, np.inf)


def test_ops_quantiser_agrees_with_the_reference():
    from self_supervised import ops
    for lo, hi in [(-1.0, 1.55), (0.0, 255.0), (3.25, 3.25), (-7.123456, 19.8765), (1e-3, 2e-3), (-3e4, 5e4)]:
        lo, hi = float(F(lo)), float(F(hi))
        want = qref.quantiser(lo, hi)
        got = ops.int8_quantiser(lo, hi)
        assert all(F(g) == w and isinstance(g, float) for g, w in zip(got, want)), (lo, hi, got, want)
        assert ops._int8_from_step(got[1]) == got[1:]            # (lo, s) alone reproduce inv_s and s2: what a loaded state relies on
    for bad in [(0.0, np.inf), (np.nan, 1.0), (-np.inf, 0.0)]:
        with pytest.raises(ValueError, match="must be finite"):
            ops.int8_quantiser(*bad)


@pytest.mark.parametrize("d", [32, 96, 448])
def test_reference_d2_equals_the_expanded_integer_form(d):
    bank, x = gauss(150, d, seed=1), gauss(40, d, seed=2) * 1.5
    lo, s, inv_s, _ = qref.quantiser_of(bank)
    xc, bc = qref.codes(x, lo, inv_s), qref.codes(bank, lo, inv_s)
    assert bc.min() == -128 and bc.max() == 127                  # lo and hi themselves take the end codes
    a, b = qref.d2_int(xc, bc), qref.d2_expanded(xc, bc)
    assert a.dtype == np.int64 and np.array_equal(a, b) and a.min() >= 0
    assert np.array_equal(a, qref.d2_blas(xc, bc)) and qref.d2_blas(xc, bc).dtype == np.int64
    assert a.max() <= d * 255 ** 2 < 2 ** 31


@pytest.mark.parametrize("d,mean", [(32, 0.0), (384, 0.0), (384, 10.0)])
def test_error_bound_on_the_reference(d, mean):
    """In exact arithmetic a value inside [lo, hi] lies within s / 2 of the value its code stands for, so the difference q - b moves
    by at most s per element and the distance by at most s sqrt(D).  The fp32 slack: v = fl(fl(x - lo) * inv_s) carries three
    roundings (the difference, inv_s itself, the product), so |v - (x - lo) / s| <= 255 (3 u + O(u^2)) <= 255 * 4 u, u = 2^-24; a
    value that close to a .5 boundary may take the neighbouring code, and the value of code 127, lo + 255 s, lies within 255 * s * u
    + |hi| u of hi (the rounding of s, then of hi_q).  Per element the decode error is therefore at most s (1/2 + 255 * 4 u) + 2
    |hi| u, and the bar becomes s sqrt(D) (1 + 2040 u) + 4 sqrt(D) max(|lo|, |hi|) u.
    Any query: with c = clamp(q) and e = q - c, d_exact^2 >= |c - b|^2 + |e|^2 (element by element b lies on the near side of the
    bound q left through), d_q^2 = |c^ - b^|^2 + |e|^2 with |c^ - b^| <= |c - b| + bar, hence d_q <= d_exact + bar."""
    bank = gauss(300, d, seed=6, mean=mean)
    lo, s, inv_s, s2 = qref.quantiser_of(bank)
    hi = float(bank.max())
    bar = float(s) * np.sqrt(d) * (1 + 2040 * qref.U) + 4 * np.sqrt(d) * max(abs(float(lo)), abs(hi)) * qref.U
    bc = qref.codes(bank, lo, inv_s)
    inside = torch.clamp(gauss(200, d, seed=5, mean=mean) * 0.8, float(lo), hi)
    outside = torch.cat([gauss(100, d, seed=7, mean=mean) * 3.0, gauss(100, d, seed=8, mean=mean) + 4.0])
    assert float(((outside < float(lo)) | (outside > hi)).float().mean()) > 0.01
    worst = 0.0
    for name, x in (("inside", inside), ("outside", outside)):
        xc = qref.codes(x, lo, inv_s)
        ex = qref.excess64(x, lo, s)
        dq = np.sqrt(float(s) ** 2 * qref.d2_int(xc, bc) + ex[:, None])
        de = qref.exact64(x, bank)
        if name == "inside":
            assert (ex == 0).all()
            ratio = np.abs(dq - de).max() / bar
            assert ratio <= 1.0, ratio
        else:
            assert (ex > 0).any()
            ratio = (dq - de).max() / bar
            assert ratio <= 1.0, ratio
            assert (dq >= np.sqrt(ex)[:, None]).all()          # an out-of-range query scores at least sqrt(excess)
        print(f"D={d} mean={mean} {name}: worst (|d_q - d_exact| or d_q - d_exact) / bar = {ratio:.4f}, s sqrt(D) = {float(s) * np.sqrt(d):.4f}")
        worst = max(worst, ratio)
    # the fp32 s2 the kernel multiplies by differs from s^2 by one rounding
    assert abs(float(s2) - float(s) ** 2) <= qref.U * float(s) ** 2


BAD = [({"bank_dtype": 'int4', "metric": 'euclidean'}, "bank_dtype must be one of"),
       ({"bank_dtype": 'int8'}, "bank_dtype='int8' needs metric='euclidean'"),
       ({"bank_dtype": 'int8', "metric": 'euclidean', "detector": 'gde'}, "applies to detector='knn' only"),
       ({"bank_dtype": 'int8', "metric": 'euclidean', "index": 'ivf'}, "bank_dtype='int8' needs index='flat'"),
       ({"bank_dtype": 'int8', "metric": 'euclidean', "gallery": 2, "patch_localization": True, "bank": 'train'},
        "bank_dtype='int8' needs gallery=None"),
       ({"bank_dtype": 'int8', "metric": 'euclidean', "patch_localization": True, "image_scores": 'reweighted'},
        "bank_dtype='int8' takes image_scores None or 'max'"),
       ({"bank_dtype": 'int8', "metric": 'euclidean', "n_neighbors": 4},
        "bank_dtype='int8' supports n_neighbors in 1..3, got 4: 4..32 need bank_dtype 'float32' or 'float16'")]


@pytest.mark.parametrize("kw,match", BAD, ids=[m[:28] for _, m in BAD])
def test_bank_dtype_argument_errors_come_before_any_file_is_read(tmp_path, kw, match):
    from self_supervised import tools
    missing = str(tmp_path / "nothing_here")
    with pytest.raises(ValueError, match=match):
        tools.inference(missing + "/model.ckpt", missing + "/", "bottle", **kw)
    with pytest.raises(ValueError, match=match):
        tools.sweep(missing + "/", missing + "/out/", ["bottle"], **{"patch_localization": False, **kw})


def test_detector_argument_errors_and_state_without_a_gpu():
    from self_supervised import models
    from self_supervised.models import AnomalyDetector, check_bank_dtype
    assert models.BANK_DTYPES == ('float32', 'float16', 'int8')
    with pytest.raises(ValueError, match="bank_dtype must be one of"):
        AnomalyDetector(metric='euclidean', bank_dtype='uint8')
    with pytest.raises(ValueError, match="bank_dtype='int8' needs metric='euclidean'"):
        AnomalyDetector(bank_dtype='int8')
    with pytest.raises(ValueError, match="bank_dtype='int8' needs index='flat'"):
        AnomalyDetector(metric='euclidean', index='ivf', bank_dtype='int8')
    with pytest.raises(ValueError, match="bank_dtype='int8' needs gallery=None"):
        AnomalyDetector(patch_level=True, batch=1, num_patches=4, metric='euclidean', gallery=2, bank_dtype='int8')
    for k in (4, 32):
        with pytest.raises(ValueError, match="supports n_neighbors in 1..3"):
            AnomalyDetector(metric='euclidean', bank_dtype='int8', n_neighbors=k)
    assert check_bank_dtype('int8', image_scores='max', n_neighbors=3) == 'int8'
    assert check_bank_dtype('float16', n_neighbors=32) == 'float16' and check_bank_dtype('float32', 'cosine', 'ivf', 3, 'reweighted', 32)
    for k in (1, 2, 3):
        assert AnomalyDetector(metric='euclidean', bank_dtype='int8', n_neighbors=k).k == k
    # the 'float16' messages, byte for byte
    for kw, msg in [({"metric": 'cosine'}, "bank_dtype='float16' needs metric='euclidean' (the half-precision kernel is Euclidean), got "
                                           "metric='cosine'"),
                    ({"index": 'ivf'}, "bank_dtype='float16' needs index='flat' (it is the exact search over the whole bank), got index='ivf'"),
                    ({"gallery": 2}, "bank_dtype='float16' needs gallery=None: the gallery kernel reads fp32 bank rows"),
                    ({"image_scores": 'reweighted'}, "bank_dtype='float16' takes image_scores None or 'max', got 'reweighted': 'reweighted' "
                                                     "takes direct fp32 differences to bank rows, which the half bank no longer holds")]:
        with pytest.raises(ValueError) as e:
            check_bank_dtype('float16', **kw)
        assert str(e.value) == msg
    det = AnomalyDetector(patch_level=True, batch=1, num_patches=4, metric='euclidean', bank_dtype='int8')
    assert det.quant is None and det.bank is None
    det.bank = torch.zeros((4, 32), dtype=torch.int8)
    det.bank_sq = torch.zeros(4, dtype=torch.int32)
    det.quant = (-1.0, 0.5)
    with pytest.raises(ValueError, match="takes image_scores None or 'max'"):
        det._check_image_scores('reweighted', 9)
    det._check_image_scores('max', 9)
    state = det.state()
    assert state["bank_dtype"] == 'int8' and state["bank"].dtype == torch.int8 and state["bank_sq"].dtype == torch.int32
    assert (state["lo"], state["s"]) == (-1.0, 0.5) and state["metric"] == 'euclidean'
    with pytest.raises(ValueError, match="fitted with bank_dtype='int8', this detector has 'float32'"):
        AnomalyDetector(metric='euclidean').load_state(state)
    with pytest.raises(ValueError, match="fitted with bank_dtype='int8', this detector has 'float16'"):
        AnomalyDetector(metric='euclidean', bank_dtype='float16').load_state(state)
    with pytest.raises(ValueError, match="fitted with bank_dtype='float32', this detector has 'int8'"):
        det.load_state({"metric": 'euclidean', "bank": torch.zeros((4, 32))})
    other = AnomalyDetector(metric='euclidean', bank_dtype='int8')
    if torch.cuda.is_available():
        other.load_state(state)
        assert torch.equal(other.bank.cpu(), state["bank"]) and torch.equal(other.bank_sq.cpu(), state["bank_sq"]) and other.quant == det.quant
        assert other.state()["lo"] == state["lo"] and other.state()["s"] == state["s"]
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # past every check: only the device is missing
            other.load_state(state)
    # the default detector carries nothing of the option
    assert "quant" not in vars(AnomalyDetector()) and "quant" not in vars(AnomalyDetector(metric='euclidean', bank_dtype='float16'))


def test_tools_pass_the_option_through():
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector
    cls, kw = tools._check_options('knn', 'euclidean', 'dense', True, 'train', True, 0.1, 'max', 9, None, bank_dtype='int8', n_neighbors=2)
    assert cls is AnomalyDetector and kw == {"coreset": 0.1, "metric": 'euclidean', "bank_dtype": 'int8', "n_neighbors": 2}
    cls, kw = tools._check_options('knn', 'euclidean', 'patches', False, 'reference', False, None, None, 9, None, bank_dtype='int8')
    assert kw == {"metric": 'euclidean', "bank_dtype": 'int8'}


def test_ops_argument_errors_come_before_any_launch_and_there_is_no_cpu_fallback():
    """Host tensors: the checks raise ValueError; past them the launch refuses the host tensors (HipExtensionError: the product path
    has no CPU fallback)."""
    from self_supervised import _hip, ops
    x, bank_q, bsq = gauss(5, 64, 1), torch.zeros((4, 64), dtype=torch.int8), torch.zeros(4, dtype=torch.int32)
    quant = (-1.0, 0.01)
    for fn in (ops.l2q_knn_fused, ops.l2q_knn_index):
        with pytest.raises(ValueError, match="multiple of 32"):
            fn(x[:, :48].contiguous(), bank_q[:, :48].contiguous(), bsq, quant)
        with pytest.raises(ValueError, match="at most 32768"):
            fn(torch.zeros((1, 32768 + 32)), torch.zeros((4, 32768 + 32), dtype=torch.int8), bsq, quant)
        with pytest.raises(ValueError, match="k must be 1, 2 or 3"):
            fn(x, bank_q, bsq, quant, k=4)
        with pytest.raises(ValueError, match="fewer than k"):
            fn(x, bank_q[:2], bsq[:2], quant, k=3)
        with pytest.raises(ValueError, match="int8 codes"):
            fn(x, bank_q.float(), bsq, quant)
        with pytest.raises(ValueError, match="int8 codes"):
            fn(x, bank_q, bsq.float(), quant)
        with pytest.raises(ValueError, match="splits must be >= 1"):
            fn(x, bank_q, bsq, quant, splits=0)
        with pytest.raises(ValueError, match="finite"):
            fn(x, bank_q, bsq, (float("nan"), 0.01))
        with pytest.raises(ValueError, match="finite and positive"):
            fn(x, bank_q, bsq, (0.0, 0.0))
        with pytest.raises(_hip.HipExtensionError):
            fn(x, bank_q, bsq, quant)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.rows_to_int8(x[:, :48].contiguous(), -1.0, 100.0, 0.01)
    with pytest.raises(_hip.HipExtensionError):
        ops.rows_to_int8(x, -1.0, 100.0, 0.01)
    assert "no CPU fallback" in _hip.__doc__


def test_header_and_signatures_agree_on_the_new_entry_points():
    from self_supervised import _hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssad.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/ssad.h"
        assert name in _hip.SIGNATURES, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(_hip.SIGNATURES[name]) == len(args), name
        for a, ct in zip(args, _hip.SIGNATURES[name]):                      # floats by value where the header has them
            assert (ct is _hip._c_f) == a.startswith("float ") , (name, a)
    src = open(os.path.join(ROOT, "self-supervised-anomaly-detection_amd", "csrc", "knn_l2_int8.hip")).read()
    for name in NEW:
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
    assert "rint(min(max((x - lo) * inv_s, 0), 255)) - 128" in src and "rint(min(max((x - lo) * inv_s, 0), 255)) - 128" in qref.__doc__
