"""Host-side tests of n_neighbors and the k = 4..32 search: argument checks that come before any launch or file read, the state's
compatibility and the C ABI.  No GPU needed."""
import ctypes
import re

import pytest
import torch

TOPK_SYMBOLS = ("ssad_l2_knn_topk", "ssad_l2_knn_topk_index", "ssad_l2h_knn_topk", "ssad_l2h_knn_topk_index")


def test_check_n_neighbors_accepts_and_refuses():
    from self_supervised.models import AnomalyDetector, check_n_neighbors
    for k in (1, 2, 3):
        for metric, index, gallery in (('cosine', 'flat', None), ('euclidean', 'flat', None), ('euclidean', 'flat', 4),
                                       ('euclidean', 'ivf', None)):
            assert check_n_neighbors(k, metric, index, gallery) == k
    for k in (4, 9, 32):
        assert check_n_neighbors(k, 'euclidean', 'flat', None) == k
        with pytest.raises(ValueError, match=rf"n_neighbors={k} needs metric='euclidean', got metric='cosine'.*flat Euclidean search only"):
            check_n_neighbors(k, 'cosine', 'flat', None)
        with pytest.raises(ValueError, match=rf"n_neighbors={k} needs index='flat', got index='ivf'.*flat Euclidean search only"):
            check_n_neighbors(k, 'euclidean', 'ivf', None)
        with pytest.raises(ValueError, match=rf"n_neighbors={k} needs gallery=None, got gallery=2.*flat Euclidean search only"):
            check_n_neighbors(k, 'euclidean', 'flat', 2)
    for bad in (0, 33, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match=r"n_neighbors must be an int in 1\.\.32"):
            check_n_neighbors(bad, 'euclidean', 'flat', None)
    # the constructor runs the same check and keeps the value as k
    assert AnomalyDetector().k == 3 and AnomalyDetector(n_neighbors=1).k == 1
    for bank_dtype in ('float32', 'float16'):
        det = AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype, n_neighbors=32)
        assert det.k == 32 and det.n_neighbors == 32
    with pytest.raises(ValueError, match="needs metric='euclidean'"):
        AnomalyDetector(n_neighbors=4)
    with pytest.raises(ValueError, match="needs index='flat'"):
        AnomalyDetector(metric='euclidean', index='ivf', n_neighbors=4)
    with pytest.raises(ValueError, match="needs gallery=None"):
        AnomalyDetector(metric='euclidean', gallery=2, patch_level=True, num_patches=25, n_neighbors=4)
    assert AnomalyDetector(metric='euclidean', gallery=2, patch_level=True, num_patches=25, n_neighbors=2).k == 2


def test_tools_refuse_before_any_model_is_loaded(tmp_path):
    from self_supervised import tools
    args = ('knn', 'euclidean', 'patches', True, 'reference', True, None, None, 9, None)
    cls, kw = tools._check_options(*args)
    assert "n_neighbors" not in kw
    assert tools._check_options(*args, n_neighbors=3)[1] == kw
    assert tools._check_options(*args, n_neighbors=9)[1]["n_neighbors"] == 9
    assert tools._check_options(*args, bank_dtype='float16', n_neighbors=32)[1]["n_neighbors"] == 32
    assert tools._check_options('knn', 'cosine', 'patches', True, 'reference', True, None, None, 9, None, n_neighbors=1)[1] == {"n_neighbors": 1}
    with pytest.raises(ValueError, match="needs metric='euclidean'"):
        tools._check_options('knn', 'cosine', 'patches', True, 'reference', True, None, None, 9, None, n_neighbors=4)
    with pytest.raises(ValueError, match="needs index='flat'"):
        tools._check_options(*args, index='ivf', n_neighbors=4)
    for detector in ('gde', 'padim'):
        with pytest.raises(ValueError, match=f"n_neighbors=1 applies to detector='knn' only, got detector='{detector}'"):
            tools._check_options(detector, 'cosine', 'dense', True, 'train', True, None, None, 9, None, n_neighbors=1)
    missing = str(tmp_path / "no_such_model.ckpt")          # never opened: the refusal comes first
    with pytest.raises(ValueError, match=r"n_neighbors must be an int in 1\.\.32"):
        tools.inference(missing, str(tmp_path) + "/", "bottle", patch_localization=True, metric='euclidean', n_neighbors=33)
    with pytest.raises(ValueError, match="needs metric='euclidean'"):
        tools.inference(missing, str(tmp_path) + "/", "bottle", patch_localization=True, n_neighbors=5)
    with pytest.raises(ValueError, match="applies to detector='knn' only"):
        tools.inference(missing, str(tmp_path) + "/", "bottle", detector='gde', bank='train', n_neighbors=5)
    with pytest.raises(ValueError, match="needs gallery=None"):
        tools.sweep(str(tmp_path), str(tmp_path), ["bottle"], metric='euclidean', bank='train', gallery=2, n_neighbors=5, train=False)


@pytest.mark.parametrize("name", ["l2_topk_mean", "l2_topk_index", "l2h_topk_mean", "l2h_topk_index"])
def test_ops_refuse_host_tensors_before_any_launch(name):
    from self_supervised import _hip, ops
    fn = getattr(ops, name)
    half = name.startswith("l2h")
    x = torch.zeros(5, 64)
    bank = torch.zeros(40, 64, dtype=torch.float16 if half else torch.float32)
    bsq = torch.zeros(40)
    before = _hip.LAUNCHES
    with pytest.raises(ValueError, match="multiple of 32"):
        fn(torch.zeros(5, 48), bank[:, :48], bsq, 8)
    for k in (0, 3, 33):
        with pytest.raises(ValueError, match=r"k must lie in 4\.\.32"):
            fn(x, bank, bsq, k)
    with pytest.raises(ValueError, match="the bank has 7 rows, fewer than k = 8"):
        fn(x, bank[:7], bsq[:7], 8)
    with pytest.raises(ValueError, match="splits must be >= 1"):
        fn(x, bank, bsq, 8, splits=0)
    with pytest.raises(ValueError, match="squared norms"):
        fn(x, bank, bsq[:39], 8)
    if half:
        with pytest.raises(ValueError, match="float16 rows"):
            fn(x, bank.float(), bsq, 8)
    assert _hip.LAUNCHES == before


def test_state_carries_n_neighbors_only_when_it_is_not_3():
    from self_supervised.models import AnomalyDetector
    bank = torch.zeros(8, 64)
    for kw in ({}, {"n_neighbors": 3}):
        det = AnomalyDetector(metric='euclidean', **kw)
        det.bank = bank
        assert set(det.state()) == {"metric", "bank"}                       # what a state held before the option
    det = AnomalyDetector(metric='euclidean', n_neighbors=5)
    det.bank = bank
    assert det.state()["n_neighbors"] == 5
    old = {"metric": 'euclidean', "bank": bank}
    with pytest.raises(ValueError, match="fitted with n_neighbors=3, this detector has 5"):
        AnomalyDetector(metric='euclidean', n_neighbors=5).load_state(old)
    with pytest.raises(ValueError, match="fitted with n_neighbors=5, this detector has 3"):
        AnomalyDetector(metric='euclidean').load_state(det.state())
    plain = AnomalyDetector(metric='euclidean')
    if torch.cuda.is_available():
        plain.load_state(old)                                               # a state written before the option still loads
        assert plain.k == 3 and tuple(plain.bank.shape) == (8, 64)
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # past every check: only the device is missing
            plain.load_state(old)


def test_abi_exports_the_new_entry_points():
    import __graft_entry__ as g
    g.build()
    from self_supervised import _hip
    header = open(g.ROOT + "/include/ssad.h").read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in TOPK_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    for name in ("ssad_l2_knn_topk", "ssad_l2h_knn_topk"):
        assert len(_hip.SIGNATURES[name + "_index"]) == len(_hip.SIGNATURES[name]) + 1
