"""GPU: the greedy k-center coreset of the kNN bank -- csrc/coreset.hip ssad_coreset_greedy (ops.coreset_greedy), the projected
selection of models.coreset_select, AnomalyDetector(coreset=...) and tools.inference(coreset=...).

Integer-valued rows make every fp32 distance exact, so the kernel must then give the selection of a float64 numpy greedy bit for bit
(ties to the smallest row, early stop); on real-valued rows each pick must be a valid greedy step within fp32 error."""
import random
import time

import numpy as np
import pytest
import torch

import two_rank_util
from coreset_ref import greedy64, replay64
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

N_TRAIN = 8


def _int_rows(r, d, distinct, seed):
    """r rows of small integers drawn from `distinct` patterns (duplicates and equal distances galore)."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(-2, 3, size=(distinct, d))
    return pool[rng.integers(0, distinct, size=r)].astype(np.float32)


@pytest.mark.parametrize("d", [4, 128, 512])
@pytest.mark.parametrize("r", [1, 2, 127, 128, 129, 4097])
def test_integer_rows_match_float64_greedy_exactly(r, d):
    from self_supervised import ops
    distinct = r if r <= 129 else 40
    for seed, n_pat in ((0, distinct), (1, max(1, distinct // 3))):
        p = _int_rows(r, d, n_pat, seed + r + d)
        pt = torch.from_numpy(p).cuda()
        for m in sorted({1, 2, min(r, 7), r, r + 3}):
            for start in sorted({0, r - 1}):
                want_sel, want_rad = greedy64(p, m, start)
                sel, rad = ops.coreset_greedy(pt, m, start=start)
                assert sel.dtype == torch.int64 and rad.dtype == torch.float32
                assert np.array_equal(sel.cpu().numpy(), want_sel), (r, d, m, start)
                assert np.array_equal(rad.cpu().numpy().astype(np.float64), want_rad), (r, d, m, start)
                assert sel.numel() <= min(m, r)


def test_all_rows_equal_stops_after_one_centre():
    from self_supervised import ops
    p = torch.ones(1000, 8, device="cuda")
    sel, rad = ops.coreset_greedy(p, 50, start=17)
    assert sel.tolist() == [17] and rad.tolist() == [float("inf")]


def _gauss(r, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(r, d, device="cuda", generator=g)


def _check_valid_steps(p, sel, rad, tol=1e-5):
    rad = rad.double().cpu().numpy()
    assert rad[0] == np.inf
    assert np.all(np.diff(rad[1:]) <= 0), "rad must be non-increasing"
    assert len(np.unique(sel.cpu().numpy())) == sel.numel()
    mx, at = replay64(p, sel)
    assert np.all(at >= (1.0 - tol) * mx), np.min(at / mx)
    assert np.all(np.abs(rad[1:] - at) <= tol * at), np.max(np.abs(rad[1:] - at) / at)


def test_gaussian_rows_are_valid_greedy_steps():
    from self_supervised import ops
    p = _gauss(20000, 128, seed=0)
    sel, rad = ops.coreset_greedy(p, 400)
    assert sel.numel() == 400 and sel[0].item() == 0
    _check_valid_steps(p, sel, rad)


def test_selection_is_the_same_for_every_grid():
    from self_supervised import ops
    for r, d in ((20000, 128), (5003, 512), (300, 4)):
        p = _gauss(r, d, seed=r)
        base = ops.coreset_greedy(p, 200)
        g0 = ops.coreset_workgroups(r)
        for wgs in sorted({1, 3, 7, g0, 157, 1000, r + 5}):
            sel, rad = ops.coreset_greedy(p, 200, wgs=wgs)
            assert torch.equal(sel, base[0]) and torch.equal(rad, base[1]), (r, d, wgs)


def test_projection_and_selection_on_it():
    from self_supervised import ops
    from self_supervised.models import coreset_projection, coreset_select
    bank = ops.l2_normalize_rows(_gauss(6000, 512, seed=3))
    om = coreset_projection(512, 128)
    pt = ops.linear_fwd(bank, om.t().contiguous().cuda())
    want = bank.double().cpu() @ om.double()
    scale = bank.double().cpu().abs() @ om.double().abs()
    assert ((pt.double().cpu() - want).abs() <= 1e-5 * scale + 1e-7).all()
    sel, rad = coreset_select(bank, 300, 128)
    s2, r2 = ops.coreset_greedy(pt, 300)
    assert torch.equal(sel, s2) and torch.equal(rad, r2)
    s3, r3 = coreset_select(bank, 300, None)
    s4, r4 = ops.coreset_greedy(bank, 300)
    assert torch.equal(s3, s4) and torch.equal(r3, r4)


def _ref64(x, bank_n, k=3):
    """float64 brute force (tests/test_hip_train_bank.py's recipe): x / ||x||, cosine distance clipped to [0, 2], mean of the k
    smallest."""
    q = x.double().cpu().numpy()
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    b = bank_n.double().cpu().numpy()
    out = np.empty(q.shape[0])
    for i in range(0, q.shape[0], 256):
        d = np.clip(1.0 - q[i:i + 256] @ b.T, 0.0, 2.0)
        out[i:i + 256] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1).mean(1)
    return out


def _states():
    return np.random.get_state(), torch.get_rng_state(), random.getstate()


def _same_states(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and a[2] == b[2])


def test_detector_coreset_bank_and_threshold():
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector, coreset_select, split_indices
    emb = _gauss(5000, 512, seed=4).cpu()
    n_fit = 5000 - int(np.ceil(0.3 * 5000))
    for cs, m in ((0.1, int(np.ceil(0.1 * n_fit))), (137, 137)):
        np.random.seed(7)
        random.seed(7)
        torch.manual_seed(7)
        det = AnomalyDetector(coreset=cs)
        det.fit(emb)
        after_cs = _states()
        np.random.seed(7)
        tr, va = split_indices(5000, 0.3)
        full = ops.l2_normalize_rows(emb[tr].cuda())
        sel, rad = det.coreset_rows
        assert sel.numel() == m and det.coreset_counts == (m, n_fit)
        assert torch.equal(det.bank, full[sel])
        s2, r2 = coreset_select(full, m, 128)
        assert torch.equal(sel, s2) and torch.equal(rad, r2)
        assert abs(det.threshold - _ref64(emb[va], det.bank).max()) <= 1e-6
        # a coreset draws from no global generator: the states equal those after a fit without one
        np.random.seed(7)
        random.seed(7)
        torch.manual_seed(7)
        AnomalyDetector().fit(emb)
        assert _same_states(after_cs, _states())


def test_detector_coreset_at_least_the_bank_is_the_exact_bank():
    from self_supervised.models import AnomalyDetector
    emb = _gauss(1000, 512, seed=5)
    x = _gauss(300, 512, seed=6)
    np.random.seed(1)
    ref = AnomalyDetector()
    ref.fit(emb)
    want = ref.predict(x)
    for cs in (700, 701, 5000, 1.0):
        np.random.seed(1)
        det = AnomalyDetector(coreset=cs)
        det.fit(emb)
        assert det.coreset_rows is None and det.coreset_counts == (700, 700)
        assert torch.equal(det.bank, ref.bank) and det.threshold == ref.threshold
        assert torch.equal(det.predict(x), want)


def test_full_size_selection_time():
    """R = 123 000 rows (70 % of bottle's 209 x 841 patches), d = 128, m = 1 % of R: under 1 s once warm (about 1 230 steps of about
    10 us each expected), every step a valid greedy step."""
    from self_supervised import ops
    p = _gauss(123000, 128, seed=8)
    ops.coreset_greedy(p[:1000], 20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sel, rad = ops.coreset_greedy(p, 1230)
    elapsed = time.perf_counter() - t0
    assert sel.numel() == 1230
    assert elapsed < 1.0, elapsed
    _check_valid_steps(p, sel, rad)


def _tree(tmp_path, seeded_sd):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=96)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


def test_inference_with_coreset(tmp_path, seeded_sd, monkeypatch, capsys):
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector
    root, ck = _tree(tmp_path, seeded_sd)
    seen = {}
    orig = AnomalyDetector.fit

    def spy(self, embeddings, split=True, groups=None):
        orig(self, embeddings, split, groups)
        seen["det"] = self
    monkeypatch.setattr(AnomalyDetector, "fit", spy)
    np.random.seed(3)
    res = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train', coreset=0.25)
    det = seen["det"]
    n_fit = (N_TRAIN - 3) * 841
    m = int(np.ceil(0.25 * n_fit))
    assert det.coreset_counts == (m, n_fit) and det.bank.shape == (m, 512)
    assert f" coreset: {m} of {n_fit} rows" in capsys.readouterr().out
    maps = res.anomaly_maps
    assert tuple(maps.shape) == (4, 1, 29, 29)
    err = np.abs(maps.reshape(-1).double().numpy() - _ref64(res.embedding_vectors.float(), det.bank)).max()
    assert err <= 2e-6, err
    # coreset=None is the call without the argument, bit for bit
    outs = []
    for kw in ({}, {"coreset": None}):
        np.random.seed(3)
        outs.append(tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                                    **kw).anomaly_maps)
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], maps)


def test_inference_with_coreset_two_ranks_equal_one_rank(tmp_path, seeded_sd):
    from self_supervised import tools
    root, ck = _tree(tmp_path, seeded_sd)
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "coreset"])
    assert r["maps_equal_across_ranks"], r
    two = torch.load(str(tmp_path / "maps_rank0.pt"))
    one = two_rank_util.inference(tools, ck, root, "coreset")
    assert torch.equal(two["embeddings"], one.embedding_vectors)
    assert torch.equal(two["maps"], one.anomaly_maps)
