"""GPU tests of the index-returning cosine kNN (csrc/knn.hip ssad_cosine_knn_index), the row selection, the image scores
built on them (csrc/image_score.hip) and their way through AnomalyDetector, tools.inference and tools.sweep.  The reference
everywhere is the float64 numpy brute force of tests/knn_index_ref.py on the same fp32 inputs; two HIP paths are compared with
each other only where bit-equality between them is the claim."""
import os

import numpy as np
import pytest
import torch

import knn_index_ref as ref
import two_rank_util
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

DIST_TOL = 2e-6        # the bound of every kNN test of this project (test_hip_train_bank.py, test_hip_coreset.py)
GAP = 1e-5             # "a valid pick" margin of test_hip_coreset.py: 5 x the distance bound
N_TRAIN = 8


def gauss(n, d, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32)


def _bank(r, d, seed):
    from self_supervised import ops
    return ops.l2_normalize_rows(gauss(r, d, seed).cuda())


# ---------------------------------------------------------------- 1. distances and indices against float64

def index_case_inputs(d, n, r):
    return gauss(n, d, seed=1000 + d + n), gauss(r, d, seed=2000 + d + r)


@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("n", [1, 130, 841, 13456])
@pytest.mark.parametrize("r", [3, 127, 588, 5000, 20000])
def test_distances_and_indices_match_float64(d, n, r):
    from self_supervised import ops
    x, raw = index_case_inputs(d, n, r)
    bank = ops.l2_normalize_rows(raw.cuda())
    bank_host = bank.cpu()
    want_d, want_i = ref.kneighbors64(x, bank_host, 4)
    q64, b64 = ref.unit_rows64(x), bank_host.double().numpy()
    for k in (1, 2, 3):
        strict = ref.strict_positions(want_d, k, GAP)
        loose_share = 1.0 - strict.mean()
        print(f"D={d} N={n} R={r} k={k}: share outside the strict index comparison {loose_share:.2e}")
        assert loose_share <= 0.02, loose_share                     # on the reference alone, before the GPU result is looked at
        dist, idx = ops.cosine_knn_index(x.cuda(), bank, k)
        assert dist.shape == (n, k) and idx.shape == (n, k) and idx.dtype == torch.int32
        dist, idx = dist.cpu().double().numpy(), idx.cpu().numpy().astype(np.int64)
        err = np.abs(dist - want_d[:, :k]).max()
        print(f"   max |dist - float64| = {err:.3e}")
        assert err <= DIST_TOL, err
        assert idx.min() >= 0 and idx.max() < r
        # the float64 distance of the returned row against the float64 j-th smallest
        d_of_idx = np.clip(1.0 - np.einsum("nd,nkd->nk", q64, b64[idx]), 0.0, 2.0)
        err_i = np.abs(d_of_idx - want_d[:, :k]).max()
        print(f"   max |float64 distance of the returned row - float64 j-th smallest| = {err_i:.3e}")
        assert err_i <= DIST_TOL, err_i
        assert np.array_equal(idx[strict], want_i[:, :k][strict])


# ---------------------------------------------------------------- 2. the same bits as the mean kernels

def _mean_of(dist, k):
    """(d0 [+ d1] [+ d2]) / k, added smallest first, in IEEE fp32 on the host (numpy) -- torch's division of a device tensor by a
    Python scalar multiplies by the rounded reciprocal, which is not the kernels' division."""
    d = dist.cpu().numpy()
    s = d[:, 0].copy()
    for j in range(1, k):
        s = s + d[:, j]
    assert s.dtype == np.float32
    return torch.from_numpy(s / np.float32(k))


@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("n", [1, 130, 841, 13456])
@pytest.mark.parametrize("r", [3, 127, 588, 5000, 20000, 50000])
def test_same_bits_as_the_mean_kernels(d, n, r):
    from self_supervised import ops
    if r == 50000 and n == 13456:
        n = 2000                                                    # (the big bank is here for the split dispatch: few queries)
    x = gauss(n, d, seed=31 + n).cuda()
    bank = _bank(r, d, seed=32 + r)
    if r >= 20000 and n <= 2000:
        assert ops.knn_splits(n, r) > 1
    for k in (1, 2, 3):
        dist, _ = ops.cosine_knn_index(x, bank, k)
        assert torch.equal(_mean_of(dist, k), ops.cosine_knn_fused(x, bank, k).cpu()), (d, n, r, k)


# ---------------------------------------------------------------- 3. ties

def tied_bank(u, d, seed):
    """A bank in which each of u distinct rows appears 2-5 times at scattered positions.  Returns (raw rows [R][d], orig [R]: the
    distinct row behind every position)."""
    rng = np.random.RandomState(seed)
    orig = np.repeat(np.arange(u), rng.randint(2, 6, size=u))
    rng.shuffle(orig)
    return gauss(u, d, seed=seed + 1)[torch.from_numpy(orig)], orig


@pytest.mark.parametrize("u,splits", [(300, None), (300, 3), (2600, None), (2600, 5)])
def test_duplicated_bank_rows(u, splits):
    from self_supervised import ops
    d = 64
    raw, orig = tied_bank(u, d, seed=5)
    r = raw.shape[0]
    if splits is None and u == 2600:
        assert ops.knn_splits(400, r) > 1                           # copies of one row on both sides of a split boundary
    bank = ops.l2_normalize_rows(raw.cuda())
    distinct = ops.l2_normalize_rows(gauss(u, d, seed=6).cuda()).cpu()
    assert torch.equal(bank.cpu(), distinct[torch.from_numpy(orig)])
    rng = np.random.RandomState(9)
    x = torch.cat([gauss(200, d, seed=7), 3.0 * raw[torch.from_numpy(rng.randint(0, r, size=200))]])
    # float64 on the DISTINCT rows, expanded: copies then carry one float64 value, as they carry one fp32 value on the device
    d64 = ref.distances64(x, distinct)[:, orig]
    order = np.argsort(d64, axis=1, kind="stable")
    first = np.take_along_axis(d64, order[:, :1], 1)[:, 0]
    d_other = np.where(orig[None, :] == orig[order[:, 0]][:, None], np.inf, d64)
    clear = d_other.min(1) - first > GAP                            # the nearest distinct row leads the second distinct row
    assert clear.mean() > 0.9
    for k in (1, 2, 3):
        dist, idx = ops.cosine_knn_index(x.cuda(), bank, k, splits=splits)
        bits = dist.cpu().view(torch.int32).numpy()
        idx = idx.cpu().numpy().astype(np.int64)
        assert np.abs(dist.cpu().double().numpy() - np.take_along_axis(d64, order[:, :k], 1)).max() <= DIST_TOL
        for q in range(x.shape[0]):
            assert len(set(idx[q])) == k                            # never the same row twice
            for a in range(k):
                for b in range(a + 1, k):
                    if orig[idx[q, a]] == orig[idx[q, b]]:          # identical rows: identical distance bits
                        assert bits[q, a] == bits[q, b]
            if clear[q]:
                c = min(k, int((orig == orig[order[q, 0]]).sum()))  # the copies of the nearest row: smallest positions first
                assert np.array_equal(idx[q, :c], order[q, :c]), (q, idx[q], order[q, :k])
                assert np.array_equal(idx[q, :c], np.flatnonzero(orig == orig[order[q, 0]])[:c])


# ---------------------------------------------------------------- 4. grid independence

def test_same_bits_for_every_split_and_for_single_rows():
    from self_supervised import ops
    raw, _ = tied_bank(2600, 64, seed=5)
    bank = ops.l2_normalize_rows(raw.cuda())
    x = torch.cat([gauss(172, 64, seed=11), 2.0 * raw[:128]]).cuda()          # 300 rows: two whole query tiles and a ragged one
    for k in (1, 3):
        d1, i1 = ops.cosine_knn_index(x, bank, k, splits=1)
        for s in range(2, 17):
            ds, is_ = ops.cosine_knn_index(x, bank, k, splits=s)
            assert torch.equal(d1, ds) and torch.equal(i1, is_), (k, s)
        dn, in_ = ops.cosine_knn_index(x, bank, k)
        assert torch.equal(d1, dn) and torch.equal(i1, in_)
        again = ops.cosine_knn_index(x, bank, k, splits=1)
        assert torch.equal(d1, again[0]) and torch.equal(i1, again[1])
        for i in (0, 150, 299):
            for s in (1, 4):
                do, io = ops.cosine_knn_index(x[i:i + 1], bank, k, splits=s)
                assert torch.equal(do[0], d1[i]) and torch.equal(io[0], i1[i]), (k, i, s)


def test_argument_errors_of_the_index_kernel():
    from self_supervised import _hip, ops
    x, bank = gauss(5, 64, 1).cuda(), _bank(2, 64, 2)
    with pytest.raises(ValueError, match="fewer than k"):
        ops.cosine_knn_index(x, bank, 3)
    idx = torch.empty((5, 3), device="cuda", dtype=torch.int32)
    dist = torch.empty((5, 3), device="cuda")
    rc = _hip.lib().ssad_cosine_knn_index(x.data_ptr(), bank.data_ptr(), None, dist.data_ptr(), idx.data_ptr(), 5, 64, 2, 3, 1, _hip.stream())
    assert rc == 2 and b"k in 1..3" in _hip.lib().ssad_last_error()


# ---------------------------------------------------------------- 5. row selection

@pytest.mark.parametrize("q", [1, 7, 83])
@pytest.mark.parametrize("r", [1, 33, 4097, 123000])
@pytest.mark.parametrize("kind", ["integers", "gaussian"])
def test_rows_smallest_index_is_the_stable_argsort(q, r, kind):
    from self_supervised import ops
    if kind == "integers":
        m = torch.from_numpy(np.random.RandomState(q + r).randint(-40, 40, size=(q, r))).float()
    else:
        m = gauss(q, r, seed=q + r)
    m64 = m.double().numpy()
    dev = m.cuda()
    for b in (1, 9, 32):
        want_v, want_c = ref.smallest_stable(m64, b)
        for wgs in (None, 1, 3, 4096 // b):
            vals, cols = ops.rows_smallest_index(dev, b, wgs=wgs)
            assert vals.shape == (q, min(b, r)) and cols.dtype == torch.int32
            assert np.array_equal(cols.cpu().numpy().astype(np.int64), want_c), (b, wgs)
            assert np.array_equal(vals.cpu().double().numpy(), want_v), (b, wgs)


def test_rows_smallest_index_on_similarities():
    """cosine=True: the values are clip(1 - m, 0, 2), formed in fp32 as the kNN kernels form them."""
    from self_supervised import ops
    m = (0.6 * gauss(7, 5000, seed=3)).clamp_(-1.5, 1.5)
    dist32 = (1.0 - m).clamp_(0.0, 2.0)
    want_v, want_c = ref.smallest_stable(dist32.double().numpy(), 9)
    vals, cols = ops.rows_smallest_index(m.cuda(), 9, cosine=True)
    assert np.array_equal(cols.cpu().numpy().astype(np.int64), want_c)
    assert np.array_equal(vals.cpu().double().numpy(), want_v)


def test_rows_argmax_takes_the_first_maximum():
    from self_supervised import ops
    s = torch.from_numpy(np.random.RandomState(0).randint(0, 30, size=(60, 841))).float()
    val, flat = ops.rows_argmax(s.cuda())
    want = s.numpy().argmax(1)
    assert np.array_equal(flat.cpu().numpy(), np.arange(60) * 841 + want)
    assert np.array_equal(val.cpu().numpy(), s.numpy().max(1))


# ---------------------------------------------------------------- 6. image scores on embeddings with structure

IMG_NOISE = 1.0      # norm of the noise on a unit centre (see structured_embeddings)


def structured_embeddings(seed=0, noise=IMG_NOISE):
    """bank = 40 random unit centres x 50 copies, each with Gaussian noise of norm about `noise`; 60 images of 841 patches drawn the
    same way, every second one with 5 patches replaced by N(0, 1) rows.  The noise is wider than 0.05: with 0.05 the 50 copies of a
    centre lie within ~1e-4 of each other, so the order of a bank row's 9th and 10th neighbours -- which the score depends on --
    would hang on gaps of a few 1e-6 for nearly every image.  The float64 part of this test, run on the CPU, leaves out of the
    'reweighted' comparison, for b = 2 / 9 / 32: 25 / 45 / 53 of the 60 images at noise 0.05, 1 / 4 / 4 at 0.3, 0 / 0 / 0 at 1.0 (the
    cap is 3).  At 1.0 normal images score at most 0.53 and planted ones at least 0.86: the float64 AUROC is 1."""
    d, p, n_img = 512, 841, 60
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn((40, d), generator=g)
    centres = centres / centres.norm(dim=1, keepdim=True)
    sigma = noise / np.sqrt(d)
    bank = centres.repeat_interleave(50, 0) + sigma * torch.randn((2000, d), generator=g)
    which = torch.randint(0, 40, (n_img * p,), generator=g)
    x = centres[which] + sigma * torch.randn((n_img * p, d), generator=g)
    labels = np.zeros(n_img, dtype=np.int64)
    for i in range(1, n_img, 2):
        at = torch.randperm(p, generator=g)[:5] + i * p
        x[at] = torch.randn((5, d), generator=g)
        labels[i] = 1
    return bank.contiguous(), x.contiguous(), labels, p


def test_image_scores_on_structured_embeddings():
    from self_supervised import metrics as mtr, ops
    from self_supervised.models import AnomalyDetector
    bank_raw, x, labels, p = structured_embeddings()
    det = AnomalyDetector(patch_level=True, batch=60, num_patches=p)
    det.fit_bank(bank_raw)
    bank_host = det.bank.cpu()
    base = ref.image_scores64(x, bank_host, p)
    got = det.image_scores(x, 'max').cpu()
    assert got.shape == (60,) and got.dtype == torch.float32
    err = np.abs(got.double().numpy() - base["s_max"]).max()
    print(f"'max': max |score - float64| = {err:.3e}")
    assert err <= 2e-6, err
    _, flat = ops.rows_argmax(det.predict(x).reshape(60, p))
    assert np.array_equal(flat.cpu().numpy() - np.arange(60) * p, base["p_star"])
    labels_t = torch.from_numpy(labels)
    for b in (2, 9, 32):
        want = ref.image_scores64(x, bank_host, p, neighbours=b)
        share = want["fragile"].mean()
        print(f"b={b}: images left out of the 'reweighted' comparison {int(want['fragile'].sum())} of 60")
        assert share <= 0.05, share                                 # on the reference alone, first
        auc64 = ref.auroc64(labels, want["score"])
        assert auc64 >= 0.9, auc64
        got = det.image_scores(x, 'reweighted', b).cpu()
        keep = ~want["fragile"]
        err = np.abs(got.double().numpy() - want["score"])[keep].max()
        print(f"b={b}: max |score - float64| = {err:.3e}, float64 AUROC {auc64:.4f}")
        assert err <= 4e-6, err
        auc = mtr.auroc_gpu(labels_t.cuda(), got.cuda())
        assert abs(auc - auc64) <= 1e-4, (auc, auc64)
        assert torch.equal(got, det.image_scores(x, 'reweighted', b, scores=det.predict(x).reshape(-1)).cpu())
    auc_max = mtr.auroc_gpu(labels_t.cuda(), det.image_scores(x, 'max'))
    assert abs(auc_max - ref.auroc64(labels, base["s_max"])) <= 1e-4


def test_detector_kneighbors():
    from self_supervised.models import AnomalyDetector
    det = AnomalyDetector()
    det.fit_bank(gauss(700, 512, seed=3))
    x = gauss(50, 512, seed=4)
    dist, idx = det.kneighbors(x)
    assert dist.shape == (50, 3) and idx.dtype == torch.int64
    want_d, want_i = ref.kneighbors64(x, det.bank.cpu(), 3)
    assert np.abs(dist.cpu().double().numpy() - want_d).max() <= DIST_TOL
    assert np.array_equal(idx.cpu().numpy(), want_i)                # (50 x 3 Gaussian picks: gaps of ~1e-2)
    d1, i1 = det.kneighbors(x, k=1)
    assert torch.equal(d1, dist[:, :1]) and torch.equal(i1, idx[:, :1])
    assert torch.equal(_mean_of(dist, 3), det.predict(x).cpu())


# ---------------------------------------------------------------- 7. through tools.inference

def _tree(tmp_path, seeded_sd):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=96)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


@pytest.mark.parametrize("bank_kw", [{"bank": "reference"}, {"bank": "train"}, {"bank": "train", "coreset": 0.25}],
                         ids=["reference", "train", "train-coreset"])
def test_inference_with_image_scores(tmp_path, seeded_sd, monkeypatch, bank_kw):
    """Wiring and order: with seeded weights the scores are ~1e-4, so the 2e-6 / 4e-6 bounds are nearly vacuous on these embeddings
    (the O(1) numerics are test_image_scores_on_structured_embeddings'); what is checked here is that the scores of the right images
    come out in file order, from the bank that was fitted, beside unchanged maps."""
    from self_supervised import ops, tools
    from self_supervised.models import AnomalyDetector
    root, ck = _tree(tmp_path, seeded_sd)
    seen = {}
    orig = AnomalyDetector.fit

    def spy(self, embeddings, split=True, groups=None):
        orig(self, embeddings, split, groups)
        seen["det"] = self
    monkeypatch.setattr(AnomalyDetector, "fit", spy)

    def run(**kw):
        np.random.seed(3)
        torch.manual_seed(3)
        return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, **bank_kw, **kw)

    plain = run()
    assert plain.image_scores is None
    for mode, tol in (("max", 2e-6), ("reweighted", 4e-6)):
        res = run(image_scores=mode, neighbours=5)
        det = seen["det"]
        assert torch.equal(res.anomaly_maps, plain.anomaly_maps)
        assert torch.equal(res.embedding_vectors, plain.embedding_vectors)
        s = res.image_scores
        assert s.dtype == torch.float32 and tuple(s.shape) == (4,) and not s.is_cuda
        want = ref.image_scores64(res.embedding_vectors.float(), det.bank.cpu(), 841, neighbours=5 if mode == "reweighted" else None)
        key = "score" if mode == "reweighted" else "s_max"
        err = np.abs(s.double().numpy() - want[key]).max()
        print(f"{bank_kw} {mode}: max |score - float64| = {err:.3e} (scores ~ {want[key].max():.2e})")
        assert err <= tol, err
        assert np.allclose(want["patch_scores"].reshape(-1), res.anomaly_maps.reshape(-1).double().numpy(), atol=DIST_TOL, rtol=0)
        assert 0.0 <= tools.image_auroc(res) <= 1.0
    # image_scores=None is the call without the argument and touches none of the new wrappers
    def boom(*a, **k):
        raise AssertionError("a new wrapper ran although image_scores is None")
    for name in ("cosine_knn_index", "rows_smallest_index", "rows_argmax", "knn_reweight"):
        monkeypatch.setattr(ops, name, boom)
    none = run(image_scores=None)
    assert none.image_scores is None and torch.equal(none.anomaly_maps, plain.anomaly_maps)
    with pytest.raises(ValueError, match="no image_scores"):
        tools.image_auroc(none)


def test_image_score_argument_errors(tmp_path):
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector
    missing = str(tmp_path / "nothing_here")
    for kw, match in (({"image_scores": "max"}, "patch_localization=True"),
                      ({"image_scores": "max", "patch_localization": True, "detector": "gde"}, "detector='knn'"),
                      ({"image_scores": "reweighted", "patch_localization": True, "neighbours": 1}, "neighbours"),
                      ({"image_scores": "reweighted", "patch_localization": True, "neighbours": 33}, "neighbours"),
                      ({"image_scores": "mean", "patch_localization": True}, "image_scores must be one of")):
        with pytest.raises(ValueError, match=match):
            tools.inference(missing + "/model.ckpt", missing + "/", "bottle", **kw)
    det = AnomalyDetector()
    det.fit_bank(gauss(10, 64, 0))
    with pytest.raises(ValueError, match="patch-level"):
        det.image_scores(gauss(4, 64, 1))


# ---------------------------------------------------------------- 8. two gloo ranks equal one rank

def test_image_scores_two_ranks_equal_one_rank(tmp_path, seeded_sd):
    from self_supervised import tools
    root, ck = _tree(tmp_path, seeded_sd)
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "image_scores"])
    assert r["equal_across_ranks"], r
    two = torch.load(str(tmp_path / "scores_rank0.pt"))
    for mode in ("max", "reweighted"):
        one = two_rank_util.inference(tools, ck, root, "image_scores", run=mode)
        assert tuple(one.image_scores.shape) == (4,)
        assert torch.equal(two[mode]["scores"], one.image_scores)
        assert torch.equal(two[mode]["maps"], one.anomaly_maps)


# ---------------------------------------------------------------- 9. sweep

def test_sweep_writes_the_image_auroc_table(tmp_path):
    from self_supervised import tools, datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), n_train=8, n_test_good=2, n_test_bad=2, size=96)
    tables = {}
    for name, kw in (("plain", {}), ("scored", {"image_scores": "max"})):
        out = str(tmp_path / name) + "/"
        np.random.seed(0)
        df = tools.sweep(root, out, ["bottle", "carpet"], imsize=(64, 64), batch_size=4, seed=0,
                         projection_training_params=(1, 0.03), fine_tune_params=(1, 0.005),
                         trainer_kwargs={"limit_train_batches": 2, "limit_val_batches": 1}, tables_output=out + "tables/", **kw)
        assert "image_auroc" not in df.columns
        tables[name] = out + "tables/csv/"
    assert not os.path.exists(tables["plain"] + "patch_image_auroc.csv")
    assert open(tables["plain"] + "patch_all_scores.csv", "rb").read() == open(tables["scored"] + "patch_all_scores.csv", "rb").read()
    import pandas as pd
    t = pd.read_csv(tables["scored"] + "patch_image_auroc.csv", index_col=0)
    assert list(t.index) == ["bottle", "carpet", "average"] and list(t.columns) == ["image_auroc"]
    assert ((t["image_auroc"] >= 0) & (t["image_auroc"] <= 1)).all()
    # (the tables are written with two decimals)
    assert abs(t.loc["average", "image_auroc"] - t.loc[["bottle", "carpet"], "image_auroc"].mean()) <= 0.011
