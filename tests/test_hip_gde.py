"""GPU: the Gaussian density estimator (GDE) scorer -- csrc/gde.hip, self_supervised/density.py, tools.inference(detector='gde').

The reference has no such scorer, so there is no reference vector: the yardstick is numpy / sklearn LedoitWolf / scipy mahalanobis in
float64 on the same fp32 rows (L2-normalised ones taken from ops.l2_normalize_rows, which both kernels reproduce bit for bit)."""
import shutil

import numpy as np
import pytest
import torch

import two_rank_util
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu


def _rows(n, d, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(d, generator=g) * 2.0
    a = torch.randn(d, d, generator=g) / d ** 0.5
    return (base + spread * (torch.randn(n, d, generator=g) @ a)).float()


def _ref_rows(x, normalize):
    from self_supervised import ops
    return (ops.l2_normalize_rows(x.cuda()) if normalize else x.cuda()).cpu().double().numpy()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("n", [1, 2, 37, 588, 5000])
def test_fit_stats_match_numpy_float64(n, d, normalize):
    from self_supervised import ops
    x = _rows(n, d, seed=n * 7 + d)
    xr = _ref_rows(x, normalize)
    mean, scatter, m4 = ops.gaussian_fit_stats(x.cuda(), normalize)
    mean2, scatter2, m42 = ops.gaussian_fit_stats(x.cuda(), normalize)
    assert torch.equal(mean, mean2) and torch.equal(scatter, scatter2) and torch.equal(m4, m42)     # deterministic
    want_mean = xr.mean(0)
    c = xr - want_mean
    want_sc = c.T @ c
    r = np.sum(c * c, axis=1)
    want_m4 = np.sum(r * r)
    mean, scatter, m4 = mean.cpu().numpy(), scatter.cpu().numpy(), m4.item()
    assert np.all(np.abs(mean - want_mean) <= 1e-10 * np.abs(xr).mean(0) + 1e-300)
    ac = np.abs(c)
    assert np.all(np.abs(scatter - want_sc) <= 1e-10 * (ac.T @ ac) + 1e-300)
    assert np.array_equal(scatter, scatter.T)
    assert abs(m4 - want_m4) <= 1e-10 * want_m4 + 1e-300


def test_fit_stats_scale_to_a_patch_bank():
    """841 patches x 200 images: the size of a patch-level bank over a whole training set."""
    from self_supervised import ops
    n, d = 841 * 200, 512
    x = _rows(n, d, seed=11)
    xr = _ref_rows(x, True)
    mean, scatter, m4 = ops.gaussian_fit_stats(x.cuda(), True)
    want_mean = xr.mean(0)
    c = xr - want_mean
    ac = np.abs(c)
    assert np.all(np.abs(mean.cpu().numpy() - want_mean) <= 1e-10 * np.abs(xr).mean(0))
    assert np.all(np.abs(scatter.cpu().numpy() - c.T @ c) <= 1e-10 * (ac.T @ ac))
    r = np.sum(c * c, axis=1)
    assert abs(m4.item() - np.sum(r * r)) <= 1e-10 * np.sum(r * r)


def _factor(xr):
    from self_supervised.density import ledoit_wolf_factor
    mean = xr.mean(0)
    c = xr - mean
    r = np.sum(c * c, axis=1)
    return ledoit_wolf_factor(mean, c.T @ c, np.sum(r * r), xr.shape[0])


def _maha_ref(qr, mu_hi, mu_lo, w):
    mu = mu_hi.astype(np.float64) + mu_lo.astype(np.float64)
    return np.linalg.norm((qr - mu) @ w.astype(np.float64).T, axis=1)


@pytest.mark.parametrize("d", [32, 64, 512])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 215296])
def test_mahalanobis_matches_numpy_float64(n, d):
    from self_supervised import ops
    fit = _rows(max(2 * d, 64), d, seed=d)
    mu_hi, mu_lo, w, _ = _factor(_ref_rows(fit, True))
    q = _rows(n, d, seed=1000 + n + d, spread=1.5)
    args = [torch.from_numpy(a).cuda() for a in (mu_hi, mu_lo, w)]
    got = ops.mahalanobis_fused(q.cuda(), *args, normalize=True).cpu().double().numpy()
    want = _maha_ref(_ref_rows(q, True), mu_hi, mu_lo, w)
    rel = np.abs(got - want) / want
    assert rel.max() <= 1e-4, (rel.max(), np.median(rel))
    # row independence: a row's score is the same bits alone and inside the launch, wherever it sits
    full = ops.mahalanobis_fused(q.cuda(), *args, normalize=True).cpu()
    for i in sorted({0, n // 2, n - 1, min(n - 1, 127), min(n - 1, 128)}):
        one = ops.mahalanobis_fused(q[i:i + 1].cuda(), *args, normalize=True).cpu()
        assert torch.equal(one[0], full[i]), i
    # without normalisation
    got = ops.mahalanobis_fused(q.cuda(), *args, normalize=False).cpu().double().numpy()
    want = _maha_ref(q.double().numpy(), mu_hi, mu_lo, w)
    assert (np.abs(got - want) / want).max() <= 1e-4


def test_mahalanobis_near_degenerate_rows_need_the_hi_lo_mean():
    """Rows at 1e-4 of their norm from the mean (what the seeded-weight embeddings of the fixtures look like): the hi + lo
    subtraction keeps the bar; a single fp32 mean would not."""
    from self_supervised import ops
    d = 512
    g = torch.Generator().manual_seed(5)
    base = torch.randn(d, generator=g)
    fit = (base + 1e-4 * base.norm() / d ** 0.5 * torch.randn(700, d, generator=g)).float()
    q = (base + 1e-4 * base.norm() / d ** 0.5 * 1.3 * torch.randn(300, d, generator=g)).float()
    mu_hi, mu_lo, w, _ = _factor(_ref_rows(fit, True))
    args = [torch.from_numpy(a).cuda() for a in (mu_hi, mu_lo, w)]
    got = ops.mahalanobis_fused(q.cuda(), *args, normalize=True).cpu().double().numpy()
    want = _maha_ref(_ref_rows(q, True), mu_hi, mu_lo, w)
    err = (np.abs(got - want) / want).max()
    assert err <= 1e-4, err
    lo0 = torch.zeros_like(args[1])
    single = ops.mahalanobis_fused(q.cuda(), args[0], lo0, args[2], normalize=True).cpu().double().numpy()
    err1 = (np.abs(single - want) / want).max()
    assert err1 > 100 * err, (err, err1)                       # the lo half carries most of the accuracy here


def _sk_scores(train, queries):
    from scipy.spatial.distance import mahalanobis
    from sklearn.covariance import LedoitWolf
    lw = LedoitWolf(assume_centered=False).fit(train)
    vi = np.linalg.inv(lw.covariance_)
    c = queries - lw.location_
    fast = np.sqrt(np.einsum("ij,jk,ik->i", c, vi, c))
    for i in (0, len(queries) // 2, len(queries) - 1):           # the vectorised form is scipy's mahalanobis
        assert abs(fast[i] - mahalanobis(queries[i], lw.location_, vi)) <= 1e-9 * fast[i]
    return fast


def test_detector_matches_sklearn_end_to_end():
    from sklearn.metrics import roc_auc_score
    from self_supervised.models import AnomalyDetector, GaussianDensityDetector, split_indices
    emb = _rows(841, 512, seed=21)
    np.random.seed(7)
    det = GaussianDensityDetector()
    det.fit(emb)
    st_gde = np.random.get_state()
    np.random.seed(7)
    AnomalyDetector().fit(emb)
    st_knn = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(st_gde, st_knn))     # same draws from the global numpy RNG
    np.random.seed(7)
    tr, va = split_indices(841, 0.3)
    rows = _ref_rows(emb, True)
    fresh = _rows(841 + 800, 512, seed=21)[841:]          # same distribution as emb, rows it has not seen
    shift = torch.randn(512, generator=torch.Generator().manual_seed(0)) * 0.05 * fresh.norm(dim=1).mean() / 512 ** 0.5
    q = torch.cat([fresh[:400], fresh[400:] + shift])      # 400 normal rows, 400 shifted "anomalous" ones
    labels = np.r_[np.zeros(400), np.ones(400)]
    got = det.predict(q).cpu().double().numpy()
    want = _sk_scores(rows[tr], _ref_rows(q, True))
    assert (np.abs(got - want) / want).max() <= 1e-4
    want_thr = _sk_scores(rows[tr], rows[va]).max()
    assert abs(det.threshold - want_thr) <= 1e-4 * want_thr
    assert abs(roc_auc_score(labels, got) - roc_auc_score(labels, want)) <= 1e-4
    # patch level: [batch, 1, dim, dim] in row order
    pd = GaussianDensityDetector(patch_level=True, batch=2, num_patches=841)
    pd.fit_bank(emb[tr])
    maps = pd.predict(emb.repeat(2, 1))
    assert tuple(maps.shape) == (2, 1, 29, 29)
    flat = det.predict(emb.repeat(2, 1))
    assert torch.equal(maps.reshape(-1), flat)
    # state round trip (the multi-rank broadcast)
    det2 = GaussianDensityDetector.from_state(det.state())
    assert torch.equal(det2.predict(q), det.predict(q))


@pytest.mark.parametrize("name,kw", [("knn", {"metric": "cosine"}), ("knn", {"metric": "euclidean"}), ("gde", {}),
                                     ("padim", {"factor": "host"}), ("padim", {"factor": "device"})])
def test_load_state_scores_like_the_fitted_detector(name, kw):
    """Every detector of models.DETECTORS, at its smallest legal shapes: state() loaded into a fresh instance constructed with the
    same arguments gives the bits of the fitted one (what a rank that receives the broadcast scores with)."""
    from self_supervised.models import DETECTORS
    if name == "padim":
        kw = {"patch_level": True, "batch": 6, "num_patches": 4, "channels": 32, **kw}        # 6 images x 4 positions x 32 columns
    elif name == "knn":
        kw = {"patch_level": True, "batch": 12, "num_patches": 4, **kw}                        # 48 rows x 32 columns
    bank, q = _rows(48 if name != "padim" else 24, 32, seed=31), _rows(48 if name != "padim" else 24, 32, seed=32, spread=1.5)
    fitted, fresh = DETECTORS[name](**kw), DETECTORS[name](**kw)
    fitted.fit(bank, split=False)
    fresh.load_state(fitted.state())
    want = fitted.predict(q)
    assert torch.isfinite(want).all() and want.min() > 0
    assert torch.equal(fresh.predict(q), want)
    if name != "gde":                   # (a Gaussian over all rows has no image score)
        assert torch.equal(fresh.image_scores(q, 'max'), fitted.image_scores(q, 'max', scores=want.reshape(-1)))


def _seeded_tree(tmp_path, seeded_sd):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=3, n_test_good=1, n_test_bad=1, size=96)
    for k in (1, 2):            # the normality image is the first of a shuffled loader: make the choice irrelevant
        shutil.copy(root + "bottle/train/good/000.png", root + f"bottle/train/good/{k:03d}.png")
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


def test_inference_gde_maps_match_float64(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import tools
    from self_supervised.density import GaussianDensityDetector
    from self_supervised.models import split_indices
    root, ck = _seeded_tree(tmp_path, seeded_sd)
    seen = {}
    orig = GaussianDensityDetector.fit

    def spy(self, embeddings, split=True):
        seen["rows"] = torch.as_tensor(embeddings).clone()
        seen["rng"] = np.random.get_state()
        return orig(self, embeddings, split)
    monkeypatch.setattr(GaussianDensityDetector, "fit", spy)
    np.random.seed(3)
    res = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, detector='gde')
    maps = res.anomaly_maps
    assert tuple(maps.shape) == (2, 1, 29, 29) and torch.isfinite(maps).all()
    rows = seen["rows"]
    assert rows.shape == (841, 512)
    np.random.set_state(seen["rng"])
    tr, _ = split_indices(841, 0.3)
    want = _sk_scores(_ref_rows(rows, True)[tr], _ref_rows(res.embedding_vectors.float(), True))
    got = maps.reshape(-1).double().numpy()
    assert (np.abs(got - want) / want).max() <= 1e-4, (np.abs(got - want) / want).max()
    # the maps go on through the rest of the pipeline
    res.anomaly_maps = tools.upsample(maps, int(res.ground_truths.shape[-1]), verbose=False)
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou'])
    ev.evaluate(res, "bottle", str(tmp_path / "out") + "/", patch_level=True)
    assert ev.scores.auroc is not None and np.isfinite(ev.scores.auroc)
    # the default is still the cosine 3-NN, bit for bit
    outs = []
    for kw in ({}, {"detector": "knn"}):
        np.random.seed(3)
        outs.append(tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, **kw).anomaly_maps)
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], maps)
    # image level: the bank is one embedding (quirk Q3)
    with pytest.raises(ValueError, match="at least 2 fit rows"):
        tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=False, detector='gde')


def test_inference_gde_two_ranks_equal_one_rank(tmp_path, seeded_sd):
    from self_supervised import tools
    root, ck = _seeded_tree(tmp_path, seeded_sd)
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "gde"])
    assert r["maps_equal_across_ranks"], r
    two = torch.load(str(tmp_path / "maps_rank0.pt"))
    one = two_rank_util.inference(tools, ck, root, "gde")
    assert torch.equal(two["embeddings"], one.embedding_vectors), "embeddings differ between the 2-rank and 1-rank runs"
    assert torch.equal(two["maps"], one.anomaly_maps)
