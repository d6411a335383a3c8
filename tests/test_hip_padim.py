"""GPU: the per-position Gaussian detector (PaDiM) -- csrc/padim.hip, self_supervised/density.py, tools.inference(detector='padim').

The reference has no such scorer: the yardstick is tests/padim_ref.py (numpy.cov + eps I, scipy's mahalanobis, float64).  The bars are
the project's own: 1e-10 of the magnitudes for the fp64 statistics and 1e-4 relative for the fp32 scores (tests/test_hip_gde.py)."""
import os

import numpy as np
import pytest
import torch

import padim_ref as R
import two_rank_util
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _sel(D, d, seed=0):
    from self_supervised.density import position_channels
    return position_channels(D, d, seed)


def _guarded(t, fill=NAN):
    """t as a view into a larger allocation whose rows before and after are NaN -> (view, whole)."""
    whole = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), fill, device="cuda", dtype=t.dtype)
    whole[1:-1] = t.cuda()
    return whole[1:-1], whole


def _guards_intact(whole):
    return bool(torch.isnan(whole[0]).all() and torch.isnan(whole[-1]).all())


# ------------------------------------------------------------------------------------------------------------ fit statistics

FIT_SHAPES = [(2, 1, 32, 32), (3, 5, 64, 32), (37, 7, 384, 96), (70, 3, 384, 160), (130, 2, 128, 128)]


@pytest.mark.parametrize("shape", FIT_SHAPES, ids=["x".join(map(str, s)) for s in FIT_SHAPES])
def test_fit_stats_match_numpy_float64(shape):
    from self_supervised import ops
    n, P, D, d = shape
    rows = R.synthetic_rows(n, P, D, seed=n + d)
    sel = _sel(D, d, seed=n)
    x, whole = _guarded(torch.from_numpy(rows).reshape(n, P * D))       # guard rows in front of image 0 and behind the last one
    x = x.reshape(n * P, D)
    mean, scatter = ops.position_gaussian_fit_stats(x, sel, n, P)
    mean2, scatter2 = ops.position_gaussian_fit_stats(x, sel, n, P)
    assert torch.equal(mean, mean2) and torch.equal(scatter, scatter2)                  # the same bits on a second call
    assert tuple(mean.shape) == (P, d) and tuple(scatter.shape) == (P, d, d) and mean.dtype == torch.float64
    want_mean, want_sc, bar_mean, bar_sc = R.stats(R.gather(rows, sel.numpy(), P))
    mean, scatter = mean.cpu().numpy(), scatter.cpu().numpy()
    assert np.isfinite(mean).all() and np.isfinite(scatter).all()
    em = (np.abs(mean - want_mean) / (bar_mean + 1e-300)).max()
    es = (np.abs(scatter - want_sc) / (bar_sc + 1e-300)).max()
    print(f"{shape}: mean {em:.2e} of mean|x|, scatter {es:.2e} of |c|^T|c| (bars 1e-10)")
    assert np.all(np.abs(mean - want_mean) <= 1e-10 * bar_mean + 1e-300)
    assert np.all(np.abs(scatter - want_sc) <= 1e-10 * bar_sc + 1e-300)
    assert np.array_equal(scatter, np.swapaxes(scatter, 1, 2))                          # the two triangles: the same bits
    assert _guards_intact(whole)


# ------------------------------------------------------------------------------------------------------------ scoring kernel

def _factor(P, D, d, seed, n_fit=None, eps=0.01, spread=1.0, gen=R.synthetic_rows):
    """(sel, mu_hi, mu_lo, W with a NaN upper triangle) as device tensors + host copies, from a float64 fit on the host."""
    from self_supervised.density import position_gaussian_factor
    n_fit = n_fit or 2 * d
    sel = _sel(D, d, seed)
    fit = gen(n_fit, P, D, seed)
    mean, scatter, _, _ = R.stats(R.gather(fit, sel.numpy(), P))
    mu_hi, mu_lo, w = position_gaussian_factor(mean, scatter, n_fit, eps)
    poisoned = w.copy()
    poisoned[:, np.triu_indices(d, 1)[0], np.triu_indices(d, 1)[1]] = np.nan          # the upper triangle must never be used
    dev = [torch.from_numpy(a).cuda() for a in (mu_hi, mu_lo, poisoned)]
    return sel, dev, (mu_hi, mu_lo, w)


def _score(rows, sel, dev, n, P):
    """The kernel over poisoned buffers: x a view between NaN guard images, out between NaN guard rows and pre-filled with NaN."""
    from self_supervised import ops
    D = rows.shape[1]
    x, xw = _guarded(torch.from_numpy(rows).reshape(n, P * D))
    ow = torch.full((n * P + 2 * P,), NAN, device="cuda")
    out = ops.position_mahalanobis(x.reshape(n * P, D), sel, *dev, n, P, out=ow[P:-P])
    torch.cuda.synchronize()
    assert torch.isnan(ow[:P]).all() and torch.isnan(ow[-P:]).all() and _guards_intact(xw)
    return out.cpu()


SCORE_SHAPES = [(1, 3, 64, 32), (127, 3, 64, 32), (128, 3, 64, 32), (129, 3, 64, 32), (40, 7, 384, 96), (40, 2, 384, 160),
                (9, 144, 384, 96), (129, 2, 256, 128), (40, 2, 256, 256)]          # the last two: d = D = exactly one / two W tiles


@pytest.mark.parametrize("shape", SCORE_SHAPES, ids=["x".join(map(str, s)) for s in SCORE_SHAPES])
def test_mahalanobis_matches_numpy_float64(shape):
    n, P, D, d = shape
    sel, dev, (mu_hi, mu_lo, w) = _factor(P, D, d, seed=d + P)
    q = R.synthetic_rows(n, P, D, seed=d + P, draw=1 + n, spread=1.5)
    got = _score(q, sel, dev, n, P)
    assert torch.isfinite(got).all(), "a NaN of W's upper triangle or of a guard row reached a score"
    want = R.scores_from_factor(q, sel.numpy(), P, mu_hi, mu_lo, w)
    rel = np.abs(got.double().numpy() - want) / want
    print(f"{shape}: max relative error {rel.max():.2e}, median {np.median(rel):.2e} (bar 1e-4)")
    assert rel.max() <= 1e-4, (rel.max(), np.median(rel))
    assert torch.equal(_score(q, sel, dev, n, P), got)                                  # the same bits on a second call


def test_scores_do_not_depend_on_the_launch():
    """An image's scores are the same bits alone and inside a launch, wherever it sits (also across the 128-image tile boundary);
    position p of a P-position launch equals the same data launched as P = 1."""
    from self_supervised import ops
    n, P, D, d = 131, 3, 64, 32
    sel, dev, _ = _factor(P, D, d, seed=3)
    q = R.synthetic_rows(n, P, D, seed=3, draw=5, spread=1.5)
    full = _score(q, sel, dev, n, P).reshape(n, P)
    rows = q.reshape(n, P, D)
    for i in (0, 1, 63, 127, 128, 130):
        trio = np.ascontiguousarray(rows[[5, 77, i]]).reshape(3 * P, D)
        assert torch.equal(_score(trio, sel, dev, 3, P).reshape(3, P)[2], full[i]), i
        assert torch.equal(_score(np.ascontiguousarray(rows[i]), sel, dev, 1, P).reshape(P), full[i]), i
    for p in range(P):
        one = [t[p:p + 1].contiguous() for t in dev]
        alone = _score(np.ascontiguousarray(rows[:, p]), sel, one, n, 1)
        assert torch.equal(alone, full[:, p]), p
    # the wrapper without an output buffer gives the same scores
    assert torch.equal(ops.position_mahalanobis(torch.from_numpy(q).cuda(), sel, *dev, n, P).cpu().reshape(n, P), full)


def _near_degenerate(n_img, P, D, seed, draw=0, spread=1.0):
    """Rows at 1e-4 of their norm from the position's mean (what seeded-weight features look like)."""
    base = np.random.RandomState(seed).randn(P, D)
    z = np.random.RandomState(seed * 1009 + draw + 1).randn(n_img, P, D)
    step = 1e-4 * np.linalg.norm(base, axis=1, keepdims=True) / np.sqrt(D)
    return (base + spread * step * z).reshape(n_img * P, D).astype(np.float32)


def test_near_degenerate_rows_keep_the_bar():
    n, P, D, d = 50, 3, 64, 32
    # eps far below the rows' variance (1e-8), so that W is the data's and not the regulariser's
    sel, dev, (mu_hi, mu_lo, w) = _factor(P, D, d, seed=9, n_fit=6 * d, eps=1e-12, gen=_near_degenerate)
    q = _near_degenerate(n, P, D, seed=9, draw=2, spread=1.3)
    got = _score(q, sel, dev, n, P).double().numpy()
    want = R.scores_from_factor(q, sel.numpy(), P, mu_hi, mu_lo, w)
    err = (np.abs(got - want) / want).max()
    print(f"near-degenerate rows: {err:.2e} (bar 1e-4)")
    assert err <= 1e-4, err


def test_bad_arguments_launch_nothing():
    from self_supervised import _hip, ops
    lib = _hip.lib()
    n, P, D, d = 3, 2, 64, 32
    i32, f64 = torch.int32, torch.float64
    x = torch.zeros(n * P, D, device="cuda")
    sel = torch.arange(d, device="cuda", dtype=i32)
    mu = torch.zeros(P, d, device="cuda")
    w = torch.zeros(P, d, d, device="cuda")
    out = torch.full((n * P,), NAN, device="cuda")
    mean = torch.full((P, d), NAN, device="cuda", dtype=f64)
    sc = torch.full((P, d, d), NAN, device="cuda", dtype=f64)
    xp, sp, mp, wp, op, mep, scp = (t.data_ptr() for t in (x, sel, mu, w, out, mean, sc))
    shapes = {"d % 32": (n, P, D, 48), "d < 32": (n, P, D, 0), "d > D": (n, P, D, 96), "D % 4": (n, P, 66, 32),
              "P < 1": (n, 0, D, d), "n_img < 1": (0, P, D, d)}
    score = {k: (xp, sp, mp, mp, wp, op) + v for k, v in shapes.items()}
    score.update({"null x": (None, sp, mp, mp, wp, op, n, P, D, d), "null sel": (xp, None, mp, mp, wp, op, n, P, D, d),
                  "null mu_hi": (xp, sp, None, mp, wp, op, n, P, D, d), "null mu_lo": (xp, sp, mp, None, wp, op, n, P, D, d),
                  "null w": (xp, sp, mp, mp, None, op, n, P, D, d), "null out": (xp, sp, mp, mp, wp, None, n, P, D, d)})
    for what, a in score.items():
        assert lib.ssad_position_mahalanobis(*a, _hip.stream()) == 2, what
        assert b"ssad_position_mahalanobis" in lib.ssad_last_error(), what
    fit = {k: (xp, sp) + v + (mep, scp) for k, v in shapes.items()}
    fit.update({"n_img < 2": (xp, sp, 1, P, D, d, mep, scp), "null x": (None, sp, n, P, D, d, mep, scp),
                "null sel": (xp, None, n, P, D, d, mep, scp), "null mean": (xp, sp, n, P, D, d, None, scp),
                "null scatter": (xp, sp, n, P, D, d, mep, None)})
    for what, a in fit.items():
        assert lib.ssad_position_gaussian_fit_stats(*a, _hip.stream()) == 2, what
        assert b"ssad_position_gaussian_fit_stats" in lib.ssad_last_error(), what
    # sel is checked on the host, where it lives, before the launch
    for bad in ([0] * 31 + [D], [-1] + [0] * 31):
        with pytest.raises(_hip.HipExtensionError, match="sel"):
            ops.position_mahalanobis(x, torch.tensor(bad), mu, mu, w, n, P, out=out)
        with pytest.raises(_hip.HipExtensionError, match="sel"):
            ops.position_gaussian_fit_stats(x, torch.tensor(bad), n, P)
    with pytest.raises(_hip.HipExtensionError, match="images"):
        ops.position_mahalanobis(x, torch.arange(d), mu, mu, w, n + 1, P, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(mean).all() and torch.isnan(sc).all()


# --------------------------------------------------------------------------------------------- detector against the reference

def test_detector_matches_the_reference_end_to_end():
    from sklearn.metrics import roc_auc_score
    from self_supervised.density import PositionGaussianDetector
    from self_supervised.models import split_rows
    P, D, d, n_all, n_q = 9, 64, 32, 96, 40                    # 96 images: the split keeps 67 >= 2 d for the fit
    emb = torch.from_numpy(R.synthetic_rows(n_all, P, D, seed=21))
    q = R.synthetic_rows(n_q, P, D, seed=21, draw=3).reshape(n_q, P, D)
    labels = np.zeros((n_q, P))
    rng = np.random.RandomState(4)
    for n, p in zip(rng.randint(0, n_q, 30), rng.randint(0, P, 30)):       # planted anomalies at known (image, position)
        q[n, p] += rng.randn(D).astype(np.float32) * 1.5
        labels[n, p] = 1
    q = q.reshape(n_q * P, D)
    np.random.seed(7)
    det = PositionGaussianDetector(batch=n_q, num_patches=P, channels=d)
    det.fit(emb)
    after = np.random.get_state()
    np.random.seed(7)
    tr, va = split_rows(n_all * P, torch.arange(n_all).repeat_interleave(P))
    assert all(np.array_equal(a, b) for a, b in zip(after, np.random.get_state()))      # the split split_rows draws, nothing else
    assert len(tr) == 67 * P and torch.equal(det.sel, _sel(D, d, 0))
    sel = det.sel.numpy()
    mean, _, vi = R.fit(emb.numpy()[tr], sel, P, eps=0.01)
    maps = det.predict(torch.from_numpy(q))
    assert tuple(maps.shape) == (n_q, 1, 3, 3)
    got = maps.reshape(-1).cpu().double().numpy()
    want = R.scores(q, sel, P, mean, vi)
    rel = (np.abs(got - want) / want).max()
    want_thr = R.scores(emb.numpy()[va], sel, P, mean, vi).max()
    print(f"detector: scores {rel:.2e}, threshold {abs(det.threshold - want_thr) / want_thr:.2e} (bars 1e-4)")
    assert rel <= 1e-4
    assert abs(det.threshold - want_thr) <= 1e-4 * want_thr
    auc_got, auc_want = roc_auc_score(labels.reshape(-1), got), roc_auc_score(labels.reshape(-1), want)
    assert abs(auc_got - auc_want) <= 1e-4 and auc_want > 0.9, (auc_got, auc_want)
    # the image score is the row maximum of the map, bit for bit
    img = det.image_scores(torch.from_numpy(q), 'max')
    assert torch.equal(img, maps.reshape(n_q, P).max(dim=1).values)
    assert torch.equal(det.image_scores(torch.from_numpy(q), 'max', scores=maps.reshape(-1)), img)
    # groups given = groups implied; fit_bank = the fit without a split
    np.random.seed(7)
    det_g = PositionGaussianDetector(batch=n_q, num_patches=P, channels=d)
    det_g.fit(emb, groups=torch.arange(n_all).repeat_interleave(P))
    assert det_g.threshold == det.threshold and torch.equal(det_g.w, det.w)
    det_b = PositionGaussianDetector(num_patches=P, channels=d)
    det_b.fit_bank(emb[torch.as_tensor(tr)])
    assert torch.equal(det_b.w, det.w) and torch.equal(det_b.predict(torch.from_numpy(q)), maps)
    # state round trip (the multi-rank broadcast): host tensors in, the same scores out
    st = det.state()
    assert set(st) >= {"sel", "mu_hi", "mu_lo", "w", "eps", "channels"} and not any(
        v.is_cuda for v in st.values() if torch.is_tensor(v))
    det2 = PositionGaussianDetector.from_state(st, batch=n_q, num_patches=P)
    assert (det2.channels, det2.eps) == (d, 0.01) and torch.equal(det2.predict(torch.from_numpy(q)), maps)


# ------------------------------------------------------------------------------------------------------ through tools.inference

SIZE, P96, N_TRAIN, CHANNELS = 96, 144, 48, 32          # 96 x 96 images: 12 x 12 maps; the split keeps 33 > 32 images for the fit
OPTS = {"channels": CHANNELS}


def _datamodule(root, **kw):
    from self_supervised.datasets import MVTecDatamodule
    return MVTecDatamodule(root, imsize=(SIZE, SIZE), **kw)


def _make(tmp_path, seeded_sd):
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=SIZE)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


@pytest.fixture()
def tree(tmp_path, seeded_sd, monkeypatch):
    """The fixture of tests/test_hip_patch_features.py with more training images: a synthetic category of 96 x 96 images, a seeded
    checkpoint, the datamodule tools.inference builds pinned to the files' own size (144 rows per image)."""
    from self_supervised import datasets, tools
    datasets._DataModule.num_workers = 0
    monkeypatch.setattr(tools, "MVTecDatamodule", _datamodule)
    return _make(tmp_path, seeded_sd)


def _spy(monkeypatch, cls, seen):
    orig = cls.fit

    def spy(self, embeddings, split=True, groups=None):
        seen["rows"] = torch.as_tensor(embeddings).detach().cpu().clone()
        seen["groups"] = None if groups is None else torch.as_tensor(groups).clone()
        seen["rng"] = np.random.get_state()
        orig(self, embeddings, split, groups)
        seen["detector"] = self
    monkeypatch.setattr(cls, "fit", spy)


def _standalone_rows(ck, root):
    """model(x)['latent_space'] of every training image in file order, in dense mode, outside tools.inference."""
    from self_supervised.models import PeraNet
    model = PeraNet.load_from_checkpoint(ck).eval()
    model.enable_dense_mode()
    model.enable_mvtec_inference()
    model.cuda()
    dm = _datamodule(root + "bottle/", batch_size=1)
    dm.setup()
    ds = dm.test_dataset
    ds.images_filenames = list(dm.train_images_filenames)
    x = torch.stack([ds[i][0] for i in range(len(ds))]).cuda()
    with torch.no_grad():
        return model(x)['latent_space'].cpu()


def _run(tools, ck, root, **kw):
    np.random.seed(3)
    return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, localization='dense',
                           bank='train', **kw)


def test_padim_through_inference(tree, tmp_path, monkeypatch):
    from self_supervised import tools
    from self_supervised.density import PositionGaussianDetector, position_gaussian_factor
    from self_supervised.models import split_rows
    root, ck = tree
    seen = {}
    _spy(monkeypatch, PositionGaussianDetector, seen)
    res = _run(tools, ck, root, detector='padim', detector_options=OPTS, image_scores='max')
    maps = res.anomaly_maps
    assert tuple(maps.shape) == (4, 1, 12, 12) and torch.isfinite(maps).all()
    rows, groups = seen["rows"], seen["groups"]
    assert tuple(rows.shape) == (N_TRAIN * P96, 384)
    assert torch.equal(rows, _standalone_rows(ck, root))                          # the fit rows are model(x) outside, bit for bit
    assert torch.equal(groups, torch.arange(N_TRAIN).repeat_interleave(P96))
    det = seen["detector"]
    assert (det.channels, det.eps, det.seed) == (CHANNELS, 0.01, 0)
    np.random.set_state(seen["rng"])
    tr, va = split_rows(rows.shape[0], groups)
    assert len(tr) == 33 * P96
    sel = det.sel.numpy()
    assert np.array_equal(sel, _sel(384, CHANNELS, 0).numpy())
    # the reference first, on the CPU: float64, and the same with W rounded to fp32 -- what that rounding alone costs on this data
    q = res.embedding_vectors.float().numpy()
    mean, _, vi = R.fit(rows.numpy()[tr], sel, P96, eps=0.01)
    want = R.scores(q, sel, P96, mean, vi)
    st_mean, st_sc, _, _ = R.stats(R.gather(rows.numpy()[tr], sel, P96))
    mu_hi, mu_lo, w32 = position_gaussian_factor(st_mean, st_sc, 33, 0.01)
    rounded = R.scores_from_factor(q, sel, P96, mu_hi, mu_lo, w32)
    cost = (np.abs(rounded - want) / want).max()
    got = maps.reshape(-1).double().numpy()
    err = (np.abs(got - want) / want).max()
    print(f"padim maps: {err:.2e} of the float64 reference (bar 1e-4); W rounded to fp32 alone costs {cost:.2e} (a quarter: 2.5e-5)")
    assert cost <= 0.25e-4, cost
    assert err <= 1e-4, err
    want_thr = R.scores(rows.numpy()[va], sel, P96, mean, vi).max()
    assert abs(det.threshold - want_thr) <= 1e-4 * want_thr
    # image scores: file order, the maps' row maxima
    assert tuple(res.image_scores.shape) == (4,)
    assert torch.equal(res.image_scores, maps.reshape(4, P96).max(dim=1).values)
    # the maps go on through the rest of the pipeline
    res.anomaly_maps = tools.upsample(maps, int(res.ground_truths.shape[-1]), verbose=False)
    assert tuple(res.anomaly_maps.shape) == (4, 1, SIZE, SIZE)
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou'])
    ev.evaluate(res, "bottle", str(tmp_path / "out") + "/", patch_level=True)
    assert ev.scores.auroc is not None and np.isfinite(ev.scores.auroc)
    assert np.isfinite(tools.image_auroc(res))


def test_padim_without_the_streamed_predict(tree, monkeypatch):
    from self_supervised import tools
    root, ck = tree
    res = _run(tools, ck, root, detector='padim', detector_options=OPTS, image_scores='max')
    monkeypatch.setenv("SSAD_FAST_PREDICT", "0")
    res0 = _run(tools, ck, root, detector='padim', detector_options=OPTS, image_scores='max')
    assert torch.equal(res0.anomaly_maps, res.anomaly_maps) and torch.equal(res0.image_scores, res.image_scores)


def test_padim_leaves_the_other_detectors_alone(tree):
    """knn and gde with the same arguments: bit-equal before and after a padim call in the same process."""
    from self_supervised import tools
    root, ck = tree
    before = [_run(tools, ck, root, detector=k).anomaly_maps for k in ('knn', 'gde')]
    default = _run(tools, ck, root).anomaly_maps
    pad = _run(tools, ck, root, detector='padim', detector_options=OPTS).anomaly_maps
    after = [_run(tools, ck, root, detector=k).anomaly_maps for k in ('knn', 'gde')]
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and torch.equal(default, before[0])
    assert not torch.equal(pad, before[0]) and not torch.equal(pad, before[1])
    # fewer training images than the fit needs for the default 96 channels is fine (the regulariser); an invalid width is not
    with pytest.raises(ValueError, match="channels"):
        _run(tools, ck, root, detector='padim', detector_options={"channels": 416})


def test_padim_sweep_one_category(tree, tmp_path):
    from self_supervised import tools
    root, ck = tree
    out = str(tmp_path / "sweep") + "/"
    os.makedirs(out + "bottle")
    os.replace(ck, out + "bottle/best_model.ckpt")
    np.random.seed(3)
    df = tools.sweep(root, out, ["bottle"], train=False, detector='padim', bank='train', localization='dense', image_scores='max',
                     detector_options=OPTS, tables_output=out + "tables/")
    assert list(df.index) == ["bottle", "average"] and np.isfinite(df.loc["bottle", "auroc"])
    assert os.path.exists(out + "tables/csv/patch_image_auroc.csv")


# ------------------------------------------------------------------------------------------------------------------ two ranks

def test_padim_two_ranks_equal_one_rank(tree, tmp_path, monkeypatch):
    """Two ranks over gloo sharing the one GPU (tests/dist_inference_worker.py, case padim): rank 0 fits and broadcasts (state,
    threshold), the other rank rebuilds the detector from the state -- maps, threshold and image scores are those of the one-rank
    run, bit for bit."""
    from self_supervised import tools
    from self_supervised.density import PositionGaussianDetector
    root, ck = tree
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "padim", CHANNELS, SIZE])
    assert r["equal_across_ranks"] and r["world"] == 2 and r["shape"] == [4, 1, 12, 12], r
    two = torch.load(str(tmp_path / "padim_rank0.pt"))
    seen = {}
    _spy(monkeypatch, PositionGaussianDetector, seen)
    one = two_rank_util.inference(tools, ck, root, "padim", channels=CHANNELS)
    assert torch.equal(two["embeddings"], one.embedding_vectors), "embeddings differ between the 2-rank and 1-rank runs"
    assert torch.equal(two["maps"], one.anomaly_maps) and torch.equal(two["image_scores"], one.image_scores)
    assert two["threshold"] == seen["detector"].threshold
