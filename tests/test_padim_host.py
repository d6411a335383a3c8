"""Host half of the per-position Gaussian detector (PaDiM; self_supervised/density.py, tools.py), no GPU: the factor against the
float64 reference of tests/padim_ref.py, the channel selection, and every refusal that must come before any file is read."""
import random

import numpy as np
import pytest
import torch

import padim_ref as R


def _case(n, P, D, d, seed):
    from self_supervised.density import position_channels
    rows = R.synthetic_rows(n, P, D, seed)
    sel = position_channels(D, d, seed).numpy()
    return rows, sel


@pytest.mark.parametrize("n,P,D,d,seed", [(70, 5, 64, 32, 0), (40, 3, 128, 96, 1), (300, 2, 64, 64, 2), (2, 4, 32, 32, 3)])
def test_factor_matches_the_reference(n, P, D, d, seed):
    """W^T W = inv(Sigma) to 1e-9 of inv(Sigma)'s largest entry in float64, before the fp32 rounding (n < d, n > d and n = 2: the
    regulariser alone keeps Sigma positive definite); W lower triangular; mu_hi + mu_lo carries the fp64 mean."""
    from self_supervised.density import position_gaussian_factor
    rows, sel = _case(n, P, D, d, seed)
    mean, scatter, _, _ = R.stats(R.gather(rows, sel, P))
    want_mean, cov, vi = R.fit(rows, sel, P, eps=0.01)
    assert np.abs(scatter / (n - 1) + 0.01 * np.eye(d) - cov).max() <= 1e-12 * np.abs(cov).max()
    mu_hi, mu_lo, w64 = position_gaussian_factor(mean, scatter, n, 0.01, dtype=np.float64)
    assert w64.shape == (P, d, d) and w64.dtype == np.float64
    for p in range(P):
        err = np.abs(w64[p].T @ w64[p] - vi[p]).max() / np.abs(vi[p]).max()
        assert err <= 1e-9, (p, err)
    assert np.array_equal(np.triu(w64, 1), np.zeros_like(w64))
    mu_hi32, mu_lo32, w = position_gaussian_factor(mean, scatter, n, 0.01)
    assert w.dtype == np.float32 and mu_hi32.dtype == np.float32 and mu_lo32.dtype == np.float32
    assert np.array_equal(w, w64.astype(np.float32)) and np.array_equal(np.triu(w, 1), np.zeros_like(w))
    assert np.array_equal(mu_hi, mu_hi32) and np.array_equal(mu_lo, mu_lo32) and mu_hi.shape == (P, d)
    ulp = np.spacing(np.abs(want_mean).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(mu_hi.astype(np.float64) + mu_lo.astype(np.float64) - want_mean) <= ulp * 2.0 ** -20 + 1e-300)
    # the factor's scores are the reference's
    q = R.synthetic_rows(5, P, D, seed, draw=1, spread=1.5)
    got = R.scores_from_factor(q, sel, P, mu_hi, mu_lo, w64)
    want = R.scores(q, sel, P, want_mean, vi)
    assert (np.abs(got - want) / want).max() <= 1e-9


def test_factor_refusals():
    from self_supervised.density import position_gaussian_factor
    m, s = np.zeros((2, 32)), np.zeros((2, 32, 32))
    with pytest.raises(ValueError, match="at least 2"):
        position_gaussian_factor(m, s, 1, 0.01)
    for eps in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            position_gaussian_factor(m, s, 5, eps)
    with pytest.raises(ValueError, match="scatter"):
        position_gaussian_factor(m, s[:1], 5, 0.01)


def test_channel_selection_is_reproducible_and_draws_nothing_global():
    from self_supervised.density import position_channels
    torch.manual_seed(11)
    np.random.seed(12)
    random.seed(13)
    before = (torch.get_rng_state().clone(), np.random.get_state(), random.getstate())
    a, b = position_channels(384, 96, 0), position_channels(384, 96, 0)
    other = position_channels(384, 96, 1)
    full = position_channels(128, 128, 5)
    assert torch.equal(torch.get_rng_state(), before[0])
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), before[1]))
    assert random.getstate() == before[2]
    assert a.dtype == torch.int64 and tuple(a.shape) == (96,) and torch.equal(a, b) and not torch.equal(a, other)
    assert torch.equal(a, a.sort().values) and len(set(a.tolist())) == 96 and 0 <= int(a.min()) and int(a.max()) < 384
    g = torch.Generator().manual_seed(0)
    assert torch.equal(a, torch.randperm(384, generator=g)[:96].sort().values)
    assert torch.equal(full, torch.arange(128))
    for d in (0, 16, 33, 100, 416, True, 96.0, None):
        with pytest.raises(ValueError, match="channels"):
            position_channels(384, d, 0)


def test_detector_refusals_come_before_any_gpu_work():
    from self_supervised.density import PositionGaussianDetector
    from self_supervised.models import PositionGaussianDetector as Reexported
    assert Reexported is PositionGaussianDetector
    with pytest.raises(ValueError, match="patch-level"):
        PositionGaussianDetector(patch_level=False, num_patches=9)
    with pytest.raises(ValueError, match="patch-level"):
        PositionGaussianDetector()
    for ch in (0, 31, 100, True, 96.0):
        with pytest.raises(ValueError, match="channels"):
            PositionGaussianDetector(num_patches=9, channels=ch)
    with pytest.raises(ValueError, match="eps"):
        PositionGaussianDetector(num_patches=9, eps=0.0)
    det = PositionGaussianDetector(num_patches=9, channels=32)
    assert (det.channels, det.eps, det.seed, det.dim, det.threshold) == (32, 0.01, 0, 3, None)
    assert PositionGaussianDetector(num_patches=9).channels == 96
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="whole images"):
        det.fit(torch.zeros(9 * 5 + 1, 64))
    with pytest.raises(ValueError, match="whole images"):
        det.fit_bank(torch.zeros(8, 64))
    with pytest.raises(ValueError, match="at least 2 fit images"):
        det.fit(torch.zeros(9 * 2, 64))                 # the 70/30 split of 2 images leaves one
    with pytest.raises(ValueError, match="at least 2 fit images"):
        det.fit_bank(torch.zeros(9, 64))
    with pytest.raises(ValueError, match="channels"):
        PositionGaussianDetector(num_patches=9, channels=96).fit(torch.zeros(9 * 10, 64))      # 96 channels of 64 columns
    with pytest.raises(ValueError, match="groups"):
        det.fit(torch.zeros(9 * 10, 64), groups=torch.arange(90) // 10)                         # images of 10 rows
    assert np.array_equal(np.random.get_state()[1], state)      # nothing drawn before a refusal
    with pytest.raises(ValueError, match="'max'"):
        det.image_scores(torch.zeros(9, 64), mode='reweighted')
    with pytest.raises(ValueError, match="not fitted"):
        det._scores(torch.zeros(9, 64))
    assert PositionGaussianDetector.fit_images(3) == 2 and PositionGaussianDetector.fit_images(2, split=False) == 2


def test_padim_has_no_cpu_fallback_without_a_gpu():
    """A check for machines without a GPU (with one the fit simply runs: tests/test_hip_padim.py covers that side)."""
    from self_supervised.density import PositionGaussianDetector
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError):
        PositionGaussianDetector(num_patches=4, channels=32).fit_bank(torch.randn(4 * 8, 64))


PADIM = {"detector": "padim", "patch_localization": True, "localization": "dense", "bank": "train"}


@pytest.mark.parametrize("kw,match", [
    ({**PADIM, "patch_localization": False, "localization": "patches"}, "patch_localization=True"),
    ({**PADIM, "localization": "patches"}, "localization='dense'"),
    ({**PADIM, "bank": "reference"}, "bank='train'"),
    ({**PADIM, "coreset": 0.1}, "coreset"),
    ({**PADIM, "image_scores": "reweighted"}, "reweighted"),
    ({**PADIM, "detector_options": {"channels": 100}}, "channels"),
    ({**PADIM, "detector_options": {"eps": 0.0}}, "eps"),
    ({**PADIM, "detector_options": {"normalize": True}}, "detector_options"),
    ({**PADIM, "detector_options": [96]}, "detector_options"),
    ({**PADIM, "detector": "knn", "detector_options": {"channels": 32}}, "detector_options"),
    ({**PADIM, "detector": "gde", "detector_options": {}}, "detector_options")])
def test_tools_refuse_from_the_arguments_alone(tmp_path, kw, match):
    """A dataset and a checkpoint that do not exist: the ValueError comes from the arguments, before anything is read."""
    from self_supervised import tools
    missing = str(tmp_path / "nowhere") + "/"
    with pytest.raises(ValueError, match=match):
        tools.inference(missing + "best_model.ckpt", missing, "bottle", mvtec_inference=True, **kw)
    with pytest.raises(ValueError, match=match):
        tools.sweep(missing, missing, ["bottle"], train=False, **kw)


def test_padim_is_a_known_detector_and_image_scores_max_is_allowed(tmp_path):
    from self_supervised import tools
    assert tuple(tools.DETECTORS) == ('knn', 'gde', 'padim')
    assert tools._check_image_scores('max', 9, True, 'padim') == 'max'
    assert tools._check_padim('padim', True, 'dense', 'train', {"channels": 32, "seed": 4}) == {"channels": 32, "seed": 4}
    assert tools._check_padim('knn', False, 'patches', 'reference', None) == {}
    # with valid arguments the first failure is the missing data: a file error, not a ValueError about the arguments
    missing = str(tmp_path / "nowhere") + "/"
    with pytest.raises(FileNotFoundError):
        tools.inference(missing + "best_model.ckpt", missing, "bottle", image_scores='max', detector_options={"channels": 32}, **PADIM)
