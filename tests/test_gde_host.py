"""Host half of the GDE scorer (self_supervised/density.py), no GPU: the Ledoit-Wolf restatement against sklearn in float64."""
import numpy as np
import pytest
import torch
from sklearn.covariance import LedoitWolf


def _stats(x):
    mean = x.mean(0)
    c = x - mean
    return mean, c.T @ c, float(np.sum(np.sum(c * c, axis=1) ** 2))


def _sample(n, d, seed):
    rng = np.random.RandomState(seed)
    a = rng.randn(d, d) / np.sqrt(d)
    return (rng.randn(n, d) @ a + rng.randn(d) * 3.0).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("n,d,seed", [(40, 64, 0), (300, 64, 1), (2, 32, 2), (700, 128, 3)])
def test_ledoit_wolf_covariance_matches_sklearn(n, d, seed):
    """n < D, n > D and n = 2: shrinkage and shrunk covariance to 1e-12 relative."""
    from self_supervised.density import ledoit_wolf_covariance
    x = _sample(n, d, seed)
    shrunk, s = ledoit_wolf_covariance(*_stats(x), n)
    lw = LedoitWolf(assume_centered=False).fit(x)
    assert abs(s - lw.shrinkage_) <= 1e-12 * abs(lw.shrinkage_) or abs(s - lw.shrinkage_) <= 1e-15
    assert np.abs(shrunk - lw.covariance_).max() <= 1e-12 * np.abs(lw.covariance_).max()


def test_ledoit_wolf_factor_refuses_two_rows():
    """At n = 2 sklearn's shrinkage is 0 and its covariance has rank 1: the factor says so instead of returning garbage."""
    from self_supervised.density import ledoit_wolf_factor
    x = _sample(2, 32, 2)
    assert LedoitWolf().fit(x).shrinkage_ <= 1e-12
    with pytest.raises(ValueError, match="singular"):
        ledoit_wolf_factor(*_stats(x), 2)


@pytest.mark.parametrize("n,d,seed", [(40, 64, 0), (300, 64, 1), (700, 128, 3)])
def test_ledoit_wolf_factor_matches_sklearn(n, d, seed):
    from self_supervised.density import ledoit_wolf_factor
    x = _sample(n, d, seed)
    mean, scatter, m4 = _stats(x)
    mu_hi, mu_lo, w, s = ledoit_wolf_factor(mean, scatter, m4, n)
    lw = LedoitWolf(assume_centered=False).fit(x)
    assert abs(s - lw.shrinkage_) <= 1e-12 * abs(lw.shrinkage_)
    # W^T W is the precision: W^T W Sigma = I (W is rounded to fp32: that error, scaled by the condition number, is the bar)
    wd = w.astype(np.float64)
    assert np.allclose(np.triu(wd, 1), 0.0)
    cond = np.linalg.cond(lw.covariance_)
    assert np.abs(wd.T @ wd @ lw.covariance_ - np.eye(d)).max() <= 1e-6 * cond
    # mu_hi + mu_lo carries the fp64 mean to far below an fp32 ulp of it
    ulp = np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(mu_hi.astype(np.float64) + mu_lo.astype(np.float64) - mean) <= ulp * 2.0 ** -20)
    assert mu_hi.dtype == np.float32 and mu_lo.dtype == np.float32 and w.dtype == np.float32


def test_ledoit_wolf_factor_scores_equal_scipy_mahalanobis():
    from scipy.spatial.distance import mahalanobis
    from self_supervised.density import ledoit_wolf_factor
    rng = np.random.RandomState(5)
    x = rng.randn(90, 32)
    mean, scatter, m4 = _stats(x)
    mu_hi, mu_lo, w, _ = ledoit_wolf_factor(mean, scatter, m4, 90)
    lw = LedoitWolf().fit(x)
    vi = np.linalg.inv(lw.covariance_)
    q = rng.randn(7, 32)
    got = np.linalg.norm((q - mean) @ w.astype(np.float64).T, axis=1)
    want = np.array([mahalanobis(r, lw.location_, vi) for r in q])
    assert np.abs(got - want).max() <= 1e-5 * want.max()


def test_fewer_than_two_fit_rows_raise_value_error():
    from self_supervised.density import GaussianDensityDetector, ledoit_wolf_factor
    from self_supervised.models import GaussianDensityDetector as Reexported
    assert Reexported is GaussianDensityDetector
    with pytest.raises(ValueError, match="at least 2"):
        ledoit_wolf_factor(np.zeros(32), np.zeros((32, 32)), 0.0, 1)
    det = GaussianDensityDetector()
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="at least 2 fit rows"):
        det.fit(torch.zeros(1, 512))                 # the image-level bank of tools.inference (quirk Q3)
    with pytest.raises(ValueError, match="at least 2 fit rows"):
        det.fit(torch.zeros(2, 512))                 # 70/30 split of 2 rows leaves one
    with pytest.raises(ValueError, match="at least 2 fit rows"):
        det.fit_bank(torch.zeros(1, 512))
    assert np.array_equal(np.random.get_state()[1], state)      # nothing drawn before the refusal


def test_detector_kind_is_checked_before_the_checkpoint_is_read(tmp_path):
    from self_supervised import tools
    with pytest.raises(ValueError, match="detector"):
        tools.inference(str(tmp_path / "missing.ckpt"), str(tmp_path), "bottle", patch_localization=True, detector="mahalanobis")
    with pytest.raises(ValueError, match="detector"):
        tools.sweep(str(tmp_path), str(tmp_path), ["bottle"], detector="GDE", train=False)


def test_gde_has_no_cpu_fallback():
    from self_supervised.density import GaussianDensityDetector
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            GaussianDensityDetector().fit_bank(torch.randn(8, 512))
        with pytest.raises(RuntimeError):
            GaussianDensityDetector(patch_level=True, batch=1, num_patches=4).fit(torch.randn(8, 512))
