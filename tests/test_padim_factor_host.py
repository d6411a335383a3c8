"""Host half of PositionGaussianDetector(factor='device') (self_supervised/density.py, tools.py), no GPU: the option's plumbing and
refusals, and the yardsticks of tests/padim_factor_ref.py against themselves.  The kernel's side is tests/test_hip_padim_factor.py."""
import numpy as np
import pytest
import torch
from scipy.linalg import solve_triangular

import padim_factor_ref as F
import padim_ref as R

PADIM = {"detector": "padim", "patch_localization": True, "localization": "dense", "bank": "train"}


def test_constructor_takes_factor():
    from self_supervised.density import PositionGaussianDetector
    assert PositionGaussianDetector(num_patches=9).factor == 'host'
    assert PositionGaussianDetector(num_patches=9, factor='host').factor == 'host'
    assert PositionGaussianDetector(num_patches=9, channels=32, factor='device').factor == 'device'
    for bad in ('gpu', 'Device', None, 1, ''):
        with pytest.raises(ValueError, match="factor"):
            PositionGaussianDetector(num_patches=9, factor=bad)
    # the kernel's width limit is the constructor's; the host factor has none
    assert PositionGaussianDetector(num_patches=9, channels=512, factor='device').channels == 512
    assert PositionGaussianDetector(num_patches=9, channels=544, factor='host').channels == 544
    with pytest.raises(ValueError, match="512"):
        PositionGaussianDetector(num_patches=9, channels=544, factor='device')


def test_tools_pass_factor_through_and_refuse_from_the_arguments_alone(tmp_path):
    from self_supervised import tools
    assert 'factor' in tools.PADIM_OPTIONS
    opts = {"channels": 32, "factor": "device"}
    assert tools._check_padim('padim', True, 'dense', 'train', opts) == opts
    with pytest.raises(ValueError, match="factor"):
        tools._check_padim('padim', True, 'dense', 'train', {"factor": "gpu"})
    missing = str(tmp_path / "nowhere") + "/"           # neither a dataset nor a checkpoint: nothing can be read
    with pytest.raises(ValueError, match="factor"):
        tools.inference(missing + "best_model.ckpt", missing, "bottle", mvtec_inference=True, detector_options={"factor": "gpu"},
                        **PADIM)
    with pytest.raises(ValueError, match="factor"):
        tools.sweep(missing, missing, ["bottle"], train=False, detector_options={"factor": "gpu"}, **PADIM)
    with pytest.raises(FileNotFoundError):              # a valid value gets as far as the files
        tools.inference(missing + "best_model.ckpt", missing, "bottle", image_scores='max', detector_options=opts, **PADIM)


def _fitted(factor):
    """A detector with hand-made members (no GPU): what state() reads."""
    from self_supervised.density import PositionGaussianDetector
    det = PositionGaussianDetector(num_patches=4, channels=32, factor=factor)
    det.sel = torch.arange(32)
    det.mu_hi, det.mu_lo, det.w = torch.zeros(4, 32), torch.zeros(4, 32), torch.zeros(4, 32, 32)
    return det


def test_state_carries_factor_and_a_missing_key_reads_as_host(monkeypatch):
    from self_supervised import ops
    from self_supervised.density import PositionGaussianDetector
    monkeypatch.setattr(PositionGaussianDetector, "_dev", staticmethod(lambda t: torch.as_tensor(t, dtype=torch.float32)))
    monkeypatch.setattr(ops, "position_sel", lambda sel, D, device: torch.as_tensor(sel).to(torch.int32))
    for factor in ('host', 'device'):
        st = _fitted(factor).state()
        assert st["factor"] == factor
        assert PositionGaussianDetector.from_state(st, num_patches=4).factor == factor
    st = _fitted('device').state()
    del st["factor"]                                    # a state from before the option
    assert PositionGaussianDetector.from_state(st, num_patches=4).factor == 'host'


@pytest.mark.parametrize("n,d,eps,scale", [(2, 32, 0.01, False), (48, 96, 0.01, False), (200, 96, 0.01, True), (64, 64, 1e-6, False)])
def test_yardsticks_hold_for_float64_factors(n, d, eps, scale):
    """LAPACK's factor (numpy / scipy) and the textbook recurrences in the kernel's order both sit under the two bars, and a factor
    that is wrong in one element by 1e-6 relative does not: the bars can fail."""
    rows = R.synthetic_rows(n, 1, d, seed=n + d)
    if scale:
        rows = rows * np.logspace(-3, 3, d).astype(np.float32)
    _, scatter, _, _ = R.stats(R.gather(rows, np.arange(d), 1))
    poisoned = scatter.copy()
    poisoned[:, np.triu_indices(d, 1)[0], np.triu_indices(d, 1)[1]] = np.nan
    sigma = F.sigma_from_stats(poisoned, n, eps)[0]
    want = scatter[0] / (n - 1) + eps * np.eye(d)
    assert np.array_equal(np.tril(sigma), np.tril(want)) and np.array_equal(sigma, sigma.T)
    c = np.linalg.cholesky(sigma)
    w = solve_triangular(c, np.eye(d), lower=True)
    cm, wm = F.factor_model(sigma)
    ratios = [F.cholesky_ratio(c, sigma), F.cholesky_ratio(cm, sigma), F.inverse_ratio(wm, cm)]
    print(f"n {n} d {d}: cholesky {ratios[0]:.3f} (LAPACK) {ratios[1]:.3f} (model), inverse {ratios[2]:.3f} (model) of the bars")
    assert max(ratios) <= 1.0, ratios
    assert F.inverse_ratio(w, c) == 0.0                 # the reference against itself
    bad = c.copy()
    bad[d // 2, d // 3] *= 1.0 + 1e-6
    assert F.cholesky_ratio(bad, sigma) > 1.0
    bad = wm.copy()
    bad[d - 1, 0] *= 1.0 + 1e-6
    assert F.inverse_ratio(bad, cm) > 1.0
    assert F.gamma(d + 1) > (d + 1) * F.U and F.gamma(d + 1) < (d + 1.001) * F.U


def test_factor_model_reports_a_bad_pivot():
    with pytest.raises(ValueError, match="pivot 0"):
        F.factor_model(-np.eye(32))
    s = np.eye(32)
    s[5, 5] = np.nan
    with pytest.raises(ValueError, match="pivot 5"):
        F.factor_model(s)
