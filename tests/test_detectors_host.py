"""Host half of what the three detectors share (self_supervised/detectors.py: the fit template, state / load_state) and of the detector
registry (models.DETECTORS, tools._check_options), no GPU.  `_dev` and the device ops are replaced by plain-torch stand-ins, as in tests/test_knn_l2_host.py: what
is under test is the host code around them -- when the global numpy generator is drawn from, which rows reach fit_bank, what
travels in a state."""
import numpy as np
import pytest
import torch

P, D, N_IMG = 4, 32, 6          # positions per image, columns, images: the smallest shapes PaDiM takes (channels = 32)


@pytest.fixture
def detectors(monkeypatch):
    """{name: constructor} of the three classes over CPU stand-ins; every fit_bank call appends (name, its rows) to ["banks"]."""
    from self_supervised import ops
    from self_supervised.density import position_gaussian_factor
    from self_supervised.models import DETECTORS

    def gaussian_stats(x, normalize):
        x = x.double() / x.double().norm(dim=1, keepdim=True) if normalize else x.double()
        c = x - x.mean(0)
        return x.mean(0), c.t() @ c, (c * c).sum(1).pow(2).sum()

    def position_stats(x, sel, n_img, p, sel_dev=None):
        g = x.double().reshape(n_img, p, -1)[:, :, sel]
        c = g - g.mean(0)
        return g.mean(0), torch.einsum('npi,npj->pij', c, c)

    def position_scores(x, sel, mu_hi, mu_lo, w, n_img, p, sel_dev=None):
        c = x.reshape(n_img, p, -1)[:, :, sel] - mu_hi - mu_lo
        return torch.einsum('pij,npj->npi', w, c).norm(dim=2).reshape(-1)
    for name, fn in (("l2_normalize_rows", lambda x: x / x.norm(dim=1, keepdim=True)),
                     ("cosine_knn_fused", lambda x, b, k: (1 - (x / x.norm(dim=1, keepdim=True)) @ b.t()).topk(k, largest=False).values.mean(1)),
                     ("row_sqnorms", lambda x: (x * x).sum(1)),
                     ("l2_knn_fused", lambda x, b, bsq, k=3, splits=None: torch.cdist(x, b).topk(k, largest=False).values.mean(1)),
                     ("gaussian_fit_stats", gaussian_stats),
                     ("mahalanobis_fused", lambda x, hi, lo, w, nrm: ((x / x.norm(dim=1, keepdim=True) if nrm else x) - hi - lo).matmul(w.t()).norm(dim=1)),
                     ("position_sel", lambda sel, width, device: torch.as_tensor(sel).to(torch.int32)),
                     ("position_gaussian_fit_stats", position_stats), ("position_mahalanobis", position_scores),
                     # (factor='device' has no kernel here: the host factor stands in for it, as tensors)
                     ("position_gaussian_factor", lambda mean, scatter, n, eps: [torch.from_numpy(a) for a in position_gaussian_factor(
                         mean.numpy(), scatter.numpy(), n, eps)]),
                     ("rows_argmax", lambda s: (s.max(1).values, s.argmax(1) + torch.arange(s.shape[0]) * s.shape[1]))):
        monkeypatch.setattr(ops, name, fn)
    banks = []
    for name, cls in DETECTORS.items():
        monkeypatch.setattr(cls, "_dev", staticmethod(lambda t: torch.as_tensor(t, dtype=torch.float32).contiguous()))

        def fit_bank(self, bank, _name=name, _orig=cls.fit_bank):
            banks.append((_name, torch.as_tensor(bank).clone()))
            _orig(self, bank)
        monkeypatch.setattr(cls, "fit_bank", fit_bank)
    make = {name: (lambda cls=cls, **kw: cls(patch_level=True, batch=N_IMG, num_patches=P, **kw)) for name, cls in DETECTORS.items()}
    make["padim"] = lambda factor='host': DETECTORS["padim"](batch=N_IMG, num_patches=P, channels=D, factor=factor)
    make["banks"] = banks
    return make


def _rows(seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((N_IMG * P, D), generator=g), torch.arange(N_IMG).repeat_interleave(P)


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _state_after_permutation(seed, n):
    np.random.seed(seed)
    np.random.permutation(n)
    return np.random.get_state()


@pytest.mark.parametrize("name", ["knn", "gde", "padim"])
def test_fit_draws_one_permutation_when_it_splits_and_none_otherwise(detectors, name):
    emb, groups = _rows()
    for given, drawn_over in ((groups, N_IMG), (None, N_IMG if name == "padim" else N_IMG * P)):    # PaDiM implies the images
        want = _state_after_permutation(7, drawn_over)
        np.random.seed(7)
        det = detectors[name]()
        det.fit(emb, True, given)
        assert _same_state(np.random.get_state(), want), (name, given is None)
        assert np.isfinite(det.threshold)
    np.random.seed(7)
    before = np.random.get_state()
    detectors[name]().fit(emb, False, groups)
    assert _same_state(np.random.get_state(), before)
    assert torch.equal(detectors["banks"][-1][1], emb)              # split=False fits on every row


def test_the_three_classes_fit_on_the_same_rows(detectors):
    from self_supervised.detectors import split_rows
    emb, groups = _rows(1)
    for name in ("knn", "gde", "padim"):
        np.random.seed(11)
        detectors[name]().fit(emb, True, groups)
    np.random.seed(11)
    train, held_out = split_rows(emb.shape[0], groups, 0.3)
    assert len(held_out) == 2 * P and [n for n, _ in detectors["banks"]] == ["knn", "gde", "padim"]
    for _, bank in detectors["banks"]:
        assert torch.equal(bank, emb[train])


def test_a_refusal_before_the_draw_leaves_the_generator_alone(detectors):
    np.random.seed(13)
    before = np.random.get_state()
    with pytest.raises(ValueError, match="at least 2 fit rows"):
        detectors["gde"]().fit(torch.zeros(1, D))
    with pytest.raises(ValueError, match="whole images"):
        detectors["padim"]().fit(torch.zeros(N_IMG * P + 1, D))
    assert _same_state(np.random.get_state(), before) and detectors["banks"] == []


@pytest.mark.parametrize("name,kw,tensors", [("knn", {}, ("bank",)), ("knn", {"metric": "euclidean"}, ("bank", "bank_sq")),
                                             ("gde", {}, ("mu_hi", "mu_lo", "w")),
                                             ("padim", {"factor": "host"}, ("sel", "_sel_dev", "mu_hi", "mu_lo", "w")),
                                             ("padim", {"factor": "device"}, ("sel", "_sel_dev", "mu_hi", "mu_lo", "w"))])
def test_load_state_restores_what_state_carries(detectors, name, kw, tensors):
    emb, groups = _rows(2)
    fitted = detectors[name](**kw)
    fitted.fit(emb, True, groups)
    fresh = detectors[name](**kw)
    fresh.load_state(fitted.state())
    loaded = [fresh] if name == "knn" else [fresh, type(fitted).from_state(fitted.state(), batch=N_IMG, num_patches=P)]
    for det in loaded:
        for t in tensors:
            assert torch.equal(getattr(det, t), getattr(fitted, t)), t
        assert torch.equal(det._scores(emb), fitted._scores(emb))
    if name == "gde":
        assert all(det.shrinkage == fitted.shrinkage and det.normalize == fitted.normalize for det in loaded)
    if name == "padim":
        assert loaded[1].factor == kw["factor"] and loaded[1].channels == D


def test_registry_and_option_check():
    from self_supervised import models, tools
    from self_supervised.models import AnomalyDetector, GaussianDensityDetector, PositionGaussianDetector
    assert list(models.DETECTORS.items()) == [('knn', AnomalyDetector), ('gde', GaussianDensityDetector),
                                              ('padim', PositionGaussianDetector)]
    assert tools.DETECTORS == tuple(models.DETECTORS)          # tools keeps the names, in the registry's order
    # (detector, metric, localization, patch_localization, bank, mvtec_inference, coreset, image_scores, neighbours, detector_options)
    assert tools._check_options('knn', 'cosine', 'patches', False, 'reference', True, None, None, 9, None) == (AnomalyDetector, {})
    assert tools._check_options('knn', 'euclidean', 'dense', True, 'train', True, 0.25, 'reweighted', 5, None) == \
        (AnomalyDetector, {"coreset": 0.25, "metric": "euclidean"})
    assert tools._check_options('gde', 'cosine', 'patches', True, 'train', True, None, None, 9, None) == (GaussianDensityDetector, {})
    opts = {"channels": 32, "factor": "device"}
    assert tools._check_options('padim', 'cosine', 'dense', True, 'train', True, None, 'max', 9, opts) == (PositionGaussianDetector, opts)
    with pytest.raises(ValueError, match=r"detector must be one of \('knn', 'gde', 'padim'\), got 'svm'"):
        tools._check_options('svm', 'cosine', 'patches', False, 'reference', True, None, None, 9, None)
