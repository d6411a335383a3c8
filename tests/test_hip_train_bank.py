"""GPU: scoring against the whole normal training set -- the bank-split cosine kNN (csrc/knn.hip ssad_cosine_knn_split) and
tools.inference(bank='train').

The split kernel must give the bits of ssad_cosine_knn_fused for every split count (min / max selection, same distance expression and
K order), so that the dispatcher may pick S freely; the float64 yardstick is a numpy brute force of the same rows."""
import numpy as np
import pytest
import torch

import two_rank_util
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

N_TRAIN = 8


def _fused(x, bank_n, k):
    """The one-launch kernel, called directly (ops.cosine_knn_fused may itself pick the split form)."""
    from self_supervised import _hip
    out = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    _hip.check(_hip.lib().ssad_cosine_knn_fused(_hip.ptr(x), _hip.ptr(bank_n), _hip.ptr(out), x.shape[0], x.shape[1],
                                                bank_n.shape[0], k, _hip.stream()))
    return out


def _ref64(x, bank_n, k):
    """float64 brute force: x / ||x||, cosine distance clipped to [0, 2], mean of the k smallest."""
    q = x.double().cpu().numpy()
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    b = bank_n.double().cpu().numpy()
    out = np.empty(q.shape[0])
    for i in range(0, q.shape[0], 256):
        d = np.clip(1.0 - q[i:i + 256] @ b.T, 0.0, 2.0)
        out[i:i + 256] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1).mean(1)
    return out


def _data(n, r, d, seed):
    from self_supervised import ops
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, device="cuda", generator=g)
    bank = ops.l2_normalize_rows(torch.randn(r, d, device="cuda", generator=g))
    return x, bank


@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("r", [3, 129, 5000, 123000])
def test_split_is_bit_identical_to_fused(r, d):
    from self_supervised import ops
    x_all, bank = _data(13456, r, d, seed=r + d)
    for n in (1, 127, 841, 13456):
        x = x_all[:n]
        for k in (1, 2, 3):
            want = _fused(x, bank, k)
            for s in (1, 2, 3, 7, 16):
                got = ops.cosine_knn_split(x, bank, k, s)
                assert torch.equal(got, want), (n, r, d, k, s, (got - want).abs().max().item())
            if n <= 841 and r <= 5000 or n == 1:
                err = np.abs(want.double().cpu().numpy() - _ref64(x, bank, k)).max()
                assert err <= 2e-6, (n, r, d, k, err)


def test_split_matches_float64_on_a_large_bank():
    """A subset of queries against a 123 000-row bank (70 % of bottle's 209 x 841 patches), splits of a few thousand rows."""
    from self_supervised import ops
    x, bank = _data(300, 123000, 512, seed=1)
    want = _ref64(x, bank, 3)
    for s in (ops.knn_splits(300, 123000), 16):
        got = ops.cosine_knn_split(x, bank, 3, s).double().cpu().numpy()
        assert np.abs(got - want).max() <= 2e-6


def test_split_row_independent_and_dispatched():
    from self_supervised import ops
    x, bank = _data(841, 50000, 512, seed=2)
    s = ops.knn_splits(841, 50000)
    assert s > 1
    full = ops.cosine_knn_fused(x, bank, 3)                # the dispatcher takes the split form here ...
    assert torch.equal(full, _fused(x, bank, 3))            # ... with the one-launch kernel's bits
    for i in (0, 1, 127, 128, 500, 840):
        assert torch.equal(ops.cosine_knn_split(x[i:i + 1], bank, 3, s)[0], full[i]), i
    # the default reference bank (588 rows) and a large query count stay on the one-launch kernel
    assert ops.knn_splits(841, 588) == 1 and ops.knn_splits(4 * 10 ** 6, 123000) == 1


def _tree(tmp_path, seeded_sd):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=96)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


def _spy(monkeypatch, cls, seen):
    orig = cls.fit

    def spy(self, embeddings, split=True, groups=None):
        seen["rows"] = torch.as_tensor(embeddings).detach().cpu().clone()
        seen["groups"] = None if groups is None else torch.as_tensor(groups).clone()
        seen["rng"] = np.random.get_state()
        orig(self, embeddings, split, groups)
        seen["threshold"] = self.threshold
    monkeypatch.setattr(cls, "fit", spy)


def _standalone_rows(ck, root, patch):
    """model(x) of every training image in file order, outside tools.inference."""
    from self_supervised.datasets import MVTecDatamodule
    from self_supervised.models import PeraNet
    model = PeraNet.load_from_checkpoint(ck).eval()
    if patch:
        model.enable_patch_level_mode()
    model.enable_mvtec_inference()
    model.cuda()
    dm = MVTecDatamodule(root + "bottle/", batch_size=1)
    dm.setup()
    ds = dm.test_dataset
    ds.images_filenames = list(dm.train_images_filenames)
    x = torch.stack([ds[i][0] for i in range(len(ds))]).cuda()
    with torch.no_grad():
        return model(x)['latent_space'].cpu()


def test_train_bank_patch_knn(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import ops, tools
    from self_supervised.models import AnomalyDetector, split_indices, split_rows
    root, ck = _tree(tmp_path, seeded_sd)
    seen = {}
    _spy(monkeypatch, AnomalyDetector, seen)
    np.random.seed(3)
    res = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train')
    maps = res.anomaly_maps
    assert tuple(maps.shape) == (4, 1, 29, 29) and torch.isfinite(maps).all()
    rows, groups = seen["rows"], seen["groups"]
    assert rows.shape == (N_TRAIN * 841, 512)
    assert torch.equal(groups, torch.arange(N_TRAIN).repeat_interleave(841))
    # the bank rows are the training images' embeddings in file order
    assert torch.equal(rows, _standalone_rows(ck, root, patch=True))
    # the 70/30 split is drawn over images: split_indices(8) once
    np.random.set_state(seen["rng"])
    tr_img, va_img = split_indices(N_TRAIN, 0.3)
    np.random.set_state(seen["rng"])
    tr, va = split_rows(rows.shape[0], groups)
    assert np.array_equal(tr, np.concatenate([np.arange(i * 841, (i + 1) * 841) for i in tr_img]))
    assert np.array_equal(va, np.concatenate([np.arange(i * 841, (i + 1) * 841) for i in va_img]))
    assert len(va_img) == 3
    bank = ops.l2_normalize_rows(rows[tr].cuda())
    q = res.embedding_vectors.float().cuda()
    want = _fused(q, bank, 3).cpu()
    assert torch.equal(maps.reshape(-1), want)
    assert seen["threshold"] == _fused(rows[va].cuda(), bank, 3).max().item()
    err = np.abs(maps.reshape(-1).double().numpy() - _ref64(q, bank, 3)).max()
    assert err <= 2e-6, err
    # the maps go on through the rest of the pipeline
    res.anomaly_maps = tools.upsample(maps, int(res.ground_truths.shape[-1]), verbose=False)
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou'])
    ev.evaluate(res, "bottle", str(tmp_path / "out") + "/", patch_level=True)
    assert ev.scores.auroc is not None and np.isfinite(ev.scores.auroc)
    # the streamed predict off: Trainer.predict over an unshuffled loader gives the same bank rows and maps
    monkeypatch.setenv("SSAD_FAST_PREDICT", "0")
    np.random.seed(3)
    res0 = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train')
    assert torch.equal(seen["rows"], rows)
    assert torch.equal(res0.anomaly_maps, maps)


def test_default_bank_unchanged(tmp_path, seeded_sd):
    from self_supervised import tools
    root, ck = _tree(tmp_path, seeded_sd)
    outs = []
    for kw in ({}, {"bank": "reference"}, {"bank": "train"}):
        np.random.seed(3)
        torch.manual_seed(0)
        outs.append(tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True,
                                    **kw).anomaly_maps)
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], outs[2])


def _ref_rows(x):
    from self_supervised import ops
    return ops.l2_normalize_rows(x.cuda()).cpu().double().numpy()


def test_train_bank_image_level_gde_matches_sklearn(tmp_path, seeded_sd, monkeypatch):
    from sklearn.covariance import LedoitWolf
    from self_supervised import tools
    from self_supervised.density import GaussianDensityDetector
    from self_supervised.models import split_indices
    root, ck = _tree(tmp_path, seeded_sd)
    # the default bank is one embedding at image level: still an error
    with pytest.raises(ValueError, match="at least 2 fit rows"):
        tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=False, detector='gde')
    seen = {}
    _spy(monkeypatch, GaussianDensityDetector, seen)
    np.random.seed(3)
    res = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=False, detector='gde',
                          bank='train')
    scores = res.anomaly_maps.reshape(-1)
    assert scores.shape == (4,) and torch.isfinite(scores).all()
    rows = seen["rows"]
    assert rows.shape == (N_TRAIN, 512)
    assert torch.equal(rows, _standalone_rows(ck, root, patch=False))
    np.random.set_state(seen["rng"])
    tr, _ = split_indices(N_TRAIN, 0.3)
    lw = LedoitWolf(assume_centered=False).fit(_ref_rows(rows)[tr])
    vi = np.linalg.inv(lw.covariance_)
    c = _ref_rows(res.embedding_vectors.float()) - lw.location_
    want = np.sqrt(np.einsum("ij,jk,ik->i", c, vi, c))
    rel = np.abs(scores.double().numpy() - want) / want
    assert rel.max() <= 1e-4, rel.max()
    # image-level kNN: 3-NN over the training images
    np.random.seed(3)
    knn = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=False, bank='train')
    assert knn.anomaly_maps.shape == (4,) and torch.isfinite(knn.anomaly_maps).all()


def test_train_bank_two_ranks_equal_one_rank(tmp_path, seeded_sd):
    from self_supervised import tools
    root, ck = _tree(tmp_path, seeded_sd)
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "train_bank"])
    assert r["maps_equal_across_ranks"], r
    two = torch.load(str(tmp_path / "maps_rank0.pt"))
    one = two_rank_util.inference(tools, ck, root, "train_bank")
    assert torch.equal(two["embeddings"], one.embedding_vectors)
    assert torch.equal(two["maps"], one.anomaly_maps)
