"""GPU: dense feature-map localisation -- the locally aware patch features kernel (csrc/patch_features.hip) per element against
float64 over poisoned buffers, the stage maps of one trunk pass, and tools.inference(localization='dense') through both detectors.

The reference, the shapes and the bar: tests/patch_features_ref.py.  Measured on the MI355X (one run): the largest error over all
shapes and row bands is 3.6 units of 2^-24 A(|x|) (bar 40); the dense rows of the trunk test sit at 4.3e-7 (layer2 block) and 4.5e-7
(layer3 block) of the block's largest reference value (bar 2e-5); the dense maps are within 4.1e-7 of the float64 brute force (bar 2e-6)."""
import numpy as np
import pytest
import torch

import patch_features_ref as R
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

N_TRAIN = 8
P = 144            # 96 x 96 images: a 12 x 12 layer2 map


def _guarded(t):
    """t as a view into a larger allocation whose rows before and after are NaN -> (view, whole)."""
    whole = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), float("nan"), device="cuda")
    whole[1:-1] = t.cuda()
    return whole[1:-1], whole


def _guards_intact(whole):
    return bool(torch.isnan(whole[0]).all() and torch.isnan(whole[-1]).all())


def _check(out, shape, what):
    _, _, ref, bar = R.case(shape)
    got = out.cpu()
    assert torch.isfinite(got).all(), f"{shape} {what}: non-finite output"
    units = R.worst_units(got, shape)
    print(f"{shape} {what}: {units:.2f} units of 2^-24 A(|x|) (bar {R.BAR_UNITS:g})")
    assert ((got.double() - ref).abs() <= bar).all(), f"{shape} {what}: {units:.2f} units, the bar is {R.BAR_UNITS:g}"


@pytest.mark.parametrize("shape", R.SHAPES, ids=["x".join(map(str, s)) for s in R.SHAPES])
def test_kernel_against_float64(shape):
    from self_supervised import ops
    fine, coarse, _, _ = R.case(shape)
    f, c = fine.cuda(), coarse.cuda()
    out = ops.local_patch_features(f, c)
    assert tuple(out.shape) == (shape[0] * shape[1] * shape[2], shape[3] + shape[6])
    _check(out, shape, "plain")
    # a call repeats its own bits, whatever row band the launcher is given
    assert torch.equal(ops.local_patch_features(f, c), out)
    for rb in R.ROWS_PER_BLOCK:
        assert torch.equal(ops.local_patch_features(f, c, rows_per_block=rb), out), (shape, rb)


@pytest.mark.parametrize("shape", R.SHAPES, ids=["x".join(map(str, s)) for s in R.SHAPES])
def test_kernel_over_poisoned_buffers(shape):
    """out pre-filled with NaN, the inputs and the output views into larger allocations with NaN rows before and after: a read or a
    write outside the maps shows as a NaN, not as a fault."""
    from self_supervised import ops
    fine, coarse, _, _ = R.case(shape)
    (f, fw), (c, cw) = _guarded(fine), _guarded(coarse)
    rows, d = shape[0] * shape[1] * shape[2], shape[3] + shape[6]
    for rb in (0,) + R.ROWS_PER_BLOCK:
        ow = torch.full((rows + 2, d), float("nan"), device="cuda")
        ops.local_patch_features(f, c, out=ow[1:-1], rows_per_block=rb)
        _check(ow[1:-1], shape, f"poisoned, rows_per_block={rb}")
        assert _guards_intact(ow) and _guards_intact(fw) and _guards_intact(cw), (shape, rb)
    assert torch.equal(f.cpu(), fine) and torch.equal(c.cpu(), coarse)


def test_bad_arguments_launch_nothing():
    from self_supervised import _hip
    lib = _hip.lib()
    f = torch.zeros(1, 2, 2, 8, device="cuda")
    c = torch.zeros(1, 1, 1, 8, device="cuda")
    out = torch.full((4, 16), float("nan"), device="cuda")
    calls = {
        "Cf % 4": (f.data_ptr(), c.data_ptr(), out.data_ptr(), 1, 2, 2, 6, 1, 1, 8),
        "Cc % 4": (f.data_ptr(), c.data_ptr(), out.data_ptr(), 1, 2, 2, 8, 1, 1, 2),
        "null fine": (None, c.data_ptr(), out.data_ptr(), 1, 2, 2, 8, 1, 1, 8),
        "null out": (f.data_ptr(), c.data_ptr(), None, 1, 2, 2, 8, 1, 1, 8),
        "N = 0": (f.data_ptr(), c.data_ptr(), out.data_ptr(), 0, 2, 2, 8, 1, 1, 8),
        "Hc = 0": (f.data_ptr(), c.data_ptr(), out.data_ptr(), 1, 2, 2, 8, 0, 1, 8),
        "Wc > 2048": (f.data_ptr(), c.data_ptr(), out.data_ptr(), 1, 2, 2, 8, 1, 2049, 8),
    }
    for what, a in calls.items():
        rc = lib.ssad_local_patch_features(*a, 0, _hip.stream())
        assert rc == 2, what
        assert b"ssad_local_patch_features" in lib.ssad_last_error(), what
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    with pytest.raises(_hip.HipExtensionError):
        from self_supervised import ops
        ops.local_patch_features(f, torch.zeros(2, 1, 1, 8, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- trunk maps

def _model(seeded_sd):
    from self_supervised.models import PeraNet
    m = PeraNet()
    m.load_state_dict(seeded_sd)
    return m.eval().cuda()


def test_trunk_maps_of_one_pass(seeded_sd):
    from oracle import weights as ow
    from oracle.peranet import OraclePeraNet
    x = ow.synthetic_images(2, 96, seed=41)
    ref = OraclePeraNet()
    ref.load_state_dict(seeded_sd)
    ref = ref.double().eval()
    with torch.no_grad():
        acts = ref.trunk_features(x.double())
    want = R.reference(acts["layer2"].permute(0, 2, 3, 1), acts["layer3"].permute(0, 2, 3, 1))
    m = _model(seeded_sd)
    xd = x.cuda()
    with torch.no_grad():
        before = m(xd)
        m.enable_dense_mode()
        dense = m(xd)
        assert (m.batch, m.num_patches) == (2, P)
        m.disable_dense_mode()
        after = m(xd)
    rows = dense["latent_space"]
    assert tuple(rows.shape) == (2 * P, 384) and tuple(dense["classifier"].shape) == (2, 4)
    for name, cols in (("layer2", slice(0, 128)), ("layer3", slice(128, 384))):
        err = (rows[:, cols].cpu().double() - want[:, cols]).abs().max().item() / want[:, cols].abs().max().item()
        print(f"dense rows, {name} block: {err:.2e} of the block's largest reference value (bar 2e-5)")
        assert err <= 2e-5, (name, err)
    # the logits are the image-level logits of the same pass; dense mode leaves nothing behind
    assert torch.equal(dense["classifier"], before["classifier"])
    assert torch.equal(after["classifier"], before["classifier"]) and torch.equal(after["latent_space"], before["latent_space"])
    # passes of one image (the OOM-halving route) give the same rows
    m.enable_dense_mode()
    m.max_samples_per_pass = 1
    with torch.no_grad():
        again = m(xd)
    assert m.last_pass_samples == 1
    assert torch.equal(again["latent_space"], rows) and torch.equal(again["classifier"], dense["classifier"])


def test_dense_mode_refusals_on_the_device(seeded_sd, monkeypatch):
    m = _model(seeded_sd)
    m.enable_dense_mode()
    with torch.no_grad():
        with pytest.raises(ValueError, match="square"):
            m(torch.zeros(1, 3, 96, 128, device="cuda"))
        with pytest.raises(ValueError, match="64 x 64"):
            m(torch.zeros(1, 3, 32, 32, device="cuda"))
        monkeypatch.setenv("SSAD_MATH", "bf16x3")
        with pytest.raises(ValueError, match="fp32"):
            m(torch.zeros(1, 3, 96, 96, device="cuda"))
        monkeypatch.delenv("SSAD_MATH")
        m.train()
        with pytest.raises(ValueError, match="eval"):
            m(torch.zeros(1, 3, 96, 96, device="cuda"))


# ------------------------------------------------------------------------------------------------------ through tools.inference

def _fused(x, bank_n, k):
    from self_supervised import ops
    return ops.cosine_knn_fused(x, bank_n, k)


def _ref64(x, bank_n, k):
    """float64 brute force: x / ||x||, cosine distance clipped to [0, 2], mean of the k smallest."""
    q = x.double().cpu().numpy()
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    b = bank_n.double().cpu().numpy()
    d = np.clip(1.0 - q @ b.T, 0.0, 2.0)
    return np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1).mean(1)


SIZE = 96


def _datamodule(root, **kw):
    from self_supervised.datasets import MVTecDatamodule
    return MVTecDatamodule(root, imsize=(SIZE, SIZE), **kw)


@pytest.fixture()
def tree(tmp_path, seeded_sd, monkeypatch):
    """A synthetic category of 96 x 96 images and a seeded checkpoint.  tools.inference has the reference's signature and reads every
    image at its datamodule's default size (256 x 256: 32 x 32 dense maps); the datamodule it builds is pinned to the files' own 96 x 96
    here, so that the pipeline runs the 12 x 12 / 6 x 6 geometry (144 rows per image) at a quarter of the work."""
    from self_supervised import datasets, tools
    datasets._DataModule.num_workers = 0
    monkeypatch.setattr(tools, "MVTecDatamodule", _datamodule)
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=SIZE)
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


def _dense(tools, ck, root, **kw):
    np.random.seed(3)
    return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, localization='dense',
                           bank='train', **kw)


def test_dense_through_inference(tree, tmp_path, monkeypatch):
    from self_supervised import ops, tools
    from self_supervised.density import GaussianDensityDetector
    from self_supervised.models import AnomalyDetector, split_rows
    root, ck = tree
    seen = {}
    _spy(monkeypatch, AnomalyDetector, seen)
    # call A: kNN against the whole training set
    res = _dense(tools, ck, root)
    maps = res.anomaly_maps
    assert tuple(maps.shape) == (4, 1, 12, 12) and torch.isfinite(maps).all()
    assert tuple(res.raw_predictions.shape) == (4, 4) and tuple(res.embedding_vectors.shape) == (4 * P, 384)
    rows, groups = seen["rows"], seen["groups"]
    assert tuple(rows.shape) == (N_TRAIN * P, 384)
    assert torch.equal(rows, _standalone_rows(ck, root))
    assert torch.equal(groups, torch.arange(N_TRAIN).repeat_interleave(P))
    np.random.set_state(seen["rng"])
    tr, _ = split_rows(rows.shape[0], groups)
    bank = ops.l2_normalize_rows(rows[tr].cuda())
    q = res.embedding_vectors.float().cuda()
    assert torch.equal(maps.reshape(-1), _fused(q, bank, 3).cpu())
    err = np.abs(maps.reshape(-1).double().numpy() - _ref64(q, bank, 3)).max()
    print(f"dense maps against the float64 brute force: {err:.2e} (bar 2e-6)")
    assert err <= 2e-6, err
    # call B: the streamed predict off -- the same rows and maps
    monkeypatch.setenv("SSAD_FAST_PREDICT", "0")
    res0 = _dense(tools, ck, root)
    monkeypatch.delenv("SSAD_FAST_PREDICT")
    assert torch.equal(seen["rows"], rows)
    assert torch.equal(res0.anomaly_maps, maps) and torch.equal(res0.raw_predictions, res.raw_predictions)
    # call C: coreset + reweighted image scores
    resc = _dense(tools, ck, root, coreset=0.1, image_scores='reweighted')
    assert tuple(resc.image_scores.shape) == (4,) and torch.isfinite(resc.image_scores).all()
    assert seen["detector"].coreset_counts[0] < seen["detector"].coreset_counts[1]
    direct = seen["detector"].predict(resc.embedding_vectors.float().cuda()).cpu()
    assert tuple(resc.anomaly_maps.shape) == (4, 1, 12, 12) and torch.equal(resc.anomaly_maps, direct)
    # call D: the Gaussian density detector
    seen_g = {}
    _spy(monkeypatch, GaussianDensityDetector, seen_g)
    resg = _dense(tools, ck, root, detector='gde')
    assert tuple(resg.anomaly_maps.shape) == (4, 1, 12, 12) and torch.isfinite(resg.anomaly_maps).all()
    assert tuple(seen_g["rows"].shape) == (N_TRAIN * P, 384)
    # the maps go on through the rest of the pipeline
    res.anomaly_maps = tools.upsample(maps, int(res.ground_truths.shape[-1]), verbose=False)
    assert tuple(res.anomaly_maps.shape) == (4, 1, 96, 96)
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou'])
    ev.evaluate(res, "bottle", str(tmp_path / "out") + "/", patch_level=True)
    assert ev.scores.auroc is not None and np.isfinite(ev.scores.auroc)


def test_default_localization_unchanged(tree):
    from self_supervised import tools
    root, ck = tree
    outs = []
    for kw in ({}, {"localization": "patches"}):
        np.random.seed(3)
        torch.manual_seed(0)
        outs.append(tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, **kw))
    assert tuple(outs[0].anomaly_maps.shape) == (4, 1, 9, 9)
    assert torch.equal(outs[0].anomaly_maps, outs[1].anomaly_maps)
    assert torch.equal(outs[0].embedding_vectors, outs[1].embedding_vectors)
    assert torch.equal(outs[0].raw_predictions, outs[1].raw_predictions)
