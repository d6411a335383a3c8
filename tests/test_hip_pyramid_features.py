"""GPU: the stage-pyramid rows (csrc/pyramid_features.hip) -- kernel, PeraNet.enable_dense_mode(features='pyramid'), the preselected
PaDiM detector and tools.inference(dense_features='pyramid').

The kernel is a copy: every comparison with tests/pyramid_features_ref.py is torch.equal.  The PaDiM scores keep the bar of
tests/test_hip_padim.py (1e-4 relative to tests/padim_ref.py's float64 scores)."""
import functools

import numpy as np
import pytest
import torch

import padim_ref as PR
import pyramid_features_ref as R
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

NAN = float("nan")
LAYERS = ('layer1', 'layer2', 'layer3')


def _sel(D, d, seed=0):
    from self_supervised.density import position_channels
    return position_channels(D, d, seed)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(maps on the host, maps on the device, {selection name: (sel, reference rows)}), computed once and left unchanged."""
    n, stages = R.CASES[name]
    ms = R.maps(n, stages, seed=len(name))
    sels = R.selections(stages, _sel)
    return ms, [m.cuda() for m in ms], {k: (s, R.reference(ms, s)) for k, s in sels.items()}


# ---------------------------------------------------------------------------------------------------------------------- kernel

@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_equals_the_reference(name):
    from self_supervised import ops
    _, dev, sels = _case(name)
    assert name != "4;64x64x64,32x32x128,16x16x256" or "padim-96" in sels
    for what, (sel, want) in sels.items():
        got = ops.stage_pyramid_rows(dev, sel)
        assert got.shape == want.shape and torch.equal(got.cpu(), want), (name, what)
        assert torch.equal(ops.stage_pyramid_rows(dev, sel), got), (name, what)                # two calls: the same bits
        for rb in (1, 3):                                                                       # however the grid is cut
            assert torch.equal(ops.stage_pyramid_rows(dev, sel, rows_per_block=rb), got), (name, what, rb)


@pytest.mark.parametrize("name", ["1;9x9x8,5x5x8,3x3x12", "2;6x10x4,3x5x8,2x3x8", "3;16x16x64,8x8x128,4x4x256"])
def test_kernel_writes_its_rows_and_nothing_else(name):
    """out is a row slice in the middle of a NaN-filled tensor: the rows around it keep their NaN bit patterns, every row inside is
    written (finite)."""
    from self_supervised import ops
    _, dev, sels = _case(name)
    for what, (sel, want) in sels.items():
        rows, d = want.shape
        pad = 5
        whole = torch.full((rows + 2 * pad, d), NAN, device="cuda")
        whole[:pad].view(torch.int32).fill_(0x7FC00BAD)                                         # NaNs with payloads of their own
        whole[-pad:].view(torch.int32).fill_(0x7FC0FEED)
        out = ops.stage_pyramid_rows(dev, sel, out=whole[pad:-pad])
        torch.cuda.synchronize()
        assert out.data_ptr() == whole[pad:-pad].data_ptr()
        bits = whole.view(torch.int32).cpu()
        assert bool((bits[:pad] == 0x7FC00BAD).all()) and bool((bits[-pad:] == 0x7FC0FEED).all()), (name, what)
        assert torch.isfinite(whole[pad:-pad]).all() and torch.equal(whole[pad:-pad].cpu(), want), (name, what)


def test_rows_do_not_depend_on_the_batch():
    from self_supervised import ops
    _, dev, sels = _case("3;16x16x64,8x8x128,4x4x256")
    sel = sels["padim-96"][0]
    for s in (None, sel):
        full = ops.stage_pyramid_rows(dev, s)
        p = 16 * 16
        for n in range(3):
            alone = ops.stage_pyramid_rows([m[n:n + 1].contiguous() for m in dev], s)
            assert torch.equal(alone, full[n * p:(n + 1) * p]), n


def test_bad_arguments_launch_nothing():
    from self_supervised import _hip, ops
    E = _hip.HipExtensionError
    z = lambda *s: torch.zeros(*s, device="cuda")
    m0, m1, m2 = z(2, 8, 8, 8), z(2, 4, 4, 16), z(2, 2, 2, 32)
    out = torch.full((2 * 64, 56), NAN, device="cuda")
    before = _hip.LAUNCHES
    with pytest.raises(E, match="multiples of 4"):
        ops.stage_pyramid_rows([z(2, 8, 8, 6), m1, m2])
    for bad, why in (([3, 1], "strictly increasing"), ([1, 1], "strictly increasing"), ([0, 56], "outside"), ([-1, 3], "outside"),
                     ([], "non-empty"), ([0.5], "int32 / int64")):
        with pytest.raises(E, match=why):
            ops.stage_pyramid_rows([m0, m1, m2], torch.tensor(bad), out=out)
    with pytest.raises(E, match="finest first"):
        ops.stage_pyramid_rows([m1, m0, m2])
    with pytest.raises(E, match="finest first"):
        ops.stage_pyramid_rows([m0, z(2, 4, 9, 16), m2])
    with pytest.raises(E, match="out is"):
        ops.stage_pyramid_rows([m0, m1, m2], out=out[:, :55])
    with pytest.raises(E, match="out is"):
        ops.stage_pyramid_rows([m0, m1, m2], torch.tensor([0, 5]), out=out)
    with pytest.raises(E, match="ROCm tensor"):
        ops.stage_pyramid_rows([m0, m1.cpu(), m2])
    with pytest.raises(E, match="ROCm tensor"):
        ops.stage_pyramid_rows([m0, m1.double(), m2])
    with pytest.raises(E, match="two or three"):
        ops.stage_pyramid_rows([m0])
    with pytest.raises(E, match="images"):
        ops.stage_pyramid_rows([m0, m1[:1], m2])
    assert _hip.LAUNCHES == before                                   # refused on the host: the library was not even called
    with pytest.raises(E):
        ops.stage_pyramid_rows([m0, m1, m2], out=out.cpu())
    # the library's own guards, for callers of the C entry
    lib, st = _hip.lib(), _hip.stream()
    p = [t.data_ptr() for t in (m0, m1, m2)]
    sel = torch.arange(4, device="cuda", dtype=torch.int32)
    geo = (8, 8, 8, 4, 4, 16, 2, 2, 32)
    calls = {"stages": (*p, None, out.data_ptr(), 2, 4, *geo, 56, 0),
             "null map": (p[0], None, p[2], None, out.data_ptr(), 2, 3, *geo, 56, 0),
             "null out": (*p, None, None, 2, 3, *geo, 56, 0),
             "C % 4": (*p, None, out.data_ptr(), 2, 3, 8, 8, 6, 4, 4, 16, 2, 2, 32, 54, 0),
             "coarser larger": (*p, None, out.data_ptr(), 2, 3, 8, 8, 8, 9, 4, 16, 2, 2, 32, 56, 0),
             "d != D": (*p, None, out.data_ptr(), 2, 3, *geo, 48, 0),
             "d > D": (*p, sel.data_ptr(), out.data_ptr(), 2, 3, *geo, 57, 0),
             "side": (*p, None, out.data_ptr(), 2, 3, 40000, 8, 8, 4, 4, 16, 2, 2, 32, 56, 0),
             "tables": (*p, None, out.data_ptr(), 2, 3, 8, 6000, 8, 4, 4, 16, 2, 2, 32, 56, 0),
             "unaligned": (p[0] + 4, p[1], p[2], None, out.data_ptr(), 2, 3, *geo, 56, 0),
             "rows_per_block": (*p, None, out.data_ptr(), 2, 3, *geo, 56, -1)}
    for what, a in calls.items():
        assert lib.ssad_stage_pyramid_rows(*a, st) == 2, what
        assert b"ssad_stage_pyramid_rows" in lib.ssad_last_error(), what
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ----------------------------------------------------------------------------------------------------------------------- model

def _model(seeded_sd):
    from self_supervised.models import PeraNet
    m = PeraNet()
    m.load_state_dict(seeded_sd)
    return m.eval().cuda()


def test_model_rows_are_the_reference_of_its_stage_maps(seeded_sd):
    from oracle import weights as ow
    from self_supervised import engine
    x = ow.synthetic_images(2, 64, seed=17).cuda()
    m = _model(seeded_sd)
    with torch.no_grad():
        m.enable_dense_mode()
        local = m(x)
        maps = dict.fromkeys(LAYERS)
        pooled = torch.empty((2, m.concatenator[0].in_features), device="cuda")
        engine.trunk_eval(m._eval_plan(), x, 0, 0, m.layer_outputs, pooled, maps)
        ms = [maps[k].cpu() for k in LAYERS]
        assert [tuple(t.shape[1:]) for t in ms] == [(16, 16, 64), (8, 8, 128), (4, 4, 256)]
        sel = _sel(448, 96, 0)
        for columns in (None, sel):
            m.enable_dense_mode(LAYERS, features='pyramid', columns=columns)
            out = m(x)
            assert (m.batch, m.num_patches) == (2, 256)
            want = R.reference(ms, columns)
            assert tuple(out["latent_space"].shape) == (512, 448 if columns is None else 96)
            assert torch.equal(out["latent_space"].cpu(), want)
            assert torch.equal(out["classifier"], local["classifier"])           # the image-level logits of the same pass
            m.max_samples_per_pass = 1                                            # one image per pass: rows land in their slices
            again = m(x)
            m.max_samples_per_pass = 131072
            assert torch.equal(again["latent_space"], out["latent_space"])
        # two layers, and back to 'local': what it returned before
        m.enable_dense_mode(('layer2', 'layer3'), features='pyramid')
        assert torch.equal(m(x)["latent_space"].cpu(), R.reference(ms[1:]))
        m.enable_dense_mode()
        after = m(x)
        assert torch.equal(after["latent_space"], local["latent_space"]) and torch.equal(after["classifier"], local["classifier"])


# ----------------------------------------------------------------------------------------------------------- PaDiM equivalence

def test_preselected_detector_meets_the_padim_bar():
    """Run A: preselected rows (what the kernel writes with a selection); run B: the full 448-column rows.  Each against the float64
    reference, at the bar of tests/test_hip_padim.py; whether A and B are bit-equal is printed, not required."""
    from self_supervised import ops
    from self_supervised.density import PositionGaussianDetector
    P, D, d, n_fit, n_q = 16, 448, 96, 200, 24
    fit = PR.synthetic_rows(n_fit, P, D, seed=31)
    q = PR.synthetic_rows(n_q, P, D, seed=31, draw=2, spread=1.5)
    sel = _sel(D, d, 0)
    # the preselected rows come from the kernel itself: the rows as a one-stage-pair pyramid of 1 x 1 ratio
    as_maps = lambda r, n: [torch.from_numpy(r).reshape(n, 4, 4, D)[..., :192].contiguous().cuda(),
                            torch.from_numpy(r).reshape(n, 4, 4, D)[..., 192:].contiguous().cuda()]
    fit_pre, q_pre = ops.stage_pyramid_rows(as_maps(fit, n_fit), sel), ops.stage_pyramid_rows(as_maps(q, n_q), sel)
    assert torch.equal(fit_pre.cpu(), torch.from_numpy(fit)[:, sel]) and torch.equal(q_pre.cpu(), torch.from_numpy(q)[:, sel])
    a = PositionGaussianDetector(batch=n_q, num_patches=P, channels=d, preselected=True, width=D)
    b = PositionGaussianDetector(batch=n_q, num_patches=P, channels=d)
    a.fit_bank(fit_pre)
    b.fit_bank(torch.from_numpy(fit))
    assert torch.equal(a.sel, sel) and torch.equal(b.sel, sel)
    assert torch.equal(a._sel_dev.cpu(), torch.arange(d, dtype=torch.int32))
    mean, _, vi = PR.fit(fit, sel.numpy(), P, eps=0.01)
    want = PR.scores(q, sel.numpy(), P, mean, vi)
    got_a = a.predict(q_pre).reshape(-1).cpu().double().numpy()
    got_b = b.predict(torch.from_numpy(q)).reshape(-1).cpu().double().numpy()
    err_a, err_b = (np.abs(got_a - want) / want).max(), (np.abs(got_b - want) / want).max()
    print(f"preselected rows {err_a:.2e}, full rows {err_b:.2e} of the float64 scores (bar 1e-4); bit-equal: "
          f"scores {np.array_equal(got_a, got_b)}, W {torch.equal(a.w, b.w)}")
    assert err_a <= 1e-4 and err_b <= 1e-4, (err_a, err_b)
    with pytest.raises(ValueError, match="chosen columns"):
        a.predict(torch.from_numpy(q))
    st = a.state()
    a2 = PositionGaussianDetector.from_state(st, batch=n_q, num_patches=P)
    assert a2.preselected and torch.equal(a2.predict(q_pre), a.predict(q_pre))


# ------------------------------------------------------------------------------------------------------ through tools.inference

SIZE, SIDE, N_TRAIN, CHANNELS = 256, 64, 10, 32
OPTS = {"channels": CHANNELS}


def _datamodule(root, **kw):
    from self_supervised.datasets import MVTecDatamodule
    return MVTecDatamodule(root, imsize=(SIZE, SIZE), **kw)


@pytest.fixture()
def tree(tmp_path, seeded_sd, monkeypatch):
    """The fixture of tests/test_hip_padim.py at 256 x 256 (64 x 64 maps), with fewer training images."""
    from self_supervised import datasets, tools
    datasets._DataModule.num_workers = 0
    monkeypatch.setattr(tools, "MVTecDatamodule", _datamodule)
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=SIZE)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


def _run(tools, ck, root, **kw):
    np.random.seed(3)
    return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, localization='dense',
                           bank='train', **kw)


PYRAMID_RUNS = {"padim": dict(detector='padim', detector_options=OPTS),
                "knn-euclidean-coreset": dict(detector='knn', metric='euclidean', coreset=0.01)}


@pytest.mark.parametrize("which", list(PYRAMID_RUNS))
def test_pyramid_through_inference(tree, which):
    from self_supervised import tools
    root, ck = tree
    kw = PYRAMID_RUNS[which]
    local = _run(tools, ck, root, **kw).anomaly_maps
    res = _run(tools, ck, root, dense_features='pyramid', **kw)
    maps = res.anomaly_maps
    assert tuple(maps.reshape(4, SIDE, SIDE).shape) == (4, SIDE, SIDE) and tuple(maps.shape) == (4, 1, SIDE, SIDE)
    assert torch.isfinite(maps).all()
    assert tuple(res.embedding_vectors.shape) == (4 * SIDE * SIDE, CHANNELS if which == "padim" else 448)
    up = tools.upsample(maps, SIZE, verbose=False, method='resize_blur')
    assert tuple(up.shape) == (4, 1, SIZE, SIZE) and torch.isfinite(up).all()
    assert tuple(tools.upsample(maps, SIZE, verbose=False).shape) == (4, 1, SIZE, SIZE)
    regions = tools.defect_regions(up, float(up.median()))
    assert tuple(regions.pred_masks.shape) == (4, 1, SIZE, SIZE) and len(regions.regions) == 4
    again = _run(tools, ck, root, dense_features='pyramid', **kw)
    assert torch.equal(again.anomaly_maps, maps) and torch.equal(again.embedding_vectors, res.embedding_vectors)
    # 'local' in the same process: what it returned before the pyramid calls
    after = _run(tools, ck, root, **kw).anomaly_maps
    assert tuple(local.shape) == (4, 1, 32, 32) and torch.equal(after, local)
