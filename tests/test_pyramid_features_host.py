"""CPU: the stage-pyramid rows' reference (tests/pyramid_features_ref.py) against F.interpolate(mode='nearest'), and the host-side
checks the feature adds: enable_dense_mode(features=, columns=), tools._check_options(dense_features=), the detector's `preselected`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pyramid_features_ref as R

INTEGER_RATIO = [k for k, (_, st) in R.CASES.items() if all(st[0][0] % h == 0 and st[0][1] % w == 0 for h, w, _ in st)]


@pytest.mark.parametrize("name", INTEGER_RATIO)
def test_reference_is_nearest_interpolation_at_integer_ratios(name):
    from self_supervised.density import position_channels
    n, stages = R.CASES[name]
    ms = R.maps(n, stages, seed=len(name))
    size = stages[0][:2]
    want = torch.cat([F.interpolate(m.permute(0, 3, 1, 2), size=size, mode='nearest') for m in ms], dim=1)
    want = want.permute(0, 2, 3, 1).reshape(n * size[0] * size[1], -1)
    for what, sel in R.selections(stages, position_channels).items():
        got = R.reference(ms, sel)
        assert torch.equal(got, want if sel is None else want[..., sel]), what


def test_reference_at_non_integer_ratios_by_hand():
    n, stages = R.CASES["1;9x9x8,5x5x8,3x3x12"]
    ms = R.maps(n, stages, seed=1)
    got = R.reference(ms).reshape(9, 9, 28)
    for i, j in ((0, 0), (1, 8), (4, 4), (8, 8), (7, 2)):
        assert torch.equal(got[i, j, :8], ms[0][0, i, j])
        assert torch.equal(got[i, j, 8:16], ms[1][0, i * 5 // 9, j * 5 // 9])
        assert torch.equal(got[i, j, 16:], ms[2][0, i * 3 // 9, j * 3 // 9])
    assert (8 * 5 // 9, 8 * 3 // 9) == (4, 2) and 1 * 5 // 9 == 0            # the last source row is reached, the first is held twice


def test_engine_stage_shapes_need_no_integer_ratio():
    from self_supervised import engine
    s = engine.stage_shapes(72, 72)
    assert [s[k][0] for k in ("layer1", "layer2", "layer3")] == [18, 9, 5]


# ------------------------------------------------------------------------------------------------------------------- the model

def _model():
    from self_supervised.models import PeraNet
    return PeraNet().eval()


def test_enable_dense_mode_layers_and_features():
    m = _model()
    m.enable_dense_mode()
    assert (m.dense_layers, m.dense_features, m.dense_columns) == (('layer2', 'layer3'), 'local', None)
    m.enable_dense_mode(('layer1', 'layer2', 'layer3'), features='pyramid')
    assert (m.dense_layers, m.dense_features, m.dense_columns) == (('layer1', 'layer2', 'layer3'), 'pyramid', None)
    m.enable_dense_mode(('layer1', 'layer3'), features='pyramid')
    assert m.dense_layers == ('layer1', 'layer3')
    m.disable_dense_mode()
    assert (m.dense_layers, m.dense_features, m.dense_columns) == (None, 'local', None)
    # 'local' keeps its own refusal, word for word
    for bad in (('layer1', 'layer2', 'layer3'), ('layer3', 'layer2'), ('layer2',), ('layer2', 'layer4')):
        with pytest.raises(ValueError, match=r"dense mode takes two of \('layer1', 'layer2', 'layer3'\), the finer stage first"):
            m.enable_dense_mode(bad)
    for bad in (('layer1',), ('layer2', 'layer1'), ('layer1', 'layer1', 'layer2'), ('layer2', 'layer3', 'layer4'),
                ('layer1', 'layer2', 'layer3', 'layer4')):
        with pytest.raises(ValueError, match="two or three of .* in ascending order"):
            m.enable_dense_mode(bad, features='pyramid')
    with pytest.raises(ValueError, match="features must be one of"):
        m.enable_dense_mode(features='nearest')
    with pytest.raises(ValueError, match="columns applies to features='pyramid' only"):
        m.enable_dense_mode(columns=[0, 1])
    assert m.dense_layers is None                                  # a refusal changes nothing


def test_enable_dense_mode_columns():
    from self_supervised.density import position_channels
    m = _model()
    layers = ('layer1', 'layer2', 'layer3')
    sel = position_channels(448, 96, 0)
    m.enable_dense_mode(layers, features='pyramid', columns=sel)
    assert torch.equal(m.dense_columns, sel) and m.dense_columns.dtype == torch.int64
    m.enable_dense_mode(layers, features='pyramid', columns=[0, 447])
    m.enable_dense_mode(('layer1', 'layer2'), features='pyramid', columns=np.array([0, 191]))
    for bad, why in (([3, 2], "sorted"), ([2, 2], "sorted"), ([0, 448], "within"), ([-1, 4], "within"), ([], "non-empty"),
                     ([0.0, 1.0], "integers"), ([[0, 1]], "vector"), ("ab", "integers"), (torch.tensor([True, False]), "integers")):
        with pytest.raises(ValueError, match=why):
            m.enable_dense_mode(layers, features='pyramid', columns=bad)
    with pytest.raises(ValueError, match=r"within \[0, 192\)"):       # the width is that of the layers named
        m.enable_dense_mode(('layer1', 'layer2'), features='pyramid', columns=[0, 192])


def test_dense_geometry_of_the_pyramid():
    m = _model()
    m.enable_dense_mode(('layer1', 'layer2', 'layer3'), features='pyramid')
    assert m._dense_geometry(torch.zeros(1, 3, 256, 256)) == ((64, 64, 64), (32, 32, 128), (16, 16, 256))
    assert m._dense_geometry(torch.zeros(1, 3, 72, 72)) == ((18, 18, 64), (9, 9, 128), (5, 5, 256))
    with pytest.raises(ValueError, match="square layer1 map"):
        m._dense_geometry(torch.zeros(1, 3, 96, 128))
    with pytest.raises(ValueError, match="64 x 64"):
        m._dense_geometry(torch.zeros(1, 3, 32, 32))
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m._dense_geometry(torch.zeros(1, 3, 96, 96))
    m.eval()
    m.enable_dense_mode()
    assert m._dense_geometry(torch.zeros(1, 3, 256, 256)) == ((32, 32, 128), (16, 16, 256))


# ------------------------------------------------------------------------------------------------------------------- the tools

def _opts(tools, **kw):
    a = dict(detector='knn', metric='cosine', localization='dense', patch_localization=True, bank='train', mvtec_inference=True,
             coreset=None, image_scores=None, neighbours=9, options=None, gallery=None)
    a.update(kw)
    return tools._check_options(**a)


def test_check_options_dense_features():
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector, GaussianDensityDetector, PositionGaussianDetector
    assert _opts(tools) == _opts(tools, dense_features='local') == (AnomalyDetector, {})
    assert _opts(tools, dense_features='pyramid') == (AnomalyDetector, {})
    assert _opts(tools, dense_features='pyramid', metric='euclidean', coreset=0.01) == \
        (AnomalyDetector, {"coreset": 0.01, "metric": "euclidean"})
    assert _opts(tools, dense_features='pyramid', metric='euclidean', gallery=3, image_scores='retrieval') == \
        (AnomalyDetector, {"metric": "euclidean", "gallery": 3})
    assert _opts(tools, dense_features='pyramid', detector='gde') == (GaussianDensityDetector, {})
    assert _opts(tools, detector='padim', options={"channels": 32}) == (PositionGaussianDetector, {"channels": 32})
    assert _opts(tools, detector='padim', dense_features='pyramid', options={"channels": 32, "seed": 5}) == \
        (PositionGaussianDetector, {"channels": 32, "seed": 5, "preselected": True, "width": 448})
    with pytest.raises(ValueError, match=r"dense_features must be one of \('local', 'pyramid'\), got 'nearest'"):
        _opts(tools, dense_features='nearest')
    for kw in ({"localization": 'patches'}, {"patch_localization": False, "localization": 'patches', "bank": 'reference'}):
        with pytest.raises(ValueError, match="dense_features='pyramid' needs patch_localization=True and localization='dense'"):
            _opts(tools, dense_features='pyramid', **kw)
    with pytest.raises(ValueError, match="channels"):                # 480 of 448 columns: refused from the arguments alone
        _opts(tools, detector='padim', dense_features='pyramid', options={"channels": 480})
    with pytest.raises(ValueError, match="detector_options must be a dict with keys among"):     # not a user option
        _opts(tools, detector='padim', dense_features='pyramid', options={"preselected": True})


def test_pyramid_columns_are_the_detectors_draw():
    from self_supervised import tools
    from self_supervised.density import position_channels
    assert tools.PYRAMID_WIDTH == 448 and 448 % 32 == 0              # (the Euclidean metric takes widths that are multiples of 32)
    assert tools._pyramid_columns('knn', {}) is None and tools._pyramid_columns('gde', {}) is None
    assert torch.equal(tools._pyramid_columns('padim', {}), position_channels(448, 96, 0))
    assert torch.equal(tools._pyramid_columns('padim', {"channels": 32, "seed": 4}), position_channels(448, 32, 4))
    state = torch.get_rng_state()
    tools._pyramid_columns('padim', {"seed": 1})
    assert torch.equal(torch.get_rng_state(), state)                 # a generator of its own: every rank draws the same columns


def test_inference_and_sweep_refuse_before_any_file_is_read(tmp_path):
    from self_supervised import tools
    missing = str(tmp_path / "nowhere") + "/"
    with pytest.raises(ValueError, match="dense_features"):
        tools.inference(missing + "best_model.ckpt", missing, "bottle", patch_localization=True, dense_features='pyramid')
    with pytest.raises(ValueError, match="dense_features"):
        tools.sweep(missing, missing, ["bottle"], train=False, dense_features='pyramid')
    with pytest.raises(FileNotFoundError):                            # valid options get as far as the files
        tools.inference(missing + "best_model.ckpt", missing, "bottle", patch_localization=True, localization='dense', bank='train',
                        detector='padim', dense_features='pyramid')


# ---------------------------------------------------------------------------------------------------------------- the detector

def test_preselected_arguments():
    from self_supervised.density import PositionGaussianDetector, position_channels
    det = PositionGaussianDetector(num_patches=4, channels=32, seed=3, preselected=True, width=448)
    assert (det.preselected, det.width) == (True, 448)
    rec, ksel = det._selection(32)
    assert torch.equal(rec, position_channels(448, 32, 3)) and torch.equal(ksel, torch.arange(32))
    with pytest.raises(ValueError, match="the rows must hold the 32 chosen columns and nothing else, got 448"):
        det._selection(448)
    with pytest.raises(ValueError, match="chosen columns"):
        det.check_fit_size(40, 10, 448)
    det.check_fit_size(40, 10, 32)
    plain = PositionGaussianDetector(num_patches=4, channels=32, seed=3)
    assert (plain.preselected, plain.width) == (False, None)
    rec, ksel = plain._selection(448)
    assert torch.equal(rec, ksel) and torch.equal(rec, position_channels(448, 32, 3))
    with pytest.raises(ValueError, match="needs width"):
        PositionGaussianDetector(num_patches=4, channels=32, preselected=True)
    with pytest.raises(ValueError, match="channels"):
        PositionGaussianDetector(num_patches=4, channels=64, preselected=True, width=32)
    with pytest.raises(ValueError, match="width belongs to preselected=True"):
        PositionGaussianDetector(num_patches=4, channels=32, width=448)
    with pytest.raises(ValueError, match="preselected must be a bool"):
        PositionGaussianDetector(num_patches=4, channels=32, preselected=1, width=448)


def test_preselected_state_round_trip(monkeypatch):
    from self_supervised import ops
    from self_supervised.density import PositionGaussianDetector, position_channels
    monkeypatch.setattr(PositionGaussianDetector, "_dev", staticmethod(lambda t: torch.as_tensor(t, dtype=torch.float32)))
    seen = []
    monkeypatch.setattr(ops, "position_sel", lambda sel, D, device: seen.append((torch.as_tensor(sel).clone(), D)) or
                        torch.as_tensor(sel).to(torch.int32))
    det = PositionGaussianDetector(num_patches=4, channels=32, seed=2, preselected=True, width=448)
    det.sel = position_channels(448, 32, 2)
    det.mu_hi, det.mu_lo, det.w = torch.zeros(4, 32), torch.zeros(4, 32), torch.zeros(4, 32, 32)
    st = det.state()
    assert st["preselected"] is True and st["width"] == 448 and torch.equal(st["sel"], position_channels(448, 32, 2))
    back = PositionGaussianDetector.from_state(st, num_patches=4)
    assert (back.preselected, back.width, back.channels, back.seed) == (True, 448, 32, 2)
    assert torch.equal(back.sel, det.sel)                               # the record: columns of the full rows
    assert torch.equal(seen[-1][0], torch.arange(32)) and seen[-1][1] == 32      # what the kernels index with: the identity
    fresh = PositionGaussianDetector(num_patches=4, channels=32, seed=2)
    fresh.load_state(st)                                                # the flag travels with the state (the multi-rank broadcast)
    assert fresh.preselected and fresh.width == 448
    # a state from before the option reads as not preselected
    old = {k: v for k, v in st.items() if k not in ("preselected", "width")}
    plain = PositionGaussianDetector.from_state(old, num_patches=4)
    assert (plain.preselected, plain.width) == (False, None)
    assert torch.equal(seen[-1][0], det.sel) and seen[-1][1] == int(det.sel.max()) + 1
