"""CPU-only checks of the dense feature-map localisation: what is refused from arguments and shapes alone, the integer sample positions
of csrc/patch_features.hip against torch's own bilinear interpolation, the reference of the GPU tests, and the way of the keyword
through tools.sweep."""
import inspect
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import patch_features_ref as R


@pytest.mark.parametrize("kw,match", [
    ({"localization": "dense"}, "patch_localization=True"),
    ({"localization": "dense", "patch_localization": False}, "patch_localization=True"),
    ({"localization": "padim", "patch_localization": True}, "localization must be one of"),
    ({"localization": None, "patch_localization": True}, "localization must be one of")])
def test_localization_checked_before_any_file_is_read(tmp_path, kw, match):
    from self_supervised import tools
    missing = str(tmp_path / "nothing_here")
    with pytest.raises(ValueError, match=match):
        tools.inference(missing + "/model.ckpt", missing + "/", "bottle", **kw)
    sweep_kw = dict(kw, patch_localization=kw.get("patch_localization", False))
    with pytest.raises(ValueError, match=match):
        tools.sweep(missing + "/", missing + "/", ["bottle"], **sweep_kw)


def test_default_is_the_window_localisation():
    from self_supervised import tools
    from self_supervised.models import PeraNet
    for fn in (tools.inference, tools.sweep):
        assert inspect.signature(fn).parameters["localization"].default == 'patches'
    assert inspect.signature(PeraNet.enable_dense_mode).parameters["layers"].default == ('layer2', 'layer3')
    assert PeraNet().dense_layers is None


@pytest.mark.parametrize("layers", [('layer3', 'layer2'), ('layer2', 'layer2'), ('layer2',), ('layer1', 'layer2', 'layer3'),
                                    ('layer2', 'layer4'), 'layer2', ('layer2', 'conv1')])
def test_dense_layers_are_two_stages_finer_first(layers):
    from self_supervised.models import PeraNet
    m = PeraNet()
    with pytest.raises(ValueError, match="finer stage first"):
        m.enable_dense_mode(layers)
    assert m.dense_layers is None
    for ok in (('layer1', 'layer2'), ('layer1', 'layer3'), ['layer2', 'layer3']):
        m.enable_dense_mode(ok)
        assert m.dense_layers == tuple(ok)
    m.disable_dense_mode()
    assert m.dense_layers is None


def test_dense_forward_refusals_come_before_the_device(monkeypatch):
    """Shapes and switches are checked first: on a machine without a GPU these raise ValueError, not the no-GPU RuntimeError."""
    from self_supervised.models import PeraNet
    m = PeraNet().eval()
    m.enable_dense_mode()
    with pytest.raises(ValueError, match="square"):
        m(torch.zeros(1, 3, 96, 128))
    with pytest.raises(ValueError, match="64 x 64"):
        m(torch.zeros(1, 3, 63, 63))
    monkeypatch.setenv("SSAD_MATH", "bf16x6")
    with pytest.raises(ValueError, match="fp32"):
        m(torch.zeros(1, 3, 96, 96))
    monkeypatch.delenv("SSAD_MATH")
    m.enable_patch_level_mode()
    with pytest.raises(ValueError, match="two localisations"):
        m(torch.zeros(1, 3, 96, 96))
    m.disable_patch_level_mode()
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m(torch.zeros(1, 3, 96, 96))
    m.eval()
    with pytest.raises(RuntimeError, match="GPU"):          # everything in order: only the device is missing
        m(torch.zeros(1, 3, 96, 96))
    assert m.batch is None and m.num_patches is None


def test_stage_shapes_follow_the_trunk():
    from self_supervised import engine
    assert engine.stage_shapes(256, 256) == {"layer1": (64, 64, 64), "layer2": (32, 32, 128), "layer3": (16, 16, 256),
                                             "layer4": (8, 8, 512)}
    assert engine.stage_shapes(96, 96)["layer2"] == (12, 12, 128) and engine.stage_shapes(96, 96)["layer3"] == (6, 6, 256)
    assert engine.stage_shapes(65, 100)["layer3"] == (5, 7, 256)          # 65 -> 33 -> 17 -> 9 -> 5, 100 -> 50 -> 25 -> 13 -> 7


RATIOS = sorted({(s[1], s[4]) for s in R.SHAPES} | {(s[2], s[5]) for s in R.SHAPES} | {(64, 32), (7, 4), (3, 8), (1, 5)})


@pytest.mark.parametrize("nf,nc", RATIOS)
def test_integer_positions_equal_torch_interpolate(nf, nc):
    """Row k of torch's float64 bilinear resampling of the nc x nc identity (one-hot inputs) is the weight every source position has in
    destination k: it must be 1 - l at tap a and l at tap b of the integer table.  torch forms its position in floating point (scale
    factor, product, subtraction: three roundings of values up to nc), so its weights are off the exact rationals by up to
    3 nc 2^-53; the bar is 4 nc 2^-53."""
    from self_supervised import ops
    a, b, num, den = ops.bilinear_taps(nf, nc)
    eye = torch.eye(nc, dtype=torch.float64).reshape(1, nc, nc, 1)       # channel s = the one-hot map of source position s
    w = F.interpolate(eye, size=(nf, 1), mode='bilinear', align_corners=False).reshape(nc, nf)
    for i in range(nf):
        assert 0 <= a[i] <= b[i] <= min(a[i] + 1, nc - 1) and 0 <= num[i] < den
        lam = Fraction(num[i], den)
        assert lam == max(Fraction((2 * i + 1) * nc, 2 * nf) - Fraction(1, 2), 0) - a[i]
        want = torch.zeros(nc, dtype=torch.float64)
        want[a[i]] += float(1 - lam)
        want[b[i]] += float(lam)
        assert (w[:, i] - want).abs().max().item() <= 4 * nc * 2.0 ** -53, (nf, nc, i)


def test_reference_is_the_library_calls():
    """patch_features_ref.reference against a direct evaluation of the definition (zero-padded 3 x 3 mean, taps of the integer table) in
    float64, on the smallest odd shape."""
    from self_supervised import ops
    shape = R.SHAPES[1]
    fine, coarse, ref, bar = R.case(shape)
    n, hf, wf, cf, hc, wc, cc = shape
    assert tuple(ref.shape) == (n * hf * wf, cf + cc) and (bar > 0).all()

    def pool(t):
        p = F.pad(t.double(), (0, 0, 1, 1, 1, 1))
        return sum(p[:, dy:dy + t.shape[1], dx:dx + t.shape[2]] for dy in range(3) for dx in range(3)) / 9.0
    pf, pc = pool(fine), pool(coarse)
    ya, yb, yn, yd = ops.bilinear_taps(hf, hc)
    xa, xb, xn, xd = ops.bilinear_taps(wf, wc)
    want = torch.empty(n, hf, wf, cf + cc, dtype=torch.float64)
    want[..., :cf] = pf
    for i in range(hf):
        for j in range(wf):
            ly, lx = yn[i] / yd, xn[j] / xd
            want[:, i, j, cf:] = ((1 - ly) * ((1 - lx) * pc[:, ya[i], xa[j]] + lx * pc[:, ya[i], xb[j]])
                                  + ly * ((1 - lx) * pc[:, yb[i], xa[j]] + lx * pc[:, yb[i], xb[j]]))
    assert (want.reshape(ref.shape) - ref).abs().max().item() <= 1e-13
    # a plain fp32 evaluation of the same library calls stays within 5 units of the bar's 40
    f32 = torch.cat([F.avg_pool2d(fine.permute(0, 3, 1, 2), 3, 1, 1),
                     F.interpolate(F.avg_pool2d(coarse.permute(0, 3, 1, 2), 3, 1, 1), size=(hf, wf), mode='bilinear',
                                   align_corners=False)], 1).permute(0, 2, 3, 1).reshape(ref.shape)
    assert R.worst_units(f32, shape) <= 5.0


def test_sweep_forwards_the_keyword(monkeypatch, tmp_path):
    from self_supervised import tools
    seen = []

    class Stop(Exception):
        pass

    def fake_inference(*a, **kw):
        seen.append(kw)
        raise Stop
    monkeypatch.setattr(tools, "inference", fake_inference)
    for kw, want in (({"localization": "dense"}, "dense"), ({"localization": "patches"}, None), ({}, None)):
        with pytest.raises(Stop):
            tools.sweep(str(tmp_path) + "/", str(tmp_path) + "/", ["bottle"], train=False, **kw)
        assert seen[-1].get("localization") == want and seen[-1]["patch_localization"] is True
