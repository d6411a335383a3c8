"""GPU: csrc/resize_gaussian.hip (ssad_resize_gaussian, ops.resize_gaussian, tools.upsample(method='resize_blur')) against the
float64 operator of tests/resize_gaussian_ref.py, which tests/test_resize_gaussian_host.py pins to scipy.ndimage.gaussian_filter
and to torch's reflect-pad convolution.

The bar, per pixel: |got - ref64| <= (K_y + K_x + 4) 2^-24 (A_y |M| A_x^T) -- (2 K + 4) u for square maps.  The kernel sums each
chain in ascending tap order with one FMA per tap, starting from 0: a term passes through at most K roundings of the partial sum
and carries the one rounding of its fp32 weight, so a chain is within (K + 1) u of its exact sum to first order, the two chains
compose to (K_y + K_x + 2) u and 2 u cover the second-order terms (resize_gaussian_ref.bar).  K counts the zero-padded taps.

The C entry writes between 0xff guards into an output that starts out as 0xff bytes (NaN: every pixel must be written); the input
and both operator tables sit between NaN guards; every case runs twice and must give the same bits."""
import os

import numpy as np
import pytest
import torch

import resize_gaussian_ref as ref
from fake_mvtec import make_tree
from self_supervised import _hip, ops, tools

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats: 256 bytes, so the payload keeps the allocation's 16-byte alignment
NAN_BITS = 0x7FC00000


def _guarded(a, guard=GUARD):
    """A device copy of `a` (float32 or int32) between two guards of NaN bit patterns -> (whole, view)."""
    flat = np.ascontiguousarray(a).reshape(-1)
    whole = np.full(flat.size + 2 * guard, NAN_BITS, np.int32)
    whole[guard:guard + flat.size] = flat.view(np.int32)
    whole = torch.from_numpy(whole).cuda()
    return whole, whole[guard:guard + flat.size]


def _tables(extent, T, sigma, border):
    first, weights, K = ref.pack(ref.operator(extent, T, sigma, border))
    return _guarded(first), _guarded(weights), K


class Out:
    """n * T * T floats between two guards, all of it 0xff bytes."""

    def __init__(self, numel, guard=GUARD):
        self.whole = torch.full(((numel + 2 * guard) * 4,), 0xFF, dtype=torch.uint8, device="cuda")
        self.guard, self.numel = guard * 4, numel

    def ptr(self):
        return self.whole.data_ptr() + self.guard

    def guards_intact(self):
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        return bool((w[:self.guard] == 0xFF).all() and (w[self.guard + 4 * self.numel:] == 0xFF).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.whole == 0xFF).all().item())

    def numpy(self, shape):
        assert self.guards_intact(), "a guard was overwritten"
        return self.whole.cpu().numpy()[self.guard:self.guard + 4 * self.numel].view(np.float32).reshape(shape).copy()


def raw(M, T, sigma, border, band=0, out_guard=GUARD):
    """ssad_resize_gaussian on numpy maps [n][h][w] -> numpy [n][T][T]; run twice, the two runs bit-equal."""
    n, h, w = M.shape
    (yf_all, yf), (yw_all, yw), Ky = _tables(h, T, sigma, border)
    (xf_all, xf), (xw_all, xw), Kx = _tables(w, T, sigma, border)
    m_all, m = _guarded(M.astype(np.float32))
    lib = _hip.lib()
    got = []
    for _ in range(2):
        out = Out(n * T * T, out_guard)
        rc = lib.ssad_resize_gaussian(m.data_ptr(), n, h, w, yf.data_ptr(), yw.data_ptr(), Ky, xf.data_ptr(), xw.data_ptr(), Kx, T, band,
                                      out.ptr(), _hip.stream())
        assert rc == 0, lib.ssad_last_error()
        got.append(out.numpy((n, T, T)))
    assert not np.isnan(got[0]).any(), "a pixel was not written (or is NaN)"
    assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32)), "two runs differ"
    return got[0]


def check(got, M, T, sigma, border, what):
    want, bar = ref.reference(M, T, sigma, border), ref.bar(M, T, sigma, border)
    err = np.abs(got.astype(np.float64) - want)
    ok = bar > 0
    worst = float((err[ok] / bar[ok]).max()) if ok.any() else 0.0
    print(f"{what}: worst |err| / bar = {worst:.3f}, max |err| = {err.max():.3g}")
    assert (err <= bar).all(), f"{what}: worst error / bar {worst}"
    return worst


KINDS = ("nonneg", "mixed", "constant", "impulse")
CASES = [(32, 32, 256, 4.0, "symmetric"), (32, 32, 256, 4.0, "reflect"), (29, 29, 256, 4.0, "symmetric"), (29, 29, 256, 4.0, "reflect"),
         (5, 9, 40, 4.0, "symmetric"), (5, 9, 40, 4.0, "reflect"),           # non-square; the borders reach every pixel
         (7, 7, 17, 4.0, "reflect"),                                         # T = radius + 1, the limit
         (3, 3, 18, 4.0, "symmetric"),
         (32, 32, 250, 4.0, "symmetric"),                                    # T % 4 != 0: scalar stores, ragged last band
         (32, 32, 64, 1.5, "symmetric"), (32, 32, 64, 1.5, "reflect")]


@pytest.mark.parametrize("h,w,T,sigma,border", CASES)
def test_kernel_against_float64(h, w, T, sigma, border):
    M = np.concatenate([ref.maps(k, 1, h, w, seed=10 + i) for i, k in enumerate(KINDS)])
    got = raw(M, T, sigma, border)
    check(got, M, T, sigma, border, f"{h} x {w} -> {T} sigma {sigma} {border}")
    # the constant map comes back as the constant (rows of A sum to 1 within 5e-16)
    c = float(M[2, 0, 0])
    Ky, Kx = ref.pack(ref.operator(h, T, sigma, border))[2], ref.pack(ref.operator(w, T, sigma, border))[2]
    assert np.abs(got[2].astype(np.float64) - c).max() <= (Ky + Kx + 4) * ref.U * c + 1e-14 * c


def test_large_map_several_bands_at_the_lds_limit():
    h, T = 128, 512
    K = ref.pack(ref.operator(h, T, 4.0, "symmetric"))[2]
    band = _hip.lib().ssad_resize_gaussian_band(h, h, T, K)
    assert 1 <= band < T // 4                                                # several bands per map
    M = np.concatenate([ref.maps("nonneg", 1, h, h, seed=21), ref.maps("mixed", 1, h, h, seed=22)])
    got = raw(M, T, 4.0, "symmetric")
    check(got, M, T, 4.0, "symmetric", f"128 x 128 -> 512, n = 2, band {band}")
    M2 = np.concatenate([ref.maps("constant", 1, h, h, seed=0), ref.maps("impulse", 1, h, h, seed=0)])
    check(raw(M2, T, 4.0, "reflect"), M2, T, 4.0, "reflect", "128 x 128 -> 512 reflect, constant + impulse")


def test_wide_map_takes_a_lower_band():
    """128 x 512 -> 512: the band of 32 rows no longer fits, 16 rows need exactly the LDS a launch may ask for."""
    h, w, T = 128, 512, 512
    Ky = ref.pack(ref.operator(h, T, 4.0, "symmetric"))[2]
    lib = _hip.lib()
    assert lib.ssad_resize_gaussian_band(h, w, T, Ky) == 16 and lib.ssad_resize_gaussian_band(h, h, T, Ky) == 32
    M = ref.maps("mixed", 1, h, w, seed=23)
    check(raw(M, T, 4.0, "symmetric"), M, T, 4.0, "symmetric", "128 x 512 -> 512, band 16")


def test_bits_do_not_depend_on_band_height_store_width_or_batch():
    h, T = 29, 256
    M = ref.maps("nonneg", 70, h, h, seed=31)
    whole = raw(M, T, 4.0, "symmetric")
    check(whole[:4], M[:4], T, 4.0, "symmetric", "29 -> 256, first 4 of n = 70")
    bits = lambda a: a.view(np.int32)
    for i in (0, 37, 69):
        assert np.array_equal(bits(raw(M[i:i + 1], T, 4.0, "symmetric")[0]), bits(whole[i])), f"map {i} alone differs from n = 70"
    three = raw(M[[5, 37, 11]], T, 4.0, "symmetric")
    assert np.array_equal(bits(three[1]), bits(whole[37])) and np.array_equal(bits(three[0]), bits(whole[5]))
    for band in (1, 5, 8, 64, 256):                                          # 5: ragged; 256: one workgroup per map
        assert np.array_equal(bits(raw(M[:2], T, 4.0, "symmetric", band=band)), bits(whole[:2])), f"band {band} differs"
    # an output that is only 4-byte aligned takes the scalar stores: same bits
    assert np.array_equal(bits(raw(M[:2], T, 4.0, "symmetric", out_guard=GUARD + 1)), bits(whole[:2]))


def test_bad_arguments_return_nonzero_and_write_nothing():
    h, T = 128, 512
    (_, yf), (_, yw), K = _tables(h, T, 4.0, "symmetric")
    _, m = _guarded(ref.maps("nonneg", 1, h, h, seed=1))
    out = Out(T * T)
    lib = _hip.lib()
    good = [m.data_ptr(), 1, h, h, yf.data_ptr(), yw.data_ptr(), K, yf.data_ptr(), yw.data_ptr(), K, T, 0, out.ptr(), _hip.stream()]

    def bad(**kw):
        names = ["maps", "n", "h", "w", "yf", "yw", "Ky", "xf", "xw", "Kx", "T", "band", "out", "stream"]
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        rc = lib.ssad_resize_gaussian(*args)
        assert rc != 0, kw
        assert b"ssad_resize_gaussian" in lib.ssad_last_error()

    bad(band=256)                                                            # 76 source rows of 128 + 512 floats: 194 KB of LDS
    bad(band=64)
    bad(band=-1)
    bad(band=257)
    for name in ("maps", "yf", "yw", "xf", "xw", "out"):
        bad(**{name: None})
    for name in ("n", "h", "w", "T", "Ky", "Kx"):
        bad(**{name: 0})
        bad(**{name: -3})
    bad(Ky=h + 1)
    assert lib.ssad_resize_gaussian_band(0, 4, 4, 1) == 0 and lib.ssad_resize_gaussian_band(4096, 4096, 4096, 40) == 0
    assert out.untouched()
    assert lib.ssad_resize_gaussian(*good) == 0                              # the arguments were otherwise fine
    assert not np.isnan(out.numpy((T, T))).any()


# ---------------------------------------------------------------------------------------------------------------- through Python

def test_ops_and_upsample():
    M = ref.maps("nonneg", 3, 32, 32, seed=41)
    dev = torch.from_numpy(M).cuda()
    for border in ("symmetric", "reflect"):
        got = ops.resize_gaussian(dev.unsqueeze(1), 256, 4.0, border)
        assert tuple(got.shape) == (3, 1, 256, 256) and got.dtype == torch.float32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy()[:, 0], raw(M, 256, 4.0, border))             # ops.py's tables are the test's own
        assert torch.equal(ops.resize_gaussian(dev, 256, 4.0, border), got)                  # [n][h][w]
        assert torch.equal(tools.upsample(dev.unsqueeze(1), 256, verbose=False, method="resize_blur", border=border), got)
    first, weights, K = ops.resize_gaussian_operator(32, 256, 4.0, "symmetric", dev.device)
    want = ref.pack(ref.operator(32, 256, 4.0, "symmetric"))
    assert first.is_cuda and K == want[2] and np.array_equal(first.cpu().numpy(), want[0]) and np.array_equal(weights.cpu().numpy(), want[1])
    # defaults: sigma 4, 'symmetric'; other sigma goes through
    sym = ops.resize_gaussian(dev, 256)
    assert torch.equal(tools.upsample(dev.unsqueeze(1), 256, verbose=False, method="resize_blur"), sym)
    got15 = tools.upsample(dev.unsqueeze(1), 64, verbose=False, method="resize_blur", sigma=1.5)
    check(got15.cpu().numpy()[:, 0], M, 64, 1.5, "symmetric", "upsample(sigma=1.5) 32 -> 64")
    # non-square, half precision input, a CPU tensor: moved to the device as the reference method does
    N = ref.maps("mixed", 2, 5, 9, seed=42)
    check(ops.resize_gaussian(torch.from_numpy(N).cuda(), 40).cpu().numpy()[:, 0], N, 40, 4.0, "symmetric", "ops 5 x 9 -> 40")
    half = torch.from_numpy(M).cuda().half()
    assert torch.equal(ops.resize_gaussian(half, 256), ops.resize_gaussian(half.float(), 256))
    cpu = tools.upsample(torch.from_numpy(M).unsqueeze(1), 256, verbose=False, method="resize_blur")
    assert cpu.is_cuda and torch.equal(cpu, sym)


def test_reference_method_is_unchanged_and_differs():
    M = torch.from_numpy(ref.maps("nonneg", 3, 32, 32, seed=43)).unsqueeze(1)
    default = tools.upsample(M, 256, verbose=False)
    assert torch.equal(tools.upsample(M, 256, verbose=False, method="reference"), default)
    assert torch.equal(tools.upsample(M, 256, verbose=False, method="reference", sigma=9.0, border="reflect"), default)
    assert torch.equal(default, ops.blur_relu_bilinear(M.cuda(), 7, 256))
    new = tools.upsample(M, 256, verbose=False, method="resize_blur")
    assert new.shape == default.shape and not torch.equal(new, default)
    assert (new - default).abs().max().item() > 1e-3
    with pytest.raises(ValueError):
        tools.upsample(M, 256, verbose=False, method="other")
    with pytest.raises(ValueError):
        tools.upsample(M, 16, verbose=False, method="resize_blur")           # radius 16 >= 16


# -------------------------------------------------------------------------------------------------------- through tools.inference

SIZE, N_TRAIN, CHANNELS = 96, 48, 32          # the fixture of tests/test_hip_padim.py: 96 x 96 images, 12 x 12 dense maps


def _datamodule(root, **kw):
    from self_supervised.datasets import MVTecDatamodule
    return MVTecDatamodule(root, imsize=(SIZE, SIZE), **kw)


@pytest.fixture()
def tree(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    monkeypatch.setattr(tools, "MVTecDatamodule", _datamodule)
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=SIZE)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


def test_padim_maps_end_to_end(tree, tmp_path):
    root, ck = tree
    np.random.seed(3)
    res = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, localization='dense',
                          bank='train', detector='padim', detector_options={"channels": CHANNELS})
    low = res.anomaly_maps
    assert tuple(low.shape) == (4, 1, 12, 12)
    M = low.detach().float().cpu().numpy()[:, 0]
    side = int(res.ground_truths.shape[-1])
    assert side == SIZE
    up = tools.upsample(low, side, verbose=False, method="resize_blur")
    assert tuple(up.shape) == (4, 1, SIZE, SIZE) and up.is_cuda
    check(up.cpu().numpy()[:, 0], M, SIZE, 4.0, "symmetric", "padim maps 12 -> 96")
    assert not torch.equal(up, tools.upsample(low, side, verbose=False))
    res.anomaly_maps = up
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou'])
    ev.evaluate(res, "bottle", str(tmp_path / "out") + "/", patch_level=True)
    assert ev.scores.auroc is not None and np.isfinite(ev.scores.auroc)
    thr = float(np.float32(np.median(ref.reference(M, SIZE))))
    regions = tools.defect_regions(up, thr)
    assert tuple(regions.pred_masks.shape) == (4, 1, SIZE, SIZE)
    assert torch.equal(regions.pred_masks.bool(), up >= thr) and sum(len(r) for r in regions.regions) >= 1
    # the sweep passes the method on and writes its table
    out = str(tmp_path / "sweep") + "/"
    os.makedirs(out + "bottle")
    os.replace(ck, out + "bottle/best_model.ckpt")
    np.random.seed(3)
    df = tools.sweep(root, out, ["bottle"], train=False, detector='padim', bank='train', localization='dense',
                     detector_options={"channels": CHANNELS}, tables_output=out + "tables/", upsample_method='resize_blur')
    assert list(df.index) == ["bottle", "average"] and np.isfinite(df.loc["bottle", "auroc"])
    assert os.path.exists(out + "tables/csv/patch_all_scores.csv")
    assert abs(float(df.loc["bottle", "auroc"]) - float(ev.scores.auroc)) <= 1e-12       # the same maps as the calls above
