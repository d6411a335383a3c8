"""GPU parity: every HIP kernel and the full scoring path against the CPU oracle / golden vectors.
All calls go through the C ABI (self_supervised.ops -> libssad_hip.so)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    return torch.device("cuda:0")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def assert_close(got, want, tol=1e-4):
    """|got-want| <= tol * max(1, max|want|): fp32 tolerance of BASELINE.json (1e-4), scale-aware."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert err <= tol * scale, f"max err {err:.3e} > {tol} * {scale:.3e}"


CONV_CASES = [
    # N, H, W, Cin, Cout, k, stride, pad, affine, residual, relu
    (3, 16, 16, 64, 64, 3, 1, 1, True, True, True),
    (2, 16, 16, 64, 128, 3, 2, 1, True, False, True),
    (2, 16, 16, 64, 128, 1, 2, 0, True, False, False),
    (5, 4, 4, 256, 256, 3, 1, 1, True, True, True),
    (7, 2, 2, 512, 512, 3, 1, 1, False, False, False),
    (1, 9, 7, 32, 96, 3, 1, 1, True, True, False),          # ragged M and Cout tails
    (2, 5, 5, 128, 588, 1, 1, 0, False, False, False),      # bank-like Cout (not a multiple of 32)
    (1, 1, 1, 64, 4, 1, 1, 0, True, False, False),          # classifier-like
    (130, 4, 4, 64, 64, 3, 1, 1, True, True, True),          # >= 128 samples on a small map: position-major rows,
    (200, 2, 2, 64, 128, 3, 1, 1, True, False, True),        #   zero-padding taps skipped as whole K-steps
    (150, 8, 8, 32, 96, 3, 2, 1, False, True, False),
    (129, 1, 1, 32, 64, 3, 1, 1, True, False, False),        # 1x1 map: only the centre tap survives
    (3, 5, 5, 64, 411, 1, 1, 0, True, True, True),           # Cout not a multiple of 4 (odd-sized k-NN bank)
    (140, 2, 2, 32, 70, 3, 1, 1, True, False, True),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_igemm(dev, case):
    from self_supervised import ops
    n, h, w, cin, cout, k, s, p, affine, res, relu = case
    g = torch.Generator().manual_seed(hash(case) % 1000)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    want = F.conv2d(x, wt, None, s, p)
    sc = sh = r = None
    if affine:
        sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
        want = want * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    if res:
        r = torch.randn(want.shape, generator=g)
        want = want + r
    if relu:
        want = want.relu()
    w_ohwi = ops.repack_oihw_to_ohwi(wt.to(dev))
    assert torch.equal(w_ohwi.cpu(), wt.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(ops.repack_ohwi_to_oihw(w_ohwi).cpu(), wt)
    got = ops.conv_fwd(nhwc(x).to(dev), w_ohwi, None if sc is None else sc.to(dev), None if sh is None else sh.to(dev),
                       None if r is None else nhwc(r).to(dev), relu, s, p)
    assert_close(nchw(got), want, 2e-5)


@pytest.mark.parametrize("case", [(130, 4, 4, 64, 64, 3, 1, 1), (200, 2, 2, 64, 128, 3, 1, 1), (150, 8, 8, 32, 96, 3, 2, 1),
                                  (70, 16, 16, 32, 64, 3, 1, 1), (300, 8, 8, 64, 128, 1, 2, 0), (129, 1, 1, 32, 64, 3, 1, 1),
                                  (4229, 4, 4, 32, 128, 3, 1, 1), (4229, 8, 8, 32, 64, 3, 2, 1), (8200, 2, 2, 32, 32, 3, 1, 1)])
def test_conv_igemm_hwnc(dev, case):
    """Position-major layout [H][W][N][C] with padding taps skipped: same numbers as conv2d.  The last three cases have more
    than 32 sample groups: the heaviest-first position order then runs chunk by chunk, with a ragged last chunk."""
    from self_supervised import ops
    n, h, w, cin, cout, k, s, p = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    want = F.conv2d(x, wt, None, s, p) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    r = torch.randn(want.shape, generator=g)
    want = (want + r).relu()
    hwnc = lambda t: t.permute(2, 3, 0, 1).contiguous()            # NCHW -> HWNC
    got = ops.conv_fwd_hwnc(hwnc(x).to(dev), ops.repack_oihw_to_ohwi(wt.to(dev)), sc.to(dev), sh.to(dev), hwnc(r).to(dev),
                            True, s, p)
    assert_close(got.permute(2, 3, 0, 1), want, 2e-5)


def test_conv_identity_asymmetric(dev):
    """A = I check with an asymmetric B (guards against a transposed C/D map)."""
    from self_supervised import ops
    cin = cout = 64
    wt = torch.zeros(cout, cin, 1, 1)
    wt[torch.arange(cout), torch.arange(cin)] = 1.0
    x = torch.arange(4 * cin * 3 * 5, dtype=torch.float32).reshape(4, cin, 3, 5) / 7.0
    got = ops.conv_fwd(nhwc(x).to(dev), ops.repack_oihw_to_ohwi(wt.to(dev)))
    assert torch.equal(nchw(got).cpu(), x)


@pytest.mark.parametrize("mode", ["image64", "image256", "patch", "up32", "up48", "odd"])
def test_stem_and_pool(dev, mode, seeded_sd):
    from self_supervised import ops
    from oracle import weights as ow, scoring as osc
    w = seeded_sd["feature_extractor.conv1.weight"]
    g = torch.Generator().manual_seed(3)
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    pd = ps = 0
    if mode == "image64":
        x = ow.synthetic_images(3, 64, seed=1); ref_in = x
    elif mode == "image256":
        x = ow.synthetic_images(1, 256, seed=2); ref_in = x
    elif mode == "patch":
        x = ow.synthetic_images(2, 64, seed=4)[:, :, :, :56].contiguous(); pd, ps = 32, 8
        p = osc.extract_patches(x, 32, 8); ref_in = F.interpolate(p.reshape(-1, 3, 32, 32), 64, mode="nearest")
    elif mode == "up32":
        x = ow.synthetic_images(2, 32, seed=5); ref_in = F.interpolate(x, 64, mode="nearest")
    elif mode == "up48":
        x = ow.synthetic_images(2, 48, seed=6); ref_in = F.interpolate(x, 64, mode="nearest")
    else:
        x = ow.synthetic_images(2, 256, seed=7)[:, :, :101, :77].contiguous(); ref_in = x
    want = (F.conv2d(ref_in, w, None, 2, 3) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).relu()
    wk = ops.pack_stem_weight(w.to(dev))
    got = ops.stem_fwd(x.to(dev), wk, sc.to(dev), sh.to(dev), True, pd, ps)
    assert_close(nchw(got), want, 2e-5)
    pooled = ops.maxpool3x3s2_fwd(got)
    assert torch.equal(nchw(pooled).cpu(), F.max_pool2d(nchw(got).cpu(), 3, 2, 1))


@pytest.mark.parametrize("hwnc", [False, True])
def test_fused_patch_stem(dev, seeded_sd, hwnc):
    """Folded 4x4 conv + affine + ReLU + max-pool == upsample, conv7x7/2, affine, ReLU, max_pool2d."""
    from self_supervised import ops
    from oracle import weights as ow, scoring as osc
    w = seeded_sd["feature_extractor.conv1.weight"]
    g = torch.Generator().manual_seed(4)
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    x = ow.synthetic_images(2, 64, seed=11)[:, :, :, :56].contiguous()
    p = osc.extract_patches(x, 32, 8).reshape(-1, 3, 32, 32)
    want = F.max_pool2d((F.conv2d(F.interpolate(p, 64, mode="nearest"), w, None, 2, 3) * sc.view(1, -1, 1, 1)
                         + sh.view(1, -1, 1, 1)).relu(), 3, 2, 1)
    got = ops.stem_patch_pool_fwd(x.to(dev), ops.pack_stem_weight_folded(w.to(dev)), sc.to(dev), sh.to(dev), 8, hwnc)
    full = got
    got = got.permute(2, 3, 0, 1) if hwnc else got.permute(0, 3, 1, 2)
    assert_close(got, want, 2e-5)
    # the ring form (layer1 shared between overlapping patches): everything outside the skipped square, bit for bit
    for lo, hi in ((4, 12), (0, 15), (7, 7)):
        ring = ops.stem_patch_pool_fwd(x.to(dev), ops.pack_stem_weight_folded(w.to(dev)), sc.to(dev), sh.to(dev), 8, hwnc, (lo, hi))
        keep = torch.ones(16, 16, dtype=torch.bool)
        keep[lo:hi + 1, lo:hi + 1] = False
        a, b = (ring[keep.to(dev)], full[keep.to(dev)]) if hwnc else (ring[:, keep.to(dev)], full[:, keep.to(dev)])
        assert torch.equal(a, b), (lo, hi)
    if hwnc:
        # the border form: rows / columns 0, 1, 15, bit for bit; nothing else written
        border = ops.stem_patch_border_fwd(x.to(dev), ops.pack_stem_weight_folded(w.to(dev)), sc.to(dev), sh.to(dev), 8)
        edge = torch.zeros(16, 16, dtype=torch.bool)
        edge[[0, 1, 15], :] = True
        edge[:, [0, 1, 15]] = True
        assert torch.equal(border[edge.to(dev)], full[edge.to(dev)])
        from self_supervised import _hip
        poisoned = torch.full_like(full, 3.25)
        xd, wfd, scd, shd = x.to(dev), ops.pack_stem_weight_folded(w.to(dev)), sc.to(dev), sh.to(dev)      # (kept alive across the launch)
        _hip.check(_hip.lib().ssad_stem_patch_border_fwd(_hip.ptr(xd), 2, 64, 56, 8, _hip.ptr(wfd), _hip.ptr(scd), _hip.ptr(shd),
                                                         _hip.ptr(poisoned), _hip.stream()))
        assert (poisoned[(~edge).to(dev)] == 3.25).all() and torch.equal(poisoned[edge.to(dev)], full[edge.to(dev)])
    # image-level 32x32 inputs take the same kernel (one window per image)
    xi = ow.synthetic_images(3, 32, seed=12)
    want = F.max_pool2d((F.conv2d(F.interpolate(xi, 64, mode="nearest"), w, None, 2, 3) * sc.view(1, -1, 1, 1)
                         + sh.view(1, -1, 1, 1)).relu(), 3, 2, 1)
    got = ops.stem_patch_pool_fwd(xi.to(dev), ops.pack_stem_weight_folded(w.to(dev)), sc.to(dev), sh.to(dev), 1, False)
    assert_close(got.permute(0, 3, 1, 2), want, 2e-5)


def test_gap(dev):
    from self_supervised import ops
    x = torch.randn(5, 8, 8, 128)
    out = torch.zeros(5, 896, device=dev)
    ops.gap_fwd(x.to(dev), out, 128)
    assert_close(out[:, 128:256], x.mean(dim=(1, 2)), 1e-6)
    assert out[:, :128].abs().max().item() == 0 and out[:, 256:].abs().max().item() == 0
    # the few-samples / large-map kernel (training batches), a small map and an odd channel count
    for (n, hw, c) in [(5, 8, 128), (3, 2, 512), (4, 7, 36)]:
        x = torch.randn(n, hw, hw, c) + 0.5
        out = torch.zeros(n, c + 8, device=dev)
        ops.gap_fwd(x.to(dev), out, 4)
        assert_close(out[:, 4:4 + c], x.double().mean(dim=(1, 2)).float(), 2e-6)
        assert out[:, :4].abs().max().item() == 0 and out[:, 4 + c:].abs().max().item() == 0


def _model(sd, dev, patch):
    from self_supervised.models import PeraNet
    m = PeraNet()
    m.load_state_dict(sd, strict=True)
    m.eval().to(dev)
    if patch:
        m.enable_patch_level_mode()
    return m


def test_forward_golden_image_level(dev, golden, seeded_sd):
    from oracle import weights as ow
    g = golden("forward")
    m = _model(seeded_sd, dev, False)
    with torch.no_grad():
        for key, x in (("img", ow.synthetic_images(2, 256, seed=1234)), ("c1", ow.synthetic_images(8, 64, seed=77)),
                       ("up", ow.synthetic_images(4, 32, seed=78)), ("up48", ow.synthetic_images(2, 48, seed=79))):
            o = m(x.to(dev))
            assert_close(o["latent_space"], torch.from_numpy(g[key + "_emb"]))
            assert_close(o["classifier"], torch.from_numpy(g[key + "_logits"]))


def test_forward_golden_patch_level(dev, golden, seeded_sd):
    from oracle import weights as ow
    g = golden("forward")
    m = _model(seeded_sd, dev, True)
    with torch.no_grad():
        o = m(ow.synthetic_images(2, 64, seed=99)[:, :, :, :48].contiguous().to(dev))
        assert [m.batch, m.num_patches] == list(g["psmall_bp"])
        assert_close(o["latent_space"], torch.from_numpy(g["psmall_emb"]))
        assert_close(o["classifier"], torch.from_numpy(g["psmall_logits"]))
        o = m(ow.synthetic_images(1, 256, seed=4321).to(dev))
        assert (m.batch, m.num_patches) == (1, 841)
        emb = o["latent_space"].cpu()
        assert_close(emb[torch.from_numpy(g["patch_rows"])], torch.from_numpy(g["patch_emb_rows"]))
        assert_close(emb.double().sum(1), torch.from_numpy(g["patch_emb_rowsum"]), 1e-4)
        assert_close(o["classifier"], torch.from_numpy(g["patch_logits"]))
        # chunked trunk passes must not change anything
        m.max_samples_per_pass = 841
        o2 = m(torch.cat([ow.synthetic_images(1, 256, seed=4321)] * 3).to(dev))
        assert torch.equal(o2["latent_space"][:841], o["latent_space"]) and torch.equal(o2["latent_space"][1682:], o["latent_space"])
        assert m.last_pass_samples == 841
        # ... nor the cap on elements per activation tensor (2 images per pass here), nor equalised passes (3 images: 2 + 1 -> 2 x 2 rounds down to 1 + ...)
        m.max_samples_per_pass = 131072
        m.max_elements_per_tensor = 2 * 841 * 16 * 16 * 64
        o3 = m(torch.cat([ow.synthetic_images(1, 256, seed=4321)] * 3).to(dev))
        assert m.last_pass_samples == 2 * 841 and torch.equal(o3["latent_space"], o2["latent_space"])
        # ... nor a pass size derived from (very little) free HBM
        m.max_elements_per_tensor = 2 ** 31 - 1
        m.hbm_fraction_per_pass = 1e-9
        o4 = m(torch.cat([ow.synthetic_images(1, 256, seed=4321)] * 3).to(dev))
        assert m.last_pass_samples == 841 and torch.equal(o4["latent_space"], o2["latent_space"])


def test_scoring_pass_just_under_2_31_elements(dev, seeded_sd):
    """One trunk pass whose layer1 tensors hold 155 x 841 x 16 x 16 x 64 = 2 135 736 320 elements (2^31 = 2 147 483 648): every
    kernel's offsets must survive the largest pass forward() ever builds.  First and last image == the same image scored alone."""
    from oracle import weights as ow
    free, _ = torch.cuda.mem_get_info()
    if free < 80 * 2 ** 30:
        pytest.skip("needs ~40 GB of free HBM")
    m = _model(seeded_sd, dev, True)
    a, b = ow.synthetic_images(1, 256, seed=11).to(dev), ow.synthetic_images(1, 256, seed=12).to(dev)
    x = torch.cat([a] + [b] * 154 + [a])                 # 156 images -> passes of 155 + 1 unless equalised: force ONE big pass
    with torch.no_grad():
        ra, rb = m(a)["latent_space"].clone(), m(b)["latent_space"].clone()
        m._samples_per_pass = lambda *args: 155
        o = m(x)["latent_space"]
    assert m.last_pass_samples == 155 * 841
    assert torch.equal(o[:841], ra) and torch.equal(o[154 * 841:155 * 841], rb) and torch.equal(o[155 * 841:], ra)
    assert torch.equal(o[77 * 841:78 * 841], rb)


def test_upsample_tiled_equals_single_workgroup(dev):
    """Maps too large for one workgroup's LDS take the tiled blur + bilinear kernel: bit-identical to the single-workgroup kernel
    where both apply (forced here through the oracle), and equal to the oracle on a 128 x 128 -> 512 x 512 map and a ragged one."""
    from self_supervised import ops
    from oracle import scoring as osc
    g = torch.Generator().manual_seed(8)
    for n, h, w, target in ((2, 128, 128, 512), (1, 90, 90, 200), (3, 80, 80, 160)):
        maps = torch.rand(n, 1, h, w, generator=g) - 0.3
        got = ops.blur_relu_bilinear(maps.to(dev), 7, target).cpu()
        want = osc.upsample(maps, target)
        assert tuple(got.shape) == (n, 1, target, target)
        assert (got - want).abs().max().item() < 2e-6, (h, w, target, (got - want).abs().max().item())


@pytest.mark.parametrize("case", [(1000, 512, 588, 3), (641, 256, 70, 3), (640, 64, 128, 2), (517, 1024, 3, 1), (70000, 512, 300, 3),
                                  (129, 256, 70, 3), (128, 64, 128, 2), (5, 1024, 3, 1)])
def test_knn_fused_equals_the_three_kernel_chain(dev, case):
    """csrc/knn.hip (normalise + similarity GEMM + k smallest in one kernel) == l2norm_rows -> igemm -> knn_mean bit for bit, on
    ragged row / column tiles, and within 1e-6 of the numpy statement of sklearn's brute-force cosine k-NN.  (Up to 512 query rows
    the chain's similarity product runs on csrc/linear_small.hip, whose contraction order differs: 1e-6 there.)"""
    from self_supervised import ops
    from oracle import scoring as osc
    n, d, r, k = case
    g = torch.Generator().manual_seed(sum(case))
    x, bank = torch.randn(n, d, generator=g) * 3, torch.randn(r, d, generator=g)
    bn = ops.l2_normalize_rows(bank.to(dev))
    chain = ops.cosine_knn_mean(ops.linear_fwd(ops.l2_normalize_rows(x.to(dev)), bn), k)
    fused = ops.cosine_knn_fused(x.to(dev), bn, k)
    if n > 512:
        assert torch.equal(fused, chain)
    else:
        assert (fused - chain).abs().max().item() < 1e-6
    if n <= 2000:
        want, _, _ = osc.cosine_knn_mean(bank.numpy(), x.numpy(), k)
        assert np.abs(fused.cpu().numpy() - want).max() < 1e-6


def test_knn_golden(dev, golden):
    from self_supervised.models import AnomalyDetector
    from oracle import weights as ow
    g = golden("detector")
    bank, qs = ow.synthetic_bank(588, 512, seed=2), ow.synthetic_bank(300, 512, seed=3)
    d = AnomalyDetector()
    d.fit_bank(bank)
    got = d.predict(qs).cpu().numpy()
    np.testing.assert_allclose(got, g["kernel_scores"], atol=2e-6)
    np.random.seed(11)
    d2 = AnomalyDetector()
    d2.fit(bank)
    np.testing.assert_allclose(d2.threshold, g["img_threshold"], atol=2e-6)
    np.testing.assert_allclose(d2.predict(qs[:17]).cpu().numpy(), g["img_scores"], atol=2e-6)


def test_scoring_path_golden(dev, golden, seeded_sd):
    """Reference order of tools.inference: bank = embeddings of one good image, split, fit, predict, upsample."""
    from self_supervised.models import AnomalyDetector
    from self_supervised import tools
    from oracle import weights as ow, scoring as osc
    g = golden("detector")
    m = _model(seeded_sd, dev, True)
    with torch.no_grad():
        bank_src = m(ow.synthetic_images(1, 256, seed=4321).to(dev))["latent_space"]
        q = m(ow.synthetic_images(2, 256, seed=2468).to(dev))["latent_space"]
    np.random.seed(7)
    d = AnomalyDetector(patch_level=True, batch=2, num_patches=m.num_patches)
    d.fit(bank_src.cpu())
    assert d.bank.shape[0] == int(g["bank_rows"])
    maps = d.predict(q)
    assert tuple(maps.shape) == (2, 1, 29, 29)
    # north-star bar: 1e-4 absolute.  With seeded random weights the embeddings are nearly parallel (map values 7e-5 ..
    # 1.9e-4), so the bar alone would be weak here: hold the maps to 5e-6 (measured 7e-7 = fp32 cancellation in 1 - cos)
    np.testing.assert_allclose(maps.cpu().numpy(), g["scores"], atol=5e-6)
    np.testing.assert_allclose(d.threshold, g["threshold"], atol=5e-6)
    up = tools.upsample(maps, 256)
    want = osc.upsample(torch.from_numpy(g["scores"]), 256)
    assert_close(up, want, 1e-4)


def test_upsample_golden(dev, golden):
    from self_supervised import tools
    g = golden("upsample")
    maps = torch.from_numpy(g["maps"]).to(dev)
    np.testing.assert_allclose(tools.upsample(maps, 256).cpu().numpy(), g["up256"], atol=2e-6)
    np.testing.assert_allclose(tools.upsample(maps, 64).cpu().numpy(), g["up64"], atol=2e-6)


def test_errors_are_python_exceptions(dev):
    from self_supervised import ops, _hip
    with pytest.raises(_hip.HipExtensionError):
        ops.conv_fwd(torch.zeros(1, 2, 2, 3, device=dev), torch.zeros(8, 1, 1, 3, device=dev))   # Cin % 32
    with pytest.raises(_hip.HipExtensionError):
        ops.conv_fwd(torch.zeros(1, 2, 2, 32), torch.zeros(8, 1, 1, 32))                           # CPU tensors


def test_full_batch_properties(dev, seeded_sd):
    """BASELINE size (256 images x 841 patches, 588-row bank) through size-independent properties: the map of an image
    does not depend on its position in the batch, on the batch size, or on how the trunk passes are chunked."""
    from self_supervised.models import AnomalyDetector
    from self_supervised import tools
    from oracle import weights as ow
    m = _model(seeded_sd, dev, True)
    base = ow.synthetic_images(4, 256, seed=77).to(dev)
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(0))
    big = base.repeat(64, 1, 1, 1)[perm.to(dev)].contiguous()          # 256 images: 64 shuffled copies of 4
    det = AnomalyDetector(patch_level=True, batch=4, num_patches=841)
    det.fit_bank(ow.synthetic_bank(588, 512, seed=2))
    with torch.no_grad():
        small_maps = tools.upsample(det.predict(m(base)["latent_space"]), 256, verbose=False)
        det.batch = 256
        big_maps = tools.upsample(det.predict(m(big)["latent_space"]), 256, verbose=False)
    assert tuple(big_maps.shape) == (256, 1, 256, 256)
    which = (torch.arange(256) % 4)[perm]
    assert torch.equal(big_maps.cpu(), small_maps.cpu()[which])
    assert torch.isfinite(big_maps).all() and float(big_maps.min()) >= 0


# ---------------------------------------------------------------------------------------------
# round 6: layer1 of the patch-scoring pass computed once per image where overlapping patches agree
# ---------------------------------------------------------------------------------------------
def test_ring_conv_and_patch_gather_kernels(dev):
    """ssad_conv_igemm_fwd_hwnc_ring == ssad_conv_igemm_fwd_hwnc on the ring, bit for bit, and leaves the skipped square untouched;
    ssad_patch_gather_hwnc == the indexing it states, exactly (several squares, a non-square patch grid)."""
    from self_supervised import ops
    g = torch.Generator().manual_seed(7)
    n = 300                                                        # ragged last sample group
    x = torch.randn(16, 16, n, 64, generator=g).to(dev)
    res = torch.randn(16, 16, n, 64, generator=g).to(dev)
    w = (torch.randn(64, 3, 3, 64, generator=g) / 24).to(dev)
    sc, sh = (torch.rand(64, generator=g) + 0.5).to(dev), torch.randn(64, generator=g).to(dev)
    full = ops.conv_fwd_hwnc(x, w, sc, sh, res, True, 1, 1)
    for lo, hi in ((3, 13), (4, 12), (6, 10), (0, 15)):
        sentinel = float("nan")
        out = ops.conv_fwd_hwnc_ring(x, w, sc, sh, res, True, lo, hi)
        # (the wrapper allocates: run again into a poisoned buffer to see what is written)
        poisoned = torch.full_like(out, sentinel)
        from self_supervised import _hip
        _hip.check(_hip.lib().ssad_conv_igemm_fwd_hwnc_ring(_hip.ptr(x), _hip.ptr(w), _hip.ptr(poisoned), _hip.ptr(sc), _hip.ptr(sh), _hip.ptr(res),
                                                            1, n, 16, 16, 64, 64, 3, 3, 1, 1, lo, hi, _hip.stream()))
        inside = torch.zeros(16, 16, dtype=torch.bool)
        inside[lo:hi + 1, lo:hi + 1] = True
        assert torch.isnan(poisoned[inside.to(dev)]).all()
        assert torch.equal(poisoned[(~inside).to(dev)], full[(~inside).to(dev)])
        assert torch.equal(out[(~inside).to(dev)], full[(~inside).to(dev)])
    b, prow, pcol, shift = 2, 5, 3, 4
    dense = torch.randn(b, shift * (prow - 1) + 16, shift * (pcol - 1) + 16 + 3, 64, generator=g).to(dev)
    for lo, hi in ((3, 13), (5, 11)):
        out = torch.zeros(16, 16, b * prow * pcol, 64, device=dev)
        ops.patch_gather_hwnc(dense, out, prow, pcol, shift, lo, hi)
        want = torch.zeros_like(out)
        for bi in range(b):
            for pr in range(prow):
                for pc in range(pcol):
                    nn_ = (bi * prow + pr) * pcol + pc
                    want[lo:hi + 1, lo:hi + 1, nn_] = dense[bi, shift * pr + lo:shift * pr + hi + 1, shift * pc + lo:shift * pc + hi + 1]
        assert torch.equal(out, want)
    # the band form: the inner square stays as it was (poisoned), everything else of the copied square as above
    for lo, hi, ilo, ihi in ((3, 13, 5, 11), (4, 12, 6, 10), (5, 11, 7, 9), (2, 14, 8, 8)):
        out = torch.full((16, 16, b * prow * pcol, 64), 7.5, device=dev)
        ops.patch_gather_hwnc(dense, out, prow, pcol, shift, lo, hi, ilo, ihi)
        want = torch.full_like(out, 7.5)
        for bi in range(b):
            for pr in range(prow):
                for pc in range(pcol):
                    nn_ = (bi * prow + pr) * pcol + pc
                    want[lo:hi + 1, lo:hi + 1, nn_] = dense[bi, shift * pr + lo:shift * pr + hi + 1, shift * pc + lo:shift * pc + hi + 1]
        want[ilo:ihi + 1, ilo:ihi + 1] = 7.5
        assert torch.equal(out, want), (lo, hi, ilo, ihi)
    with pytest.raises(RuntimeError):
        ops.patch_gather_hwnc(dense[:, :20], torch.zeros(16, 16, b * prow * pcol, 64, device=dev), prow, pcol, shift, 3, 13)


def test_layer1_dedup_equals_patchwise(dev, seeded_sd, monkeypatch):
    """The patch-scoring trunk with layer1 shared between overlapping patches (engine._trunk_eval_dedup) against the patch-wise trunk
    (SSAD_DEDUP=0) on the same images: 256 x 256 (841 patches, stride 8), a non-square image, and stride 4 through the engine itself.
    Same exact-fp32 products, another summation order inside a position: 2e-6 of the largest value; the reference fixture itself is
    test_forward_golden_patch_level, which runs with the sharing on."""
    from oracle import weights as ow
    from self_supervised import engine
    m = _model(seeded_sd, dev, True)
    xs = [ow.synthetic_images(2, 256, seed=11), ow.synthetic_images(1, 256, seed=12)[:, :, :192, :].contiguous()]
    with torch.no_grad():
        for x in xs:
            monkeypatch.setenv("SSAD_DEDUP", "0")
            ref = m(x.to(dev))
            monkeypatch.setenv("SSAD_DEDUP", "1")
            got = m(x.to(dev))
            for k in ("latent_space", "classifier"):
                scale = ref[k].abs().max().item()
                assert (got[k] - ref[k]).abs().max().item() <= 2e-6 * max(1.0, scale), k
        # stride 4 (extract_patches' own default, functional.py:77): 15 x 15 windows of a 88 x 88 image, pooled shift 2
        plan = m._eval_plan()
        x = ow.synthetic_images(1, 256, seed=13)[:, :, :88, :88].contiguous().to(dev)
        outs = []
        for flag in ("0", "1"):
            monkeypatch.setenv("SSAD_DEDUP", flag)
            pooled = torch.empty((15 * 15, m.concatenator[0].in_features), device=dev)
            engine.trunk_eval(plan, x, 32, 4, m.layer_outputs, pooled)
            outs.append(pooled)
        assert (outs[0] - outs[1]).abs().max().item() <= 2e-6 * max(1.0, outs[0].abs().max().item())
        # small and odd geometries through the engine: eight 64 x 64 images (5 x 5 windows each, dense maps of 32 x 32), a 96 x 64
        # batch, windows that barely overlap (stride 16: pooled shift 8), windows one pooled position apart (stride 2)
        for (bsz, hh, ww, ps) in ((8, 64, 64, 8), (4, 96, 64, 8), (6, 112, 80, 16), (1, 72, 66, 2)):
            xx = ow.synthetic_images(bsz, 256, seed=14 + ps)[:, :, :hh, :ww].contiguous().to(dev)
            npat = ((hh - 32) // ps + 1) * ((ww - 32) // ps + 1)
            assert bsz * npat >= 128
            outs = []
            for flag in ("0", "1"):
                monkeypatch.setenv("SSAD_DEDUP", flag)
                pooled = torch.empty((bsz * npat, m.concatenator[0].in_features), device=dev)
                engine.trunk_eval(plan, xx, 32, ps, m.layer_outputs, pooled)
                outs.append(pooled)
            err = (outs[0] - outs[1]).abs().max().item()
            assert err <= 2e-6 * max(1.0, outs[0].abs().max().item()), (bsz, hh, ww, ps, err)
