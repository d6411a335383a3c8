"""GPU: the device covariance factor of the per-position Gaussian detector -- ssad_position_gaussian_factor (csrc/padim.hip),
ops.position_gaussian_factor, PositionGaussianDetector(factor='device'), tools.inference(detector_options={'factor': 'device'}).

Yardsticks (tests/padim_factor_ref.py): Higham's componentwise bounds with their textbook constants for the fp64 factor -- the
kernel keeps the textbook operation order, one fma chain per element -- and the project's 1e-4 of tests/padim_ref.py for scores.
Statistics come from ops.position_gaussian_fit_stats, the kernel's real input; every output is a view between guard rows."""
import numpy as np
import pytest
import torch

import padim_factor_ref as F
import padim_ref as R
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _stats(n, P, d, seed, D=None, scale=False):
    """(mean [P][d], scatter [P][d][d]) fp64 device tensors of seeded random rows, through the fit-statistics kernel."""
    from self_supervised import ops
    from self_supervised.density import position_channels
    D = D or d
    rows = R.synthetic_rows(n, P, D, seed)
    if scale:
        rows = rows * np.logspace(-3, 3, D).astype(np.float32)
    return ops.position_gaussian_fit_stats(torch.from_numpy(rows).cuda(), position_channels(D, d, seed), n, P)


def _poison(scatter):
    """A copy whose strict upper triangles are NaN: the kernel may read the lower triangle only."""
    s = scatter.clone()
    d = s.shape[-1]
    iu = torch.triu_indices(d, d, 1, device=s.device)
    s[:, iu[0], iu[1]] = NAN
    return s


def _guarded(shape, dtype, fill):
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, device="cuda", dtype=dtype)
    return whole[1:-1], whole


def _same(a, b):
    """Bit equality that also holds for NaN fills."""
    return torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def _call(mean, scatter, n, eps, want64=True):
    """The C entry point over poisoned buffers -> dict of outputs (views), the consumed workspace and the return code; asserts that
    every guard row came back untouched."""
    from self_supervised import _hip
    P, d = mean.shape
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    ws = _poison(scatter)
    bufs = {"mu_hi": _guarded((P, d), f32, NAN), "mu_lo": _guarded((P, d), f32, NAN), "w": _guarded((P, d, d), f32, NAN),
            "info": _guarded((P,), i32, -7)}
    if want64:
        bufs.update({"c64": _guarded((P, d, d), f64, NAN), "w64": _guarded((P, d, d), f64, NAN)})
    before = {k: whole.clone() for k, (_, whole) in bufs.items()}
    ptr = {k: v.data_ptr() for k, (v, _) in bufs.items()}
    rc = _hip.lib().ssad_position_gaussian_factor(mean.data_ptr(), ws.data_ptr(), P, d, n, eps, ptr["mu_hi"], ptr["mu_lo"],
                                                  ptr["w"], ptr.get("c64"), ptr.get("w64"), ptr["info"], _hip.stream())
    torch.cuda.synchronize()
    for k, (_, whole) in bufs.items():
        assert _same(whole[0], before[k][0]) and _same(whole[-1], before[k][-1]), f"guard rows of {k}"
    out = {k: v for k, (v, _) in bufs.items()}
    out["rc"], out["ws"] = rc, ws
    return out


def _check(mean, scatter, n, eps, what):
    """One launch against every bar of this file; returns (outputs, cholesky ratio, inverse ratio)."""
    from self_supervised.density import position_gaussian_factor
    P, d = mean.shape
    o = _call(mean, scatter, n, eps)
    assert o["rc"] == 0
    assert torch.equal(o["info"], torch.zeros_like(o["info"]))
    c64, w64, w = o["c64"].cpu().numpy(), o["w64"].cpu().numpy(), o["w"].cpu().numpy()
    assert np.isfinite(c64).all() and np.isfinite(w64).all(), "a NaN of the upper triangle reached the factor"
    iu = np.triu_indices(d, 1)
    for a in (c64, w64, w):                                                 # exact +0 above the diagonal
        assert not a[:, iu[0], iu[1]].any() and not np.signbit(a[:, iu[0], iu[1]]).any()
    assert np.array_equal(w.view(np.uint32), w64.astype(np.float32).view(np.uint32))       # W rounded once, bit for bit
    # the workspace: W in the lower triangle, the NaN above untouched
    ws = o["ws"].cpu().numpy()
    assert np.array_equal(np.tril(ws), w64) and np.isnan(ws[:, iu[0], iu[1]]).all()
    sigma = F.sigma_from_stats(scatter.cpu().numpy(), n, eps)
    rc = max(F.cholesky_ratio(c64[p], sigma[p]) for p in range(P))
    ri = max(F.inverse_ratio(w64[p], c64[p]) for p in range(P))
    print(f"{what}: |C C^T - Sigma| {rc:.3f} of gamma_(d+1) |C||C|^T, |W - inv(C)| {ri:.3f} of 2 (d+1) u |W||C||W| (bars 1)")
    assert rc <= 1.0 and ri <= 1.0, (rc, ri)
    mu_hi, mu_lo, _ = position_gaussian_factor(mean.cpu().numpy(), scatter.cpu().numpy(), n, eps)      # the host path's pair
    assert np.array_equal(o["mu_hi"].cpu().numpy().view(np.uint32), mu_hi.view(np.uint32))
    assert np.array_equal(o["mu_lo"].cpu().numpy().view(np.uint32), mu_lo.view(np.uint32))
    return o, rc, ri


# d x four n (2, d / 2, d, 2 d: n <= d makes Sigma eps I plus low rank); P walks 1, 3, 5; D > d at 96 and 160 so that the columns are a real selection
CASES = [(d, n, (1, 3, 5)[(i + j) % 3]) for i, d in enumerate((32, 64, 96, 160)) for j, n in enumerate((2, d // 2, d, 2 * d))]
CASES += [(384, n, 2) for n in (2, 192, 384, 768)]


@pytest.mark.parametrize("d,n,P", CASES, ids=[f"d{d}-n{n}-P{P}" for d, n, P in CASES])
def test_factor_meets_the_componentwise_bounds(d, n, P):
    mean, scatter = _stats(n, P, d, seed=d + n + P, D={96: 128, 160: 384}.get(d))
    o, _, _ = _check(mean, scatter, n, 0.01, f"d {d} n {n} P {P}")
    again = _call(mean, scatter, n, 0.01)
    assert all(_same(o[k], again[k]) for k in ("mu_hi", "mu_lo", "w", "info", "c64", "w64"))      # the same bits on a second call


def test_columns_scaled_over_six_decades():
    mean, scatter = _stats(192, 3, 96, seed=5, scale=True)
    _check(mean, scatter, 192, 0.01, "columns 1e-3..1e3")


def test_small_regulariser():
    for n in (48, 300):                 # rank-deficient scatter + 1e-6 I, and a full-rank one
        mean, scatter = _stats(n, 3, 160, seed=n)
        _check(mean, scatter, n, 1e-6, f"eps 1e-6, n {n}")


def test_a_position_does_not_depend_on_the_launch():
    """Position p of a P = 5 launch is the same bits as that matrix launched alone, with and without the fp64 copies."""
    for d in (96, 160):
        mean, scatter = _stats(d, 5, d, seed=d)
        full = _call(mean, scatter, d, 0.01)
        lean = _call(mean, scatter, d, 0.01, want64=False)
        assert all(_same(full[k], lean[k]) for k in ("mu_hi", "mu_lo", "w", "info"))
        for p in range(5):
            one = _call(mean[p:p + 1].contiguous(), scatter[p:p + 1].contiguous(), d, 0.01)
            assert all(_same(one[k][0], full[k][p]) for k in ("mu_hi", "mu_lo", "w", "info", "c64", "w64")), (d, p)


def test_the_op_returns_the_kernels_bits_and_consumes_scatter():
    from self_supervised import ops
    mean, scatter = _stats(64, 3, 96, seed=1)
    want = _call(mean, scatter, 64, 0.01)
    ws = _poison(scatter)
    mu_hi, mu_lo, w, c64, w64 = ops.position_gaussian_factor(mean, ws, 64, 0.01, want64=True)
    assert all(_same(a, want[k]) for a, k in ((mu_hi, "mu_hi"), (mu_lo, "mu_lo"), (w, "w"), (c64, "c64"), (w64, "w64")))
    assert _same(ws, want["ws"])                                    # consumed: W in the lower triangle
    three = ops.position_gaussian_factor(mean, _poison(scatter), 64, 0.01)
    assert len(three) == 3 and _same(three[2], w)
    assert w.dtype == torch.float32 and c64.dtype == torch.float64 and w.is_cuda


@pytest.mark.parametrize("base,col,value", [(-1.0, 0, None), (1.0, 0, NAN), (1.0, 40, -1.0), (1.0, 63, float("inf"))],
                         ids=["minus-identity", "nan-pivot-0", "negative-pivot-40", "inf-pivot-63"])
def test_a_bad_pivot_is_a_status(base, col, value):
    """One position of three holds a handcrafted scatter (Sigma = base I, one diagonal entry replaced) whose pivot `col` is the first
    that is not finite and positive: info = 1 + col there and 0 elsewhere, its w is NaN, the other positions are the bits of a launch
    without it, and the op raises naming the position."""
    from self_supervised import ops
    d, n, eps = 64, 64, 0.01
    mean, scatter = _stats(n, 3, d, seed=11)
    good = _call(mean, scatter, n, eps)
    bad = scatter.clone()
    bad[1] = torch.diag(torch.full((d,), (base - eps) * (n - 1), dtype=torch.float64))        # Sigma = scatter / (n - 1) + eps I
    if value is not None:
        bad[1, col, col] = (value - eps) * (n - 1)
    o = _call(mean, bad, n, eps)
    assert o["rc"] == 0
    assert o["info"].tolist() == [0, col + 1, 0]
    assert torch.isnan(o["w"][1]).all() and torch.isnan(o["c64"][1]).all() and torch.isnan(o["w64"][1]).all()
    for k in ("mu_hi", "mu_lo"):
        assert _same(o[k], good[k])
    for k in ("w", "c64", "w64"):
        assert _same(o[k][0], good[k][0]) and _same(o[k][2], good[k][2]), k
    with pytest.raises(ValueError, match=rf"position 1 .*pivot {col} "):
        ops.position_gaussian_factor(mean, _poison(bad), n, eps)


def test_bad_arguments_launch_nothing():
    from self_supervised import _hip
    lib = _hip.lib()
    P, d = 2, 64
    f32, f64 = torch.float32, torch.float64
    mean = torch.zeros(P, d, device="cuda", dtype=f64)
    sc = torch.full((P, d, d), NAN, device="cuda", dtype=f64)
    mu_hi, mu_lo = (torch.full((P, d), NAN, device="cuda", dtype=f32) for _ in range(2))
    w = torch.full((P, d, d), NAN, device="cuda", dtype=f32)
    c64, w64 = (torch.full((P, d, d), NAN, device="cuda", dtype=f64) for _ in range(2))
    info = torch.full((P,), -7, device="cuda", dtype=torch.int32)
    ok = dict(mean=mean.data_ptr(), scatter=sc.data_ptr(), P=P, d=d, n=5, eps=0.01, mu_hi=mu_hi.data_ptr(), mu_lo=mu_lo.data_ptr(),
              w=w.data_ptr(), c_out=c64.data_ptr(), w64_out=w64.data_ptr(), info=info.data_ptr())
    bad = {"d = 48": {"d": 48}, "d = 0": {"d": 0}, "d = 16": {"d": 16}, "d = 544": {"d": 544}, "n = 1": {"n": 1}, "eps = 0": {"eps": 0.0},
           "eps < 0": {"eps": -1.0}, "eps nan": {"eps": NAN}, "P = 0": {"P": 0}, "null w": {"w": None}, "null mean": {"mean": None},
           "null scatter": {"scatter": None}, "null mu_hi": {"mu_hi": None}, "null mu_lo": {"mu_lo": None}, "null info": {"info": None}}
    for what, change in bad.items():
        assert lib.ssad_position_gaussian_factor(*{**ok, **change}.values(), _hip.stream()) == 2, what
        assert b"ssad_position_gaussian_factor" in lib.ssad_last_error(), what
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (sc, mu_hi, mu_lo, w, c64, w64)) and (info == -7).all()


# --------------------------------------------------------------------------------------------- detector against the reference

def _planted(P, D, n_q):
    """tests/test_hip_padim.py's planted-anomaly queries: 30 rows shifted at known (image, position)."""
    q = R.synthetic_rows(n_q, P, D, seed=21, draw=3).reshape(n_q, P, D)
    labels = np.zeros((n_q, P))
    rng = np.random.RandomState(4)
    for n, p in zip(rng.randint(0, n_q, 30), rng.randint(0, P, 30)):
        q[n, p] += rng.randn(D).astype(np.float32) * 1.5
        labels[n, p] = 1
    return q.reshape(n_q * P, D), labels.reshape(-1)


def test_device_factor_detector_matches_the_reference():
    from sklearn.metrics import roc_auc_score
    from self_supervised.density import PositionGaussianDetector
    from self_supervised.models import split_rows
    P, D, d, n_all, n_q = 9, 64, 32, 96, 40
    emb = torch.from_numpy(R.synthetic_rows(n_all, P, D, seed=21))
    q, labels = _planted(P, D, n_q)
    dets = {}
    for factor in ('device', 'host'):
        np.random.seed(7)
        dets[factor] = PositionGaussianDetector(batch=n_q, num_patches=P, channels=d, factor=factor)
        dets[factor].fit(emb)
    np.random.seed(7)
    tr, va = split_rows(n_all * P, torch.arange(n_all).repeat_interleave(P))
    det = dets['device']
    sel = det.sel.numpy()
    mean, _, vi = R.fit(emb.numpy()[tr], sel, P, eps=0.01)
    maps = det.predict(torch.from_numpy(q))
    got = maps.reshape(-1).cpu().double().numpy()
    want = R.scores(q, sel, P, mean, vi)
    want_thr = R.scores(emb.numpy()[va], sel, P, mean, vi).max()
    rel = (np.abs(got - want) / want).max()
    host = dets['host'].predict(torch.from_numpy(q)).reshape(-1).cpu().double().numpy()
    print(f"factor='device': scores {rel:.2e}, threshold {abs(det.threshold - want_thr) / want_thr:.2e} of the reference (bars 1e-4); "
          f"{(np.abs(got - host) / host).max():.2e} from factor='host'")
    assert rel <= 1e-4
    assert abs(det.threshold - want_thr) <= 1e-4 * want_thr
    auc_got, auc_want = roc_auc_score(labels, got), roc_auc_score(labels, want)
    assert abs(auc_got - auc_want) <= 1e-4 * auc_want and auc_want > 0.9, (auc_got, auc_want)
    assert torch.equal(det.mu_hi, dets['host'].mu_hi) and torch.equal(det.mu_lo, dets['host'].mu_lo)
    assert det.w.is_cuda and not torch.triu(det.w, 1).any()
    # the broadcast state keeps the option and the scores
    det2 = PositionGaussianDetector.from_state(det.state(), batch=n_q, num_patches=P)
    assert det2.factor == 'device' and torch.equal(det2.predict(torch.from_numpy(q)), maps)


# ------------------------------------------------------------------------------------------------------ through tools.inference

SIZE, P96, N_TRAIN, CHANNELS = 96, 144, 48, 32          # the 48 / 4-image 96 x 96 category of tests/test_hip_padim.py


def _datamodule(root, **kw):
    from self_supervised.datasets import MVTecDatamodule
    return MVTecDatamodule(root, imsize=(SIZE, SIZE), **kw)


@pytest.fixture()
def tree(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import datasets, tools
    datasets._DataModule.num_workers = 0
    monkeypatch.setattr(tools, "MVTecDatamodule", _datamodule)
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=SIZE)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


def _run(tools, ck, root, **opts):
    np.random.seed(3)
    return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, localization='dense',
                           bank='train', detector='padim', image_scores='max', detector_options={"channels": CHANNELS, **opts})


def test_device_factor_through_inference(tree, monkeypatch):
    from self_supervised import tools
    from self_supervised.density import PositionGaussianDetector
    from self_supervised.models import split_rows
    root, ck = tree
    host0 = _run(tools, ck, root, factor='host')
    seen = {}
    orig = PositionGaussianDetector.fit

    def spy(self, embeddings, split=True, groups=None):
        seen.update(rows=torch.as_tensor(embeddings).detach().cpu().clone(), groups=torch.as_tensor(groups).clone(),
                    rng=np.random.get_state(), detector=self)
        orig(self, embeddings, split, groups)
    monkeypatch.setattr(PositionGaussianDetector, "fit", spy)
    res = _run(tools, ck, root, factor='device')
    monkeypatch.setattr(PositionGaussianDetector, "fit", orig)
    assert seen["detector"].factor == 'device'
    maps = res.anomaly_maps
    assert tuple(maps.shape) == (4, 1, 12, 12) and torch.isfinite(maps).all()
    rows = seen["rows"].numpy()
    np.random.set_state(seen["rng"])
    tr, va = split_rows(rows.shape[0], seen["groups"])
    sel = seen["detector"].sel.numpy()
    mean, _, vi = R.fit(rows[tr], sel, P96, eps=0.01)
    want = R.scores(res.embedding_vectors.float().numpy(), sel, P96, mean, vi)
    got = maps.reshape(-1).double().numpy()
    err = (np.abs(got - want) / want).max()
    want_thr = R.scores(rows[va], sel, P96, mean, vi).max()
    host = host0.anomaly_maps.reshape(-1).double().numpy()
    print(f"factor='device' maps: {err:.2e} of the float64 reference (bar 1e-4), {(np.abs(got - host) / host).max():.2e} from "
          f"factor='host'")
    assert err <= 1e-4
    assert abs(seen["detector"].threshold - want_thr) <= 1e-4 * want_thr
    assert torch.equal(res.image_scores, maps.reshape(4, P96).max(dim=1).values)
    # the host path is where it was: the default, and factor='host' before and after a device fit
    host1 = _run(tools, ck, root, factor='host')
    default = _run(tools, ck, root)
    assert torch.equal(host1.anomaly_maps, host0.anomaly_maps) and torch.equal(host1.image_scores, host0.image_scores)
    assert torch.equal(default.anomaly_maps, host0.anomaly_maps)
