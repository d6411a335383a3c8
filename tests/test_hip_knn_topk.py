"""GPU tests of the flat Euclidean search for k = 4..32 (csrc/knn_topk.hip: ssad_l2_knn_topk / _index, ssad_l2h_knn_topk / _index),
of ops.l2_topk_* / l2h_topk_* and of n_neighbors through AnomalyDetector and tools.inference.  References: the float64 brute force
of tests/knn_l2_ref.py (on the rounded rows for the half kernels: tests/knn_l2_half_ref.py); HIP paths are compared with each
other only where bit-equality between them is the claim (the k <= 3 kernels' prefix, splits, batches, the mean form).

The bar on a squared distance is the project's: TAU = 64 units of 2^-24 A for fp32 operands, A from scale_a at the
returned row; for fp16 operands the bar tests/test_hip_knn_l2_half.py applies to the rounded rows, min(16, D + 8) units of 2^-24 A~."""
import numpy as np
import pytest
import torch

import knn_l2_half_ref as href
import knn_l2_ref as ref
import knn_topk_ref as tref
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NAN = float("nan")
TAU = 64.0
KS = (4, 5, 8, 9, 16, 17, 32)
GAUSS_SHAPES = ((300, 1000, 64, 32), (200, 700, 96, 16), (130, 300, 32, 9))      # (N, R, D, k)


def tau_half(d):
    return min(16.0, d + 8.0)


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


class Side:
    """One operand type: the ops, the k <= 3 ops, the float64 module and the bar."""

    def __init__(self, half):
        from self_supervised import ops
        self.half = half
        self.mod = href if half else ref
        self.index, self.mean = (ops.l2h_topk_index, ops.l2h_topk_mean) if half else (ops.l2_topk_index, ops.l2_topk_mean)
        self.index3 = ops.l2h_knn_index if half else ops.l2_knn_index

    def tau(self, d):
        return tau_half(d) if self.half else TAU

    def bank(self, rows):
        """(bank as the ops take it, its squared norms) on the device"""
        from self_supervised import ops
        rows = rows.cuda()
        return ops.rows_to_half(rows) if self.half else (rows, ops.row_sqnorms(rows))


@pytest.fixture(scope="module", params=[False, True], ids=["fp32", "fp16"])
def side(request):
    return Side(request.param)


@pytest.fixture(scope="module")
def gauss_cases():
    """The Gaussian shapes with their float64 squared distances and scales, computed once per operand type."""
    cache = {}

    def get(i, half):
        if (i, half) not in cache:
            n, r, d, k = GAUSS_SHAPES[i]
            x, bank = gauss(n, d, 11 + i), gauss(r, d, 21 + i)
            mod = href if half else ref
            cache[(i, half)] = (x, bank, mod.d2_64(x, bank), mod.scale_a(x, bank))
        return cache[(i, half)]
    return get


# ---------------------------------------------------------------- 1. exact, with massive ties; 5. the mean form

@pytest.mark.parametrize("k", KS)
def test_exact_on_integer_rows_with_ties(side, k):
    for d in (32, 64):
        for r in sorted({k, k + 1, 127, 128, 129, 300}):
            if r < k:
                continue
            xs, bank_h = tref.integer_rows(300, r, d, seed=1000 * k + r + d)
            bank, bsq = side.bank(bank_h)
            for n in (1, 130, 300):
                x = xs[:n]
                d2_all = ref.d2_64(x, bank_h)               # exact integers: rounding to fp16 changes nothing
                want_d2, want_i = ref.smallest_stable(d2_all, k)
                dist, idx = side.index(x.cuda(), bank, bsq, k)
                out = side.mean(x.cuda(), bank, bsq, k)
                dist, idx, out = dist.cpu(), idx.cpu(), out.cpu()
                assert idx.dtype == torch.int32 and np.array_equal(idx.numpy().astype(np.int64), want_i), (d, r, n)
                root = np.sqrt(want_d2)
                assert (np.abs(dist.double().numpy() - root) <= 2 * EPS * root).all(), (d, r, n)          # 1 ulp <= 2^-23 relative
                if n > 1 and r >= 127:
                    assert (want_d2[:, 0] == 0).sum() >= 2 and (want_d2[:, 1:] == want_d2[:, :-1]).any()      # the ties are there
                # the mean form: the index form's row summed one after the other in fp32, those bits; and against float64
                assert torch.equal(tref.sequential_mean(dist, k), out), (d, r, n)
                mean_ref = side.mod.patch_scores64(x, bank_h, k)
                assert (np.abs(out.double().numpy() - mean_ref) <= (k + 3) * 2 * EPS * mean_ref).all(), (d, r, n)


# ---------------------------------------------------------------- 2. against float64 on Gaussian rows

@pytest.mark.parametrize("case", range(len(GAUSS_SHAPES)))
def test_gaussian_rows_against_float64(side, gauss_cases, case):
    n, r, d, k = GAUSS_SHAPES[case]
    x, bank_h, d2_all, a_all = gauss_cases(case, side.half)
    bank, bsq = side.bank(bank_h)
    dist, idx = side.index(x.cuda(), bank, bsq, k)
    tref.check_topk_against_float64(dist.cpu(), idx.cpu(), k, d2_all, a_all, side.tau(d), max_loose=0.03)
    out = side.mean(x.cuda(), bank, bsq, k).cpu()
    assert torch.equal(tref.sequential_mean(dist, k), out)
    want = side.mod.patch_scores64(x, bank_h, k)
    assert (np.abs(out.double().numpy() - want) <= tref.scores_tol(x, bank_h, k, side.tau(d), side.mod)).all()


# ---------------------------------------------------------------- 3. the prefix is the k <= 3 kernels'

@pytest.mark.parametrize("k", [4, 9, 32])
@pytest.mark.parametrize("case", range(len(GAUSS_SHAPES)))
def test_prefix_is_the_three_nearest_kernel(side, gauss_cases, case, k):
    x, bank_h = gauss_cases(case, side.half)[:2]
    bank, bsq = side.bank(bank_h)
    x = x.cuda()
    dist, idx = side.index(x, bank, bsq, k)
    d3, i3 = side.index3(x, bank, bsq, 3)
    d1, i1 = side.index3(x, bank, bsq, 1)
    assert torch.equal(dist[:, :3], d3) and torch.equal(idx[:, :3], i3)
    assert torch.equal(dist[:, :1], d1) and torch.equal(idx[:, :1], i1)


# ---------------------------------------------------------------- 4. split and batch invariance, bit for bit

@pytest.mark.parametrize("k", [4, 9, 32])
def test_same_bits_for_every_split_batch_and_call(side, k):
    xs, bank_h = gauss(300, 64, 31), gauss(300, 64, 32)
    bank_h[40] = bank_h[7]
    bank_h[299] = bank_h[7]                                   # equal keys but for the row, in different splits
    bank, bsq = side.bank(bank_h)
    x = xs.cuda()
    dist, idx = side.index(x, bank, bsq, k, splits=1)
    out = side.mean(x, bank, bsq, k, splits=1)
    for s in (1, 2, 4, 7):                                     # rows_per = 384, 256, 128, 128: splits short of k rows, and empty ones
        d2, i2 = side.index(x, bank, bsq, k, splits=s)
        assert torch.equal(d2, dist) and torch.equal(i2, idx), s
        assert torch.equal(side.mean(x, bank, bsq, k, splits=s), out), s
        for n in (1, 130):
            dn, inn = side.index(x[:n].contiguous(), bank, bsq, k, splits=s)
            assert torch.equal(dn, dist[:n]) and torch.equal(inn, idx[:n]), (s, n)
            assert torch.equal(side.mean(x[:n].contiguous(), bank, bsq, k, splits=s), out[:n]), (s, n)
        one = x[177:178].contiguous()
        d1, i1 = side.index(one, bank, bsq, k, splits=s)
        assert torch.equal(d1, dist[177:178]) and torch.equal(i1, idx[177:178]), s


# ---------------------------------------------------------------- 6. guards and argument errors

def guarded_out(shape, dtype=torch.float32):
    """(whole buffer, view): an output between two guard rows; floats are NaN-filled, ints hold -7."""
    fill = NAN if dtype == torch.float32 else -7
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
    return buf, buf[1:-1]


def guards_intact(buf):
    g = torch.stack([buf[0].reshape(-1), buf[-1].reshape(-1)])
    return bool(torch.isnan(g).all()) if buf.dtype == torch.float32 else bool((g == -7).all())


def raw_call(half, index, x, xsq, bank, bsq, part, outs, n, d, r, k, s):
    from self_supervised import _hip
    L = _hip.lib()
    st = _hip.stream()
    P = lambda t: None if t is None else t.data_ptr()
    name = "ssad_l2h_knn_topk" if half else "ssad_l2_knn_topk"
    fn = getattr(L, name + ("_index" if index else ""))
    head = (P(x), P(xsq), P(bank), P(bsq)) if half else (P(x), P(bank), P(bsq))
    return fn(*head, P(part), *[P(o) for o in outs], n, d, r, k, s, st)


@pytest.mark.parametrize("k", [4, 16, 32])
def test_outputs_and_workspace_between_poisoned_margins(side, k):
    from self_supervised import ops
    n, r, d = 130, 300, 64
    xs, bank_h = gauss(n, d, 41), gauss(r, d, 42)
    bank, bsq = side.bank(bank_h)
    x, xsq = ops.rows_to_half(xs.cuda()) if side.half else (xs.cuda(), None)
    want_d, want_i = side.index(xs.cuda(), bank, bsq, k, splits=1)
    want_o = side.mean(xs.cuda(), bank, bsq, k, splits=1)
    for s in (1, 4):
        dbuf, dist = guarded_out((n, k))
        ibuf, idx = guarded_out((n, k), torch.int32)
        obuf, out = guarded_out((n,))
        pbuf, part = guarded_out((s, n, k), torch.int64)
        assert raw_call(side.half, True, x, xsq, bank, bsq, part, (dist, idx), n, d, r, k, s) == 0
        assert raw_call(side.half, False, x, xsq, bank, bsq, part, (out,), n, d, r, k, s) == 0
        torch.cuda.synchronize()
        assert guards_intact(dbuf) and guards_intact(ibuf) and guards_intact(obuf) and guards_intact(pbuf)
        assert torch.isfinite(dist).all() and torch.isfinite(out).all() and (idx >= 0).all() and (idx < r).all()
        assert torch.equal(dist, want_d) and torch.equal(idx, want_i) and torch.equal(out, want_o)
        if s > 1:
            assert (part != -7).all()                       # every workspace entry is written (NOKEY where a split is short)
        else:
            assert (part == -7).all()                       # and none without splits


def test_argument_errors_leave_the_outputs_untouched():
    from self_supervised import _hip, ops
    L = _hip.lib()
    n, d, r = 5, 64, 40
    xs, bank_h = gauss(n, d, 1).cuda(), gauss(r, d, 2).cuda()
    out = torch.full((n,), NAN, device="cuda")
    dist = torch.full((n, 32), NAN, device="cuda")
    idx = torch.full((n, 32), -7, dtype=torch.int32, device="cuda")
    part = torch.full((2, n, 32), -7, dtype=torch.int64, device="cuda")
    for half in (False, True):
        bank, bsq = ops.rows_to_half(bank_h) if half else (bank_h, ops.row_sqnorms(bank_h))
        x, xsq = ops.rows_to_half(xs) if half else (xs, None)
        good = dict(x=x, xsq=xsq, bank=bank, bsq=bsq, part=part, n=n, d=d, r=r, k=8, s=2)
        bad = [dict(x=None), dict(bank=None), dict(bsq=None), dict(d=48), dict(d=65536 + 32), dict(k=0), dict(k=3), dict(k=33),
               dict(r=7), dict(s=0), dict(part=None)]
        if half:
            bad.append(dict(xsq=None))
        for change in bad:
            a = dict(good, **change)
            for index, outs in ((True, (dist, idx)), (False, (out,))):
                rc = raw_call(half, index, a["x"], a["xsq"], a["bank"], a["bsq"], a["part"], outs, a["n"], a["d"], a["r"], a["k"], a["s"])
                assert rc == 2, (half, change, index)
        assert raw_call(half, True, x, xsq, bank, bsq, part, (None, idx), n, d, r, 8, 2) == 2
        assert raw_call(half, True, x, xsq, bank, bsq, part, (dist, None), n, d, r, 8, 2) == 2
        assert raw_call(half, False, x, xsq, bank, bsq, part, (None,), n, d, r, 8, 2) == 2
        assert raw_call(half, True, x, xsq, bank, bsq, part, (dist, idx), n, d, 7, 8, 1) == 2 and b"k in 4..32" in L.ssad_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(dist).all() and (idx == -7).all() and (part == -7).all()


# ---------------------------------------------------------------- 7. the detector

def _fit_split(n, seed):
    np.random.seed(seed)
    perm = np.random.permutation(n)
    cut = int(n * 0.3)
    return perm[cut:], perm[:cut]


@pytest.mark.parametrize("patch_level", [False, True], ids=["image", "patch"])
@pytest.mark.parametrize("bank_dtype", ["float32", "float16"])
@pytest.mark.parametrize("k", [1, 5, 9])
def test_detector_scores_and_threshold_against_float64(k, bank_dtype, patch_level):
    from self_supervised.models import AnomalyDetector
    half = bank_dtype == 'float16'
    mod, t = (href, tau_half(64)) if half else (ref, TAU)
    emb = gauss(900, 64, seed=3) * 0.5 + gauss(1, 64, seed=4)
    kw = dict(patch_level=True, batch=8, num_patches=25) if patch_level else {}
    np.random.seed(5)
    det = AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype, n_neighbors=k, **kw)
    det.fit(emb)
    assert det.k == k and det.n_neighbors == k
    tr, va = _fit_split(900, 5)
    rows = emb[tr]
    x = gauss(200, 64, seed=9) * 0.5 + gauss(1, 64, seed=4)
    got = det.predict(x)
    assert tuple(got.shape) == ((8, 1, 5, 5) if patch_level else (200,))
    got = got.reshape(-1).cpu().double().numpy()
    assert (np.abs(got - mod.patch_scores64(x, rows, k)) <= tref.scores_tol(x, rows, k, t, mod)).all()
    thr = mod.patch_scores64(emb[va], rows, k)
    assert abs(det.threshold - thr.max()) <= tref.scores_tol(emb[va], rows, k, t, mod).max()
    dist, idx = det.kneighbors(x)
    assert tuple(dist.shape) == (200, k) and idx.dtype == torch.int64
    assert torch.equal(tref.sequential_mean(dist, k), det.predict(x).reshape(-1).cpu())


@pytest.mark.parametrize("bank_dtype", ["float32", "float16"])
def test_detector_kneighbors_16_and_image_scores(bank_dtype):
    from self_supervised.models import AnomalyDetector
    half = bank_dtype == 'float16'
    mod, t = (href, tau_half(64)) if half else (ref, TAU)
    bank = gauss(700, 64, seed=13)
    x = gauss(8 * 25, 64, seed=14)
    det = AnomalyDetector(patch_level=True, batch=8, num_patches=25, metric='euclidean', bank_dtype=bank_dtype, n_neighbors=5)
    det.fit_bank(bank)
    dist, idx = det.kneighbors(x, 16)
    tref.check_topk_against_float64(dist.cpu(), idx.cpu().int(), 16, mod.d2_64(x, bank), mod.scale_a(x, bank), t)
    d3, i3 = det.kneighbors(x, 3)
    assert torch.equal(dist[:, :3], d3) and torch.equal(idx[:, :3], i3)
    s = det.image_scores(x, 'max').cpu().double().numpy()
    want = mod.patch_scores64(x, bank, 5).reshape(8, 25)
    tol = tref.scores_tol(x, bank, 5, t, mod).reshape(8, 25).max(1)
    assert (np.abs(s - want.max(1)) <= tol).all()
    if not half:                    # 'reweighted' keeps its own `neighbours` and route, on the k-mean s_max
        w = det.image_scores(x, 'reweighted', neighbours=4)
        assert tuple(w.shape) == (8,) and torch.isfinite(w).all() and (w.cpu() <= det.image_scores(x, 'max').cpu()).all()
    with pytest.raises(ValueError, match="fewer than k"):
        AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype, n_neighbors=9).fit(gauss(8, 64, 1), split=False)


def _detectors(**kw):
    from self_supervised.models import AnomalyDetector
    return AnomalyDetector(**kw), AnomalyDetector(n_neighbors=3, **kw)


@pytest.mark.parametrize("path", ["cosine", "cosine_unfused", "euclidean", "fp16", "gallery", "ivf"])
def test_default_is_n_neighbors_3_on_every_path(path):
    d = 48 if path == "cosine_unfused" else 64
    kw = {"cosine": {}, "cosine_unfused": {}, "euclidean": dict(metric='euclidean'),
          "fp16": dict(metric='euclidean', bank_dtype='float16'),
          "gallery": dict(metric='euclidean', gallery=2, patch_level=True, batch=4, num_patches=25),
          "ivf": dict(metric='euclidean', index='ivf', nlist=4, nprobe=2)}[path]
    emb = gauss(20 * 25, d, seed=6) + gauss(1, d, seed=7)
    x = gauss(4 * 25, d, seed=8) + gauss(1, d, seed=7)
    a, b = _detectors(**kw)
    for det in (a, b):
        np.random.seed(2)
        det.fit(emb, split=False)
        assert det.k == 3
    assert a.threshold == b.threshold and torch.equal(a.predict(x), b.predict(x))
    assert a.state().keys() == b.state().keys() and "n_neighbors" not in a.state()
    if d % 32 == 0:
        for k in (None, 1, 2):
            da, ia = a.kneighbors(x, k)
            db, ib = b.kneighbors(x, k)
            assert torch.equal(da, db) and torch.equal(ia, ib)


@pytest.mark.parametrize("path", ["cosine", "cosine_unfused", "euclidean", "fp16", "gallery", "ivf"])
@pytest.mark.parametrize("k", [1, 2])
def test_small_n_neighbors_run_on_every_path(path, k):
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector
    d = 48 if path == "cosine_unfused" else 64
    kw = {"cosine": {}, "cosine_unfused": {}, "euclidean": dict(metric='euclidean'),
          "fp16": dict(metric='euclidean', bank_dtype='float16'),
          "gallery": dict(metric='euclidean', gallery=20, patch_level=True, batch=4, num_patches=25),
          "ivf": dict(metric='euclidean', index='ivf', nlist=4, nprobe=4)}[path]
    emb = gauss(20 * 25, d, seed=6) + gauss(1, d, seed=7)
    x = gauss(4 * 25, d, seed=8) + gauss(1, d, seed=7)
    det = AnomalyDetector(n_neighbors=k, **kw)
    np.random.seed(2)
    det.fit(emb, split=False)
    assert det.k == k
    got = det.predict(x).reshape(-1).cpu().double().numpy()
    if path.startswith("cosine"):
        e64, x64 = emb.double().numpy(), x.double().numpy()
        e64 /= np.linalg.norm(e64, axis=1, keepdims=True)
        x64 /= np.linalg.norm(x64, axis=1, keepdims=True)
        want = np.sort(np.clip(1.0 - x64 @ e64.T, 0, 2), axis=1)[:, :k].mean(1)
        assert np.abs(got - want).max() <= 1e-5
    else:                           # the gallery holds every bank image and every cell is probed: the exact search
        mod, t = (href, tau_half(64)) if path == "fp16" else (ref, TAU)
        assert (np.abs(got - mod.patch_scores64(x, emb, k)) <= tref.scores_tol(x, emb, k, t, mod)).all()
    assert det.threshold == det._scores(det._dev(emb)).max().item()         # the threshold goes through the same k


def test_state_round_trip_and_mismatch():
    from self_supervised.models import AnomalyDetector
    emb, x = gauss(300, 64, seed=6), gauss(50, 64, seed=8)
    det = AnomalyDetector(metric='euclidean', n_neighbors=7)
    det.fit(emb, split=False)
    st = det.state()
    assert st["n_neighbors"] == 7
    other = AnomalyDetector(metric='euclidean', n_neighbors=7)
    other.load_state(st)
    assert torch.equal(other.predict(x), det.predict(x))
    with pytest.raises(ValueError, match="n_neighbors=7"):
        AnomalyDetector(metric='euclidean').load_state(st)
    with pytest.raises(ValueError, match="n_neighbors=3"):
        AnomalyDetector(metric='euclidean', n_neighbors=7).load_state({"metric": 'euclidean', "bank": emb})
    plain = AnomalyDetector(metric='euclidean')
    plain.load_state({"metric": 'euclidean', "bank": emb})                   # a state written before the option
    three = AnomalyDetector(metric='euclidean', n_neighbors=3)
    three.fit_bank(emb)
    assert torch.equal(plain.predict(x), three.predict(x))


# ---------------------------------------------------------------- 8. through tools.inference

def test_inference_with_one_neighbour(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import datasets, tools
    from self_supervised.models import AnomalyDetector
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=8, n_test_good=2, n_test_bad=2, size=96)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    seen = {}
    orig = AnomalyDetector.fit

    def spy(self, embeddings, split=True, groups=None):
        orig(self, embeddings, split, groups)
        seen["det"] = self
    monkeypatch.setattr(AnomalyDetector, "fit", spy)

    def run(**more):
        np.random.seed(3)
        torch.manual_seed(3)
        return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                               metric='euclidean', **more)

    default = run()
    three = run(n_neighbors=3)
    assert torch.equal(default.anomaly_maps, three.anomaly_maps) and torch.equal(default.embedding_vectors, three.embedding_vectors)
    res = run(n_neighbors=1)
    det = seen["det"]
    assert det.k == 1 and det.n_neighbors == 1
    rows = res.embedding_vectors.float()
    assert torch.equal(res.anomaly_maps.reshape(-1).cpu(), det.predict(rows).reshape(-1).cpu())       # the detector's bits
    want = ref.patch_scores64(rows, det.bank.cpu(), 1)
    tol = tref.scores_tol(rows, det.bank.cpu(), 1, TAU)
    assert (np.abs(res.anomaly_maps.reshape(-1).double().numpy() - want) <= tol).all()
    assert not torch.equal(res.anomaly_maps, default.anomaly_maps)
    five = run(n_neighbors=5)
    assert seen["det"].k == 5
    want5 = ref.patch_scores64(rows, seen["det"].bank.cpu(), 5)
    assert (np.abs(five.anomaly_maps.reshape(-1).double().numpy() - want5) <= tref.scores_tol(rows, seen["det"].bank.cpu(), 5, TAU)).all()
