"""GPU tests of the Euclidean metric of the kNN detector: csrc/knn_l2.hip (ssad_row_sqnorms, ssad_l2_knn_fused / _index,
ssad_l2_from_dots, ssad_knn_reweight_l2) and its way through AnomalyDetector(metric='euclidean'), tools.inference and
tools.sweep.  The reference everywhere is the float64 numpy brute force of tests/knn_l2_ref.py on the same fp32 inputs; two HIP
paths are compared with each other only where bit-equality between them is the claim.

The bar.  For a (query, bank row) pair A = |q|^2 + |b|^2 + 2 sum |q_i| |b_i|; a squared distance is held to
|d2 - d2_ref| <= tau 2^-24 A, a returned distance through its square plus one rounding of the root (2^-23 d2_ref).  tau is not a
guess: the worst ratio |d^2 - d2_ref| / (2^-24 A) over every shape of this file, root rounding included, was measured on an MI355X
against float64 (the tests print it per case): 3.05 / 2.49 / 2.76 for N(0, 1) rows at D = 32 / 64 / 384, 2.63 against 20 000 bank
rows, 3.10 and 9.77 for N(10, 1) rows at D = 32 and 384, 6.10 and 9.30 for queries that copy a bank row (N(0, 1) and N(10, 1),
D = 384).  tau is 4 x the worst of them, 39.1, rounded up to a power of two -- the data are one seed of one distribution -- and never above the
a-priori bound D + 8: tau(D) = min(64, D + 8)."""
import os

import numpy as np
import pytest
import torch

import coreset_ref
import knn_l2_ref as ref
import two_rank_util
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TAU_MEASURED = 64.0    # worst ratio measured on an MI355X: 9.77 (see above); 4 x 9.77 = 39.1 -> 64
REW_TAU = 8.0          # 'reweighted': worst |score - float64| / (2^-24 s_max max(1, dmax)) measured 1.47 (b = 9; 1.31 for b = 2 and 32),
                       # worst |w - float64| / (2^-24 max(1, dmax)) with the data x 100: 0.20; 4 x 1.47 = 5.9 -> 8


def tau(d):
    return min(TAU_MEASURED, d + 8.0)
NAN = float("nan")
N_TRAIN = 8


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


def guarded(t, fill=NAN):
    """A device copy of t as a view between two guard rows of `fill`: a read outside the view shows as a NaN in the result."""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    buf[1:-1] = t
    buf = buf.cuda()
    return buf, buf[1:-1]


def guarded_out(shape, dtype=torch.float32):
    """(whole buffer, view): an output between two guard rows; floats are NaN-filled, ints hold -7."""
    fill = NAN if dtype == torch.float32 else -7
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
    return buf, buf[1:-1]


def guards_intact(buf):
    g = torch.stack([buf[0].reshape(-1), buf[-1].reshape(-1)])
    return bool(torch.isnan(g).all()) if buf.dtype == torch.float32 else bool((g == -7).all())


def raw_knn(x, bank, bsq, k, splits=None, index=False):
    """The C entry points on caller-owned, guarded outputs.  splits None: one launch without a workspace; S: S splits with one.  Returns
    the output views (out,) or (dist, idx) after checking the guard rows."""
    from self_supervised import _hip
    L = _hip.lib()
    n, d = x.shape
    r = bank.shape[0]
    st = _hip.stream()
    s = splits or 1
    ws = None if splits is None else torch.empty((s, n, 3), dtype=torch.int64 if index else torch.float32, device="cuda")
    part = None if ws is None else ws.data_ptr()
    if index:
        dbuf, dist = guarded_out((n, k))
        ibuf, idx = guarded_out((n, k), torch.int32)
        rc = L.ssad_l2_knn_index(x.data_ptr(), bank.data_ptr(), bsq.data_ptr(), part, dist.data_ptr(), idx.data_ptr(), n, d, r, k, s, st)
        assert rc == 0, L.ssad_last_error()
        torch.cuda.synchronize()
        assert guards_intact(dbuf) and guards_intact(ibuf)
        return dist, idx
    obuf, out = guarded_out((n,))
    rc = L.ssad_l2_knn_fused(x.data_ptr(), bank.data_ptr(), bsq.data_ptr(), part, out.data_ptr(), n, d, r, k, s, st)
    assert rc == 0, L.ssad_last_error()
    torch.cuda.synchronize()
    assert guards_intact(obuf)
    return (out,)


def _mean_of(dist, k):
    """(d0 [+ d1] [+ d2]) / k, added smallest first, in IEEE fp32 on the host -- the kernels' epilogue."""
    d = dist.cpu().numpy()
    s = d[:, 0].copy()
    for j in range(1, k):
        s = s + d[:, j]
    assert s.dtype == np.float32
    return torch.from_numpy(s / np.float32(k))


def check_against_float64(x, bank, dist, idx, out, k, d2_all, a_all, strict_indices=True):
    """dist / idx [N][k] of the index form and out [N] of the mean form (host tensors) against float64.  Returns (worst ratio of
    the squared-distance error to 2^-24 A, share of (query, j) cases outside the strict index comparison).  strict_indices=False
    leaves out the index-for-index comparison (3) and its 2 % cap; the valid-pick check (2) holds every index either way."""
    n, r = d2_all.shape
    t = tau(x.shape[1])
    want_d2, want_i = ref.smallest_stable(d2_all, min(k + 1, r))
    dist64, idx = dist.double().numpy(), idx.numpy().astype(np.int64)
    assert np.isfinite(dist64).all() and (dist64 >= 0).all()
    assert idx.min() >= 0 and idx.max() < r
    assert all(len(set(row)) == k for row in idx)
    # (1) the returned distance against the float64 distance of the returned row, through its square
    d2_row = np.take_along_axis(d2_all, idx, 1)
    a_row = np.take_along_axis(a_all, idx, 1)
    err = np.abs(dist64 ** 2 - d2_row)
    ratio = float((err / (EPS * a_row)).max())
    print(f"   worst |d^2 - d2_ref| / (2^-24 A) = {ratio:.3f}")
    assert (err <= t * EPS * a_row + 2 * EPS * d2_row).all(), ratio
    # (2) the returned row is a valid j-th pick: its float64 d2 against the float64 j-th smallest (a swap needs both errors)
    a_ref = np.take_along_axis(a_all, want_i[:, :k], 1)
    bar2 = 2 * t * EPS * np.maximum(a_row, a_ref)
    assert (np.abs(d2_row - want_d2[:, :k]) <= bar2).all()
    # (3) indices equal wherever the float64 gaps to both neighbours in the order exceed twice the bar
    strict = np.ones((n, k), dtype=bool)
    for j in range(k):
        if j > 0:
            strict[:, j] &= want_d2[:, j] - want_d2[:, j - 1] > bar2[:, j]
        if j + 1 < want_d2.shape[1]:
            strict[:, j] &= want_d2[:, j + 1] - want_d2[:, j] > bar2[:, j]
    loose = 1.0 - strict.mean()
    if strict_indices:
        assert loose <= 0.02, loose                                 # on the reference alone
        assert np.array_equal(idx[strict], want_i[:, :k][strict])
    # (4) the mean form: the index form's distances averaged, bit for bit -- and against float64 directly
    assert torch.equal(_mean_of(dist, k), out), "mean form differs from the averaged index distances"
    dref = np.sqrt(want_d2[:, :k])
    e = bar2 + 2 * EPS * want_d2[:, :k]
    tol_d = np.minimum(np.sqrt(e), e / np.maximum(dref, 1e-300))
    mean_ref = dref.mean(1)
    assert (np.abs(out.double().numpy() - mean_ref) <= tol_d.mean(1) + 4 * EPS * mean_ref).all()
    return ratio, loose


# ---------------------------------------------------------------- 1. row norms

@pytest.mark.parametrize("d", [32, 64, 384, 100])
def test_row_sqnorms(d):
    from self_supervised import ops
    rows = gauss(300, d, seed=d)
    rows[17] = rows[3]
    rows[299] = rows[3]
    rows[130] = rows[3]
    buf, x = guarded(rows)
    got = ops.row_sqnorms(x).cpu()
    want = ref.sqnorms64(rows)
    err = np.abs(got.double().numpy() - want) / (EPS * want)
    print(f"D={d}: worst |sum x^2 - float64| / (2^-24 sum x^2) = {err.max():.3f} (bound D + 2 = {d + 2})")
    assert err.max() <= d + 2
    bits = got.view(torch.int32)
    assert bits[17] == bits[3] and bits[299] == bits[3] and bits[130] == bits[3]
    for i in (3, 130, 299):
        assert torch.equal(ops.row_sqnorms(x[i:i + 1]).cpu().view(torch.int32)[0], bits[3])


# ---------------------------------------------------------------- 2. values and indices against float64

NS = (1, 127, 128, 129, 300)
RS = (3, 127, 128, 129, 257)


@pytest.mark.parametrize("d,mean", [(32, 0.0), (64, 0.0), (384, 0.0), (32, 10.0), (384, 10.0)],
                         ids=["D32", "D64", "D384", "D32-mean10", "D384-mean10"])
def test_values_and_indices_match_float64(d, mean):
    """Every N x R x k of the issue.  N(10, 1) rows are where cancellation is at its worst: A is ~100 x that of N(0, 1) rows while
    the gaps between neighbours stay, so the bar covers most gaps and an index-for-index comparison says little.  Computed on the
    CPU from the float64 reference alone, at tau(D): the share of (query, j) cases outside the strict comparison is at most 0.8 %
    for N(0, 1) rows at every shape; for N(10, 1) rows it is at most 0.8 % at D = 32, R = 3 and 1.8 % at D = 384, R = 3,
    N = 300, and between 2.6 % and 22 % at the larger banks.  So N(10, 1) rows get the strict comparison at those shapes, and
    values, valid picks and the mean form's bits at all of them."""
    from self_supervised import ops
    worst, worst_loose = 0.0, 0.0
    xs = {n: gauss(n, d, seed=1000 + d + n, mean=mean) for n in NS}
    for r in RS:
        bank_h = gauss(r, d, seed=2000 + d + r, mean=mean)
        bbuf, bank = guarded(bank_h)
        bsq = ops.row_sqnorms(bank)
        for n in NS:
            xbuf, x = guarded(xs[n])
            d2_all, a_all = ref.d2_64(xs[n], bank_h), ref.scale_a(xs[n], bank_h)
            for k in (1, 2, 3):
                print(f"D={d} mean={mean} N={n} R={r} k={k}")
                dist, idx = raw_knn(x, bank, bsq, k, index=True)
                (out,) = raw_knn(x, bank, bsq, k)
                strict = mean == 0.0 or (r == 3 and (d == 32 or n == 300))
                ratio, loose = check_against_float64(xs[n], bank_h, dist.cpu(), idx.cpu(), out.cpu(), k, d2_all, a_all, strict)
                worst, worst_loose = max(worst, ratio), max(worst_loose, loose)
    print(f"D={d} mean={mean}: worst ratio {worst:.3f}, largest share outside the strict index comparison {worst_loose:.2e}")


@pytest.mark.parametrize("d", [32, 384])
def test_split_forms_on_a_large_bank(d):
    from self_supervised import ops
    r, n = 20000, 129
    x_h, bank_h = gauss(n, d, seed=7 + d), gauss(r, d, seed=8 + d)
    xbuf, x = guarded(x_h)
    bbuf, bank = guarded(bank_h)
    bsq = ops.row_sqnorms(bank)
    assert ops.knn_splits(n, r) > 1
    d2_all, a_all = ref.d2_64(x_h, bank_h), ref.scale_a(x_h, bank_h)
    for k in (1, 2, 3):
        print(f"D={d} N={n} R={r} k={k}")
        d1, i1 = raw_knn(x, bank, bsq, k, index=True)
        (o1,) = raw_knn(x, bank, bsq, k)
        check_against_float64(x_h, bank_h, d1.cpu(), i1.cpu(), o1.cpu(), k, d2_all, a_all)
        for s in (1, 2, 4, 7, 16, 157, 200):                       # 157 = one bank tile per split; 200: splits past the bank's end
            ds, is_ = raw_knn(x, bank, bsq, k, splits=s, index=True)
            (os_,) = raw_knn(x, bank, bsq, k, splits=s)
            assert torch.equal(d1, ds) and torch.equal(i1, is_) and torch.equal(o1, os_), (k, s)
        # the dispatch of the wrappers (ops.knn_splits, S > 1 here) and SSAD_KNN_SPLIT=0
        dw, iw = ops.l2_knn_index(x, bank, bsq, k)
        assert torch.equal(dw, d1) and torch.equal(iw, i1) and torch.equal(ops.l2_knn_fused(x, bank, bsq, k), o1)


# ---------------------------------------------------------------- 3. bit equality across grids and calls

def tied_bank(u, d, seed):
    """A bank in which each of u distinct rows appears 2-5 times at scattered positions: (rows [R][d], orig [R])."""
    rng = np.random.RandomState(seed)
    orig = np.repeat(np.arange(u), rng.randint(2, 6, size=u))
    rng.shuffle(orig)
    return gauss(u, d, seed=seed + 1)[torch.from_numpy(orig)], orig


def test_same_bits_for_every_split_single_rows_and_calls(monkeypatch):
    from self_supervised import ops
    raw, _ = tied_bank(2600, 64, seed=5)
    bank = raw.cuda()
    bsq = ops.row_sqnorms(bank)
    x = torch.cat([gauss(172, 64, seed=11), 2.0 * raw[:128]]).cuda()          # 300 rows: two whole query tiles and a ragged one
    for k in (1, 2, 3):
        d1, i1 = ops.l2_knn_index(x, bank, bsq, k, splits=1)
        o1 = ops.l2_knn_fused(x, bank, bsq, k, splits=1)
        assert torch.equal(_mean_of(d1, k), o1.cpu())
        for s in range(2, 17):
            ds, is_ = ops.l2_knn_index(x, bank, bsq, k, splits=s)
            assert torch.equal(d1, ds) and torch.equal(i1, is_), (k, s)
            assert torch.equal(o1, ops.l2_knn_fused(x, bank, bsq, k, splits=s)), (k, s)
        again = ops.l2_knn_index(x, bank, bsq, k, splits=1)
        assert torch.equal(d1, again[0]) and torch.equal(i1, again[1])
        assert torch.equal(o1, ops.l2_knn_fused(x, bank, bsq, k))
        for i in (0, 150, 299):
            for s in (1, 4):
                do, io = ops.l2_knn_index(x[i:i + 1], bank, bsq, k, splits=s)
                assert torch.equal(do[0], d1[i]) and torch.equal(io[0], i1[i]), (k, i, s)
                assert torch.equal(ops.l2_knn_fused(x[i:i + 1], bank, bsq, k, splits=s)[0], o1[i])
    monkeypatch.setenv("SSAD_KNN_SPLIT", "0")
    assert ops.knn_splits(300, 20000) == 1


# ---------------------------------------------------------------- 4. duplicates

@pytest.mark.parametrize("u,splits", [(300, None), (300, 3), (2600, 5)])
def test_duplicated_bank_rows(u, splits):
    from self_supervised import ops
    d = 64
    raw, orig = tied_bank(u, d, seed=5)
    r = raw.shape[0]
    distinct = gauss(u, d, seed=6)
    bank = raw.cuda()
    bsq = ops.row_sqnorms(bank)
    x = gauss(200, d, seed=7)
    d64 = ref.d2_64(x, distinct)[:, orig]                           # copies carry one float64 value, as they carry one fp32 value
    a64 = ref.scale_a(x, distinct)[:, orig]
    order = np.argsort(d64, axis=1, kind="stable")
    first = np.take_along_axis(d64, order[:, :1], 1)[:, 0]
    d_other = np.where(orig[None, :] == orig[order[:, 0]][:, None], np.inf, d64)
    clear = d_other.min(1) - first > 4 * tau(d) * EPS * a64.max(1)     # the nearest distinct row leads the second distinct row
    assert clear.mean() > 0.9
    for k in (1, 2, 3):
        dist, idx = ops.l2_knn_index(x.cuda(), bank, bsq, k, splits=splits)
        bits = dist.cpu().view(torch.int32).numpy()
        idx = idx.cpu().numpy().astype(np.int64)
        for q in range(x.shape[0]):
            assert len(set(idx[q])) == k
            for a in range(k):
                for b in range(a + 1, k):
                    if orig[idx[q, a]] == orig[idx[q, b]]:          # identical rows: identical distance bits, smaller row first
                        assert bits[q, a] == bits[q, b] and idx[q, a] < idx[q, b]
            if clear[q]:
                c = min(k, int((orig == orig[order[q, 0]]).sum()))
                assert np.array_equal(idx[q, :c], np.flatnonzero(orig == orig[order[q, 0]])[:c]), (q, idx[q])


@pytest.mark.parametrize("mean", [0.0, 10.0])
def test_queries_that_duplicate_bank_rows(mean):
    """Exact copies of bank rows and copies plus 1e-3 noise: the cancellation case of the expanded form.  Finite, >= 0, within the
    bar -- the clamp comes before the root."""
    from self_supervised import ops
    d, r = 384, 257
    bank_h = gauss(r, d, seed=3, mean=mean)
    pick = torch.from_numpy(np.random.RandomState(1).randint(0, r, size=150))
    x_h = torch.cat([bank_h[pick], bank_h[pick] + 1e-3 * gauss(150, d, seed=4)])
    xbuf, x = guarded(x_h)
    bbuf, bank = guarded(bank_h)
    bsq = ops.row_sqnorms(bank)
    d2_all, a_all = ref.d2_64(x_h, bank_h), ref.scale_a(x_h, bank_h)
    for k in (1, 3):
        dist, idx = raw_knn(x, bank, bsq, k, index=True)
        (out,) = raw_knn(x, bank, bsq, k)
        dist, idx, out = dist.cpu(), idx.cpu(), out.cpu()
        assert torch.isfinite(dist).all() and (dist >= 0).all() and torch.isfinite(out).all() and (out >= 0).all()
        d2_row = np.take_along_axis(d2_all, idx.numpy().astype(np.int64), 1)
        a_row = np.take_along_axis(a_all, idx.numpy().astype(np.int64), 1)
        err = np.abs(dist.double().numpy() ** 2 - d2_row)
        print(f"mean={mean} k={k}: worst |d^2 - d2_ref| / (2^-24 A) = {(err / (EPS * a_row)).max():.3f}; "
              f"largest first distance of an exact copy {dist[:150, 0].max():.3e}")
        assert (err <= tau(d) * EPS * a_row + 2 * EPS * d2_row).all()
        assert torch.equal(_mean_of(dist, k), out)


# ---------------------------------------------------------------- 5. argument errors

def test_argument_errors_leave_the_outputs_untouched():
    from self_supervised import _hip, ops
    L = _hip.lib()
    st = _hip.stream()
    x, bank = gauss(5, 64, 1).cuda(), gauss(4, 64, 2).cuda()
    bsq = ops.row_sqnorms(bank)
    out = torch.full((5,), NAN, device="cuda")
    dist = torch.full((5, 3), NAN, device="cuda")
    idx = torch.full((5, 3), -7, dtype=torch.int32, device="cuda")
    partf = torch.full((2, 5, 3), NAN, device="cuda")
    partk = torch.full((2, 5, 3), -7, dtype=torch.int64, device="cuda")
    P = lambda t: t.data_ptr()
    bad = [  # (x, bank, bsq, out / dist, idx, D, R, k)
        (None, P(bank), P(bsq), 64, 4, 3), (P(x), None, P(bsq), 64, 4, 3), (P(x), P(bank), None, 64, 4, 3),
        (P(x), P(bank), P(bsq), 48, 4, 3), (P(x), P(bank), P(bsq), 65536 + 32, 4, 3), (P(x), P(bank), P(bsq), 64, 4, 0),
        (P(x), P(bank), P(bsq), 64, 4, 4), (P(x), P(bank), P(bsq), 64, 2, 3)]
    for xa, ba, sa, d, r, k in bad:
        assert L.ssad_l2_knn_fused(xa, ba, sa, None, P(out), 5, d, r, k, 1, st) == 2
        assert L.ssad_l2_knn_fused(xa, ba, sa, P(partf), P(out), 5, d, r, k, 2, st) == 2
        assert L.ssad_l2_knn_index(xa, ba, sa, None, P(dist), P(idx), 5, d, r, k, 1, st) == 2
        assert L.ssad_l2_knn_index(xa, ba, sa, P(partk), P(dist), P(idx), 5, d, r, k, 2, st) == 2
    good = (P(x), P(bank), P(bsq))
    assert L.ssad_l2_knn_fused(*good, None, None, 5, 64, 4, 3, 1, st) == 2
    assert L.ssad_l2_knn_index(*good, None, P(dist), None, 5, 64, 4, 3, 1, st) == 2
    assert L.ssad_l2_knn_fused(*good, None, P(out), 5, 64, 4, 3, 2, st) == 2
    assert L.ssad_l2_knn_index(*good, None, P(dist), P(idx), 5, 64, 4, 3, 2, st) == 2
    assert L.ssad_l2_knn_fused(*good, P(partf), P(out), 5, 64, 4, 3, 0, st) == 2
    assert L.ssad_l2_knn_index(*good, P(partk), P(dist), P(idx), 5, 64, 4, 3, 0, st) == 2
    assert L.ssad_l2_knn_index(*good, P(partk) + 4, P(dist), P(idx), 5, 64, 4, 3, 2, st) == 2 and b"8-byte" in L.ssad_last_error()
    assert L.ssad_row_sqnorms(None, P(out), 5, 64, st) == 2 and L.ssad_row_sqnorms(P(x), None, 5, 64, st) == 2
    assert L.ssad_l2_knn_index(*good, None, P(dist), P(idx), 5, 64, 2, 3, 1, st) == 2 and b"k in 1..3" in L.ssad_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(dist).all() and (idx == -7).all()
    assert torch.isnan(partf).all() and (partk == -7).all()
    # S = 1 needs no workspace: a null part is accepted and gives the bits of the run with one
    out2, dist2, idx2 = out.clone(), dist.clone(), idx.clone()
    assert L.ssad_l2_knn_fused(*good, None, P(out), 5, 64, 4, 3, 1, st) == 0
    assert L.ssad_l2_knn_fused(*good, P(partf), P(out2), 5, 64, 4, 3, 1, st) == 0
    assert L.ssad_l2_knn_index(*good, None, P(dist), P(idx), 5, 64, 4, 3, 1, st) == 0
    assert L.ssad_l2_knn_index(*good, P(partk), P(dist2), P(idx2), 5, 64, 4, 3, 1, st) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and (idx >= 0).all()
    assert torch.equal(out, out2) and torch.equal(dist, dist2) and torch.equal(idx, idx2)
    with pytest.raises(ValueError, match="fewer than k"):
        ops.l2_knn_index(x, bank[:2], bsq[:2], 3)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.l2_knn_fused(x[:, :48].contiguous(), bank[:, :48].contiguous(), bsq, 3)


# ---------------------------------------------------------------- 6. image scores on embeddings with structure

def structured_embeddings(seed=0, noise=1.0, d=32, scale=1.0):
    """tests/test_hip_knn_index.py's construction at D = 32: bank = 40 random unit centres x 50 copies, each with Gaussian noise of
    norm about `noise`; 60 images of 841 patches drawn the same way, every second one with 5 patches replaced by N(0, 1) rows.
    Everything times `scale`."""
    p, n_img = 841, 60
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn((40, d), generator=g)
    centres = centres / centres.norm(dim=1, keepdim=True)
    sigma = noise / np.sqrt(d)
    bank = centres.repeat_interleave(50, 0) + sigma * torch.randn((2000, d), generator=g)
    which = torch.randint(0, 40, (n_img * p,), generator=g)
    x = centres[which] + sigma * torch.randn((n_img * p, d), generator=g)
    labels = np.zeros(n_img, dtype=np.int64)
    for i in range(1, n_img, 2):
        at = torch.randperm(p, generator=g)[:5] + i * p
        x[at] = torch.randn((5, d), generator=g)
        labels[i] = 1
    return (scale * bank).contiguous(), (scale * x).contiguous(), labels, p


@pytest.fixture(scope="module")
def structured():
    bank, x, labels, p = structured_embeddings()
    return bank, x, labels, p, {b: ref.image_scores64(x, bank, p, neighbours=b) for b in (2, 9, 32)}


def test_image_scores_on_structured_embeddings(structured):
    from self_supervised import metrics as mtr, ops
    from self_supervised.models import AnomalyDetector
    bank, x, labels, p, want_b = structured
    det = AnomalyDetector(patch_level=True, batch=60, num_patches=p, metric='euclidean')
    det.fit_bank(bank)
    maps = det.predict(x)
    got = det.image_scores(x, 'max')
    assert got.shape == (60,) and got.dtype == torch.float32
    assert torch.equal(got, maps.reshape(60, p).max(1).values)                      # 'max' is the row maximum, bit for bit
    base = want_b[2]
    _, flat = ops.rows_argmax(maps.reshape(60, p))
    assert np.array_equal(flat.cpu().numpy() - np.arange(60) * p, base["p_star"])
    labels_t = torch.from_numpy(labels)
    for b in (2, 9, 32):
        want = want_b[b]
        print(f"b={b}: images left out of the 'reweighted' comparison {int(want['fragile'].sum())} of 60")
        assert want["fragile"].mean() <= 0.05                                       # on the reference alone, first
        auc64 = ref.auroc64(labels, want["score"])
        assert auc64 >= 0.9, auc64
        got = det.image_scores(x, 'reweighted', b).cpu()
        assert torch.isfinite(got).all()
        keep = ~want["fragile"]
        dmax = np.sqrt(np.take_along_axis(ref.d2_64(x[np.arange(60) * p + want["p_star"]], bank), want["nbr"], 1)).max(1)
        unit = EPS * want["s_max"] * np.maximum(1.0, dmax)
        ratio = (np.abs(got.double().numpy() - want["score"]) / unit)[keep].max()
        print(f"b={b}: worst |score - float64| / (2^-24 s_max max(1, dmax)) = {ratio:.3f}, float64 AUROC {auc64:.4f}")
        assert ratio <= REW_TAU, ratio
        auc = mtr.auroc_gpu(labels_t.cuda(), got.cuda())
        assert abs(auc - auc64) <= 1e-4, (auc, auc64)
        assert torch.equal(got, det.image_scores(x, 'reweighted', b, scores=maps.reshape(-1)).cpu())
    auc_max = mtr.auroc_gpu(labels_t.cuda(), det.image_scores(x, 'max'))
    assert abs(auc_max - ref.auroc64(labels, base["s_max"])) <= 1e-4


def test_reweighting_survives_distances_in_the_hundreds():
    """The data times 100: the planted images' distances are in the hundreds, where exp(d) overflows fp32 (above 88) and the
    unshifted weight is inf / inf.  The shifted form keeps every weight finite and inside [0, 1).  (Noise 0.1 here: at 1.0 x 100 the
    neighbour distances of a planted patch differ by more than 40, and 1 - exp(-40) is 1 in float64 already; at 0.1 the float64
    weights end 4e-5 below 1 -- computed on the CPU, b = 32 -- far above fp32's 6e-8.)"""
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector
    bank, x, labels, p = structured_embeddings(scale=100.0, noise=0.1)
    det = AnomalyDetector(patch_level=True, batch=60, num_patches=p, metric='euclidean')
    det.fit_bank(bank)
    maps = det.predict(x)
    smax, flat = ops.rows_argmax(maps.reshape(60, p))
    assert int((smax > 88.0).sum()) == 30                              # every planted image
    xs = x.cuda().index_select(0, flat)
    _, mstar = ops.l2_knn_index(xs, det.bank, det.bank_sq, 1)
    rows = mstar.reshape(-1).long()
    d2 = ops.l2_from_dots(ops.linear_fwd(det.bank.index_select(0, rows), det.bank), det.bank_sq.index_select(0, rows), det.bank_sq)
    for b in (2, 9, 32):
        _, nbr = ops.rows_smallest_index(d2, b)
        w = ops.knn_reweight_l2(xs, det.bank, mstar, nbr, torch.ones_like(smax)).cpu()
        print(f"b={b}: weights in [{float(w.min()):.6f}, {float(w.max()):.6f}]")
        assert torch.isfinite(w).all() and (w >= 0).all() and (w < 1).all()
        score = det.image_scores(x, 'reweighted', b, scores=maps.reshape(-1)).cpu()
        assert torch.isfinite(score).all()
        want = ref.image_scores64(x, bank, p, neighbours=b)
        keep = ~want["fragile"]
        assert (want["w"] < 1.0 - 1e-5).all()
        dmax = np.sqrt(np.take_along_axis(ref.d2_64(x[np.arange(60) * p + want["p_star"]], bank), want["nbr"], 1)).max(1)
        ratio = (np.abs(w.double().numpy() - want["w"]) / (EPS * np.maximum(1.0, dmax)))[keep].max()
        print(f"b={b}: worst |w - float64| / (2^-24 max(1, dmax)) = {ratio:.3f} over {int(keep.sum())} images")
        assert ratio <= REW_TAU, ratio


def test_l2_from_dots_is_the_kernel_expression():
    from self_supervised import ops
    sim, qsq, bsq = gauss(7, 5000, 1), gauss(7, 1, 2).abs().reshape(-1) * 50, gauss(5000, 1, 3).abs().reshape(-1) * 50
    got = ops.l2_from_dots(sim.cuda(), qsq.cuda(), bsq.cuda()).cpu()
    want = np.maximum((qsq.numpy()[:, None] + bsq.numpy()[None, :]) - np.float32(2) * sim.numpy(), np.float32(0))
    assert want.dtype == np.float32 and np.array_equal(got.numpy(), want) and (got >= 0).all()


# ---------------------------------------------------------------- 7. the detector

def _brute_maps(rows, bank):
    return ref.patch_scores64(rows, bank, 3)


def _maps_tol(rows, bank):
    """Per-row bound on |score - float64| from the bar: the score is a mean of three roots of squared distances held to
    2 tau 2^-24 A (the selection may swap rows within the bar), |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b))."""
    d2, idx = ref.kneighbors64(rows, bank, 3)
    a = np.concatenate([np.take_along_axis(ref.scale_a(rows[i:i + 512], bank), idx[i:i + 512], 1) for i in range(0, rows.shape[0], 512)])
    e = 2 * tau(rows.shape[1]) * EPS * a + 2 * EPS * d2
    dref = np.sqrt(d2)
    return np.minimum(np.sqrt(e), e / np.maximum(dref, 1e-300)).mean(1) + 4 * EPS * dref.mean(1)


@pytest.mark.parametrize("coreset", [None, 0.25])
def test_detector_against_float64(coreset):
    from self_supervised.models import AnomalyDetector, coreset_projection
    emb = gauss(900, 64, seed=3) * 0.5 + gauss(1, 64, seed=4)
    np.random.seed(5)
    det = AnomalyDetector(coreset=coreset, coreset_dim=32, metric='euclidean')
    det.fit(emb)
    np.random.seed(5)
    perm = np.random.permutation(900)
    tr, va = perm[270:], perm[:270]
    rows = emb[tr]
    if coreset is not None:
        proj = (rows.cuda() @ coreset_projection(64, 32).cuda()).cpu()              # close to the kernel's GEMM; compared below
        sel, rad = det.coreset_rows
        m = int(np.ceil(0.25 * 630))
        assert det.coreset_counts == (m, 630) and sel.shape[0] == m
        want_sel, _ = coreset_ref.greedy64(proj.double().numpy(), m)
        assert np.array_equal(sel.cpu().numpy(), want_sel)                          # coreset_rows index the rows after the split
        rows = rows[sel.cpu()]
    assert torch.equal(det.bank.cpu(), rows) and det.bank_sq.shape == (rows.shape[0],)
    from self_supervised import ops
    assert torch.equal(det.bank_sq, ops.row_sqnorms(det.bank))
    x = gauss(200, 64, seed=9) * 0.5 + gauss(1, 64, seed=4)
    got = det.predict(x).cpu().double().numpy()
    assert (np.abs(got - _brute_maps(x, rows)) <= _maps_tol(x, rows)).all()
    thr = _brute_maps(emb[va], rows)
    assert abs(det.threshold - thr.max()) <= _maps_tol(emb[va], rows).max()
    dist, idx = det.kneighbors(x)
    want_d2, want_i = ref.kneighbors64(x, rows, 3)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want_i)   # (Gaussian picks: gaps far above the bar)
    assert np.abs(dist.cpu().double().numpy() - np.sqrt(want_d2)).max() <= _maps_tol(x, rows).max()
    assert torch.equal(_mean_of(dist, 3), det.predict(x).cpu())
    with pytest.raises(ValueError, match="multiple of 32"):
        AnomalyDetector(metric='euclidean').fit_bank(gauss(10, 48, 0))
    with pytest.raises(ValueError, match="metric must be one of"):
        AnomalyDetector(metric='l2')


# ---------------------------------------------------------------- 8. through tools.inference

def _tree(tmp_path, seeded_sd):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=96)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


CASES = {"patches": {}, "dense": {"localization": "dense"}, "train": {"bank": "train"}, "coreset": {"bank": "train", "coreset": 0.1},
         "reweighted": {"bank": "train", "image_scores": "reweighted", "neighbours": 5}, "unstreamed": {"bank": "train"}}


def _standalone_rows(ck, root, dense):
    """model(x) of every training image in file order, outside tools.inference: [images][P][D]."""
    from self_supervised.datasets import MVTecDatamodule
    from self_supervised.models import PeraNet
    model = PeraNet.load_from_checkpoint(ck).eval()
    if dense:
        model.enable_dense_mode()
    else:
        model.enable_patch_level_mode()
    model.enable_mvtec_inference()
    model.cuda()
    dm = MVTecDatamodule(root + "bottle/", batch_size=1)
    dm.setup()
    ds = dm.test_dataset
    ds.images_filenames = list(dm.train_images_filenames)
    x = torch.stack([ds[i][0] for i in range(len(ds))]).cuda()
    with torch.no_grad():
        rows = model(x)['latent_space'].cpu()
    return rows.reshape(len(ds), -1, rows.shape[1])


@pytest.mark.parametrize("case", list(CASES))
def test_inference_euclidean(tmp_path, seeded_sd, monkeypatch, case):
    from self_supervised import ops, tools
    from self_supervised.models import AnomalyDetector
    root, ck = _tree(tmp_path, seeded_sd)
    kw = CASES[case]
    seen = {}
    orig = AnomalyDetector.fit

    def spy(self, embeddings, split=True, groups=None):
        seen["fit_rows"] = torch.as_tensor(embeddings).detach().cpu().clone()
        orig(self, embeddings, split, groups)
        seen["det"] = self
    monkeypatch.setattr(AnomalyDetector, "fit", spy)

    def run(**more):
        np.random.seed(3)
        torch.manual_seed(3)
        return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, **kw, **more)

    before = run()
    before_kw = run(metric='cosine')
    assert seen["det"].metric == 'cosine' and seen["det"].bank_sq is None
    res = run(metric='euclidean')
    det, fit_rows = seen["det"], seen["fit_rows"]
    assert det.metric == 'euclidean'
    if case == "unstreamed":                                        # the streamed predict off: the same rows and maps
        monkeypatch.setenv("SSAD_FAST_PREDICT", "0")
        res0 = run(metric='euclidean')
        monkeypatch.delenv("SSAD_FAST_PREDICT")
        assert torch.equal(seen["fit_rows"], fit_rows) and torch.equal(res0.anomaly_maps, res.anomaly_maps)
        assert torch.equal(seen["det"].bank, det.bank) and seen["det"].threshold == det.threshold
    # the fit rows are the model's rows, bit for bit: every training image (bank='train') or the one drawn image
    outside = _standalone_rows(ck, root, dense=kw.get("localization") == "dense")
    if kw.get("bank") == "train":
        assert torch.equal(fit_rows, outside.reshape(-1, outside.shape[2]))
    else:
        assert any(torch.equal(fit_rows, o) for o in outside)
    # maps within the bar of the brute force on the fitted bank
    bank = det.bank.cpu()
    rows = res.embedding_vectors.float()
    assert rows.shape[1] % 32 == 0 and torch.equal(det.bank_sq.cpu(), ops.row_sqnorms(det.bank).cpu())
    maps = res.anomaly_maps
    got = maps.reshape(-1).double().numpy()
    want, tol = _brute_maps(rows, bank), _maps_tol(rows, bank)
    print(f"{case}: max |map - float64| = {np.abs(got - want).max():.3e} (values ~ {want.max():.3e}, bound ~ {tol.max():.3e})")
    assert (np.abs(got - want) <= tol).all()
    assert maps.shape == before.anomaly_maps.shape and maps.dtype == before.anomaly_maps.dtype
    assert not torch.equal(maps, before.anomaly_maps)
    if case == "coreset":
        assert det.coreset_counts[0] == int(np.ceil(0.1 * det.coreset_counts[1])) == bank.shape[0]
    if case == "reweighted":
        p = rows.shape[0] // 4
        w64 = ref.image_scores64(rows, bank, p, neighbours=5)
        s = res.image_scores
        assert s.dtype == torch.float32 and tuple(s.shape) == (4,) and torch.isfinite(s).all()
        keep = ~w64["fragile"]
        dmax = np.sqrt(np.take_along_axis(ref.d2_64(rows[np.arange(4) * p + w64["p_star"]], bank), w64["nbr"], 1)).max(1)
        bound = REW_TAU * EPS * w64["s_max"] * np.maximum(1.0, dmax) + tol.max()
        assert (np.abs(s.double().numpy() - w64["score"])[keep] <= bound[keep]).all()
    # on through upsample and the Evaluator
    res.anomaly_maps = tools.upsample(maps, int(res.ground_truths.shape[-1]), verbose=False)
    assert tuple(res.anomaly_maps.shape[-2:]) == tuple(res.ground_truths.shape[-2:])
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou'])
    ev.evaluate(res, "bottle", str(tmp_path / "out") + "/", patch_level=True)
    assert ev.scores.auroc is not None and np.isfinite(ev.scores.auroc)
    # the cosine call, with and without the argument, before and after a Euclidean call: the same bits
    for other in (before_kw, run(), run(metric='cosine')):
        assert torch.equal(before.anomaly_maps, other.anomaly_maps)
        assert torch.equal(before.embedding_vectors, other.embedding_vectors)
        if before.image_scores is not None:
            assert torch.equal(before.image_scores, other.image_scores)


def test_sweep_euclidean_writes_its_tables(tmp_path):
    from self_supervised import tools, datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), n_train=8, n_test_good=2, n_test_bad=2, size=96)
    out = str(tmp_path / "l2") + "/"
    np.random.seed(0)
    df = tools.sweep(root, out, ["bottle"], imsize=(64, 64), batch_size=4, seed=0, projection_training_params=(1, 0.03),
                     fine_tune_params=(1, 0.005), trainer_kwargs={"limit_train_batches": 2, "limit_val_batches": 1},
                     tables_output=out + "tables/", metric='euclidean', image_scores='max')
    assert list(df.index) == ["bottle", "average"]
    assert os.path.exists(out + "tables/csv/patch_all_scores.csv") and os.path.exists(out + "tables/csv/patch_image_auroc.csv")


# ---------------------------------------------------------------- 9. two gloo ranks equal one rank

def test_two_ranks_equal_one_rank(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import tools
    root, ck = _tree(tmp_path, seeded_sd)
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "knn_l2"])
    assert r["equal_across_ranks"] and r["world"] == 2, r
    two = torch.load(str(tmp_path / "l2_rank0.pt"))
    from self_supervised.models import AnomalyDetector
    seen = {}
    orig = AnomalyDetector.predict

    def spy(self, x):
        seen["threshold"] = self.threshold
        return orig(self, x)
    monkeypatch.setattr(AnomalyDetector, "predict", spy)
    one = two_rank_util.inference(tools, ck, root, "knn_l2")
    assert torch.equal(two["scores"], one.image_scores) and torch.equal(two["maps"], one.anomaly_maps)
    assert two["threshold"] == seen["threshold"] and np.isfinite(seen["threshold"])
