"""GPU tests of SPADE's image-conditioned gallery of the Euclidean kNN detector: csrc/knn_gallery.hip (ssad_group_means, ssad_l2_direct,
ssad_l2_knn_gallery / _index) and its way through AnomalyDetector(gallery=K), tools.inference and tools.sweep.

Two yardsticks.  (1) The whole-bank kernels of csrc/knn_l2.hip on the gallery's blocks gathered into one contiguous bank: the gallery
kernel claims to be that arithmetic on an indirect bank, so the comparison is bit for bit.  (2) The float64 numpy reference of
tests/knn_gallery_ref.py on the same fp32 inputs, at the bar tests/test_hip_knn_l2.py holds the Euclidean kernels to: a squared
distance within tau(D) 2^-24 A, A = |q|^2 + |b|^2 + 2 sum |q_i| |b_i|, tau(D) = min(64, D + 8), one more rounding for the root;
indices strict wherever the reference's gap exceeds twice the bar.  Inputs are views between NaN guard rows, outputs sit between
guard rows."""
import os

import numpy as np
import pytest
import torch

import knn_gallery_ref as ref
import knn_l2_ref as l2ref
import two_rank_util
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NAN = float("nan")
N_TRAIN = 8


def tau(d):
    return min(64.0, d + 8.0)


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


def guarded(t, fill=NAN):
    """A device copy of t as a view between two guard rows of `fill`: a read outside the view shows as a NaN in the result."""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    buf[1:-1] = t
    buf = buf.cuda()
    return buf, buf[1:-1]


def guarded_ids(gal):
    """int32 gallery [Q][K] between guard rows that name images far outside any bank."""
    buf = torch.full((gal.shape[0] + 2, gal.shape[1]), 2 ** 30, dtype=torch.int32)
    buf[1:-1] = torch.as_tensor(gal, dtype=torch.int32)
    buf = buf.cuda()
    return buf, buf[1:-1]


def guarded_out(shape, dtype=torch.float32):
    fill = NAN if dtype == torch.float32 else -7
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
    return buf, buf[1:-1]


def guards_intact(buf):
    g = torch.stack([buf[0].reshape(-1), buf[-1].reshape(-1)])
    return bool(torch.isnan(g).all()) if buf.dtype == torch.float32 else bool((g == -7).all())


def raw_gallery(x, bank, bsq, gal, p, k, s=1, index=False):
    """The C entry points on caller-owned, guarded outputs -> (out,) or (dist, idx), after checking the guard rows."""
    from self_supervised import _hip
    L = _hip.lib()
    n, d = x.shape
    q, t, kk = n // p, bank.shape[0] // p, gal.shape[1]
    st = _hip.stream()
    if index:
        dbuf, dist = guarded_out((n, k))
        ibuf, idx = guarded_out((n, k), torch.int32)
        part = torch.empty((s, n, 3), dtype=torch.int64, device="cuda") if s > 1 else None
        rc = L.ssad_l2_knn_gallery_index(x.data_ptr(), bank.data_ptr(), bsq.data_ptr(), gal.data_ptr(), part.data_ptr() if s > 1 else None,
                                         dist.data_ptr(), idx.data_ptr(), q, p, t, kk, d, k, s, st)
        assert rc == 0, L.ssad_last_error()
        torch.cuda.synchronize()
        assert guards_intact(dbuf) and guards_intact(ibuf)
        return dist, idx
    obuf, out = guarded_out((n,))
    part = torch.empty((s, n, 3), dtype=torch.float32, device="cuda") if s > 1 else None
    rc = L.ssad_l2_knn_gallery(x.data_ptr(), bank.data_ptr(), bsq.data_ptr(), gal.data_ptr(), part.data_ptr() if s > 1 else None,
                               out.data_ptr(), q, p, t, kk, d, k, s, st)
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


def sorted_gallery(q, t, kk, seed):
    """kk distinct bank images per query image, ascending (the gathered bank then keeps the global row order)."""
    rng = np.random.RandomState(seed)
    return np.stack([np.sort(rng.permutation(t)[:kk]) for _ in range(q)]).astype(np.int64)


def reference_case(x_h, bank_h, gal, p, k, d2_all, a_all):
    """Everything the float64 comparison needs that the reference alone gives: the k + 1 nearest gallery rows, the bar of every
    pick and where the index comparison is strict; asserts the 2 % cap on it."""
    n = x_h.shape[0]
    t_ = tau(x_h.shape[1])
    want_d2, want_i, want_a = ref.restricted_knn64(x_h, bank_h, gal, p, k + 1)
    bar2 = 2 * t_ * EPS * want_a[:, :k]
    strict = np.ones((n, k), dtype=bool)
    for j in range(k):
        if j > 0:
            strict[:, j] &= want_d2[:, j] - want_d2[:, j - 1] > np.maximum(bar2[:, j], bar2[:, j - 1])
        nxt = want_d2[:, j + 1]
        nxt_bar = np.where(np.isfinite(nxt), 2 * t_ * EPS * np.nan_to_num(want_a[:, j + 1]), 0.0)
        strict[:, j] &= nxt - want_d2[:, j] > np.maximum(bar2[:, j], nxt_bar)
    return want_d2, want_i, want_a, bar2, strict


def check_against_float64(x_h, gal, p, dist, idx, out, k, d2_all, a_all, refc):
    """dist / idx [N][k] of the index form and out [N] of the mean form (host tensors) against float64 -> worst ratio of the
    squared-distance error to 2^-24 A."""
    want_d2, want_i, want_a, bar2, strict = refc
    t_ = tau(x_h.shape[1])
    dist64, idx = dist.double().numpy(), idx.numpy().astype(np.int64)
    assert np.isfinite(dist64).all() and (dist64 >= 0).all()
    for q in range(gal.shape[0]):                                     # every pick is a row of the image's gallery, none twice
        assert np.isin(idx[q * p:(q + 1) * p] // p, gal[q]).all()
    assert all(len(set(row)) == k for row in idx)
    # (1) the returned distance against the float64 distance of the returned row, through its square
    d2_row, a_row = np.take_along_axis(d2_all, idx, 1), np.take_along_axis(a_all, idx, 1)
    err = np.abs(dist64 ** 2 - d2_row)
    ratio = float((err / (EPS * a_row)).max())
    assert (err <= t_ * EPS * a_row + 2 * EPS * d2_row).all(), ratio
    # (2) the returned row is a valid j-th pick: its float64 d2 against the float64 j-th smallest (a swap needs both errors)
    assert (np.abs(d2_row - want_d2[:, :k]) <= 2 * t_ * EPS * np.maximum(a_row, want_a[:, :k])).all()
    # (3) indices equal wherever the float64 gaps to both neighbours in the order exceed twice the bar
    assert np.array_equal(idx[strict], want_i[:, :k][strict])
    # (4) the mean form: the index form's distances averaged, bit for bit -- and against float64 directly
    assert torch.equal(_mean_of(dist, k), out), "mean form differs from the averaged index distances"
    dref = np.sqrt(want_d2[:, :k])
    e = bar2 + 2 * EPS * want_d2[:, :k]
    tol_d = np.minimum(np.sqrt(e), e / np.maximum(dref, 1e-300))
    mean_ref = dref.mean(1)
    assert (np.abs(out.double().numpy() - mean_ref) <= tol_d.mean(1) + 4 * EPS * mean_ref).all()
    return ratio


PS = (1, 64, 127, 128, 129, 300)
TK = ((1, 1), (3, 1), (3, 2), (3, 3), (5, 1), (5, 2), (5, 5))         # T in {1, 3, 5} x K in {1, 2, T}
QS = (1, 3)


def shape_cases(d, p):
    """(t, kk, q, x_h, bank_h, gal) of one (D, P): the inputs of the kernel tests, from seeds alone."""
    for t, kk in TK:
        bank_h = gauss(t * p, d, seed=3000 + 7 * d + 11 * p + t)
        for q in QS:
            x_h = gauss(q * p, d, seed=4000 + 7 * d + 11 * p + q)
            yield t, kk, q, x_h, bank_h, sorted_gallery(q, t, kk, seed=100 * t + 10 * kk + q)


# ---------------------------------------------------------------- 1. the kernel: gathered whole-bank run, float64, splits, calls

@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("d", [32, 64, 384])
def test_gallery_kernel_matches_the_gathered_run_and_float64(d, p):
    """Every P x T x K x Q x k x S of one width: (a) bit-equal to ops.l2_knn_fused(splits=1) / ops.l2_knn_index on the gallery's
    blocks gathered with index_select (idx mapped back to global rows: the gallery is ascending, so are the gathered rows); (b) float64
    at the bar, the 2 % cap asserted on the reference first; (c) the same bits for S in {1, 2, K} and on a second call."""
    from self_supervised import ops
    worst, worst_loose = 0.0, 0.0
    for t, kk, q, x_h, bank_h, gal in shape_cases(d, p):
        bbuf, bank = guarded(bank_h)
        xbuf, x = guarded(x_h)
        gbuf, gal_d = guarded_ids(gal)
        bsq = ops.row_sqnorms(bank)
        d2_all, a_all = l2ref.d2_64(x_h, bank_h), l2ref.scale_a(x_h, bank_h)
        rows = [torch.from_numpy(ref.gallery_rows(gal[i], p)).cuda() for i in range(q)]
        gathered = [(bank.index_select(0, r).contiguous(), bsq.index_select(0, r).contiguous()) for r in rows]
        for k in (1, 2, 3):
            if kk * p < k:
                continue
            refc = reference_case(x_h, bank_h, gal, p, k, d2_all, a_all)
            loose = 1.0 - refc[4].mean()
            assert loose <= 0.02, (t, kk, q, k, loose)                 # on the reference alone, first
            dist, idx = raw_gallery(x, bank, bsq, gal_d, p, k, 1, index=True)
            (out,) = raw_gallery(x, bank, bsq, gal_d, p, k, 1)
            for i in range(q):                                      # (a)
                xq = x[i * p:(i + 1) * p]
                gb, gs = gathered[i]
                assert torch.equal(out[i * p:(i + 1) * p], ops.l2_knn_fused(xq, gb, gs, k, splits=1)), (t, kk, q, k, i)
                gd, gi = ops.l2_knn_index(xq, gb, gs, k, splits=1)
                assert torch.equal(dist[i * p:(i + 1) * p], gd), (t, kk, q, k, i)
                assert torch.equal(idx[i * p:(i + 1) * p].long(), rows[i][gi.long()]), (t, kk, q, k, i)
            ratio = check_against_float64(x_h, gal, p, dist.cpu(), idx.cpu(), out.cpu(), k, d2_all, a_all, refc)      # (b)
            worst, worst_loose = max(worst, ratio), max(worst_loose, loose)
            for s in sorted({1, 2, kk}):                            # (c)  (s = 1: the second call)
                ds, is_ = raw_gallery(x, bank, bsq, gal_d, p, k, s, index=True)
                (os_,) = raw_gallery(x, bank, bsq, gal_d, p, k, s)
                assert torch.equal(dist, ds) and torch.equal(idx, is_) and torch.equal(out, os_), (t, kk, q, k, s)
            dw, iw = ops.l2_knn_gallery_index(x, bank, bsq, gal_d, p, k)
            assert torch.equal(dw, dist) and torch.equal(iw, idx) and torch.equal(ops.l2_knn_gallery(x, bank, bsq, gal_d, p, k), out)
    print(f"D={d} P={p}: worst |d^2 - d2_ref| / (2^-24 A) = {worst:.3f}, largest share outside the strict comparison {worst_loose:.2e}")


# ---------------------------------------------------------------- 2. ties, invalid entries, argument errors

def test_ties_go_to_the_smaller_global_row_whatever_the_gallery_order():
    """Image 3 holds copies of image 1's rows and the gallery names 3 before 1: the copies carry equal distance bits and the smaller
    global row comes first -- the one place where this kernel's tie order can differ from the gathered run's (there the copy in
    image 3 would stand first)."""
    from self_supervised import ops
    p, d, t = 129, 64, 5
    bank_h = gauss(t * p, d, seed=1)
    bank_h[3 * p:4 * p] = bank_h[1 * p:2 * p]
    x_h = torch.cat([bank_h[1 * p:2 * p] + 1e-2 * gauss(p, d, seed=2), gauss(p, d, seed=3)])
    gal = np.array([[3, 0, 1], [4, 3, 1]])
    bbuf, bank = guarded(bank_h)
    xbuf, x = guarded(x_h)
    gbuf, gal_d = guarded_ids(gal)
    bsq = ops.row_sqnorms(bank)
    want_d2, want_i, _ = ref.restricted_knn64(x_h, bank_h, gal, p, 3)
    assert np.array_equal(want_i[:p, 0], np.arange(p, 2 * p)) and np.array_equal(want_i[:p, 1], np.arange(3 * p, 4 * p))
    for s in (1, 2, 3):
        dist, idx = raw_gallery(x, bank, bsq, gal_d, p, 3, s, index=True)
        bits, idx = dist.cpu().view(torch.int32).numpy(), idx.cpu().numpy().astype(np.int64)
        assert np.array_equal(idx[:p, 0], np.arange(p, 2 * p)) and np.array_equal(idx[:p, 1], np.arange(3 * p, 4 * p))   # the near copies
        assert np.array_equal(bits[:p, 0], bits[:p, 1])
        src = np.where(idx // p == 3, idx - 2 * p, idx)             # a row of image 3 as its original in image 1
        for a in range(3):
            for b in range(a + 1, 3):
                same = src[:, a] == src[:, b]
                assert (bits[same, a] == bits[same, b]).all() and (idx[same, a] < idx[same, b]).all()
        assert same_or_sorted(dist.cpu().numpy())
        (out,) = raw_gallery(x, bank, bsq, gal_d, p, 3, s)
        assert torch.equal(_mean_of(dist, 3), out.cpu())


def same_or_sorted(d):
    return bool((np.diff(d, axis=1) >= 0).all())


def test_invalid_entries_are_skipped_and_an_empty_gallery_gives_inf():
    from self_supervised import ops
    p, d, t = 129, 64, 5
    bank_h, x_h = gauss(t * p, d, seed=4), gauss(3 * p, d, seed=5)
    bbuf, bank = guarded(bank_h)
    xbuf, x = guarded(x_h)
    bsq = ops.row_sqnorms(bank)
    clean = np.array([[0, 3], [1, 4], [2, 0]])
    dirty = np.array([[-1, 0, t, 3], [1, -1, 4, t + 7], [2 ** 31 - 1, 2, 0, -1]])
    empty = np.array([[0, 3], [-1, t], [2, 0]])                     # the second image has no valid entry
    gb1, g_clean = guarded_ids(clean)
    gb2, g_dirty = guarded_ids(dirty)
    gb3, g_empty = guarded_ids(empty)
    for k in (1, 3):
        for s in (1, 2, 4):
            dc, ic = raw_gallery(x, bank, bsq, g_clean, p, k, min(s, 2), index=True)
            (oc,) = raw_gallery(x, bank, bsq, g_clean, p, k, min(s, 2))
            dd, id_ = raw_gallery(x, bank, bsq, g_dirty, p, k, s, index=True)
            (od,) = raw_gallery(x, bank, bsq, g_dirty, p, k, s)
            assert torch.equal(dc, dd) and torch.equal(ic, id_) and torch.equal(oc, od), (k, s)
            assert torch.isfinite(od).all() and int(id_.min()) >= 0 and int(id_.max()) < t * p
            de, ie = raw_gallery(x, bank, bsq, g_empty, p, k, min(s, 2), index=True)
            (oe,) = raw_gallery(x, bank, bsq, g_empty, p, k, min(s, 2))
            mid = slice(p, 2 * p)
            assert (oe[mid] == float("inf")).all() and (de[mid] == float("inf")).all() and (ie[mid] == -1).all()
            keep = torch.cat([torch.arange(0, p), torch.arange(2 * p, 3 * p)]).cuda()
            assert torch.equal(oe[keep], oc[keep]) and torch.equal(de[keep], dc[keep]) and torch.equal(ie[keep], ic[keep])
    # fewer valid rows than k: P = 1, one valid entry of two, k = 2
    b1, x1 = gauss(3, 32, 6), gauss(2, 32, 7)
    _, b1d = guarded(b1)
    _, x1d = guarded(x1)
    _, g1 = guarded_ids(np.array([[1, -1], [5, 2]]))
    dist, idx = raw_gallery(x1d, b1d, ops.row_sqnorms(b1d), g1, 1, 2, 1, index=True)
    (out,) = raw_gallery(x1d, b1d, ops.row_sqnorms(b1d), g1, 1, 2, 1)
    assert idx.cpu().tolist() == [[1, -1], [2, -1]] and torch.isfinite(dist[:, 0]).all()
    assert (dist[:, 1] == float("inf")).all() and (out == float("inf")).all()


def test_argument_errors_leave_the_outputs_untouched():
    from self_supervised import _hip, ops
    L = _hip.lib()
    st = _hip.stream()
    p = 4
    x, bank = gauss(2 * p, 64, 1).cuda(), gauss(3 * p, 64, 2).cuda()
    bsq = ops.row_sqnorms(bank)
    gal = torch.tensor([[0, 1], [2, 1]], dtype=torch.int32, device="cuda")
    out = torch.full((2 * p,), NAN, device="cuda")
    dist = torch.full((2 * p, 3), NAN, device="cuda")
    idx = torch.full((2 * p, 3), -7, dtype=torch.int32, device="cuda")
    partf = torch.full((2, 2 * p, 3), NAN, device="cuda")
    partk = torch.full((2, 2 * p, 3), -7, dtype=torch.int64, device="cuda")
    desc = torch.full((2, 64), NAN, device="cuda")
    P = lambda t: t.data_ptr()
    good = dict(x=P(x), bank=P(bank), bsq=P(bsq), gal=P(gal), Q=2, P=p, T=3, K=2, D=64, k=3, S=2)
    bad = [dict(x=None), dict(bank=None), dict(bsq=None), dict(gal=None), dict(Q=0), dict(Q=65536), dict(P=0), dict(T=0), dict(K=0),
           dict(D=48), dict(D=0), dict(D=65536 + 32), dict(k=0), dict(k=4), dict(S=0), dict(S=65536), dict(P=1, K=2, k=3)]
    for change in bad:
        a = {**good, **change}
        for s_, part_f, part_k in ((a["S"], P(partf), P(partk)), (1 if "S" not in change else a["S"], None, None)):
            assert L.ssad_l2_knn_gallery(a["x"], a["bank"], a["bsq"], a["gal"], part_f, P(out), a["Q"], a["P"], a["T"], a["K"], a["D"],
                                         a["k"], s_, st) == 2, change
            assert L.ssad_l2_knn_gallery_index(a["x"], a["bank"], a["bsq"], a["gal"], part_k, P(dist), P(idx), a["Q"], a["P"], a["T"],
                                               a["K"], a["D"], a["k"], s_, st) == 2, change
    a = good
    args = (a["Q"], a["P"], a["T"], a["K"], a["D"], a["k"])
    assert L.ssad_l2_knn_gallery(a["x"], a["bank"], a["bsq"], a["gal"], None, P(out), *args, 2, st) == 2          # S > 1 without part
    assert L.ssad_l2_knn_gallery(a["x"], a["bank"], a["bsq"], a["gal"], P(partf), None, *args, 2, st) == 2
    assert L.ssad_l2_knn_gallery_index(a["x"], a["bank"], a["bsq"], a["gal"], None, P(dist), P(idx), *args, 2, st) == 2
    assert L.ssad_l2_knn_gallery_index(a["x"], a["bank"], a["bsq"], a["gal"], P(partk), None, P(idx), *args, 2, st) == 2
    assert L.ssad_l2_knn_gallery_index(a["x"], a["bank"], a["bsq"], a["gal"], P(partk), P(dist), None, *args, 2, st) == 2
    assert L.ssad_l2_knn_gallery_index(a["x"], a["bank"], a["bsq"], a["gal"], P(partk) + 4, P(dist), P(idx), *args, 2, st) == 2
    assert b"8-byte aligned" in L.ssad_last_error()
    assert L.ssad_group_means(None, P(desc), 2, p, 64, st) == 2 and L.ssad_group_means(P(x), None, 2, p, 64, st) == 2
    assert L.ssad_group_means(P(x), P(desc), 0, p, 64, st) == 2 and L.ssad_group_means(P(x), P(desc), 2, 0, 64, st) == 2
    assert L.ssad_l2_direct(None, P(bank), P(desc), 2, 3, 64, st) == 2 and L.ssad_l2_direct(P(x), P(bank), None, 2, 3, 64, st) == 2
    assert L.ssad_l2_direct(P(x), P(bank), P(desc), 2, 0, 64, st) == 2 and L.ssad_l2_direct(P(x), P(bank), P(desc), 2, 3, 0, st) == 2
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(dist).all() and (idx == -7).all() and torch.isnan(desc).all()
    assert torch.isnan(partf).all() and (partk == -7).all()
    with pytest.raises(ValueError, match="fewer than k = 3 rows"):
        ops.l2_knn_gallery(x[:2], bank[:3], bsq[:3], gal, 1, k=3)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.l2_knn_gallery_index(x[:, :48].contiguous(), bank[:, :48].contiguous(), bsq, gal, p)


# ---------------------------------------------------------------- 3. stage 1: descriptors and their distances

@pytest.mark.parametrize("d", [32, 384])
@pytest.mark.parametrize("p", [1, 127, 300])
def test_group_means(p, d):
    from self_supervised import ops
    rows = gauss(3 * p, d, seed=p + d) + 0.25
    buf, x = guarded(rows)
    got = ops.group_means(x, p)
    want = ref.descriptors64(rows, p)
    err = np.abs(got.cpu().double().numpy() - want)
    print(f"P={p} D={d}: worst |mean - float64| / (2^-24 |mean|) = {(err / (EPS * np.abs(want))).max():.3f}")
    assert (err <= EPS * np.abs(want)).all()
    for g in range(3):                                              # the same bits alone as inside the batch
        alone = ops.group_means(x[g * p:(g + 1) * p], p)
        assert torch.equal(alone[0].view(torch.int32), got[g].view(torch.int32))
    assert torch.equal(ops.group_means(x, p), got)


def l2_direct_bar(d, d2):
    return (d / 64.0 + 10.0) * EPS * d2


@pytest.mark.parametrize("d", [32, 384, 100])
def test_l2_direct(d):
    """(D / 64 + 10) 2^-24 sum (q - b)^2: the a-priori bound of the chain -- a lane's fma chain has ceil(D / 64) terms, the butterfly
    six additions, the difference and its square one rounding each, and all terms are non-negative."""
    from self_supervised import ops
    for q_n, t in ((1, 1), (3, 5), (7, 130)):
        b_h = gauss(t, d, seed=10 + t) + 0.5
        q_h = gauss(q_n, d, seed=20 + q_n) + 0.5
        q_h[0] = b_h[t - 1]
        _, b = guarded(b_h)
        _, q = guarded(q_h)
        got = ops.l2_direct(q, b)
        want = ref.direct_d2_64(q_h, b_h)
        err = np.abs(got.cpu().double().numpy() - want)
        assert (err <= l2_direct_bar(d, want)).all(), (err / np.maximum(EPS * want, 1e-300)).max()
        assert float(got[0, t - 1]) == 0.0                           # a copy: exactly 0
        one = ops.l2_direct(q[q_n - 1:], b[t // 2:t // 2 + 1])       # a pair's bits do not depend on Q or T
        assert torch.equal(one[0, 0].view(torch.int32), got[q_n - 1, t // 2].view(torch.int32))


def root_tol(bar, d2):
    """|sqrt(a) - sqrt(d2)| for |a - d2| <= bar."""
    return np.minimum(np.sqrt(bar), bar / np.maximum(np.sqrt(d2), 1e-300))


def stage1_valid(got_gal, all_d2, kq, d, cap=None):
    """The device's gallery against the float64 one: equal wherever the reference's gaps exceed twice the bar (-> share outside;
    held to `cap` on the reference alone, first), and every pick a valid j-th pick within the bar."""
    order = np.argsort(all_d2, axis=1, kind="stable")
    srt = np.take_along_axis(all_d2, order, 1)
    bar2 = 2 * l2_direct_bar(d, srt)
    strict = np.ones((all_d2.shape[0], kq), dtype=bool)
    for j in range(kq):
        if j > 0:
            strict[:, j] &= srt[:, j] - srt[:, j - 1] > bar2[:, j]
        if j + 1 < srt.shape[1]:
            strict[:, j] &= srt[:, j + 1] - srt[:, j] > bar2[:, j + 1]
    if cap is not None:
        assert 1.0 - strict.mean() <= cap, 1.0 - strict.mean()
    picked = np.take_along_axis(all_d2, got_gal, 1)
    assert (np.abs(picked - srt[:, :kq]) <= np.maximum(bar2[:, :kq], 2 * l2_direct_bar(d, picked))).all()
    assert np.array_equal(got_gal[strict], order[:, :kq][strict])
    return 1.0 - strict.mean()


def test_stage1_gallery_matches_float64():
    """group_means -> l2_direct -> stable sort against the float64 gallery of the same descriptors: equal outside twice the bar
    (at most 2 % of the picks inside it, asserted on the reference first), equal distances to the smaller image."""
    from self_supervised import ops
    p, d, t, q, kk = 16, 384, 60, 24, 10
    bank_h, x_h = gauss(t * p, d, seed=31), gauss(q * p, d, seed=32)
    bank_h[5 * p:6 * p] = bank_h[2 * p:3 * p]                       # two bank images with one descriptor
    x_h[:p] = bank_h[2 * p:3 * p]
    _, bank = guarded(bank_h)
    _, x = guarded(x_h)
    d2 = ops.l2_direct(ops.group_means(x, p), ops.group_means(bank, p))
    vals, order = torch.sort(d2, dim=1, stable=True)
    gal = order[:, :kk].cpu().numpy().astype(np.int64)
    _, _, all_d2 = ref.gallery64(x_h, bank_h, p, kk)
    loose = stage1_valid(gal, all_d2, kk, d, cap=0.02)
    print(f"stage 1: share of picks inside twice the bar {loose:.4f}")
    assert gal[0, 0] == 2 and gal[0, 1] == 5 and float(vals[0, 0]) == 0.0 and float(vals[0, 1]) == 0.0


# ---------------------------------------------------------------- 4. the detector

def _maps_tol(want_d2, want_a, d):
    e = 2 * tau(d) * EPS * want_a + 2 * EPS * want_d2
    dref = np.sqrt(want_d2)
    return np.minimum(np.sqrt(e), e / np.maximum(dref, 1e-300)).mean(1) + 4 * EPS * dref.mean(1)


def test_detector_against_float64():
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector
    n_img, p, d, kk = 6, 64, 32, 2
    emb = gauss(n_img * p, d, seed=3) * 0.5 + gauss(n_img, d, seed=4).repeat_interleave(p, 0)       # images around their own centres
    groups = torch.arange(n_img).repeat_interleave(p)
    np.random.seed(5)
    det = AnomalyDetector(patch_level=True, batch=3, num_patches=p, metric='euclidean', gallery=kk)
    det.fit(emb, groups=groups)
    np.random.seed(5)
    perm = np.random.permutation(n_img)
    tr, va = perm[2:], perm[:2]
    bank_h = torch.cat([emb[i * p:(i + 1) * p] for i in tr])
    val_h = torch.cat([emb[i * p:(i + 1) * p] for i in va])
    assert torch.equal(det.bank.cpu(), bank_h) and torch.equal(det.bank_sq, ops.row_sqnorms(det.bank))
    assert torch.equal(det.bank_desc, ops.group_means(det.bank, p)) and det.bank_desc.shape == (4, d)
    x_h = gauss(3 * p, d, seed=9) * 0.5 + gauss(n_img, d, seed=4)[[1, 4, 0]].repeat_interleave(p, 0)

    def reference(rows):
        gal, gd2, all_d2 = ref.gallery64(rows, bank_h, p, kk)
        got_gal, got_d2 = det.retrieve(rows.cuda())
        assert got_gal.dtype == torch.int32 and tuple(got_gal.shape) == (rows.shape[0] // p, kk)
        assert stage1_valid(got_gal.cpu().numpy().astype(np.int64), all_d2, kk, d) == 0.0     # centres far apart: nothing ambiguous
        assert (np.abs(got_d2.cpu().double().numpy() - gd2) <= l2_direct_bar(d, gd2)).all()
        return gal, gd2, ref.restricted_knn64(rows, bank_h, gal, p, 3)

    gal, gd2, (want_d2, want_i, want_a) = reference(x_h)
    got = det.predict(x_h)
    assert tuple(got.shape) == (3, 1, 8, 8)
    tol = _maps_tol(want_d2, want_a, d)
    assert (np.abs(got.cpu().double().numpy().reshape(-1) - np.sqrt(want_d2).mean(1)) <= tol).all()
    _, _, (val_d2, _, val_a) = reference(val_h)
    assert abs(det.threshold - np.sqrt(val_d2).mean(1).max()) <= _maps_tol(val_d2, val_a, d).max()
    dist, idx = det.kneighbors(x_h)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want_i)       # (Gaussian picks: gaps far above the bar)
    assert np.abs(dist.cpu().double().numpy() - np.sqrt(want_d2)).max() <= tol.max()
    assert torch.equal(_mean_of(dist, 3), got.reshape(-1).cpu())
    # image scores: 'max' is the row maximum; 'retrieval' the mean of the K stage-1 distances
    assert torch.equal(det.image_scores(x_h, 'max'), got.reshape(3, p).max(1).values)
    retr = det.image_scores(x_h, 'retrieval').cpu().double().numpy()
    want_r = ref.retrieval_scores64(x_h, bank_h, p, kk)
    tol_r = root_tol(l2_direct_bar(d, gd2), gd2).mean(1) + 4 * EPS * want_r
    assert retr.shape == (3,) and (np.abs(retr - want_r) <= tol_r).all()
    with pytest.raises(ValueError, match="does not go with a gallery"):
        det.image_scores(x_h, 'reweighted')
    with pytest.raises(ValueError, match="not whole images"):
        det.predict(x_h[:100])
    # the state travels with its gallery; bank_sq and bank_desc are recomputed to the same bits
    other = AnomalyDetector(patch_level=True, batch=3, num_patches=p, metric='euclidean', gallery=kk)
    other.load_state(det.state())
    assert torch.equal(other.bank_desc, det.bank_desc) and torch.equal(other.bank_sq, det.bank_sq)
    assert torch.equal(other.predict(x_h), got)
    # K >= T: every bank image -- the maps of the same detector without a gallery, bit for bit (duplicate-free data)
    for big in (4, 50):
        np.random.seed(5)
        all_of = AnomalyDetector(patch_level=True, batch=3, num_patches=p, metric='euclidean', gallery=big)
        all_of.fit(emb, groups=groups)
        np.random.seed(5)
        plain = AnomalyDetector(patch_level=True, batch=3, num_patches=p, metric='euclidean')
        plain.fit(emb, groups=groups)
        assert torch.equal(all_of.bank, plain.bank) and all_of.threshold == plain.threshold
        assert torch.equal(all_of.predict(x_h), plain.predict(x_h))
        da, ia = all_of.kneighbors(x_h)
        dp, ip = plain.kneighbors(x_h)
        assert torch.equal(da, dp) and torch.equal(ia, ip)


# ---------------------------------------------------------------- 5. through tools.inference and tools.sweep

def _tree(tmp_path, seeded_sd):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=96)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


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


@pytest.mark.parametrize("image_scores", ["max", "retrieval"])
@pytest.mark.parametrize("localization", ["patches", "dense"])
def test_inference_with_a_gallery(tmp_path, seeded_sd, monkeypatch, localization, image_scores):
    from self_supervised import ops, tools
    from self_supervised.models import AnomalyDetector
    root, ck = _tree(tmp_path, seeded_sd)
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
        return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                               metric='euclidean', localization=localization, **more)

    before = run(image_scores='max')
    assert seen["det"].gallery is None and seen["det"].bank_desc is None and sorted(seen["det"].state()) == ["bank", "metric"]
    res = run(gallery=3, image_scores=image_scores)
    det, fit_rows = seen["det"], seen["fit_rows"]
    assert det.gallery == 3 and det.metric == 'euclidean'
    outside = _standalone_rows(ck, root, dense=localization == "dense")
    p, d = outside.shape[1], outside.shape[2]
    assert torch.equal(fit_rows, outside.reshape(-1, d))            # the fit rows are model(x) of every training image, bit for bit
    bank_h = det.bank.cpu()                                         # 5 of the 8 images (70 %), whole blocks, none twice
    blocks = bank_h.reshape(-1, p, d)
    which = [[i for i in range(N_TRAIN) if torch.equal(b, outside[i])] for b in blocks]
    assert len(blocks) == N_TRAIN - 3 and all(len(w) >= 1 for w in which) and len({w[0] for w in which}) == len(blocks)
    assert det.bank_desc.shape == (N_TRAIN - 3, d) and torch.equal(det.bank_desc, ops.group_means(det.bank, p))
    rows = res.embedding_vectors.float()
    n_img = rows.shape[0] // p
    assert n_img == 4 and d % 32 == 0
    # stage 1 against float64 at its bar, then stage 2 on the device's gallery against float64 at its bar
    _, _, all_d2 = ref.gallery64(rows, bank_h, p, 3)
    gal_d, got_d2 = det.retrieve(rows.cuda())
    gal = gal_d.cpu().numpy().astype(np.int64)
    loose = stage1_valid(gal, all_d2, 3, d)
    print(f"{localization}: share of stage-1 picks inside twice the bar {loose:.3f}")
    want_d2, _, want_a = ref.restricted_knn64(rows, bank_h, gal, p, 3)
    maps = res.anomaly_maps
    got = maps.reshape(-1).double().numpy()
    want, tol = np.sqrt(want_d2).mean(1), _maps_tol(want_d2, want_a, d)
    print(f"{localization}: max |map - float64| = {np.abs(got - want).max():.3e} (values ~ {want.max():.3e}, bound ~ {tol.max():.3e})")
    assert (np.abs(got - want) <= tol).all()
    assert maps.shape == before.anomaly_maps.shape and maps.dtype == before.anomaly_maps.dtype
    full = l2ref.patch_scores64(rows, bank_h, 3)
    assert (got >= full - tol).all()                                # fewer candidates: never nearer than the whole bank
    s = res.image_scores
    assert s.dtype == torch.float32 and tuple(s.shape) == (4,) and torch.isfinite(s).all()
    if image_scores == 'max':
        assert torch.equal(s, maps.reshape(4, -1).max(1).values)
    else:
        picked = np.take_along_axis(all_d2, gal, 1)
        want_r = np.sqrt(picked).mean(1)
        tol_r = root_tol(l2_direct_bar(d, picked), picked).mean(1) + 4 * EPS * want_r
        assert (np.abs(s.double().numpy() - want_r) <= tol_r).all()
    # on through upsample and the Evaluator
    res.anomaly_maps = tools.upsample(maps, int(res.ground_truths.shape[-1]), verbose=False)
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou'])
    ev.evaluate(res, "bottle", str(tmp_path / "out") + "/", patch_level=True)
    assert ev.scores.auroc is not None and np.isfinite(ev.scores.auroc)
    # the call without a gallery, with and without the argument, after a gallery call: the same bits as before it
    for other in (run(image_scores='max'), run(image_scores='max', gallery=None)):
        assert torch.equal(before.anomaly_maps, other.anomaly_maps) and torch.equal(before.image_scores, other.image_scores)
        assert torch.equal(before.embedding_vectors, other.embedding_vectors)


def test_sweep_with_a_gallery_writes_its_tables(tmp_path):
    from self_supervised import tools, datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), n_train=8, n_test_good=2, n_test_bad=2, size=96)
    out = str(tmp_path / "gal") + "/"
    np.random.seed(0)
    df = tools.sweep(root, out, ["bottle"], imsize=(64, 64), batch_size=4, seed=0, projection_training_params=(1, 0.03),
                     fine_tune_params=(1, 0.005), trainer_kwargs={"limit_train_batches": 2, "limit_val_batches": 1},
                     tables_output=out + "tables/", metric='euclidean', bank='train', image_scores='retrieval', gallery=3)
    assert list(df.index) == ["bottle", "average"]
    assert os.path.exists(out + "tables/csv/patch_all_scores.csv") and os.path.exists(out + "tables/csv/patch_image_auroc.csv")


# ---------------------------------------------------------------- 6. two gloo ranks equal one rank

def test_two_ranks_equal_one_rank(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import tools
    root, ck = _tree(tmp_path, seeded_sd)
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "knn_gallery"])
    assert r["equal_across_ranks"] and r["world"] == 2, r
    two = torch.load(str(tmp_path / "gallery_rank0.pt"))
    from self_supervised.models import AnomalyDetector
    seen = {}
    orig = AnomalyDetector.predict

    def spy(self, x):
        seen["threshold"] = self.threshold
        return orig(self, x)
    monkeypatch.setattr(AnomalyDetector, "predict", spy)
    one = two_rank_util.inference(tools, ck, root, "knn_gallery")
    assert torch.equal(two["scores"], one.image_scores) and torch.equal(two["maps"], one.anomaly_maps)
    assert two["threshold"] == seen["threshold"] and np.isfinite(seen["threshold"])
