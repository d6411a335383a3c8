"""GPU tests of the inverted-file index of the Euclidean kNN detector: csrc/knn_ivf.hip (ssad_segment_means, ssad_l2_knn_ivf /
_index), ops.kmeans_l2 and the way through AnomalyDetector(index='ivf'), tools.inference and two ranks.

Two yardsticks.  (1) The whole-bank kernels of csrc/knn_l2.hip on the original, unsorted bank: with every cell probed the index
claims to be that search, so the comparison is bit for bit.  (2) The float64 numpy reference of tests/ivf_ref.py on the same fp32
inputs at the bar tests/knn_l2_ref.py states: a squared distance within 64 units of 2^-24 A, A = |q|^2 + |b|^2 + 2 sum |q_i| |b_i|,
one more rounding for the root; rows strict wherever the reference's gaps to both neighbours exceed the bars of both (at most 1 % of
the (query, slot) pairs are left out, asserted on the reference alone).  Inputs are views between guard rows (NaN, or ids far outside),
outputs are pre-filled with NaN / -7 and sit between guard rows.  The cells are built by hand: 0, 1, 2, 127, 128, 129 and 300 rows."""
import numpy as np
import pytest
import torch

import ivf_ref as ref
import knn_l2_ref as l2ref
import two_rank_util
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NAN = float("nan")
INF = float("inf")
SIZES = (0, 1, 2, 127, 128, 129, 300)
NLIST = len(SIZES)
R = sum(SIZES)
N_TRAIN = 8


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


def guarded(t, fill=None):
    """A device copy of t as a view between two guard rows (NaN for floats, 2^30 for ids): a read outside the view shows in the result."""
    if fill is None:
        fill = NAN if t.dtype == torch.float32 else 2 ** 30
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    buf[1:-1] = t
    buf = buf.cuda()
    return buf, buf[1:-1]


def guarded_out(shape, dtype=torch.float32):
    fill = NAN if dtype == torch.float32 else -7
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
    return buf, buf[1:-1]


def guards_intact(buf):
    g = torch.stack([buf[0].reshape(-1), buf[-1].reshape(-1)])
    return bool(torch.isnan(g).all()) if buf.dtype == torch.float32 else bool((g == -7).all())


class Index:
    """A hand-built inverted file over gauss rows: cells of SIZES rows, a random permutation as `perm`; everything on the device as
    guarded views, the original bank and cell_of_row on the host for the references."""

    def __init__(self, d, seed):
        from self_supervised import ops
        self.d = d
        self.bank_h = gauss(R, d, seed)                              # original row order
        self.perm_h = torch.from_numpy(np.random.RandomState(seed).permutation(R).astype(np.int32))
        self.offsets_h = torch.tensor(np.concatenate([[0], np.cumsum(SIZES)]), dtype=torch.int32)
        self.cell_of_row = np.empty(R, dtype=np.int64)
        self.cell_of_row[self.perm_h.numpy()] = np.repeat(np.arange(NLIST), SIZES)
        self.keep = [guarded(self.bank_h[self.perm_h.long()]), guarded(self.perm_h), guarded(self.offsets_h), guarded(self.bank_h)]
        self.sorted, self.perm, self.offsets, self.bank = (v for _, v in self.keep)
        self.bsq_sorted, self.bsq = ops.row_sqnorms(self.sorted), ops.row_sqnorms(self.bank)


_CACHE = {}


def index_of(d):
    if d not in _CACHE:
        _CACHE[d] = Index(d, seed=900 + d)
    return _CACHE[d]


def raw_ivf(ix, x, probes, k, index=True):
    """The C entry points on caller-owned, pre-filled, guarded outputs -> (dist, idx) or out, after checking the guard rows."""
    from self_supervised import _hip, ops
    L = _hip.lib()
    n, d = x.shape
    tiles, pairs = ops.ivf_schedule(probes, NLIST)
    part = torch.empty((n * probes.shape[1], 3), dtype=torch.int64, device="cuda")
    common = (x.data_ptr(), ix.sorted.data_ptr(), ix.bsq_sorted.data_ptr(), ix.offsets.data_ptr(), ix.perm.data_ptr(), probes.data_ptr(),
              tiles.data_ptr(), pairs.data_ptr(), part.data_ptr())
    sizes = (n, d, R, NLIST, probes.shape[1], tiles.shape[1], k, _hip.stream())
    if index:
        dbuf, dist = guarded_out((n, k))
        ibuf, idx = guarded_out((n, k), torch.int32)
        rc = L.ssad_l2_knn_ivf_index(*common, dist.data_ptr(), idx.data_ptr(), *sizes)
        assert rc == 0, L.ssad_last_error()
        torch.cuda.synchronize()
        assert guards_intact(dbuf) and guards_intact(ibuf)
        return dist, idx
    obuf, out = guarded_out((n,))
    rc = L.ssad_l2_knn_ivf(*common, out.data_ptr(), *sizes)
    assert rc == 0, L.ssad_last_error()
    torch.cuda.synchronize()
    assert guards_intact(obuf)
    return out


def _mean_of(dist, k):
    """(d0 [+ d1] [+ d2]) / k, added smallest first, in IEEE fp32 on the host -- the kernels' epilogue."""
    d = dist.cpu().numpy()
    s = d[:, 0].copy()
    for j in range(1, k):
        s = s + d[:, j]
    assert s.dtype == np.float32
    return torch.from_numpy(s / np.float32(k))


def random_probes(n, nprobe, seed):
    """nprobe distinct cells per query, in random order."""
    rng = np.random.RandomState(seed)
    return np.stack([rng.permutation(NLIST)[:nprobe] for _ in range(n)]).astype(np.int32)


NS = (1, 127, 129, 300)


# ---------------------------------------------------------------- 1. exact where it is defined: every cell probed

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", [32, 64])
def test_every_cell_probed_equals_the_flat_search_bit_for_bit(d, n):
    from self_supervised import ops
    ix = index_of(d)
    xbuf, x = guarded(gauss(n, d, seed=100 + n + d))
    pbuf, probes = guarded(torch.from_numpy(random_probes(n, NLIST, seed=n)))
    for k in (1, 2, 3):
        want_d, want_i = ops.l2_knn_index(x, ix.bank, ix.bsq, k, splits=1)
        want_o = ops.l2_knn_fused(x, ix.bank, ix.bsq, k, splits=1)
        dist, idx = raw_ivf(ix, x, probes, k)
        out = raw_ivf(ix, x, probes, k, index=False)
        assert torch.equal(dist, want_d) and torch.equal(idx, want_i), (d, n, k)
        assert torch.equal(out, want_o), (d, n, k)
        dw, iw = ops.l2_knn_ivf_index(x, ix.sorted, ix.bsq_sorted, ix.offsets, probes, ix.perm, k)
        assert torch.equal(dw, dist) and torch.equal(iw, idx)
        assert torch.equal(ops.l2_knn_ivf(x, ix.sorted, ix.bsq_sorted, ix.offsets, probes, ix.perm, k), out)


# ---------------------------------------------------------------- 2. the restricted search against float64

@pytest.mark.parametrize("nprobe", [1, 3])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", [32, 64])
def test_restricted_search_matches_float64(d, n, nprobe):
    ix = index_of(d)
    x_h = gauss(n, d, seed=200 + n + d)
    probes_h = random_probes(n, nprobe, seed=7 * n + nprobe)
    xbuf, x = guarded(x_h)
    pbuf, probes = guarded(torch.from_numpy(probes_h))
    d2_all, a_all = l2ref.d2_64(x_h, ix.bank_h), l2ref.scale_a(x_h, ix.bank_h)
    worst = 0.0
    for k in (1, 2, 3):
        want_d2, want_i, want_a, strict, loose = ref.reference_case(x_h, ix.bank_h, ix.cell_of_row, probes_h, NLIST, k)
        dist, idx = raw_ivf(ix, x, probes, k)
        out = raw_ivf(ix, x, probes, k, index=False)
        dist64, idx_h = dist.cpu().double().numpy(), idx.cpu().numpy().astype(np.int64)
        missing = want_i < 0
        assert np.array_equal(idx_h < 0, missing) and (idx_h[missing] == -1).all() and np.isinf(dist64[missing]).all()
        have = ~missing
        safe = np.where(have, idx_h, 0)
        assert np.isin(ix.cell_of_row[safe][have], np.arange(NLIST)).all()
        assert all(ix.cell_of_row[r] in probes_h[i] for i in range(n) for r in idx_h[i] if r >= 0)      # a row of a probed cell
        assert all(len(set(row[row >= 0])) == (row >= 0).sum() for row in idx_h)                        # none twice
        # the returned distance against the float64 distance of the returned row, through its square
        d2_row, a_row = np.take_along_axis(d2_all, safe, 1), np.take_along_axis(a_all, safe, 1)
        err = np.abs(dist64 ** 2 - d2_row)[have]
        assert (err <= (ref.TAU * EPS * a_row + 2 * EPS * d2_row)[have]).all()
        worst = max(worst, float((err / (EPS * a_row[have])).max()) if have.any() else 0.0)
        # the returned row is a valid j-th pick, and THE j-th pick wherever the reference is strict
        assert (np.abs(d2_row - want_d2)[have] <= (ref.TAU * EPS * (a_row + np.nan_to_num(want_a)))[have]).all()
        assert np.array_equal(idx_h[strict], want_i[strict])
        # the mean form: the index form's distances averaged, bit for bit (+inf where a slot is missing)
        assert torch.equal(_mean_of(dist, k), out.cpu())
        assert np.array_equal(np.isinf(out.cpu().numpy()), missing.any(1))
    print(f"D={d} N={n} nprobe={nprobe}: worst |d^2 - d2_ref| / (2^-24 A) = {worst:.3f}")


# ---------------------------------------------------------------- 3. missing slots and skipped entries

def test_missing_slots_and_skipped_probe_entries():
    ix = index_of(64)
    x_h = gauss(6, 64, seed=5)
    # cells 0, 1, 2 hold 0, 1, 2 rows; -1 and NLIST are no cells
    probes_h = np.array([[0, -1, NLIST], [1, 0, -1], [2, NLIST, 0], [1, 2, -1], [-1, NLIST, 2 ** 30], [3, -1, 1]], dtype=np.int32)
    rows_in = [0, 1, 2, 3, 0, 128]
    xbuf, x = guarded(x_h)
    pbuf, probes = guarded(torch.from_numpy(probes_h))
    for k in (1, 2, 3):
        want_d2, want_i, _ = ref.restricted_knn64(x_h, ix.bank_h, ix.cell_of_row, probes_h, NLIST, k)
        dist, idx = raw_ivf(ix, x, probes, k)
        out = raw_ivf(ix, x, probes, k, index=False)
        idx_h, dist_h = idx.cpu().numpy(), dist.cpu().numpy()
        for i, have in enumerate(rows_in):
            m = min(have, k)
            assert (idx_h[i, m:] == -1).all() and np.isinf(dist_h[i, m:]).all() and (idx_h[i, :m] >= 0).all(), (k, i)
            assert np.isfinite(dist_h[i, :m]).all()
            assert bool(np.isinf(out[i].item())) == (have < k), (k, i)
        assert np.array_equal(idx_h, want_i)                        # (gauss rows: the few candidates are far apart)
    # the skipped entries change nothing: the same cells without them
    clean = np.array([[1, 2], [3, 1]], dtype=np.int32)
    dirty = np.array([[-1, 1, NLIST, 2], [3, 2 ** 31 - 1, 1, -5]], dtype=np.int32)
    _, xc = guarded(x_h[:2])
    _, pc = guarded(torch.from_numpy(clean))
    _, pd = guarded(torch.from_numpy(dirty))
    dc, ic = raw_ivf(ix, xc, pc, 3)
    dd, id_ = raw_ivf(ix, xc, pd, 3)
    assert torch.equal(dc, dd) and torch.equal(ic, id_)
    assert torch.equal(raw_ivf(ix, xc, pc, 3, index=False), raw_ivf(ix, xc, pd, 3, index=False))
    # a cell named twice counts once
    _, p2 = guarded(torch.from_numpy(np.array([[1, 2, 2, 1], [3, 1, 3, 3]], dtype=np.int32)))
    d2_, i2_ = raw_ivf(ix, xc, p2, 3)
    assert torch.equal(dc, d2_) and torch.equal(ic, i2_)


# ---------------------------------------------------------------- 4. independence of the tiling

@pytest.mark.parametrize("d", [32, 64])
def test_bits_do_not_depend_on_the_batch_the_query_order_or_the_probe_order(d):
    ix = index_of(d)
    n, nprobe = 300, 3
    x_h = gauss(n, d, seed=300 + d)
    probes_h = random_probes(n, nprobe, seed=31)
    probes_h[:200, 0] = 6                                            # a crowded cell: its pairs fill more than one tile
    probes_h[:200, 1:] = np.stack([np.random.RandomState(i).permutation(6)[:2] for i in range(200)])
    _, x = guarded(x_h)
    _, probes = guarded(torch.from_numpy(probes_h))
    dist, idx = raw_ivf(ix, x, probes, 3)
    out = raw_ivf(ix, x, probes, 3, index=False)
    again = raw_ivf(ix, x, probes, 3)
    assert torch.equal(dist, again[0]) and torch.equal(idx, again[1])
    # the queries permuted, results permuted back
    order = torch.from_numpy(np.random.RandomState(1).permutation(n))
    _, xp = guarded(x_h[order])
    _, pp = guarded(torch.from_numpy(probes_h)[order])
    dp, ip = raw_ivf(ix, xp, pp, 3)
    op = raw_ivf(ix, xp, pp, 3, index=False)
    inv = torch.argsort(order).cuda()
    assert torch.equal(dp[inv], dist) and torch.equal(ip[inv], idx) and torch.equal(op[inv], out)
    # the batch cut in two calls
    cut = 171
    parts = []
    for sl in (slice(0, cut), slice(cut, n)):
        _, xs = guarded(x_h[sl])
        _, ps = guarded(torch.from_numpy(probes_h[sl]))
        parts.append(raw_ivf(ix, xs, ps, 3) + (raw_ivf(ix, xs, ps, 3, index=False),))
    assert torch.equal(torch.cat([p[0] for p in parts]), dist) and torch.equal(torch.cat([p[1] for p in parts]), idx)
    assert torch.equal(torch.cat([p[2] for p in parts]), out)
    # the entries of every probes row in another order
    shuffled = np.stack([row[np.random.RandomState(i).permutation(nprobe)] for i, row in enumerate(probes_h)])
    _, psh = guarded(torch.from_numpy(shuffled))
    ds, is_ = raw_ivf(ix, x, psh, 3)
    assert torch.equal(ds, dist) and torch.equal(is_, idx) and torch.equal(raw_ivf(ix, x, psh, 3, index=False), out)


def test_argument_errors_leave_the_outputs_untouched_and_the_search_does_not_synchronise():
    from self_supervised import _hip, ops
    L = _hip.lib()
    st = _hip.stream()
    ix = index_of(64)
    x = gauss(5, 64, 1).cuda()
    probes = torch.from_numpy(random_probes(5, 2, 3)).cuda()
    tiles, pairs = ops.ivf_schedule(probes, NLIST)
    part = torch.full((10, 3), -7, dtype=torch.int64, device="cuda")
    out = torch.full((5,), NAN, device="cuda")
    dist = torch.full((5, 3), NAN, device="cuda")
    idx = torch.full((5, 3), -7, dtype=torch.int32, device="cuda")
    cent = torch.full((NLIST, 64), NAN, device="cuda")
    P = lambda t: t.data_ptr()
    good = dict(x=P(x), bank=P(ix.sorted), bsq=P(ix.bsq_sorted), off=P(ix.offsets), perm=P(ix.perm), probes=P(probes), tiles=P(tiles),
                pairs=P(pairs), part=P(part), N=5, D=64, R=R, nlist=NLIST, nprobe=2, G=int(tiles.shape[1]), k=3)
    names = ("x", "bank", "bsq", "off", "perm", "probes", "tiles", "pairs", "part")
    bad = [{nm: None} for nm in names] + [dict(N=0), dict(D=48), dict(D=0), dict(D=65536 + 32), dict(R=0), dict(nlist=0), dict(nprobe=0),
                                          dict(G=0), dict(k=0), dict(k=4), dict(x=P(x) + 4), dict(part=P(part) + 4), dict(N=2 ** 31)]
    for change in bad:
        a = {**good, **change}
        ptrs = tuple(a[nm] for nm in names)
        nums = (a["N"], a["D"], a["R"], a["nlist"], a["nprobe"], a["G"], a["k"], st)
        assert L.ssad_l2_knn_ivf(*ptrs, P(out), *nums) == 2, change
        assert L.ssad_l2_knn_ivf_index(*ptrs, P(dist), P(idx), *nums) == 2, change
    ptrs = tuple(good[nm] for nm in names)
    nums = (5, 64, R, NLIST, 2, int(tiles.shape[1]), 3, st)
    assert L.ssad_l2_knn_ivf(*ptrs, None, *nums) == 2
    assert L.ssad_l2_knn_ivf_index(*ptrs, None, P(idx), *nums) == 2 and L.ssad_l2_knn_ivf_index(*ptrs, P(dist), None, *nums) == 2
    order = torch.arange(5, dtype=torch.int32, device="cuda")
    off = torch.tensor([0, 5] + [5] * (NLIST - 1), dtype=torch.int32, device="cuda")
    for args in ((None, P(order), P(off), P(cent), 5, NLIST, 64), (P(x), None, P(off), P(cent), 5, NLIST, 64),
                 (P(x), P(order), None, P(cent), 5, NLIST, 64), (P(x), P(order), P(off), None, 5, NLIST, 64),
                 (P(x), P(order), P(off), P(cent), 0, NLIST, 64), (P(x), P(order), P(off), P(cent), 5, 0, 64),
                 (P(x), P(order), P(off), P(cent), 5, 65536, 64), (P(x), P(order), P(off), P(cent), 5, NLIST, 0)):
        assert L.ssad_segment_means(*args, st) == 2, args
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(dist).all() and (idx == -7).all() and (part == -7).all() and torch.isnan(cent).all()
    # between the queries arriving and the scores leaving nothing waits for the device
    cents = gauss(NLIST, 64, 9).cuda()
    csq = ops.row_sqnorms(cents)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pr = ops.ivf_probes(x, cents, csq, 3)
        got = ops.l2_knn_ivf(x, ix.sorted, ix.bsq_sorted, ix.offsets, pr, ix.perm, 3)
        gd, gi = ops.l2_knn_ivf_index(x, ix.sorted, ix.bsq_sorted, ix.offsets, pr, ix.perm, 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(_mean_of(gd, 3), got.cpu())
    want = ref.probes64(x.cpu(), cents.cpu(), 3)                    # (gauss centroids: far apart)
    assert np.array_equal(pr.cpu().numpy(), want)


# ---------------------------------------------------------------- 5. segment_means

@pytest.mark.parametrize("d", [32, 100])
def test_segment_means(d):
    from self_supervised import ops
    lengths = (0, 1, 3, 1000, 0)
    n = sum(lengths)
    rows = gauss(n, d, seed=d) + 0.25
    order_h = torch.from_numpy(np.random.RandomState(d).permutation(n).astype(np.int32))
    offsets_h = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)
    xb, x = guarded(rows)
    ob, order = guarded(order_h)
    fb, offsets = guarded(offsets_h)
    prev = gauss(len(lengths), d, seed=d + 1)
    buf, out = guarded_out((len(lengths), d))
    out.copy_(prev)
    got = ops.segment_means(x, order, offsets, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and guards_intact(buf)
    want = ref.segment_means64(rows, order_h.numpy(), offsets_h.numpy(), prev)
    got_h = got.cpu()
    for g, length in enumerate(lengths):
        if length == 0:
            assert torch.equal(got_h[g], prev[g])                   # untouched
        else:
            err = np.abs(got_h[g].double().numpy() - want[g])
            assert (err <= np.spacing(np.abs(want[g]).astype(np.float32))).all(), (g, err.max())      # within 1 ulp of fp32
    again = ops.segment_means(x, order, offsets, out=prev.cuda())
    assert torch.equal(again, got)
    fresh = ops.segment_means(x, order, offsets)                    # no `out`: empty segments are zeros
    assert torch.equal(fresh[3], got[3]) and bool((fresh[0] == 0).all())


# ---------------------------------------------------------------- 6. kmeans_l2

def blobs(nlist, per, d, seed, spread=0.5, scale=6.0):
    centres = gauss(nlist, d, seed) * scale
    sizes = [per + 7 * i for i in range(nlist)]
    rows = torch.cat([centres[i] + spread * gauss(s, d, seed + 1 + i) for i, s in enumerate(sizes)])
    return rows[torch.from_numpy(np.random.RandomState(seed).permutation(rows.shape[0]))].contiguous()


@pytest.mark.parametrize("train_rows,seed", [(None, 5), (200, 4)])
def test_kmeans_matches_lloyd_in_float64(train_rows, seed):
    """Blobs whose centres are far apart against their spread, and seeds for which the reference's own assertion holds at every
    iteration: no row's two nearest centroids are nearer to each other than the bars of both (checked on the CPU, in assign64)."""
    from self_supervised import ops
    nlist, d, iters = 5, 32, 4
    rows = blobs(nlist, 100, d, seed=40)
    n = rows.shape[0]
    sample, init = ops.kmeans_init(n, nlist, seed=seed, train_rows=train_rows)
    assert (sample is None) == (train_rows is None)
    train = rows if sample is None else rows[sample]
    xb, x = guarded(rows)
    objs = []
    for it in range(iters + 1):                                     # a run of `it` iterations is the prefix of a longer one
        cent, assign = ops.kmeans_l2(x, nlist, iters=it, seed=seed, train_rows=train_rows)
        want_c, _, _ = ref.lloyd64(train, init.numpy(), it)         # asserts the separation at every iteration
        want_a, _ = ref.assign64(rows, want_c)
        assert assign.dtype == torch.int32 and np.array_equal(assign.cpu().numpy().astype(np.int64), want_a), it
        err = np.abs(cent.cpu().double().numpy() - want_c)
        assert (err <= np.spacing(np.abs(want_c).astype(np.float32))).all(), (it, err.max())
        objs.append(ref.objective64(train, cent.cpu()))
    assert (np.diff(objs) <= 0).all(), objs                         # the float64 objective never rises
    c2, a2 = ops.kmeans_l2(x, nlist, iters=iters, seed=seed, train_rows=train_rows)
    assert torch.equal(c2, cent) and torch.equal(a2, assign)        # the same seed: the same bits
    c3, _ = ops.kmeans_l2(x, nlist, iters=0, seed=seed + 1, train_rows=train_rows)
    assert not torch.equal(c3, ops.kmeans_l2(x, nlist, iters=0, seed=seed, train_rows=train_rows)[0])


def test_kmeans_keeps_the_centroid_of_a_cell_that_loses_its_rows():
    from self_supervised import ops
    one = gauss(1, 32, 50)
    rows = torch.cat([one.repeat(7, 1), gauss(1, 32, 51) + 9.0])     # seven equal rows and one far away, three cells
    _, init = ops.kmeans_init(8, 3, seed=0)
    equal_cells = [c for c, r in enumerate(init.tolist()) if r < 7]
    assert len(equal_cells) >= 2                                      # two cells start on equal rows: the larger one empties
    cent, assign = ops.kmeans_l2(rows.cuda(), 3, iters=3, seed=0)
    want_c, want_a, _ = ref.lloyd64(rows, init.numpy(), 3, check_bar=False)      # exact ties: the (d2, cell) rule decides both sides
    assert np.array_equal(assign.cpu().numpy().astype(np.int64), want_a)
    assert (np.abs(cent.cpu().double().numpy() - want_c) <= np.spacing(np.abs(want_c).astype(np.float32))).all()
    for c in equal_cells[1:]:
        assert c not in set(assign.cpu().tolist()) and torch.equal(cent[c].cpu(), one[0])
    with pytest.raises(ValueError, match="nlist must lie in 1..8"):
        ops.kmeans_l2(rows.cuda(), 9)


# ---------------------------------------------------------------- 7. the detector, on the rows of a synthetic category

def _tree(tmp_path, seeded_sd):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=96)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


def _run(ck, root, **more):
    from self_supervised import tools
    np.random.seed(3)
    torch.manual_seed(3)
    return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                           metric='euclidean', localization='dense', **more)


def _spy_fit(monkeypatch):
    from self_supervised.models import AnomalyDetector
    seen = {}
    orig = AnomalyDetector.fit

    def spy(self, embeddings, split=True, groups=None):
        seen["rows"], seen["groups"] = torch.as_tensor(embeddings).detach().cpu().clone(), groups
        orig(self, embeddings, split, groups)
        seen["det"] = self
    monkeypatch.setattr(AnomalyDetector, "fit", spy)
    return seen


def test_detector_with_an_index(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector
    root, ck = _tree(tmp_path, seeded_sd)
    seen = _spy_fit(monkeypatch)
    res = _run(ck, root)
    monkeypatch.undo()
    rows, groups = seen["rows"], seen["groups"]
    x_h = res.embedding_vectors.float()
    n_img = 4
    p = x_h.shape[0] // n_img
    kw = dict(patch_level=True, batch=n_img, num_patches=p, metric='euclidean')

    def fitted(**more):
        np.random.seed(5)
        det = AnomalyDetector(**kw, **more)
        det.fit(rows, groups=groups)
        return det

    flat = fitted()
    r = int(flat.bank.shape[0])
    every = fitted(index='ivf', nlist=6, nprobe=6)
    assert every.ivf["nlist"] == 6 and every.ivf["nprobe"] == 6 and int(every.ivf["offsets"][-1]) == r
    assert torch.equal(every.bank, flat.bank.index_select(0, every.ivf["perm"].long()))         # the same rows, cell after cell
    assert sorted(every.ivf["perm"].tolist()) == list(range(r))
    # every cell probed: threshold, maps and kneighbors of the flat detector, bit for bit
    assert every.threshold == flat.threshold
    maps_flat = flat.predict(x_h)
    assert torch.equal(every.predict(x_h), maps_flat)
    de, ie = every.kneighbors(x_h)
    df, if_ = flat.kneighbors(x_h)
    assert ie.dtype == torch.int64 and torch.equal(de, df) and torch.equal(ie, if_)
    assert fitted(index='ivf', nlist=6, nprobe=50).ivf["nprobe"] == 6                            # nprobe is clamped to nlist
    # the default nlist, two cells probed: the maps are ops.l2_knn_ivf on the detector's state, never below the exact ones
    two = fitted(index='ivf', nprobe=2)
    iv = two.ivf
    assert iv["nlist"] == int(np.ceil(np.sqrt(r))) and iv["nprobe"] == 2
    line = two.describe_fit()
    assert "nlist %d" % iv["nlist"] in line and "nprobe 2" in line and "empty" in line
    x = x_h.cuda()
    probes = ops.ivf_probes(x, iv["centroids"], iv["cent_sq"], 2)
    outside = ops.l2_knn_ivf(x, two.bank, two.bank_sq, iv["offsets"], probes, iv["perm"], 3)
    maps = two.predict(x_h)
    assert tuple(maps.shape) == tuple(maps_flat.shape) and torch.equal(maps.reshape(-1), outside)
    assert bool((maps >= maps_flat).all()) and bool(torch.isfinite(maps).all())
    assert two.threshold >= flat.threshold
    assert int(probes.min()) >= 0 and int(probes.max()) < iv["nlist"] and bool((probes[:, 0] != probes[:, 1]).all())
    dist, idx = two.kneighbors(x_h)
    assert torch.equal(_mean_of(dist, 3), maps.reshape(-1).cpu()) and int(idx.min()) >= 0 and int(idx.max()) < r
    assert torch.equal(two.image_scores(x_h, 'max'), maps.reshape(n_img, p).max(1).values)
    for mode in ('reweighted', 'retrieval'):
        with pytest.raises(ValueError, match="does not go with index='ivf'"):
            two.image_scores(x_h, mode)
    # the state round trip: equal bits
    other = AnomalyDetector(**kw, index='ivf', nprobe=2)
    other.load_state(two.state())
    assert torch.equal(other.bank_sq, two.bank_sq) and torch.equal(other.ivf["cent_sq"], iv["cent_sq"])
    assert torch.equal(other.predict(x_h), maps)
    do, io = other.kneighbors(x_h)
    assert torch.equal(do, dist) and torch.equal(io, idx)
    with pytest.raises(ValueError, match="this detector has 'flat'"):
        AnomalyDetector(**kw).load_state(two.state())
    with pytest.raises(ValueError, match="this detector has 'ivf'"):
        AnomalyDetector(**kw, index='ivf').load_state(flat.state())
    # image level: rows are images
    np.random.seed(6)
    img_flat = AnomalyDetector(metric='euclidean')
    img_flat.fit(rows[:300])
    np.random.seed(6)
    img_ivf = AnomalyDetector(metric='euclidean', index='ivf', nlist=4, nprobe=4)
    img_ivf.fit(rows[:300])
    assert img_ivf.threshold == img_flat.threshold and torch.equal(img_ivf.predict(x_h[:50]), img_flat.predict(x_h[:50]))


# ---------------------------------------------------------------- 8. through tools.inference

@pytest.mark.parametrize("coreset", [None, 0.1])
def test_inference_with_an_index(tmp_path, seeded_sd, monkeypatch, coreset):
    from self_supervised import tools
    root, ck = _tree(tmp_path, seeded_sd)
    seen = _spy_fit(monkeypatch)
    more = {} if coreset is None else {"coreset": coreset}
    before = _run(ck, root, **more)
    flat_det = seen["det"]
    assert flat_det.index == 'flat' and flat_det.ivf is None and sorted(flat_det.state()) == ["bank", "metric"]
    res = _run(ck, root, index='ivf', nprobe=3, image_scores='max', **more)
    det = seen["det"]
    r = int(det.bank.shape[0])
    assert det.index == 'ivf' and det.ivf["nprobe"] == 3 and det.ivf["nlist"] == int(np.ceil(np.sqrt(r))) and r == flat_det.bank.shape[0]
    assert torch.equal(det.bank, flat_det.bank.index_select(0, det.ivf["perm"].long()))         # the rows the split / coreset kept
    if coreset is not None:
        assert det.coreset_counts[0] == r and r < det.coreset_counts[1]
    maps = res.anomaly_maps
    assert maps.shape == before.anomaly_maps.shape and maps.dtype == before.anomaly_maps.dtype and torch.isfinite(maps).all()
    assert bool((maps >= before.anomaly_maps).all())                # fewer candidates: never nearer than the whole bank
    assert torch.equal(res.embedding_vectors, before.embedding_vectors)
    assert torch.equal(res.image_scores, maps.reshape(4, -1).max(1).values)
    # on through upsample and the Evaluator
    res.anomaly_maps = tools.upsample(maps, int(res.ground_truths.shape[-1]), verbose=False)
    ev = tools.Evaluator(evaluation_metrics=['auroc', 'aupro', 'iou'])
    ev.evaluate(res, "bottle", str(tmp_path / "out") + "/", patch_level=True)
    assert ev.scores.auroc is not None and np.isfinite(ev.scores.auroc)
    # index='flat' is not passing it, also after an index call
    again = _run(ck, root, index='flat', **more)
    assert torch.equal(before.anomaly_maps, again.anomaly_maps) and torch.equal(before.embedding_vectors, again.embedding_vectors)


# ---------------------------------------------------------------- 9. two gloo ranks equal one rank

def test_two_ranks_equal_one_rank(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import tools
    root, ck = _tree(tmp_path, seeded_sd)
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "knn_ivf"])
    assert r["equal_across_ranks"] and r["world"] == 2, r
    two = torch.load(str(tmp_path / "ivf_rank0.pt"))
    from self_supervised.models import AnomalyDetector
    seen = {}
    orig = AnomalyDetector.predict

    def spy(self, x):
        seen["threshold"] = self.threshold
        return orig(self, x)
    monkeypatch.setattr(AnomalyDetector, "predict", spy)
    one = two_rank_util.inference(tools, ck, root, "knn_ivf")
    assert torch.equal(two["scores"], one.image_scores) and torch.equal(two["maps"], one.anomaly_maps)
    assert two["threshold"] == seen["threshold"] and np.isfinite(seen["threshold"])
