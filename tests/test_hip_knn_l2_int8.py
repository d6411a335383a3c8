"""GPU tests of the flat Euclidean search on an 8-bit scalar-quantised bank: csrc/knn_l2_int8.hip (ssad_rows_to_int8,
ssad_l2q_knn_fused / _index) and its way through AnomalyDetector(bank_dtype='int8') and tools.inference.  The reference everywhere is
tests/knn_l2_int8_ref.py: the codes by the fp32 expression, D2 in int64, neighbours by a stable argsort of (D2, row).

The bars.  Codes, their squared norms and every index are EQUAL to the reference: all of them are integers.  excess: the squared-norm
bar of the neighbouring tests, (D + 2) units of 2^-24 of the float64 sum (a chain of D fused multiply-adds and the butterfly).  A
distance: 4 fp32 ulp of the float64 evaluation of sqrt(s2 D2 + excess) with the excess the search was given -- the conversion of D2
(up to 2^31), the fused multiply-add and the root are three roundings, the root halving what came before it: under 2 ulp.  The mean
form: the bits of the sequential fp32 mean of the index form's own row.

Measured (one run on one MI355X, the tests print it per case): excess at most 1.34 units of 2^-24 of itself (bound D + 2); distances at
most 0.85 ulp from float64 at every D."""
import numpy as np
import pytest
import torch

import coreset_ref
import knn_l2_int8_ref as qref
import two_rank_util
from fake_mvtec import make_tree
from knn_paths_util import fp32_rows_held

pytestmark = pytest.mark.gpu

NAN = float("nan")
N_TRAIN = 8
ULPS = 4.0
F = np.float32


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


def rand_codes(n, d, seed, lo=-128, hi=128):
    return torch.from_numpy(np.random.RandomState(seed).randint(lo, hi, size=(n, d)).astype(np.int8))


def guarded(t, fill):
    """A device copy of t as a view between two guard rows of `fill`."""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    buf[1:-1] = t
    buf = buf.cuda()
    return buf, buf[1:-1]


def guarded_out(shape, dtype=torch.float32):
    """(whole buffer, view): an output between two guard rows, the whole buffer poisoned; floats are NaN-filled, ints hold -7."""
    fill = NAN if dtype.is_floating_point else -7
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
    return buf, buf[1:-1]


def guards_intact(buf):
    g = torch.stack([buf[0].reshape(-1), buf[-1].reshape(-1)])
    return bool(torch.isnan(g).all()) if buf.dtype.is_floating_point else bool((g == -7).all())


def raw_to_int8(rows, lo, inv_s, s):
    """ssad_rows_to_int8 from a guarded fp32 input into guarded, poisoned outputs: (codes, sq, excess) views."""
    from self_supervised import _hip
    L = _hip.lib()
    n, d = rows.shape
    xbuf, x = guarded(rows, NAN)
    cbuf, codes = guarded_out((n, d), torch.int8)
    sbuf, sq = guarded_out((n,), torch.int32)
    ebuf, ex = guarded_out((n,))
    rc = L.ssad_rows_to_int8(x.data_ptr(), codes.data_ptr(), sq.data_ptr(), ex.data_ptr(), n, d, float(lo), float(inv_s), float(s),
                             _hip.stream())
    assert rc == 0, L.ssad_last_error()
    torch.cuda.synchronize()
    assert guards_intact(cbuf) and guards_intact(sbuf) and guards_intact(ebuf) and guards_intact(xbuf)
    return codes, sq, ex


class Side:
    """Codes on the device between guard rows of code 0x55 / norm -7 / excess NaN, with their int32 norms."""

    def __init__(self, codes, excess=None):
        self.host = codes.numpy()
        self.cbuf, self.codes = guarded(codes, 0x55)
        self.sbuf, self.sq = guarded(torch.from_numpy(qref.sq64(self.host).astype(np.int32)), -7)
        ex = torch.zeros(codes.shape[0]) if excess is None else excess
        self.ex_host = ex.double().numpy()
        self.ebuf, self.ex = guarded(ex, NAN)


def raw_knn(x, b, k, s2, splits=1, index=False):
    """The C entry points on caller-owned, guarded, poisoned outputs."""
    from self_supervised import _hip
    L = _hip.lib()
    n, d = x.codes.shape
    r = b.codes.shape[0]
    st = _hip.stream()
    P = lambda t: t.data_ptr()
    part = None
    if index:
        dbuf, dist = guarded_out((n, k))
        ibuf, idx = guarded_out((n, k), torch.int32)
        if splits > 1:
            part = torch.full((splits, n, 3), -7, dtype=torch.int64, device="cuda")
        rc = L.ssad_l2q_knn_index(P(x.codes), P(x.sq), P(x.ex), P(b.codes), P(b.sq), None if part is None else P(part), P(dist), P(idx),
                                  n, d, r, k, splits, float(s2), st)
        assert rc == 0, L.ssad_last_error()
        torch.cuda.synchronize()
        assert guards_intact(dbuf) and guards_intact(ibuf)
        return dist.cpu(), idx.cpu()
    obuf, out = guarded_out((n,))
    if splits > 1:
        part = torch.full((splits, n, 3), -7, dtype=torch.int32, device="cuda")
    rc = L.ssad_l2q_knn_fused(P(x.codes), P(x.sq), P(x.ex), P(b.codes), P(b.sq), None if part is None else P(part), P(out), n, d, r, k,
                              splits, float(s2), st)
    assert rc == 0, L.ssad_last_error()
    torch.cuda.synchronize()
    assert guards_intact(obuf)
    return out.cpu()


def check_search(x, b, k, s2, d2_all, splits=(1, 2, 3, 7), label=""):
    """idx equal to the stable sort's, dist within ULPS of float64, the mean form the bits of the index row's mean; a second call and
    every split count bit-equal.  Returns the largest distance error in ulp."""
    want_d2, want_i = qref.kneighbors(d2_all, k)
    want_d = qref.dist64(want_d2, F(s2), x.ex_host)
    dist, idx = raw_knn(x, b, k, s2, 1, index=True)
    out = raw_knn(x, b, k, s2, 1)
    assert np.array_equal(idx.numpy().astype(np.int64), want_i), label
    err = qref.ulps32(dist.numpy(), want_d).max()
    assert err <= ULPS, (label, err)
    assert np.array_equal(qref.mean_of(dist, k).view(np.int32), out.numpy().view(np.int32)), label
    again_d, again_i = raw_knn(x, b, k, s2, 1, index=True)
    assert torch.equal(dist.view(torch.int32), again_d.view(torch.int32)) and torch.equal(idx, again_i), label
    for s in splits:
        if s == 1:
            continue
        ds, is_ = raw_knn(x, b, k, s2, s, index=True)
        os_ = raw_knn(x, b, k, s2, s)
        assert torch.equal(ds.view(torch.int32), dist.view(torch.int32)) and torch.equal(is_, idx), (label, s)
        assert torch.equal(os_.view(torch.int32), out.view(torch.int32)), (label, s)
    return err


# ---------------------------------------------------------------- 1. the quantiser pass

def boundary_rows(n, d):
    """lo = 0, s = 1: values on the .5 code boundaries and one fp32 step to either side, at lo and hi, below and above, NaN."""
    rng = np.random.RandomState(n * 1000 + d)
    k = rng.randint(0, 255, size=(n, d)).astype(F)
    x = k + F(0.5)
    side = rng.randint(0, 3, size=(n, d))
    x = np.where(side == 1, np.nextafter(x, F(-1e9)), np.where(side == 2, np.nextafter(x, F(1e9)), x)).astype(F)
    flat = x.reshape(-1)
    special = np.array([0.0, 255.0, -0.0, -1.0, -1e-10, 256.0, 255.00002, 3e18, -3e18, np.nan, 254.5, 0.5, 1.5, 2.5, 127.5, 128.5], dtype=F)
    for i, v in enumerate(special):                                     # spread over the rows: the NaN's row is not the only one outside
        flat[(i * (flat.size // special.size) + 5) % flat.size] = v
    return torch.from_numpy(flat.reshape(n, d))


@pytest.mark.parametrize("d", [32, 96, 384, 448])
def test_rows_to_int8(d):
    from self_supervised import ops
    worst = 0.0
    for n in (1, 7, 8, 9, 300):
        cases = [("boundaries", boundary_rows(n, d), qref.quantiser(0.0, 255.0))]
        g = gauss(n, d, seed=d + n) * 0.7 + 0.3
        wide = g.clone()
        wide[n // 2, :: 3] *= 4.0                                       # one row leaves the range of the others
        cases.append(("gauss", wide, qref.quantiser_of(g)))
        cases.append(("hi == lo", torch.full((n, d), 3.25) + (torch.arange(d) == 1).float() * 2.0, qref.quantiser(3.25, 3.25)))
        for name, rows, (lo, s, inv_s, _) in cases:
            if n == 300:
                rows[17] = rows[3]
                rows[299] = rows[3]
            codes, sq, ex = raw_to_int8(rows, lo, inv_s, s)
            want = qref.codes(rows, lo, inv_s)
            assert codes.dtype == torch.int8 and np.array_equal(codes.cpu().numpy(), want), (name, n, d)
            assert sq.dtype == torch.int32 and np.array_equal(sq.cpu().numpy().astype(np.int64), qref.sq64(want)), (name, n, d)
            e64 = qref.excess64(rows, lo, s)
            got = ex.cpu().double().numpy()
            nan = np.isnan(e64)
            assert np.array_equal(np.isnan(got), nan), (name, n, d)     # a row with a NaN has a NaN excess, and no other row
            assert (got[(e64 == 0) & ~nan] == 0).all()                  # rows inside the range: exactly 0
            err = np.abs(got - e64)[~nan] / (2.0 ** -24 * np.maximum(e64[~nan], 1e-300))
            worst = max(worst, float(err.max()) if err.size else 0.0)
            assert (err <= d + 2).all(), (name, n, d, err.max())
            if name == "boundaries":
                assert nan.sum() >= 1 and (want[np.isnan(rows.numpy())] == -128).all()
                assert n == 1 or (e64[~nan] > 0).any()
            if name == "hi == lo":
                assert (want[:, 0] == -128).all() and (want[:, 1] == -126).all() and (e64 == 0).all()
            if n == 300:
                b = ex.cpu().view(torch.int32)
                assert b[17] == b[3] and b[299] == b[3]                 # equal rows, equal bits wherever they stand
                wc, wsq, wex = ops.rows_to_int8(rows.cuda(), float(lo), float(inv_s), float(s))      # the wrapper: the same bits
                assert torch.equal(wc, codes) and torch.equal(wsq, sq) and torch.equal(wex.view(torch.int32), ex.view(torch.int32))
    print(f"D={d}: worst |excess - float64| / (2^-24 excess) = {worst:.3f} (bound D + 2 = {d + 2})")


# ---------------------------------------------------------------- 2. the search against the reference

NS = (1, 127, 128, 129, 300)
RS = (3, 127, 128, 129, 257, 1000)


@pytest.mark.parametrize("d", [32, 64, 96, 384, 448])
def test_search_equals_the_reference(d):
    """Every N x R x k x splits of the issue on random codes over the whole int8 range; queries carry a random excess (half of them
    0) and the scale an arbitrary fp32 s2."""
    s2 = F(0.0123) * F(0.0123)
    worst = 0.0
    xs = {}
    for n in NS:
        ex = torch.from_numpy(np.random.RandomState(n).uniform(0, 50, size=n).astype(F))
        ex[::2] = 0.0
        xs[n] = Side(rand_codes(n, d, seed=1000 + d + n), ex)
    for r in RS:
        b = Side(rand_codes(r, d, seed=2000 + d + r))
        for n in NS:
            d2_all = qref.d2_blas(xs[n].host, b.host)
            for k in (1, 2, 3):
                worst = max(worst, check_search(xs[n], b, k, s2, d2_all, label=f"D={d} N={n} R={r} k={k}"))
    print(f"D={d}: worst |dist - float64| = {worst:.3f} ulp")


@pytest.mark.parametrize("d", [32, 64, 96])
def test_operand_maps_with_asymmetric_codes(d):
    """Query code = f(row, column), bank code = another function of (row, column), neither symmetric: a swapped row / column or a
    permuted k changes D2.  R = 3, k = 3 returns every D2 of the tile's first rows; s2 = 1 and excess 0 make dist^2 = D2 < 2^21, so
    D2 itself is recovered exactly.  R = 257 checks the winners over three bank tiles."""
    n = 300
    i, j = np.meshgrid(np.arange(n), np.arange(d), indexing="ij")
    xq = torch.from_numpy((((i * 7 + j * 3 + (i * j) % 5) % 61) - 30).astype(np.int8))
    for r in (3, 257):
        bi, bj = np.meshgrid(np.arange(r), np.arange(d), indexing="ij")
        bq = torch.from_numpy((((bi * 5 + bj * 11 + bi * bj) % 53) - 26).astype(np.int8))
        x, b = Side(xq), Side(bq)
        d2_all = qref.d2_int(x.host, b.host)
        assert d2_all.max() < 2 ** 21                               # the fp32 root squared stays within 1/4 of D2
        for k in (1, 3):
            check_search(x, b, k, 1.0, d2_all, splits=(1, 2), label=f"D={d} R={r} k={k}")
        dist, idx = raw_knn(x, b, 3, 1.0, index=True)
        got_d2 = np.rint(dist.double().numpy() ** 2).astype(np.int64)
        assert np.array_equal(got_d2, np.take_along_axis(d2_all, idx.numpy().astype(np.int64), 1))
        assert np.array_equal(got_d2, qref.kneighbors(d2_all, 3)[0])


@pytest.mark.parametrize("d", [32, 384])
def test_ties_go_to_the_smaller_row(d):
    """Five distinct rows repeated over 1000 bank rows: almost every D2 ties, across lane halves, waves, tiles and splits."""
    distinct = rand_codes(5, d, seed=3, lo=-20, hi=21)
    which = np.random.RandomState(4).randint(0, 5, size=1000)
    b = Side(distinct[torch.from_numpy(which)])
    x = Side(torch.cat([rand_codes(172, d, seed=5, lo=-20, hi=21), distinct[torch.from_numpy(which[:128])]]))
    d2_all = qref.d2_blas(x.host, b.host)
    assert (np.sort(d2_all, axis=1)[:, 0] == np.sort(d2_all, axis=1)[:, 2]).mean() > 0.9
    for k in (1, 2, 3):
        check_search(x, b, k, 1.0, d2_all, label=f"ties D={d} k={k}")


def test_largest_width_and_largest_squared_distance():
    """D = 32768: queries of code -128 against rows of code 127 give D2 = 32768 * 255^2 = 2 130 739 200 < 2^31, exactly."""
    d = 32768
    xq = torch.full((2, d), -128, dtype=torch.int8)
    bq = torch.full((4, d), 127, dtype=torch.int8)
    bq[1, ::2] = 126
    bq[2, :100] = -128
    bq[3] = rand_codes(1, d, seed=1)[0]
    x, b = Side(xq), Side(bq)
    d2_all = qref.d2_blas(x.host, b.host)
    assert d2_all[0, 0] == 32768 * 65025 and np.array_equal(d2_all, qref.d2_int(x.host, b.host))
    for k in (1, 2, 3):
        check_search(x, b, k, 1.0, d2_all, splits=(1, 2), label=f"D={d} k={k}")
    dist, idx = raw_knn(x, Side(bq[:1]), 1, 1.0, index=True)
    assert idx[0, 0] == 0 and qref.ulps32(dist.numpy(), np.sqrt(np.float64(32768 * 65025))).max() <= ULPS


@pytest.mark.parametrize("n,r", [(129, 129), (300, 257), (5, 1), (130, 2), (3, 3)])
def test_padded_rows_never_win(n, r):
    """Queries of small codes against bank rows of large codes: a padded row (it reads code 0) would be nearer than any real row.
    The last real row is the nearest; k = R where R <= 3."""
    d = 96
    xq = rand_codes(n, d, seed=n, lo=-3, hi=4)
    bq = rand_codes(r, d, seed=r, lo=60, hi=128)
    bq[-1] = 40
    x, b = Side(xq), Side(bq)
    d2_all = qref.d2_blas(x.host, b.host)
    assert (d2_all.argmin(1) == r - 1).all() and d2_all.min() > qref.sq64(x.host).max()
    for k in range(1, min(r, 3) + 1):
        check_search(x, b, k, 0.25, d2_all, label=f"N={n} R={r} k={k}")
        dist, idx = raw_knn(x, b, k, 0.25, index=True)
        assert (idx[:, 0] == r - 1).all() and idx.min() >= 0 and idx.max() < r


def test_argument_errors_leave_the_outputs_untouched():
    from self_supervised import _hip, ops
    L = _hip.lib()
    st = _hip.stream()
    x, b = Side(rand_codes(5, 64, 1)), Side(rand_codes(4, 64, 2))
    out = torch.full((5,), NAN, device="cuda")
    dist = torch.full((5, 3), NAN, device="cuda")
    idx = torch.full((5, 3), -7, dtype=torch.int32, device="cuda")
    part = torch.full((2, 5, 3), -7, dtype=torch.int64, device="cuda")
    P = lambda t: t.data_ptr()
    good = (P(x.codes), P(x.sq), P(x.ex), P(b.codes), P(b.sq))
    fused = lambda a, pt, o, n, d, r, k, s: L.ssad_l2q_knn_fused(*a, pt, o, n, d, r, k, s, 1.0, st)
    index = lambda a, pt, dd, ii, n, d, r, k, s: L.ssad_l2q_knn_index(*a, pt, dd, ii, n, d, r, k, s, 1.0, st)
    bad = [tuple(None if j == i else g for j, g in enumerate(good)) + (5, 64, 4, 3, 1) for i in range(5)]
    bad += [good + (5, 48, 4, 3, 1), good + (5, 32768 + 32, 4, 3, 1), good + (5, 64, 4, 0, 1), good + (5, 64, 4, 4, 1), good + (5, 64, 2, 3, 1),
            good + (0, 64, 4, 3, 1), good + (5, 0, 4, 3, 1), good + (5, 64, 0, 1, 1), good + (5, 64, 4, 3, 0), good + (5, 64, 4, 3, 65536),
            (good[0] + 8,) + good[1:] + (5, 64, 4, 3, 1), good[:3] + (good[3] + 4,) + good[4:] + (5, 64, 4, 3, 1)]
    for *a, n, d, r, k, s in bad:
        for pt in (None, P(part)):
            assert fused(a, pt, P(out), n, d, r, k, s) == 2, (n, d, r, k, s)
            assert index(a, pt, P(dist), P(idx), n, d, r, k, s) == 2, (n, d, r, k, s)
    assert fused(good, None, None, 5, 64, 4, 3, 1) == 2
    assert index(good, None, None, P(idx), 5, 64, 4, 3, 1) == 2 and index(good, None, P(dist), None, 5, 64, 4, 3, 1) == 2
    assert fused(good, None, P(out), 5, 64, 4, 3, 2) == 2 and index(good, None, P(dist), P(idx), 5, 64, 4, 3, 2) == 2      # S > 1, no workspace
    assert fused(good, P(part) + 4, P(out), 5, 64, 4, 3, 2) == 2 and b"8-byte" in L.ssad_last_error()
    assert index(good, P(part) + 4, P(dist), P(idx), 5, 64, 4, 3, 2) == 2
    assert index(good, None, P(dist), P(idx), 5, 64, 2, 3, 1) == 2 and b"k in 1..3" in L.ssad_last_error()
    assert fused(good, None, P(out), 5, 32768 + 32, 4, 3, 1) == 2 and b"32768" in L.ssad_last_error()
    src = gauss(5, 64, 1).cuda()
    codes = torch.full((5, 64), -7, dtype=torch.int8, device="cuda")
    sq = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    ex = torch.full((5,), NAN, device="cuda")
    ok = (P(src), P(codes), P(sq), P(ex))
    for args in [tuple(None if j == i else g for j, g in enumerate(ok)) + (5, 64) for i in range(4)] + \
                [ok + (5, 48), ok + (0, 64), ok + (5, 0), ok + (5, 32768 + 32), (ok[0] + 4,) + ok[1:] + (5, 64), (ok[0], ok[1] + 4) + ok[2:] + (5, 64)]:
        assert L.ssad_rows_to_int8(*args, 0.0, 1.0, 1.0, st) == 2, args[4:]
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(dist).all() and (idx == -7).all() and (part == -7).all()
    assert (codes == -7).all() and (sq == -7).all() and torch.isnan(ex).all()
    with pytest.raises(ValueError, match="fewer than k"):
        ops.l2q_knn_index(src, b.codes[:2], b.sq[:2], (0.0, 1.0), 3)


# ---------------------------------------------------------------- 3. the detector

def _reference_scores(x, rows, quant, k, excess=None):
    """float64 patch scores, (D2, idx) of the k nearest and the excess of the queries x against the fp32 bank rows, by the reference."""
    lo, s, inv_s, s2 = quant
    xc, bc = qref.codes(x, lo, inv_s), qref.codes(rows, lo, inv_s)
    d2, idx = qref.kneighbors(qref.d2_blas(xc, bc), k)
    ex = qref.excess64(x, lo, s) if excess is None else excess
    return qref.dist64(d2, s2, ex), idx, ex


def _score_tol(d64, ex, d):
    """|score - float64| allowed: ULPS on each distance, plus what the excess bar ((D + 2) 2^-24 excess, under the root: half of it
    relative to d) lets through, plus the two roundings of the mean."""
    spacing = np.spacing(d64.astype(F)).astype(np.float64)
    per = ULPS * spacing + 0.5 * (d + 2) * 2.0 ** -24 * ex[:, None] / np.maximum(d64, 1e-300)
    return per.mean(1) + 4 * 2.0 ** -24 * d64.mean(1)


@pytest.mark.parametrize("coreset", [None, 0.1])
@pytest.mark.parametrize("patch_level", [False, True])
def test_detector_against_the_reference(coreset, patch_level):
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector, coreset_projection
    d = 64
    emb = gauss(900, d, seed=3) * 0.5 + gauss(1, d, seed=4)
    np.random.seed(5)
    level = dict(patch_level=True, batch=2, num_patches=100) if patch_level else {}
    det = AnomalyDetector(coreset=coreset, coreset_dim=32, metric='euclidean', bank_dtype='int8', **level)
    det.fit(emb)
    np.random.seed(5)
    perm = np.random.permutation(900)
    tr, va = perm[270:], perm[:270]
    rows = emb[tr]
    if coreset is not None:
        proj = (rows.cuda() @ coreset_projection(d, 32).cuda()).cpu()               # the selection runs on the fp32 rows
        sel, rad = det.coreset_rows
        m = int(np.ceil(0.1 * 630))
        assert det.coreset_counts == (m, 630) and sel.shape[0] == m
        want_sel, _ = coreset_ref.greedy64(proj.double().numpy(), m)
        assert np.array_equal(sel.cpu().numpy(), want_sel)
        rows = rows[sel.cpu()]
    quant = qref.quantiser_of(rows)                                                 # lo / hi of the rows that are kept
    lo, s, inv_s, s2 = quant
    assert det.quant == (float(lo), float(s)) and fp32_rows_held(det) == []
    assert det.bank.dtype == torch.int8 and det.bank_sq.dtype == torch.int32
    bc = qref.codes(rows, lo, inv_s)
    assert np.array_equal(det.bank.cpu().numpy(), bc) and np.array_equal(det.bank_sq.cpu().numpy().astype(np.int64), qref.sq64(bc))
    assert bc.min() == -128 and bc.max() == 127
    x = gauss(200, d, seed=9) * 0.5 + gauss(1, d, seed=4)
    x[150:] *= 3.0                                                                  # these leave the bank's range
    _, _, dev_ex = ops.rows_to_int8(x.cuda(), float(lo), float(inv_s), float(s))
    want_d, want_i, ex = _reference_scores(x, rows, quant, 3)
    assert (ex[:150] == 0).mean() > 0.9 and (ex[150:] > 0).all()
    got = det.predict(x).reshape(-1).cpu().double().numpy()
    assert (np.abs(got - want_d.mean(1)) <= _score_tol(want_d, ex, d)).all()
    assert (got >= np.sqrt(ex) * (1 - (d + 4) * 2.0 ** -24)).all()                  # an out-of-range query scores at least sqrt(excess)
    assert (got[150:] >= np.sqrt(dev_ex.cpu().double().numpy()[150:]) * (1 - 2.0 ** -22)).all()
    if patch_level:
        assert tuple(det.predict(x).shape) == (2, 1, 10, 10)
    thr_d, _, thr_ex = _reference_scores(emb[va], rows, quant, 3)
    assert abs(det.threshold - thr_d.mean(1).max()) <= _score_tol(thr_d, thr_ex, d).max()
    dist, idx = det.kneighbors(x)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want_i)
    exact_d = qref.dist64(qref.kneighbors(qref.d2_blas(qref.codes(x, lo, inv_s), bc), 3)[0], s2, dev_ex.cpu().double().numpy())
    assert qref.ulps32(dist.cpu().numpy(), exact_d).max() <= ULPS                   # with the device's own excess: the search's bar
    assert np.array_equal(qref.mean_of(dist.cpu(), 3).view(np.int32), det.predict(x).reshape(-1).cpu().numpy().view(np.int32))
    for k in (1, 2):
        dk, ik = det.kneighbors(x, k)
        assert torch.equal(dk, dist[:, :k]) and torch.equal(ik, idx[:, :k])
    with pytest.raises(ValueError, match="k must be 1, 2 or 3"):
        det.kneighbors(x, 4)
    # state / load_state: codes, integer norms, lo and s travel; nothing is recomputed
    state = det.state()
    assert state["bank"].dtype == torch.int8 and state["bank_dtype"] == 'int8' and state["bank_sq"].dtype == torch.int32
    assert (state["lo"], state["s"]) == det.quant
    other = AnomalyDetector(metric='euclidean', bank_dtype='int8', **level)
    other.load_state(state)
    assert torch.equal(other.bank, det.bank) and torch.equal(other.bank_sq, det.bank_sq) and other.quant == det.quant
    assert torch.equal(other.predict(x), det.predict(x))
    with pytest.raises(ValueError, match="fitted with bank_dtype='int8'"):
        AnomalyDetector(metric='euclidean', **level).load_state(state)
    flat = det.predict(x).reshape(-1)
    det.patch_level, det.dim = True, 10                                             # image_scores('max') on the same scores
    assert torch.equal(det.image_scores(x, 'max'), flat.reshape(2, 100).max(1).values)
    with pytest.raises(ValueError, match="takes image_scores None or 'max'"):
        det.image_scores(x, 'reweighted')


def test_non_finite_bank_is_refused():
    from self_supervised.models import AnomalyDetector
    emb = gauss(50, 32, seed=1)
    emb[7, 3] = float("inf")
    with pytest.raises(ValueError, match="must be finite"):
        AnomalyDetector(metric='euclidean', bank_dtype='int8').fit_bank(emb)
    emb[7, 3] = float("nan")
    with pytest.raises(ValueError, match="must be finite"):
        AnomalyDetector(metric='euclidean', bank_dtype='int8').fit_bank(emb)


@pytest.mark.parametrize("bank_dtype", ['float32', 'float16'])
def test_other_bank_dtypes_reach_the_entry_points_they_reached(monkeypatch, bank_dtype):
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector
    names = []
    orig = ops._run

    def spy(kernel, *a, **kw):
        names.append(kernel)
        return orig(kernel, *a, **kw)
    monkeypatch.setattr(ops, "_run", spy)
    det = AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype)
    np.random.seed(1)
    det.fit(gauss(400, 64, seed=2))
    x = gauss(50, 64, seed=3)
    det.predict(x)
    det.kneighbors(x)
    want = {'float32': {"row_sqnorms", "l2_knn_fused", "l2_knn_index"},
            'float16': {"rows_to_half", "l2h_knn_fused", "l2h_knn_index"}}[bank_dtype]
    assert set(names) == want, names
    assert not hasattr(det, "quant")
    names.clear()
    q = AnomalyDetector(metric='euclidean', bank_dtype='int8')
    np.random.seed(1)
    q.fit(gauss(400, 64, seed=2))
    q.predict(x)
    q.kneighbors(x)
    assert set(names) == {"rows_to_int8", "l2q_knn_fused", "l2q_knn_index"}, names


# ---------------------------------------------------------------- 4. through tools.inference

def _tree(tmp_path, seeded_sd):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=96)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


@pytest.mark.parametrize("localization", ["patches", "dense"])
def test_inference_int8_bank_equals_the_detector_called_by_hand(tmp_path, seeded_sd, monkeypatch, localization):
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector
    root, ck = _tree(tmp_path, seeded_sd)
    seen = {}
    orig = AnomalyDetector.fit_bank

    def spy(self, bank):
        seen["rows32"] = torch.as_tensor(bank).detach().float().cpu().clone()
        orig(self, bank)
        seen["det"] = self
    monkeypatch.setattr(AnomalyDetector, "fit_bank", spy)

    def run(**more):
        np.random.seed(3)
        torch.manual_seed(3)
        return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, localization=localization,
                               bank='train', image_scores='max', metric='euclidean', **more)

    before = run()
    assert seen["det"].bank.dtype == torch.float32
    res = run(bank_dtype='int8')
    det, rows32 = seen["det"], seen["rows32"]
    assert det.bank_dtype == 'int8' and det.bank.dtype == torch.int8 and fp32_rows_held(det) == []
    rows = res.embedding_vectors.float()
    assert torch.equal(rows, before.embedding_vectors.float()) and rows.shape[1] % 32 == 0
    hand = AnomalyDetector(metric='euclidean', bank_dtype='int8')
    monkeypatch.setattr(AnomalyDetector, "fit_bank", orig)
    hand.fit_bank(rows32)
    assert hand.quant == det.quant and torch.equal(hand.bank, det.bank) and torch.equal(hand.bank_sq, det.bank_sq)
    maps = res.anomaly_maps
    assert torch.equal(hand.predict(rows).cpu(), maps.reshape(-1).cpu())
    assert hand.kneighbors(rows)[1].max() < rows32.shape[0]
    lo, s, inv_s, s2 = quant = qref.quantiser_of(rows32)
    assert det.quant == (float(lo), float(s))
    want_d, _, ex = _reference_scores(rows, rows32, quant, 3)
    got = maps.reshape(-1).double().numpy()
    print(f"{localization}: max |map - reference| = {np.abs(got - want_d.mean(1)).max():.3e} (values ~ {want_d.max():.3e})")
    assert (np.abs(got - want_d.mean(1)) <= _score_tol(want_d, ex, rows.shape[1])).all()
    assert maps.shape == before.anomaly_maps.shape and maps.dtype == before.anomaly_maps.dtype
    assert not torch.equal(maps, before.anomaly_maps)                               # the distances are those between the codes
    p = rows.shape[0] // 4
    assert torch.equal(res.image_scores, maps.reshape(4, p).max(1).values)
    monkeypatch.setattr(AnomalyDetector, "fit_bank", spy)
    for other in (run(), run(bank_dtype='float32')):                                # the default after an int8 call: the bits before it
        assert seen["det"].bank.dtype == torch.float32
        assert torch.equal(before.anomaly_maps, other.anomaly_maps) and torch.equal(before.image_scores, other.image_scores)


# ---------------------------------------------------------------- 5. two gloo ranks equal one rank

def test_two_ranks_equal_one_rank(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import tools
    root, ck = _tree(tmp_path, seeded_sd)
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "knn_l2_int8"])
    assert r["equal_across_ranks"] and r["world"] == 2, r
    two = torch.load(str(tmp_path / "l2q_rank0.pt"))
    from self_supervised.models import AnomalyDetector
    seen = {}
    orig = AnomalyDetector.predict

    def spy(self, x):
        seen.update(threshold=self.threshold, bank=self.bank.cpu(), bank_sq=self.bank_sq.cpu(), quant=self.quant)
        return orig(self, x)
    monkeypatch.setattr(AnomalyDetector, "predict", spy)
    one = two_rank_util.inference(tools, ck, root, "knn_l2_int8")
    assert torch.equal(two["scores"], one.image_scores) and torch.equal(two["maps"], one.anomaly_maps)
    assert two["bank"].dtype == torch.int8 and torch.equal(two["bank"], seen["bank"]) and torch.equal(two["bank_sq"], seen["bank_sq"])
    assert tuple(two["quant"]) == tuple(seen["quant"])
    assert two["threshold"] == seen["threshold"] and np.isfinite(seen["threshold"])
