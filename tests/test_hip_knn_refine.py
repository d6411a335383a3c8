"""GPU tests of the refined search: csrc/knn_refine.hip (ssad_rerank_l2 / _index, ssad_topk_l2q_index) and its way through
AnomalyDetector(bank_dtype='float16' | 'int8', refine=r) and tools.inference.  The references are tests/knn_refine_ref.py (float64
re-rank, stable sort by (d2, row, place)) and tests/knn_l2_int8_ref.py (exact integer D2).

The bars.  Every index of the int8 top-k equals the integer reference.  A re-rank distance has the bits of sqrt(ops.l2_direct) of the
gathered pair; against float64 its square lies within knn_refine_ref.bar_units(D) = (ceil(D / 64) + 8) (1 + 2^-12) units of 2^-24 (derived there);
on integer-valued rows every d2 is exact, so every index equals the reference and a distance is within 1 ulp (the root).  int8
distances: 4 ulp, the k <= 3 kernel's bar.  Outputs and workspaces of every C call stand between poisoned margins.

Measured (one run on one MI355X, printed by the tests): a direct d2 at most 2.95 units of 2^-24 from float64 (bars 9 .. 26), a
distance on integer rows at most 0.5 ulp, int8 top-k distances under 1 ulp; the seeded case leaves no query out."""
import numpy as np
import pytest
import torch

import knn_l2_int8_ref as qref
import knn_margins_util as mu
import knn_refine_ref as ref
import two_rank_util
from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
ULPS_INT8 = 4.0


def _lib():
    from self_supervised import _hip
    return _hip.lib(), _hip.stream()


def _inputs(x, bank, cand):
    """The three operands in the middle of larger buffers: NaN rows around the queries and the bank, in-range rows around the lists."""
    xb = mu.embedded(x, mu.TILE, mu.TILE, mu.NAN)
    bb = mu.embedded(bank, mu.TILE, mu.TILE, mu.NAN)
    cb = mu.embedded(cand, mu.TILE, mu.TILE, 0)
    return xb, bb, cb


def raw_rerank(queries, rows, lists, topk, mean=False, expect=0, **over):
    """The C entry points on caller-owned operands between margins -> host outputs; with expect != 0 the outputs stay untouched.
    over: arguments of the C call by their names in the header, in place of the real ones."""
    L, st = _lib()
    (xbuf, xv), (bbuf, bv), (cbuf, cv) = _inputs(queries, rows, lists)
    n, d = queries.shape
    a = dict(N=n, D=d, R=rows.shape[0], r=lists.shape[1], k=topk, x=xv.data_ptr(), bank=bv.data_ptr(), cand=cv.data_ptr())
    a.update(over)
    k = topk
    if mean:
        obuf, out = mu.poisoned((n,), torch.float32)
        rc = L.ssad_rerank_l2(a["x"], a["bank"], a["cand"], a.get("out", out.data_ptr()), a["N"], a["D"], a["R"], a["r"], a["k"], st)
        outs = [(obuf, out)]
    else:
        dbuf, dist = mu.poisoned((n, max(k, 1)), torch.float32)
        ibuf, idx = mu.poisoned((n, max(k, 1)), torch.int32)
        rc = L.ssad_rerank_l2_index(a["x"], a["bank"], a["cand"], a.get("dist", dist.data_ptr()), a.get("idx", idx.data_ptr()), a["N"],
                                    a["D"], a["R"], a["r"], a["k"], st)
        outs = [(dbuf, dist), (ibuf, idx)]
    torch.cuda.synchronize()
    assert (rc == 0) == (expect == 0), (rc, L.ssad_last_error())
    for buf, view in outs:
        assert mu.guards_intact(buf, view)
        assert mu.untouched(view) if expect else mu.all_written(view)
    got = [v.cpu() for _, v in outs]
    return got[0] if mean else got


def _ulps(got, want64):
    return qref.ulps32(got, want64)


def _lists(n, r, rows, seed, spoil=False):
    """[n][r] int32 listed rows, drawn with repetition (a row listed twice appears twice); spoil: some entries -1 or >= rows."""
    rng = np.random.RandomState(seed)
    cand = rng.randint(0, rows, size=(n, r)).astype(np.int32)
    if spoil:
        bad = rng.rand(n, r) < 0.3
        cand[bad] = rng.choice(np.array([-1, rows, rows + 5, -2 ** 31, 2 ** 31 - 1]), size=int(bad.sum()))
    return torch.from_numpy(cand)


NS, RS_LIST, ROWS = (1, 3, 4, 5, 257), (1, 2, 3, 4, 31, 32), (1, 5, 300)
# the issue's widths, and one in every further instantiation: 200 (four chunks), 300 (six), 1100 (rounds of 512 columns)
DS = (1, 32, 63, 64, 65, 96, 448, 200, 300, 1100)


@pytest.mark.parametrize("d", DS)
def test_rerank_on_integer_rows_with_massive_ties_equals_the_reference(d):
    """Rows of small integers: every difference, square and sum is exact in fp32, equal distances abound, so the device's order is
    the reference's at every place; a distance is the root of an exact d2: within 1 ulp."""
    worst = 0.0
    for rows in ROWS:
        bank = torch.from_numpy(np.random.RandomState(10 + rows + d).randint(-2, 3, size=(rows, d)).astype(F))
        for n in NS:
            x = torch.from_numpy(np.random.RandomState(20 + n + d).randint(-2, 3, size=(n, d)).astype(F))
            for r in RS_LIST:
                cand = _lists(n, r, rows, 30 + n + r + rows, spoil=(n == 5))
                want_d, want_i = ref.rerank(x, bank, cand, r)
                for k in sorted({1, min(3, r), r}):
                    dist, idx = raw_rerank(x, bank, cand, k)
                    assert np.array_equal(idx.numpy().astype(np.int64), want_i[:, :k]), (n, r, k, d, rows)
                    fin = np.isfinite(want_d[:, :k])
                    assert np.array_equal(np.isposinf(dist.numpy()), ~fin)
                    if fin.any():
                        worst = max(worst, _ulps(dist.numpy()[fin], want_d[:, :k][fin]).max())
                    mean = raw_rerank(x, bank, cand, k, mean=True)
                    assert np.array_equal(mean.numpy().view(np.int32), ref.mean_of(dist, k).view(np.int32))
    print(f"D = {d}: integer rows, largest distance error {worst:.3f} ulp")
    assert worst <= 1.0


@pytest.mark.parametrize("d", DS)
def test_rerank_on_gaussian_rows_has_l2_directs_bits_and_meets_float64(d):
    """Every d2 is ops.l2_direct's for the gathered pair (the root of those bits, and the order of those bits by (d2, row, place));
    its square meets float64 within the derived bar."""
    from self_supervised import ops
    units = ref.bar_units(d)
    ratio = 0.0
    for rows in ROWS:
        bank = ref.gauss(rows, d, 40 + rows + d)
        for n in NS:
            x = ref.gauss(n, d, 50 + n + d)
            direct = ops.l2_direct(x.cuda(), bank.cuda()).cpu().numpy()             # [n][rows] fp32 d2
            for r in RS_LIST:
                cand = _lists(n, r, rows, 60 + n + r + rows, spoil=(n == 4))
                c = cand.numpy().astype(np.int64)
                ok = (c >= 0) & (c < rows)
                g = np.take_along_axis(direct, np.where(ok, c, 0), 1)
                dist, idx = raw_rerank(x, bank, cand, r)
                want64, _ = ref.gathered_d2(x, bank, cand)
                for i in range(n):
                    order = sorted((j for j in range(r) if ok[i, j]), key=lambda j: (g[i, j].view(np.uint32), c[i, j], j))
                    m = len(order)
                    assert idx[i, :m].tolist() == c[i, order].tolist() and (idx[i, m:] == -1).all(), (n, r, d, rows, i)
                    assert np.array_equal(dist[i, :m].numpy().view(np.int32), np.sqrt(g[i, order]).view(np.int32))
                    assert np.isposinf(dist[i, m:].numpy()).all()
                    if m:
                        w = want64[i, order]
                        ratio = max(ratio, (np.abs(g[i, order].astype(np.float64) - w) / (U * np.maximum(w, 1e-300))).max())
    print(f"D = {d}: |d2 - float64| at most {ratio:.3f} units of 2^-24 d2 (bar {units})")
    assert ratio <= units


def test_rerank_order_against_float64_on_the_seeded_case():
    """The device's rows against the float64 order, on the queries the host test (tests/test_knn_refine_host.py) does not leave out."""
    x, bank, cand = ref.gauss_case()
    r = ref.GAUSS_CASE["r"]
    dropped, close, pairs = ref.near_ties(x, bank, cand, ref.bar_units(ref.GAUSS_CASE["d"]))
    assert dropped.mean() <= ref.LEFT_OUT_CAP
    dist, idx = raw_rerank(x, bank, cand, r)
    want_d, want_i = ref.rerank(x, bank, cand, r)
    keep = ~dropped
    assert np.array_equal(idx.numpy()[keep].astype(np.int64), want_i[keep])
    assert _ulps(dist.numpy(), want_d).max() <= ref.bar_units(ref.GAUSS_CASE["d"])      # the root halves the relative error of d2
    print(f"seeded case: {int(keep.sum())} of {len(keep)} queries compared, {close} of {pairs} adjacent pairs under twice the bar")


def test_rerank_skips_invalid_entries_and_lists_duplicates_twice():
    x, bank = ref.gauss(3, 96, 70), ref.gauss(5, 96, 71)
    cand = torch.tensor([[-1, 5, 7, -9], [2, 2, 9, 2], [4, -1, 0, 4]], dtype=torch.int32)
    dist, idx = raw_rerank(x, bank, cand, 4)
    assert idx[0].tolist() == [-1] * 4 and np.isposinf(dist[0].numpy()).all()        # nothing valid
    assert idx[1].tolist() == [2, 2, 2, -1] and dist[1, 0] == dist[1, 1] == dist[1, 2] and np.isposinf(dist[1, 3].item())
    assert sorted(idx[2, :3].tolist()) == [0, 4, 4] and idx[2, 3] == -1
    mean = raw_rerank(x, bank, cand, 3, mean=True)
    assert np.isposinf(mean[0].item()) and np.isfinite(mean[1].item()) and np.isfinite(mean[2].item())
    assert np.isposinf(raw_rerank(x, bank, cand, 4, mean=True).numpy()).all()          # every query misses its fourth entry
    want_d, want_i = ref.rerank(x, bank, cand, 4)
    assert np.array_equal(idx.numpy().astype(np.int64), want_i)


def test_rerank_bits_do_not_depend_on_the_call_or_the_batch():
    x, bank, cand = ref.gauss_case()
    a = raw_rerank(x, bank, cand, 16)
    b = raw_rerank(x, bank, cand, 16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    parts = [raw_rerank(x[lo:hi], bank, cand[lo:hi].contiguous(), 16) for lo, hi in ((0, 1), (1, 130), (130, 257))]
    assert torch.equal(torch.cat([p[0] for p in parts]), a[0]) and torch.equal(torch.cat([p[1] for p in parts]), a[1])
    m = raw_rerank(x, bank, cand, 16, mean=True)
    assert torch.equal(m, torch.cat([raw_rerank(x[lo:hi], bank, cand[lo:hi].contiguous(), 16, mean=True) for lo, hi in ((0, 200), (200, 257))]))
    # a pair's bits do not depend on r or its place: the single nearest of a longer list is that of the list reversed
    rev = raw_rerank(x, bank, torch.flip(cand, [1]).contiguous(), 16)
    assert torch.equal(rev[0], a[0]) and torch.equal(rev[1], a[1])


BAD_RERANK = [dict(x=None), dict(bank=None), dict(cand=None), dict(N=0), dict(N=-1), dict(D=0), dict(R=0), dict(r=0), dict(r=33),
              dict(k=0), dict(k=5), dict(N=4 * 2147483647)]


@pytest.mark.parametrize("over", BAD_RERANK, ids=[str(o) for o in BAD_RERANK])
def test_rerank_argument_errors_leave_the_outputs_untouched(over):
    x, bank, cand = ref.gauss(6, 32, 1), ref.gauss(9, 32, 2), _lists(6, 4, 9, 3)
    for mean in (False, True):
        raw_rerank(x, bank, cand, 3, mean=mean, expect=2, **over)
    for name in ("dist", "idx"):
        raw_rerank(x, bank, cand, 3, expect=2, **{name: None})
    raw_rerank(x, bank, cand, 3, mean=True, expect=2, out=None)


# ---------------------------------------------------------------- the int8 top-k

def rand_codes(n, d, seed, lo=-128, hi=128):
    return torch.from_numpy(np.random.RandomState(seed).randint(lo, hi, size=(n, d)).astype(np.int8))


class Side:
    """Codes on the device between margins of code 0x55, with their int32 norms (margins -7) and excess (margins NaN)."""

    def __init__(self, codes, excess=None):
        self.host = codes.numpy()
        self.cbuf, self.codes = mu.embedded(codes, mu.TILE, mu.TILE, 0x55)
        self.sbuf, self.sq = mu.embedded(torch.from_numpy(qref.sq64(self.host).astype(np.int32)), mu.TILE, mu.TILE, -7)
        ex = torch.zeros(codes.shape[0]) if excess is None else excess
        self.ex_host = ex.double().numpy()
        self.ebuf, self.ex = mu.embedded(ex, mu.TILE, mu.TILE, mu.NAN)


def raw_topk(x, b, topk, s2, splits=1, expect=0, **over):
    k = topk
    L, st = _lib()
    n, d = x.codes.shape
    P = lambda t: t.data_ptr()
    dbuf, dist = mu.poisoned((n, k if 0 < k <= 64 else 1), torch.float32)
    ibuf, idx = mu.poisoned((n, k if 0 < k <= 64 else 1), torch.int32)
    pbuf, part = mu.poisoned((max(splits, 1) * n * max(min(k, 64), 1),), torch.int64)
    a = dict(xq=P(x.codes), x_sq=P(x.sq), x_excess=P(x.ex), bankq=P(b.codes), bank_sq=P(b.sq), part=P(part) if splits != 1 else None,
             dist=P(dist), idx=P(idx), N=n, D=d, R=b.codes.shape[0], k=k, S=splits)
    a.update(over)
    rc = L.ssad_topk_l2q_index(a["xq"], a["x_sq"], a["x_excess"], a["bankq"], a["bank_sq"], a["part"], a["dist"], a["idx"], a["N"],
                                   a["D"], a["R"], a["k"], a["S"], float(s2), st)
    torch.cuda.synchronize()
    assert (rc == 0) == (expect == 0), (rc, L.ssad_last_error())
    for buf, view in ((dbuf, dist), (ibuf, idx), (pbuf, part)):
        assert mu.guards_intact(buf, view)
    if expect:
        assert mu.untouched(dist) and mu.untouched(idx) and mu.untouched(part)
        return None
    assert mu.all_written(dist) and mu.all_written(idx)
    assert mu.untouched(part) if splits == 1 else mu.all_written(part)
    return dist.cpu(), idx.cpu()


def raw_knn3(x, b, s2):
    L, st = _lib()
    n, d = x.codes.shape
    P = lambda t: t.data_ptr()
    dbuf, dist = mu.poisoned((n, 3), torch.float32)
    ibuf, idx = mu.poisoned((n, 3), torch.int32)
    rc = L.ssad_l2q_knn_index(P(x.codes), P(x.sq), P(x.ex), P(b.codes), P(b.sq), None, P(dist), P(idx), n, d, b.codes.shape[0], 3, 1,
                              float(s2), st)
    torch.cuda.synchronize()
    assert rc == 0, L.ssad_last_error()
    return dist.cpu(), idx.cpu()


TOPK_KS, TOPK_NS, TOPK_SPLITS = (4, 5, 8, 9, 16, 17, 32), (1, 130, 300), (1, 2, 4, 7)


@pytest.mark.parametrize("d", (32, 96, 448))
def test_int8_topk_equals_the_integer_reference_for_every_split_count(d):
    s2 = F(0.0123) * F(0.0123)
    worst = 0.0
    for n in TOPK_NS:
        ex = torch.from_numpy(np.random.RandomState(n + d).rand(n).astype(F) * (np.arange(n) % 3 == 0))
        x = Side(rand_codes(n, d, 100 + n + d), ex)
        for k in TOPK_KS:
            for rows in sorted({k, k + 1, 127, 128, 129, 300}):
                b = Side(rand_codes(rows, d, 200 + rows + d))
                want_d2, want_i = ref.int8_topk(x.host, b.host, k)
                base = None
                for splits in TOPK_SPLITS:
                    dist, idx = raw_topk(x, b, k, s2, splits)
                    assert np.array_equal(idx.numpy().astype(np.int64), want_i), (n, rows, k, d, splits)
                    if base is None:
                        base = (dist, idx)
                        worst = max(worst, _ulps(dist.numpy(), qref.dist64(want_d2, s2, x.ex_host)).max())
                        d3, i3 = raw_knn3(x, b, s2)
                        assert torch.equal(dist[:, :3], d3) and torch.equal(idx[:, :3], i3)
                    else:
                        assert torch.equal(dist, base[0]) and torch.equal(idx, base[1])
    print(f"D = {d}: int8 top-k distances at most {worst:.3f} ulp from float64")
    assert worst <= ULPS_INT8


def test_int8_topk_ties_and_asymmetric_operands():
    d, s2 = 96, F(1.0)
    five = rand_codes(5, d, 7)
    b = Side(five.repeat(60, 1))                                                    # 300 rows, every D2 sixty times
    x = Side(rand_codes(130, d, 8))
    for k in (4, 17, 32):
        want_d2, want_i = ref.int8_topk(x.host, b.host, k)
        for splits in (1, 4):
            dist, idx = raw_topk(x, b, k, s2, splits)
            assert np.array_equal(idx.numpy().astype(np.int64), want_i)            # equal D2: the smaller row
    # queries at one end of the code range, the bank at the other: the largest D2; s2 = 1 and excess 0 make dist = sqrt(D2), and at
    # D = 32 (D2 <= 32 x 255^2 < 2^21) the square of the rounded root is within 2^-23 D2 < 0.25 of D2: rint recovers the integer
    xa, ba = Side(rand_codes(130, 32, 9, -128, -100)), Side(rand_codes(129, 32, 10, 100, 128))
    want_d2, want_i = ref.int8_topk(xa.host, ba.host, 8)
    dist, idx = raw_topk(xa, ba, 8, s2, 2)
    assert np.array_equal(idx.numpy().astype(np.int64), want_i)
    assert np.array_equal(np.rint(dist.double().numpy() ** 2).astype(np.int64), want_d2) and 2 ** 20 < want_d2.max() < 2 ** 21


BAD_TOPK = [dict(xq=None), dict(x_sq=None), dict(x_excess=None), dict(bankq=None), dict(bank_sq=None), dict(dist=None), dict(idx=None),
            dict(N=0), dict(D=0), dict(D=48), dict(D=32768 + 32), dict(R=0), dict(k=3), dict(k=33), dict(k=10, R=9), dict(S=0),
            dict(S=65536), dict(S=2, part=None), dict(N=128 * 2147483647), "xq+1", "bankq+1", "part+4"]


@pytest.mark.parametrize("over", BAD_TOPK, ids=[str(o) for o in BAD_TOPK])
def test_int8_topk_argument_errors_leave_the_outputs_untouched(over):
    x, b = Side(rand_codes(6, 64, 1)), Side(rand_codes(40, 64, 2))
    splits = 1
    if isinstance(over, str):
        name, off = over.split("+")
        if name == "part":
            splits, over = 2, dict(S=2, part=torch.zeros(4096, dtype=torch.int64, device="cuda").data_ptr() + int(off))
        else:
            over = {name: getattr(x if name == "xq" else b, "codes").data_ptr() + int(off)}
    raw_topk(x, b, 8, 1.0, splits, expect=2, **over)


def test_ops_topk_and_rerank_through_the_wrappers():
    from self_supervised import ops
    rows, x = ref.gauss(300, 96, 1), ref.gauss(130, 96, 2)
    lo, s, inv_s, s2 = qref.quantiser_of(rows)
    bank_q, bank_sq, _ = ops.rows_to_int8(rows.cuda(), float(lo), float(inv_s), float(s))
    dist, idx = ops.l2q_topk_index(x.cuda(), bank_q, bank_sq, (float(lo), float(s)), 16)
    _, want_i = ref.int8_topk(qref.codes(x, lo, inv_s), qref.codes(rows, lo, inv_s), 16)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), want_i)
    for splits in (1, 3):
        d2, i2 = ops.l2q_topk_index(x.cuda(), bank_q, bank_sq, (float(lo), float(s)), 16, splits=splits)
        assert torch.equal(d2, dist) and torch.equal(i2, idx)
    d3, i3 = ops.l2q_knn_index(x.cuda(), bank_q, bank_sq, (float(lo), float(s)), 3)
    assert torch.equal(dist[:, :3], d3) and torch.equal(idx[:, :3], i3)
    rd, ri = ops.l2_rerank_index(x.cuda(), rows.cuda(), idx, 3)
    want_d, want_i = ref.rerank(x, rows, idx, 3)
    dropped, _, _ = ref.near_ties(x, rows, idx, ref.bar_units(96))
    assert np.array_equal(ri.cpu().numpy().astype(np.int64)[~dropped], want_i[~dropped])
    assert np.array_equal(ops.l2_rerank_mean(x.cuda(), rows.cuda(), idx, 3).cpu().numpy().view(np.int32), ref.mean_of(rd, 3).view(np.int32))


# ---------------------------------------------------------------- the detector

def _one_cell_bank(d=32):
    """26 rows: 24 inside one code cell (offsets of 1e-4 m, m = 24 .. 1, along the first column, inside a code step of about 4e-3:
    the smaller the row number the FARTHER from the query) and two far rows that fix lo / hi."""
    bank = torch.zeros((26, d), dtype=torch.float32)
    bank[:24, 0] = torch.arange(24, 0, -1, dtype=torch.float32) * 1e-4
    bank[24], bank[25] = -0.45, 0.55                # zero codes at 114.75 of a step: the cell's rows stay clear of a rounding boundary
    x = torch.zeros((2, d), dtype=torch.float32)
    x[1, 1] = 2e-4
    return x, bank


def test_a_refined_int8_detector_orders_the_rows_of_one_code_cell():
    """Fails without the feature (there is no `refine`).  All 24 near rows share their codes: the coarse D2 ties and the int8 search
    answers rows 0, 1, 2, the three FARTHEST of the cell; refined over the whole bank (R = 26 <= r = 32) the answer is float64's."""
    from self_supervised.models import AnomalyDetector
    x, bank = _one_cell_bank()
    lo, s, inv_s, _ = qref.quantiser_of(bank)
    codes = qref.codes(bank, lo, inv_s)
    assert 3e-3 < float(s) < 5e-3 and (codes[:24] == codes[0]).all()                # one code cell
    det = AnomalyDetector(metric='euclidean', bank_dtype='int8', refine=32)
    det.fit_bank(bank)
    assert torch.equal(det.bank_f32.cpu(), bank) and det.bank.dtype == torch.int8
    want_d, want_i = ref.rerank(x, bank, torch.arange(26, dtype=torch.int32).repeat(2, 1), 3)
    assert want_i.tolist() == [[23, 22, 21], [23, 22, 21]]
    dist, idx = det.kneighbors(x)
    assert np.array_equal(idx.cpu().numpy(), want_i)
    units = ref.bar_units(32)
    assert (np.abs(dist.cpu().double().numpy() - want_d) <= units * U * want_d).all()
    got = det.predict(x).reshape(-1).cpu().double().numpy()
    assert (np.abs(got - want_d.mean(1)) <= (units + 3) * U * want_d.mean(1)).all()
    d26, i26 = det.kneighbors(x, 26)
    assert np.array_equal(i26.cpu().numpy(), ref.rerank(x, bank, torch.arange(26, dtype=torch.int32).repeat(2, 1), 26)[1])
    with pytest.raises(ValueError, match="gives a shortlist of 26 rows, fewer than k = 27"):
        det.kneighbors(x, 27)
    plain = AnomalyDetector(metric='euclidean', bank_dtype='int8')
    plain.fit_bank(bank)
    _, pidx = plain.kneighbors(x)
    assert pidx.cpu().tolist() == [[0, 1, 2], [0, 1, 2]]                            # the case bites: the unrefined answer differs
    assert not torch.equal(plain.predict(x), det.predict(x))


def _tree(tmp_path, seeded_sd, n_train=8):
    from self_supervised import datasets
    datasets._DataModule.num_workers = 0
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=n_train, n_test_good=2, n_test_bad=2, size=96)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    return root, ck


def _coarse(det, x, r):
    from self_supervised import ops
    if det.bank_dtype == 'int8':
        return ops.l2q_topk_index(x, det.bank, det.bank_sq, det.quant, r)[1]
    return ops.l2h_topk_index(x, det.bank, det.bank_sq, r)[1]


@pytest.mark.parametrize("bank_dtype", ['float16', 'int8'])
@pytest.mark.parametrize("patch_level", [False, True])
def test_refined_kneighbors_is_the_rerank_of_the_coarse_shortlist(bank_dtype, patch_level):
    """Test B on seeded rows at both levels, and test C: a refined score lies between the exact float64 k-NN mean (minus the bar) and
    the float64 mean over the coarse shortlist (plus the bar)."""
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector
    d = 96
    level = dict(patch_level=True, batch=2, num_patches=100) if patch_level else {}
    rows, x = ref.gauss(500, d, 11) * 0.5, ref.gauss(200, d, 12) * 0.5
    units = ref.bar_units(d)
    exact = np.sort(qref.exact64(x, rows), axis=1)[:, :3]
    for r in (4, 16):
        det = AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype, refine=r, **level)
        det.fit_bank(rows)
        cand = _coarse(det, x.cuda(), r)
        for k in (1, 3, r):
            want = ops.l2_rerank_index(x.cuda(), det.bank_f32, cand, k)
            got = det.kneighbors(x, k)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1].long())
        scores = det.predict(x)
        assert tuple(scores.shape) == ((2, 1, 10, 10) if patch_level else (200,))
        assert torch.equal(scores.reshape(-1), ops.l2_rerank_mean(x.cuda(), det.bank_f32, cand, 3))
        got = scores.reshape(-1).cpu().double().numpy()
        short = ref.rerank(x, rows, cand, 3)[0].mean(1)
        slack = (units + 3) * U
        assert (got >= exact.mean(1) * (1 - slack)).all() and (got <= short * (1 + slack)).all()
        print(f"{bank_dtype} r = {r}: refined mean equals the exact 3-NN mean (to the bar) for "
              f"{(np.abs(got - exact.mean(1)) <= slack * exact.mean(1)).mean():.3f} of the queries")


@pytest.mark.parametrize("localization", ["patches", "dense"])
@pytest.mark.parametrize("bank_dtype", ['float16', 'int8'])
def test_inference_with_refine_equals_the_detector_called_by_hand(tmp_path, seeded_sd, monkeypatch, localization, bank_dtype):
    """Test B on the fake category and test D's tools.inference(..., refine=8) against the detector's bits."""
    from self_supervised import ops, tools
    from self_supervised.models import AnomalyDetector
    root, ck = _tree(tmp_path, seeded_sd)
    seen = {}
    orig = AnomalyDetector.fit_bank

    def spy(self, bank):
        seen["rows32"] = torch.as_tensor(bank).detach().float().cpu().clone()
        orig(self, bank)
        seen["det"] = self
    monkeypatch.setattr(AnomalyDetector, "fit_bank", spy)
    np.random.seed(3)
    torch.manual_seed(3)
    res = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, localization=localization,
                          bank='train', image_scores='max', metric='euclidean', bank_dtype=bank_dtype, refine=8)
    det, rows32 = seen["det"], seen["rows32"]
    assert det.refine == 8 and torch.equal(det.bank_f32.cpu(), rows32)
    monkeypatch.setattr(AnomalyDetector, "fit_bank", orig)
    hand = AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype, refine=8)
    hand.fit_bank(rows32)
    rows = res.embedding_vectors.float()
    assert torch.equal(hand.predict(rows).cpu(), res.anomaly_maps.reshape(-1).cpu())
    cand = _coarse(hand, rows.cuda(), 8)
    for k in (3, 8):
        want = ops.l2_rerank_index(rows.cuda(), hand.bank_f32, cand, k)
        got = hand.kneighbors(rows, k)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1].long())
    p = rows.shape[0] // 4
    assert torch.equal(res.image_scores, res.anomaly_maps.reshape(4, p).max(1).values)


@pytest.mark.parametrize("bank_dtype", ['float16', 'int8'])
def test_state_coreset_and_the_default_path(monkeypatch, bank_dtype):
    """Test D: state round trip, a coreset whose selection is the unrefined detector's, and refine=None on the entry points and
    state keys it had."""
    from self_supervised import ops
    from self_supervised.models import AnomalyDetector
    emb, x = ref.gauss(400, 64, 2), ref.gauss(50, 64, 3)
    names = []
    orig = ops._run

    def spy(kernel, *a, **kw):
        names.append(kernel)
        return orig(kernel, *a, **kw)
    monkeypatch.setattr(ops, "_run", spy)
    plain = AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype, coreset=0.5)
    np.random.seed(1)
    plain.fit(emb)
    names.clear()
    plain.predict(x)
    plain.kneighbors(x)
    want = {'float16': {"rows_to_half", "l2h_knn_fused", "l2h_knn_index"}, 'int8': {"rows_to_int8", "l2q_knn_fused", "l2q_knn_index"}}
    assert set(names) == want[bank_dtype], names
    keys = {'float16': {"metric", "bank", "bank_dtype"}, 'int8': {"metric", "bank", "bank_dtype", "bank_sq", "lo", "s"}}[bank_dtype]
    assert set(plain.state()) == keys and not hasattr(plain, "bank_f32") and plain.refine is None
    det = AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype, coreset=0.5, refine=8)
    np.random.seed(1)
    det.fit(emb)
    assert torch.equal(det.coreset_rows[0], plain.coreset_rows[0]) and torch.equal(det.bank, plain.bank)
    assert torch.equal(det.bank_sq, plain.bank_sq) and det.coreset_counts == plain.coreset_counts
    assert det.bank_f32.shape == (plain.bank.shape[0], 64) and det.bank_f32.dtype == torch.float32
    if bank_dtype == 'float16':
        assert torch.equal(ops.rows_to_half(det.bank_f32)[0], det.bank)             # the fp32 rows ARE the rows of the coarse bank
    else:
        assert det.quant == plain.quant and torch.equal(ops.rows_to_int8(det.bank_f32, det.quant[0], 1.0 / det.quant[1], det.quant[1])[1],
                                                        det.bank_sq)
    assert np.isfinite(det.threshold)
    names.clear()
    det.predict(x)
    det.kneighbors(x)
    coarse = {'float16': {"rows_to_half", "l2h_topk_index"}, 'int8': {"rows_to_int8", "l2q_topk_index"}}[bank_dtype]
    assert set(names) == coarse | {"l2_rerank_mean", "l2_rerank_index"}, names
    state = det.state()
    assert set(state) == keys | {"refine", "bank_f32"} and state["refine"] == 8
    other = AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype, refine=8)
    other.load_state(state)
    assert torch.equal(other.bank_f32, det.bank_f32) and torch.equal(other.bank, det.bank) and torch.equal(other.bank_sq, det.bank_sq)
    assert torch.equal(other.predict(x), det.predict(x))
    a, b = other.kneighbors(x, 8), det.kneighbors(x, 8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="fitted with refine=8, this detector has None"):
        AnomalyDetector(metric='euclidean', bank_dtype=bank_dtype).load_state(state)


def test_two_ranks_equal_one_rank(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector
    import dist_refine_worker as w
    root, ck = _tree(tmp_path, seeded_sd)
    r = two_rank_util.launch("dist_refine_worker.py", [tmp_path, root, ck])
    assert r["equal_across_ranks"] and r["world"] == 2, r
    two = torch.load(str(tmp_path / w.FILE))
    seen = {}
    orig = AnomalyDetector.predict

    def spy(self, x):
        seen.update(threshold=self.threshold, bank=self.bank.cpu(), bank_f32=self.bank_f32.cpu(), refine=self.refine)
        return orig(self, x)
    monkeypatch.setattr(AnomalyDetector, "predict", spy)
    one = w.inference(tools, ck, root)
    assert torch.equal(two["maps"], one.anomaly_maps) and torch.equal(two["scores"], one.image_scores)
    assert two["bank_f32"].dtype == torch.float32 and torch.equal(two["bank_f32"], seen["bank_f32"]) and torch.equal(two["bank"], seen["bank"])
    assert two["threshold"] == seen["threshold"] and np.isfinite(seen["threshold"]) and two["refine"] == seen["refine"] == 8
