"""GPU tests of every kNN search kernel and helper between adversarial margins (tests/knn_margins_util.py): the cosine searches of
csrc/knn.hip, the Euclidean searches of csrc/knn_l2.hip, knn_l2_half.hip, knn_l2_int8.hip, knn_topk.hip, knn_gallery.hip and
knn_ivf.hip, their row-preparation helpers and the image-score kernels of csrc/image_score.hip.

Every operand of a call stands in the middle of a larger buffer at once.  Beyond a bank stand twins of the queries (distance 0, while
every real row is at least 1.0 away: tests/test_knn_margins_host.py), beyond its norms their true norms or -1e30 (both are run),
beyond the queries NaN, beyond an integer array in-range values that name twin rows; outputs and workspaces stand between NaN / -7
guards and are passed to the C entry points directly.  A kernel that reads or writes one row too far changes the answer.  For every
form: the outputs are torch.equal to the same entry point on tight operands, meet float64 at the bar and tie rule of that path's own
test file or ref module (imported, not restated), leave every guard intact, are finite with every index in [0, R), and the workspace
is wholly written where splits are used and untouched where not."""
import numpy as np
import pytest
import torch

import ivf_ref
import knn_gallery_ref as gref
import knn_index_ref as cref
import knn_l2_half_ref as href
import knn_l2_int8_ref as qref
import knn_l2_ref as ref
import knn_margins_util as mu
import knn_topk_ref as tref
import test_hip_knn_gallery as gallery_tests
import test_hip_knn_l2 as l2_tests
import test_hip_knn_l2_half as half_tests
from test_hip_knn_gallery import l2_direct_bar
from test_hip_knn_index import DIST_TOL, GAP
from test_hip_knn_l2_int8 import ULPS

pytestmark = pytest.mark.gpu

EPS = ref.EPS
F32, F16, I8, I32, I64 = torch.float32, torch.float16, torch.int8, torch.int32, torch.int64
MAX_LOOSE = 0.02        # share of positions the index comparison may leave out, asserted on the reference alone


def P(t):
    return None if t is None else t.data_ptr()


def std(ins, tail, null_part=False):
    """The usual argument order: inputs, [workspace], outputs, sizes.  null_part: a null pointer stands where no workspace is given."""
    return lambda part, outs: [P(t) for t in ins] + ([P(part)] if part is not None or null_part else []) + [P(o) for o in outs] + list(tail)


def run(name, args, out_specs, part_spec=None):
    """Entry point `name` on outputs and a workspace that stand between guards -> (output views, workspace view), guards checked."""
    from self_supervised import _hip
    L = _hip.lib()
    outs = [mu.poisoned(shape, dtype) for shape, dtype in out_specs]
    part = mu.poisoned(*part_spec) if part_spec else None
    rc = getattr(L, name)(*args(None if part is None else part[1], [v for _, v in outs]), _hip.stream())
    assert rc == 0, (name, L.ssad_last_error())
    torch.cuda.synchronize()
    for buf, view in outs + ([part] if part else []):
        assert mu.guards_intact(buf, view), name
    return [v for _, v in outs], (None if part is None else part[1])


def run_both(name, tight, embedded_sets, tail, out_specs, part_spec=None, part_written=False, rows=None, what=(), null_part=False):
    """`name` on the tight inputs and on every set of embedded ones: the same bits, sane outputs, the workspace written or not."""
    want, _ = run(name, std(tight, tail, null_part), out_specs, part_spec)
    for v, ins in enumerate(embedded_sets):
        got, part = run(name, std(ins, tail, null_part), out_specs, part_spec)
        for g, w in zip(got, want):
            assert torch.equal(g, w), (name, v) + tuple(what)
            if g.dtype.is_floating_point:
                assert torch.isfinite(g).all(), (name, v) + tuple(what)
            elif rows is not None:
                assert (g >= 0).all() and (g < rows).all(), (name, v) + tuple(what)
        if part is not None:
            assert mu.all_written(part) if part_written else mu.untouched(part), (name, v) + tuple(what)
    return [w.cpu() for w in want]


def nan_embedded(t):
    return mu.embedded(t, mu.TILE, mu.TILE, mu.NAN)[1]


# ---------------------------------------------------------------- the flat searches

class Flat:
    """The operands of one flat search case in one representation: tight, and embedded with either kind of norm margin."""

    def __init__(self, kind, n, r, d):
        from self_supervised import ops
        self.kind, self.n, self.r, self.d = kind, n, r, d
        self.x_h, self.bank_h = mu.flat_inputs(n, r, d, cosine=kind == "cosine")
        x, bank = self.x_h.cuda(), self.bank_h.cuda()
        m = mu.margin(n)
        self.s2 = None
        if kind == "cosine":
            q, b, twins, bsq = (x,), ops.l2_normalize_rows(bank), ops.l2_normalize_rows(x), None
            q_fill = (mu.NAN,)
            self.bank_host = b.cpu()
        elif kind == "l2":
            q, b, twins, bsq, tsq = (x,), bank, x, ops.row_sqnorms(bank), ops.row_sqnorms(x)
            q_fill = (mu.NAN,)
        elif kind == "half":
            xh, xsq = ops.rows_to_half(x)
            b, bsq = ops.rows_to_half(bank)
            q, twins, tsq = (xh, xsq), xh, xsq
            q_fill = (mu.NAN, mu.NAN)
        else:
            lo, s, inv_s, s2 = (float(v) for v in mu.int8_quantiser(self.x_h, self.bank_h))
            self.quant, self.s2 = (lo, s, inv_s), s2
            xq, xsq, xex = ops.rows_to_int8(x, lo, inv_s, s)
            b, bsq, _ = ops.rows_to_int8(bank, lo, inv_s, s)
            q, twins, tsq = (xq, xsq, xex), xq, xsq
            q_fill = (-128, d * 128 * 128, mu.NAN)          # a NaN row in this representation: code -128 throughout, NaN excess
        self.tight = q + (b,) + (() if bsq is None else (bsq,))
        eq = tuple(mu.embedded(t, mu.TILE, mu.TILE, f)[1] for t, f in zip(q, q_fill))
        eb = mu.embedded(b, m, m, twins)[1]
        if bsq is None:
            self.embedded = [eq + (eb,)]
        else:
            self.embedded = [eq + (eb, mu.embedded(bsq, m, m, fill)[1]) for fill in (tsq, mu.BSQ_POISON[bsq.dtype])]


FLAT_ENTRIES = {        # kind -> (mean form, index form, workspace dtypes of the two, mean form of the case without a workspace or None)
    "cosine": ("ssad_cosine_knn_split", "ssad_cosine_knn_index", F32, I64, "ssad_cosine_knn_fused"),
    "l2": ("ssad_l2_knn_fused", "ssad_l2_knn_index", F32, I64, "ssad_l2_knn_fused"),
    "half": ("ssad_l2h_knn_fused", "ssad_l2h_knn_index", F32, I64, "ssad_l2h_knn_fused"),
    "int8": ("ssad_l2q_knn_fused", "ssad_l2q_knn_index", I32, I64, None),
    "topk_l2": ("ssad_l2_knn_topk", "ssad_l2_knn_topk_index", I64, I64, None),
    "topk_half": ("ssad_l2h_knn_topk", "ssad_l2h_knn_topk_index", I64, I64, None),
}
# ssad_cosine_knn_split is the two-launch form for every S: its workspace is written for S = 1 too; the others go without it there
ALWAYS_SPLIT = ("ssad_cosine_knn_split",)


def flat_results(c, entries, k):
    """[(dist, idx, out)] on the host of every (mean, index) pair of runs of the case, checked by run_both: S = 1 without a workspace
    (a null part; ssad_cosine_knn_fused has neither argument), then every S of mu.SPLITS with one."""
    n, r, d = c.n, c.r, c.d
    mean, index, pdt_mean, pdt_index, mean1 = entries
    width = k if c.kind.startswith("topk") else 3
    extra = () if c.s2 is None else (c.s2,)
    mean_spec, index_spec = [((n,), F32)], [((n, k), F32), ((n, k), I32)]
    res = []
    if mean1:
        null = mean1 == mean
        (out,) = run_both(mean1, c.tight, c.embedded, (n, d, r, k, 1) if null else (n, d, r, k), mean_spec, what=(n, r, d, k),
                          null_part=null)
        dist, idx = run_both(index, c.tight, c.embedded, (n, d, r, k, 1), index_spec, rows=r, what=(n, r, d, k), null_part=True)
        res.append((dist, idx, out))
    for s in mu.SPLITS:
        tail = (n, d, r, k, s) + extra
        (out,) = run_both(mean, c.tight, c.embedded, tail, mean_spec, ((s * n, width), pdt_mean), s > 1 or mean in ALWAYS_SPLIT,
                          what=(n, r, d, k, s))
        dist, idx = run_both(index, c.tight, c.embedded, tail, index_spec, ((s * n, width), pdt_index), s > 1, rows=r,
                             what=(n, r, d, k, s))
        res.append((dist, idx, out))
    return res


@pytest.mark.parametrize("d", mu.DS)
def test_cosine_searches(d):
    for r in mu.RS:
        for n in mu.NS:
            c = Flat("cosine", n, r, d)
            want_d, want_i = cref.kneighbors64(c.x_h, c.bank_host, 4)
            for k in (k for k in mu.KS if k <= r):
                strict = cref.strict_positions(want_d, k, GAP)
                assert 1.0 - strict.mean() <= MAX_LOOSE, (n, r, d, k)                   # on the reference alone, first
                for dist, idx, out in flat_results(c, FLAT_ENTRIES["cosine"], k):
                    assert np.abs(dist.double().numpy() - want_d[:, :k]).max() <= DIST_TOL, (n, r, d, k)
                    idx = idx.numpy().astype(np.int64)
                    d_of_idx = np.take_along_axis(cref.distances64(c.x_h, c.bank_host), idx, 1)
                    assert np.abs(d_of_idx - want_d[:, :k]).max() <= DIST_TOL, (n, r, d, k)
                    assert np.array_equal(idx[strict], want_i[:, :k][strict]), (n, r, d, k)
                    assert np.abs(out.double().numpy() - want_d[:, :k].mean(1)).max() <= DIST_TOL, (n, r, d, k)


def test_unfused_cosine_chain():
    """ssad_l2_normalize_rows -> the 1 x 1 GEMM -> ssad_cosine_knn_mean at a width that is no multiple of 32; the normalised queries and
    the similarity matrix stand between NaN row margins on their way from kernel to kernel."""
    from self_supervised import ops
    d = mu.D_UNFUSED
    for r in mu.RS:
        for n in mu.NS:
            x_h, raw = mu.flat_inputs(n, r, d, cosine=True)
            x, bank = x_h.cuda(), ops.l2_normalize_rows(raw.cuda())
            eb = mu.embedded(bank, mu.margin(n), mu.margin(n), ops.l2_normalize_rows(x))[1]
            (xn,), _ = run("ssad_l2_normalize_rows", std((nan_embedded(x),), (n, d)), [((n, d), F32)])
            assert torch.equal(xn, ops.l2_normalize_rows(x))
            gemm = lambda part, outs: [P(xn), P(eb), P(outs[0]), None, None, None, 0, n, 1, 1, d, r, 1, 1, 1, 0]
            (sim,), _ = run("ssad_conv_igemm_fwd", gemm, [((n, r), F32)])
            assert torch.equal(sim, ops.linear_fwd(ops.l2_normalize_rows(x), bank)) and torch.isfinite(sim).all()
            want_d, _ = cref.kneighbors64(x_h, bank.cpu(), 3)
            for k in (k for k in mu.KS if k <= r):
                (out,), _ = run("ssad_cosine_knn_mean", std((sim,), (n, r, k)), [((n,), F32)])
                assert torch.equal(out, ops.cosine_knn_mean(ops.linear_fwd(ops.l2_normalize_rows(x), bank), k))
                assert np.abs(out.cpu().double().numpy() - want_d[:, :k].mean(1)).max() <= DIST_TOL, (n, r, k)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("d", mu.DS)
def test_flat_euclidean_searches(d, half):
    mod = href if half else ref
    for r in mu.RS:
        for n in mu.NS:
            c = Flat("half" if half else "l2", n, r, d)
            d2_all, a_all = mod.d2_64(c.x_h, c.bank_h), mod.scale_a(c.x_h, c.bank_h)
            for k in (k for k in mu.KS if k <= r):
                for dist, idx, out in flat_results(c, FLAT_ENTRIES[c.kind], k):
                    if half:
                        _, loose = half_tests.check_against_float64(d, dist, idx, out, k, d2_all, a_all)
                    else:
                        _, loose = l2_tests.check_against_float64(c.x_h, c.bank_h, dist, idx, out, k, d2_all, a_all)
                    assert loose <= MAX_LOOSE


@pytest.mark.parametrize("d", mu.DS)
def test_int8_searches(d):
    for r in mu.RS:
        for n in mu.NS:
            c = Flat("int8", n, r, d)
            lo, s, inv_s = c.quant
            xc, bc = qref.codes(c.x_h, lo, inv_s), qref.codes(c.bank_h, lo, inv_s)
            d2_all = qref.d2_blas(xc, bc)
            ex = qref.excess64(c.x_h, lo, s)
            for k in (k for k in mu.KS if k <= r):
                want_d2, want_i = qref.kneighbors(d2_all, k)
                want_d = qref.dist64(want_d2, np.float32(c.s2), ex)
                for dist, idx, out in flat_results(c, FLAT_ENTRIES["int8"], k):
                    assert np.array_equal(idx.numpy().astype(np.int64), want_i), (n, r, d, k)      # integers: the stable sort, exactly
                    assert qref.ulps32(dist.numpy(), want_d).max() <= ULPS, (n, r, d, k)
                    assert np.array_equal(qref.mean_of(dist, k).view(np.int32), out.numpy().view(np.int32)), (n, r, d, k)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("d", mu.DS)
def test_topk_searches(d, half):
    """k <= R leaves the 3-row bank to the three-nearest kernels."""
    mod, t = (href, half_tests.tau(d)) if half else (ref, l2_tests.tau(d))
    for r in (r for r in mu.RS if r >= max(mu.KS_TOPK)):
        for n in mu.NS:
            c = Flat("half" if half else "l2", n, r, d)
            c.kind = "topk_half" if half else "topk_l2"
            d2_all, a_all = mod.d2_64(c.x_h, c.bank_h), mod.scale_a(c.x_h, c.bank_h)
            for k in mu.KS_TOPK:
                tol = tref.scores_tol(c.x_h, c.bank_h, k, t, mod)
                for dist, idx, out in flat_results(c, FLAT_ENTRIES[c.kind], k):
                    tref.check_topk_against_float64(dist, idx, k, d2_all, a_all, t, max_loose=MAX_LOOSE)
                    assert torch.equal(tref.sequential_mean(dist, k), out), (n, r, d, k)
                    assert (np.abs(out.double().numpy() - mod.patch_scores64(c.x_h, c.bank_h, k)) <= tol).all(), (n, r, d, k)


# ---------------------------------------------------------------- the gallery and the inverted file

def bank_sets(x, bank, m, more):
    """Embedded (queries, bank, norms) + `more` for both kinds of norm margin; the twins are the queries."""
    from self_supervised import ops
    bsq, tsq = ops.row_sqnorms(bank), ops.row_sqnorms(x)
    ex, eb = nan_embedded(x), mu.embedded(bank, m, m, x)[1]
    return (x, bank, bsq), [(ex, eb, mu.embedded(bsq, m, m, fill)[1]) + tuple(more) for fill in (tsq, mu.BSQ_POISON[F32])]


@pytest.mark.parametrize("p", mu.PATCHES)
@pytest.mark.parametrize("d", mu.DS)
def test_gallery_searches(d, p):
    c = mu.GalleryCase(p, d)
    n = c.Q * p
    gal = torch.from_numpy(c.gallery).to(I32).cuda()
    twin_ids = torch.full((1, c.K), c.TWIN, dtype=I32)
    tight, emb = bank_sets(c.x.cuda(), c.bank.cuda(), c.m, (mu.embedded(gal, mu.TILE, mu.TILE, twin_ids)[1],))
    tight = tight + (gal,)
    d2_all, a_all = ref.d2_64(c.x, c.bank), ref.scale_a(c.x, c.bank)
    for k in mu.KS:
        refc = gallery_tests.reference_case(c.x, c.bank, c.gallery, p, k, d2_all, a_all)
        assert 1.0 - refc[4].mean() <= MAX_LOOSE, (p, d, k)                             # on the reference alone, first
        for s in mu.SPLITS:
            tail = (c.Q, p, c.T, c.K, d, k, s)
            (out,) = run_both("ssad_l2_knn_gallery", tight, emb, tail, [((n,), F32)], ((s * n, 3), F32), s > 1, what=(p, d, k, s))
            dist, idx = run_both("ssad_l2_knn_gallery_index", tight, emb, tail, [((n, k), F32), ((n, k), I32)], ((s * n, 3), I64), s > 1,
                                 rows=c.T * p, what=(p, d, k, s))
            assert not (idx // p == c.TWIN).any()
            gallery_tests.check_against_float64(c.x, c.gallery, p, dist, idx, out, k, d2_all, a_all, refc)


@pytest.mark.parametrize("n", mu.NS)
@pytest.mark.parametrize("d", mu.DS)
def test_ivf_searches(d, n):
    from self_supervised import ops
    c = mu.IvfCase(n, d)
    dev = lambda a: torch.as_tensor(a, dtype=I32).cuda()
    offsets, perm, probes = dev(c.offsets), dev(c.perm), dev(c.probes)
    tiles, pairs = ops.ivf_schedule(probes, c.nlist)
    g = int(tiles.shape[1])
    side = (offsets, perm, probes, tiles, pairs)
    fills = (dev(c.offsets[c.TWIN:c.TWIN + 2]), dev(c.twin_rows), torch.full((1, mu.NPROBE), c.TWIN, dtype=I32),
             torch.full((1, g), c.TWIN, dtype=I32), 0)
    tight, emb = bank_sets(c.x.cuda(), c.sorted.cuda(), c.m, [mu.embedded(t, mu.TILE, mu.TILE, f)[1] for t, f in zip(side, fills)])
    tight = tight + side
    d2_all, a_all = ref.d2_64(c.x, c.bank), ref.scale_a(c.x, c.bank)
    part = ((n * mu.NPROBE, 3), I64)
    for k in mu.KS:
        want_d2, want_i, want_a, strict, loose = ivf_ref.reference_case(c.x, c.bank, c.cell_of_row, c.probes, c.nlist, k)
        assert loose <= MAX_LOOSE and (want_i >= 0).all()                               # on the reference alone, first
        tail = (n, d, c.r, c.nlist, mu.NPROBE, g, k)
        (out,) = run_both("ssad_l2_knn_ivf", tight, emb, tail, [((n,), F32)], part, True, what=(n, d, k))
        dist, idx = run_both("ssad_l2_knn_ivf_index", tight, emb, tail, [((n, k), F32), ((n, k), I32)], part, True, rows=c.r,
                             what=(n, d, k))
        idx = idx.numpy().astype(np.int64)
        assert (c.cell_of_row[idx] != c.TWIN).all() and all(c.cell_of_row[r] in c.probes[i] for i in range(n) for r in idx[i])
        d2_row, a_row = np.take_along_axis(d2_all, idx, 1), np.take_along_axis(a_all, idx, 1)
        assert (np.abs(dist.double().numpy() ** 2 - d2_row) <= ivf_ref.TAU * EPS * a_row + 2 * EPS * d2_row).all(), (n, d, k)
        assert (np.abs(d2_row - want_d2) <= ivf_ref.TAU * EPS * (a_row + want_a)).all(), (n, d, k)
        assert np.array_equal(idx[strict], want_i[strict]), (n, d, k)
        assert torch.equal(l2_tests._mean_of(dist, k), out), (n, d, k)


@pytest.mark.parametrize("n", mu.NS)
@pytest.mark.parametrize("d", mu.DS)
def test_ivf_probes(d, n):
    """The coarse step (row_sqnorms, the GEMM, ssad_l2_from_dots and the selection) with twins of the queries beyond the centroids."""
    from self_supervised import ops
    c = mu.IvfCase(n, d)
    real = [g for g in range(c.nlist) if g != c.TWIN]
    cent_h = torch.stack([c.sorted[c.offsets[g]:c.offsets[g + 1]].double().mean(0).float() for g in real])
    nlist = len(real)
    x, cent = c.x.cuda(), cent_h.cuda()
    tight, emb = bank_sets(x, cent, c.m, ())
    d2 = ivf_ref.d2_64(c.x, cent_h)
    order = np.argsort(d2, axis=1, kind="stable")
    sd = np.take_along_axis(d2, order, 1)
    bar = ivf_ref.TAU * EPS * np.take_along_axis(ivf_ref.scale_a(c.x, cent_h), order, 1)
    strict = np.ones((n, mu.NPROBE), dtype=bool)
    for j in range(mu.NPROBE):
        if j > 0:
            strict[:, j] &= sd[:, j] - sd[:, j - 1] > bar[:, j] + bar[:, j - 1]
        strict[:, j] &= sd[:, j + 1] - sd[:, j] > bar[:, j] + bar[:, j + 1]
    assert 1.0 - strict.mean() <= MAX_LOOSE                                             # on the reference alone, first
    want = ops.ivf_probes(*tight, mu.NPROBE)
    for ex, ec, esq in emb:
        got = ops.ivf_probes(ex, ec, esq, mu.NPROBE)
        assert got.dtype == I32 and torch.equal(got, want) and (got >= 0).all() and (got < nlist).all()
    got = want.cpu().numpy().astype(np.int64)
    assert np.array_equal(got[strict], ivf_ref.probes64(c.x, cent_h, mu.NPROBE)[strict])
    assert (np.abs(np.take_along_axis(d2, got, 1) - sd[:, :mu.NPROBE]) <= 2 * bar[:, :mu.NPROBE]).all()


# ---------------------------------------------------------------- the helpers

def helper(name, ins, tail, out_specs, part_spec=None, part_written=False, args=None):
    """`name` on ins = (tight inputs, embedded inputs) in the usual argument order, or in that of args(inputs) -> the host outputs."""
    if args is None:
        return run_both(name, ins[0], [ins[1]], tail, out_specs, part_spec, part_written)
    want, _ = run(name, args(ins[0]), out_specs, part_spec)
    got, part = run(name, args(ins[1]), out_specs, part_spec)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), name
    assert part is None or (mu.all_written(part) if part_written else mu.untouched(part)), name
    return [w.cpu() for w in want]


def margins(*ins):
    """(tight inputs, the same between NaN margins)"""
    return ins, [nan_embedded(t) for t in ins]


@pytest.mark.parametrize("d", mu.DS + (mu.D_UNFUSED,))
def test_row_helpers(d):
    """ssad_l2_normalize_rows, ssad_row_sqnorms, ssad_rows_to_half and ssad_rows_to_int8: one wave or one thread group per row."""
    for n in mu.NS + mu.RS:
        x_h = mu.gauss(n, d, seed=100 + d + n)
        x = x_h.cuda()
        (xn,) = helper("ssad_l2_normalize_rows", margins(x), (n, d), [((n, d), F32)])
        want = cref.unit_rows64(x_h)
        assert (np.abs(xn.double().numpy() - want) <= (d + 2) * EPS * np.abs(want)).all()        # the norm's bound (below), then one root
        (sq,) = helper("ssad_row_sqnorms", margins(x), (n, d), [((n,), F32)])
        s64 = ref.sqnorms64(x_h)
        assert (np.abs(sq.double().numpy() - s64) <= (d + 2) * EPS * s64).all()                   # test_hip_knn_l2.test_row_sqnorms
        if d % 32:
            continue
        xh, hsq = helper("ssad_rows_to_half", margins(x), (n, d), [((n, d), F16), ((n,), F32)])
        h = href.h(x_h)
        assert np.array_equal(half_tests.half_bits(xh), h.view(np.uint16))
        s64 = (h.astype(np.float64) ** 2).sum(1)
        assert (np.abs(hsq.double().numpy() - s64) <= (d + 2) * EPS * s64).all()                  # test_hip_knn_l2_half.test_rows_to_half
        wide = x_h.clone()
        wide[n // 2, ::3] *= 4.0                                                                    # one row leaves the coded range
        lo, s, inv_s, _ = (float(v) for v in qref.quantiser_of(x_h))
        codes, csq, ex = helper("ssad_rows_to_int8", margins(wide.cuda()), (n, d, lo, inv_s, s), [((n, d), I8), ((n,), I32), ((n,), F32)])
        want_c = qref.codes(wide, lo, inv_s)
        assert np.array_equal(codes.numpy(), want_c) and np.array_equal(csq.numpy().astype(np.int64), qref.sq64(want_c))
        e64 = qref.excess64(wide, lo, s)
        assert (ex.numpy()[e64 == 0] == 0).all() and (np.abs(ex.double().numpy() - e64) <= (d + 2) * EPS * e64).all()


@pytest.mark.parametrize("d", mu.DS)
def test_gallery_helpers(d):
    """ssad_group_means and ssad_l2_direct at the bars of tests/test_hip_knn_gallery.py."""
    for p in mu.PATCHES:
        x_h = mu.gauss(3 * p, d, seed=200 + d + p) + 0.25
        (got,) = helper("ssad_group_means", margins(x_h.cuda()), (3, p, d), [((3, d), F32)])
        want = gref.descriptors64(x_h, p)
        assert (np.abs(got.double().numpy() - want) <= EPS * np.abs(want)).all()
    for n in mu.NS:
        for r in mu.RS:
            q_h, b_h = mu.gauss(n, d, seed=300 + d + n) + 0.5, mu.gauss(r, d, seed=400 + d + r) + 0.5
            q_h[0] = b_h[r - 1]
            (got,) = helper("ssad_l2_direct", margins(q_h.cuda(), b_h.cuda()), (n, r, d), [((n, r), F32)])
            want = gref.direct_d2_64(q_h, b_h)
            assert (np.abs(got.double().numpy() - want) <= l2_direct_bar(d, want)).all() and float(got[0, r - 1]) == 0.0


def test_l2_from_dots():
    for n in mu.NS:
        for r in mu.RS:
            sim, qsq, bsq = mu.gauss(n, r, 1), mu.gauss(n, 1, 2).abs().reshape(-1) * 50, mu.gauss(r, 1, 3).abs().reshape(-1) * 50
            (got,) = helper("ssad_l2_from_dots", margins(sim.cuda(), qsq.cuda(), bsq.cuda()), (n, r), [((n, r), F32)])
            want = np.maximum((qsq.numpy()[:, None] + bsq.numpy()[None, :]) - np.float32(2) * sim.numpy(), np.float32(0))
            assert want.dtype == np.float32 and np.array_equal(got.numpy(), want)              # test_hip_knn_l2: the kernel's expression


@pytest.mark.parametrize("cosine", [False, True], ids=["values", "similarities"])
def test_rows_smallest_index_and_rows_argmax(cosine):
    """Both senses of ssad_rows_smallest_index, one column past its 4096-column chunk included, and ssad_rows_argmax: exact."""
    from self_supervised import ops
    for q in mu.NS:
        for r in mu.RS + (ops.ROWS_SMALLEST_COLS_PER_WG + 1,):
            m_h = (0.6 * mu.gauss(q, r, seed=500 + q + r)).clamp_(-1.5, 1.5)
            vals64 = ((1.0 - m_h).clamp_(0.0, 2.0) if cosine else m_h).double().numpy()
            m = m_h.cuda()
            for b in (1, 32):
                bp = min(b, r)
                want_v, want_c = cref.smallest_stable(vals64, b)
                for wgs in sorted({ops.rows_smallest_workgroups(r, b), 3}):
                    order = lambda ins: (lambda part, outs: [P(ins[0]), q, r, b, int(cosine), wgs, P(part), P(outs[0]), P(outs[1])])
                    vals, cols = helper("ssad_rows_smallest_index", margins(m), None, [((q, bp), F32), ((q, bp), I32)],
                                        ((q * wgs, b), I64), True, args=order)
                    assert np.array_equal(cols.numpy().astype(np.int64), want_c) and np.array_equal(vals.double().numpy(), want_v)
            if not cosine:
                order = lambda ins: (lambda part, outs: [P(ins[0]), q, r, P(outs[0]), P(outs[1])])
                val, flat = helper("ssad_rows_argmax", margins(m), None, [((q,), F32), ((q,), I64)], args=order)
                assert torch.equal(val, m_h.max(1).values)
                assert np.array_equal(flat.numpy(), np.arange(q) * r + m_h.double().numpy().argmax(1))


@pytest.mark.parametrize("d", mu.DS)
def test_reweight_kernels(d):
    """ssad_knn_reweight and ssad_knn_reweight_l2.  The bank's last row is NaN and in range; the margins of mstar and nbr name it."""
    from self_supervised import ops
    rng = np.random.RandomState(d)
    for q in mu.NS:
        for r in mu.RS:
            bp = min(9, r)
            xs_h, rows_h = mu.gauss(q, d, seed=600 + d + q), mu.gauss(r, d, seed=700 + d + r)
            smax_h = torch.from_numpy(rng.uniform(0.5, 1.5, size=q).astype(np.float32))
            mstar_h, nbr_h = rng.randint(0, r, size=q), rng.randint(0, r, size=(q, bp))
            dev = lambda a: torch.as_tensor(a, dtype=I32).cuda()
            nan_row = torch.full((1, d), mu.NAN)
            ids = [mu.embedded(dev(a), mu.TILE, mu.TILE, r)[1] for a in (mstar_h, nbr_h)]
            for l2 in (False, True):
                bank_h = rows_h if l2 else torch.from_numpy(cref.unit_rows64(rows_h).astype(np.float32))
                bank = torch.cat([bank_h, nan_row]).cuda()
                tight = (xs_h.cuda(), bank, dev(mstar_h), dev(nbr_h), smax_h.cuda())
                emb = (nan_embedded(tight[0]), nan_embedded(bank), ids[0], ids[1], nan_embedded(tight[4]))
                name = "ssad_knn_reweight_l2" if l2 else "ssad_knn_reweight"
                (got,) = helper(name, (tight, emb), (q, d, r + 1, bp), [((q,), F32)])
                got = got.double().numpy()
                x64, b64 = xs_h.double().numpy(), bank_h.double().numpy()
                if l2:
                    d_m = np.sqrt(((x64 - b64[mstar_h]) ** 2).sum(1))
                    d_n = np.sqrt(((x64[:, None, :] - b64[nbr_h]) ** 2).sum(2))
                    dmax = d_n.max(1)
                    want = (1.0 - np.exp(d_m - dmax) / np.exp(d_n - dmax[:, None]).sum(1)) * smax_h.double().numpy()
                    unit = EPS * smax_h.double().numpy() * np.maximum(1.0, dmax)
                    assert (np.abs(got - want) <= l2_tests.REW_TAU * unit).all(), (q, r, d)
                else:
                    dist = cref.distances64(xs_h, bank_h)
                    w = 1.0 - np.exp(dist[np.arange(q), mstar_h]) / np.exp(np.take_along_axis(dist, nbr_h, 1)).sum(1)
                    # test_hip_knn_index holds a reweighted score (a weight times an s_max of at most 2) to twice the distance bound
                    assert (np.abs(got - w * smax_h.double().numpy()) <= 2 * DIST_TOL).all(), (q, r, d)
