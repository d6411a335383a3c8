"""The GDE table without a GPU (tests/gde_table.py): the rows the table exists for are all there, every branch is reached (over the launch
geometry restated in Python), every bar is finite and positive, e_ss < ss for every scorer row, the integer rows stay below 2^24, and the
references themselves agree with scipy's mahalanobis and with math.fsum.

Without a GPU the rows of ssad_l2_normalize_rows are replaced by x / ||x|| computed in float64 and rounded to fp32 (within a few ulps of
them): bars and coverage are computed from these, never a comparison with a kernel."""
import math

import numpy as np
import pytest
import torch

import gde_table as T

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the fit reference needs an extended-precision longdouble"


def test_row_ids_unique_and_listed_values_present():
    ids = [r.id for r in T.SCORE + T.INTEGER + T.FIT] + [f"selector_{j}_{k}" for j, k in T.SEL_PAIRS]
    assert len(ids) == len(set(ids))
    gen = [r for r in T.SCORE if r.kind == "gen"]
    want = {(d, n, nz) for d in (32, 160) for n in (1, 127, 128, 129, 300) for nz in (0, 1)}
    want |= {(d, 129, nz) for d in (96, 128, 256, 1024) for nz in (0, 1)}
    assert {(r.d, r.n, r.normalize) for r in gen} == want and len(gen) == len(want)
    assert {(r.d, r.n, r.normalize) for r in T.SCORE if r.kind == "degenerate"} == {(160, 129, 0), (160, 129, 1)}
    assert {(r.d, r.n) for r in T.INTEGER} == {(96, 129), (160, 129), (1024, 129)}
    d = T.SEL_D
    assert (T.SEL_D, T.SEL_N) == (160, 129) and T.SEL_PAIRS == [(d - 1, 0), (d - 1, 31), (d - 1, 32), (d - 1, 63), (d - 1, 64), (d - 1, d - 1),
                                                                (0, 0), (127, 127), (128, 0), (128, 128)]
    assert all(k <= j < d for j, k in T.SEL_PAIRS)
    assert (T.INDEP_D, T.INDEP_N, T.INDEP_POSITIONS) == (160, 300, (0, 63, 127, 128, 299))
    fit = {(d, n, nz) for d in (32, 96, 160, 512) for n in (1, 2, 33, 257, 588) for nz in (0, 1)}
    fit |= {(1088, 3, nz) for nz in (0, 1)} | {(1120, 3, nz) for nz in (0, 1)} | {(32, 262400, nz) for nz in (0, 1)}
    assert {(r.d, r.n, r.normalize) for r in T.FIT} == fit and len(T.FIT) == len(fit)
    assert T.BAD_D_FIT == (0, 48, 4128) and T.BAD_D_SCORE == (0, 48, 1056)


@pytest.mark.parametrize("case", list(T.SCORE_CASES))
def test_every_scorer_case_is_reached(case):
    assert [r.id for r in T.SCORE if T.SCORE_CASES[case](r)], f"no row reaches: {case}"


@pytest.mark.parametrize("case", list(T.FIT_CASES))
def test_every_fit_case_is_reached(case):
    assert [r.id for r in T.FIT if T.FIT_CASES[case](r)], f"no row reaches: {case}"


def test_restated_geometry():
    g = T.fit_geometry
    assert g(257, 512)[:4] == (8, 36, 2, 129) and g(588, 512)[:4] == (8, 36, 3, 196)
    assert g(3, 1088) == T.Geometry(17, 153, 1, 3, 1, 3, 1, 3) and g(300, 1024).tiles == 136
    assert g(262400, 32) == T.Geometry(1, 1, 1022, 257, 2035, 129, 2035, 129)
    assert g(588, 96)[4:] == (5, 118, 10, 59) and g(33, 160) == T.Geometry(3, 6, 1, 33, 1, 33, 1, 33)
    assert g(1, 32) == T.Geometry(1, 1, 1, 1, 1, 1, 1, 1)
    for r in T.FIT:                                                     # no empty trailing block, every row in exactly one
        q = g(r.n, r.d)
        for s, per in ((q.s, q.sc_rows), (q.s1, q.cs_rows), (q.s3, q.m4_rows)):
            assert (s - 1) * per < r.n <= s * per
    assert T.k_cols(160).tolist() == [128] * 128 + [160] * 32 and T.k_cols(96).tolist() == [96] * 96
    k = T.k_cols(1024)
    assert k[0] == 128 and k[127] == 128 and k[128] == 256 and k[1023] == 1024 and T.w_tiles(1024) == 8 and T.w_tiles(160) == 2
    assert T.w_tiles(128) == 1 and T.w_tiles(96) == 1


def _rows_seen(c):
    return T.host_normalized(c.x) if c.row.normalize else c.x


@pytest.mark.parametrize("row", T.SCORE, ids=lambda r: r.id)
def test_scorer_bars(row):
    """Every bar finite and positive, e_ss < ss (the first-order square root), the poisoned W is poisoned exactly above the diagonal, the
    reference is scipy's mahalanobis on three rows."""
    from scipy.spatial.distance import mahalanobis
    c = T.score_case(row)
    v = _rows_seen(c)
    want, bar, ss, e_ss = T.score_ref(v, c.mu_hi, c.mu_lo, c.w)
    assert np.isfinite(bar).all() and (bar > 0).all() and np.isfinite(want).all() and (want > 0).all()
    assert (e_ss < ss).all()
    assert (e_ss <= 2.0 ** -9 * ss).all(), float((e_ss / ss).max())           # the second order of the square root: e_ss / (4 ss) <= 2^-11
    p = T.poisoned(c.w)
    up = torch.triu(torch.ones(row.d, row.d, dtype=torch.bool), 1)
    assert bool(torch.isnan(p[up]).all()) and torch.equal(p[~up], c.w[~up]) and bool((c.w[up] == 0).all())
    assert bool((torch.diagonal(c.w) > 0).all())
    w64 = c.w.double().numpy()
    vi = w64.T @ w64
    mu = (c.mu_hi.double() + c.mu_lo.double()).numpy()
    for i in sorted({0, row.n // 2, row.n - 1}):
        ref = mahalanobis(v[i].double().numpy(), mu, vi)
        assert abs(ref - want[i]) <= 1e-9 * ref, (i, ref, want[i])
    if row.kind == "degenerate":                                              # rows at 1e-4 of their norm from the mean
        dist = (v.double() - torch.from_numpy(mu)).norm(dim=1) / v.double().norm(dim=1)
        assert float(dist.max()) < 1e-3


def test_fitted_w_is_dense_below_the_diagonal():
    for d in T.SCORE_D:
        w = T.score_fit(d, 1)[2]
        assert float((torch.tril(w) != 0).double().mean()) > 0.49             # every element below the diagonal is a non-zero


@pytest.mark.parametrize("row", T.INTEGER, ids=lambda r: r.id)
def test_integer_rows_stay_exact(row):
    c = T.int_case(row)
    want, reach, ssmax = T.int_ref(c)
    assert reach < T.INT_LIMIT and ssmax < T.INT_LIMIT == 2 ** 24
    assert bool((torch.tril(c.w).abs() == torch.tril(torch.ones(row.d, row.d))).all()) and bool((c.mu_lo == 0).all())    # dense: +-1 everywhere
    # the reference: float64 ||W c|| of the same integers
    y = (c.x.double() - c.mu_hi.double()) @ c.w.double().T
    assert torch.equal(want, y.norm(dim=1).float()) or float((want.double() - y.norm(dim=1)).abs().max()) <= 2.0 ** -24 * float(want.max())
    assert bool((want > 0).all())


def test_selector_rows():
    x = T.sel_case()
    assert bool((x[T.SEL_ZERO_ROW] == 0).all()) and int((x == 0).all(1).sum()) == 1
    assert T.sel_values_ok(x) and T.sel_values_ok(T.host_normalized(x))
    assert not T.sel_values_ok(torch.tensor([2.0 ** -61])) and T.sel_values_ok(torch.tensor([0.0, -2.0 ** -60]))
    for j, k in T.SEL_PAIRS:
        w = T.sel_w(j, k)
        assert int(torch.isnan(w).sum()) == T.SEL_D * (T.SEL_D - 1) // 2 and float(torch.nan_to_num(w).sum()) == 1.0 and w[j, k] == 1.0
    # sqrt(fl(x^2)) == |x| in fp32 on the values the rows hold
    v = T.host_normalized(x).reshape(-1)
    assert torch.equal(torch.sqrt(v * v), v.abs())


@pytest.mark.parametrize("row", [r for r in T.FIT if r.n <= 588], ids=lambda r: r.id)
def test_fit_bars_and_reference(row):
    x = T.fit_case(row)
    v = T.host_normalized(x) if row.normalize else x
    ref = T.fit_ref(row, v)
    for nm in ("mean", "scatter", "m4"):
        want, bar = ref[nm]
        assert np.isfinite(want).all() and np.isfinite(bar).all(), (row.id, nm)
        if row.n == 1 and nm != "mean":                   # one row is its own mean: every centred value, so scatter and m4, is exactly 0
            assert not want.any() and not bar.any()
        else:
            assert (bar > 0).all(), (row.id, nm)
    xl, mean, scatter, m4 = ref["_long"]
    col, a, b = row.d // 3, row.d - 1, row.d // 2
    xs = v.double().numpy()
    fs_mean = math.fsum(xs[:, col].tolist()) / row.n
    assert abs(float(mean[col]) - fs_mean) <= 4 * T.UD * abs(fs_mean) + 1e-300
    # one scatter element from exact products of the centred doubles (the centring itself is the longdouble reference's)
    ca, cb = (xl[:, a] - mean[a]).astype(np.float64), (xl[:, b] - mean[b]).astype(np.float64)
    fs = math.fsum((float(p) * float(q)) for p, q in zip(ca, cb))
    mag = math.fsum(abs(float(p) * float(q)) for p, q in zip(ca, cb))
    assert abs(float(scatter[a, b]) - fs) <= 8 * T.UD * mag + 1e-300
    assert np.array_equal(scatter, scatter.T)
    if row.n == 1:
        assert not scatter.any() and float(m4) == 0.0


def test_long_fit_row_bars():
    row = [r for r in T.FIT if r.n == T.FIT_LONG[1] and r.normalize == 0][0]
    ref = T.fit_ref(row, T.fit_case(row))
    for nm in ("mean", "scatter", "m4"):
        assert np.isfinite(ref[nm][1]).all() and (ref[nm][1] > 0).all()
    xl, mean, _, _ = ref["_long"]
    assert abs(float(mean[7]) - math.fsum(xl[:, 7].astype(np.float64).tolist()) / row.n) <= 4 * T.UD * abs(float(mean[7]))


def test_no_row_is_large():
    for r in T.SCORE + T.INTEGER:
        assert 4 * (r.n * r.d + 2 * r.d * r.d + 2 * r.d + r.n) <= T.MAX_HOST_BYTES
    for r in T.FIT:
        assert T.fit_host_bytes(r) <= T.MAX_HOST_BYTES
    assert max(T.fit_host_bytes(r) for r in T.FIT) == 4 * 262400 * 32 + 8 * (32 * 32 + 33)
    assert 8 * 1088 * 1088 < 10 << 20 and 4 * 1024 * 1024 == 4 << 20
