"""The scoring-tail table without a GPU (tests/scoring_tail_table.py): every case the table exists for is reached by a row (over the
dispatch rules restated in Python); the tiled kernel's LDS indices stay inside what the host's rmax allocates; every reference agrees
with an independent statement (sklearn's brute-force cosine neighbours, zero rows included; oracle.scoring.upsample and F.interpolate
in float64; einsum; permute); and every bar is non-vacuous: a reference with one wrong tap, an off-by-one row or h and w swapped fails it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scoring_tail_table as T
from oracle import scoring as osc


def test_row_ids_unique_and_listed_values_present():
    ids = [T.row_id(kr) for kr in T.ROWS]
    assert len(ids) == len(set(ids))
    assert {(r.n, r.d) for r in T.L2} >= {(n, d) for n in (1, 3, 4, 5, 1025) for d in (1, 32, 63, 64, 65, 100, 512, 2048)}
    assert {(r.h, r.w, r.ks, r.target) for r in T.BLUR if r.kernel == "single"} == {
        (4, 4, 7, 8), (7, 7, 7, 16), (7, 7, 1, 16), (9, 5, 3, 10), (40, 100, 7, 64), (78, 78, 7, 156), (16, 16, 5, 8), (16, 16, 7, 16)}
    assert {(r.h, r.w, r.ks, r.target) for r in T.BLUR if r.kernel != "single"} >= {
        (79, 78, 7, 156), (60, 110, 7, 128), (110, 60, 7, 65), (80, 80, 7, 40), (90, 90, 7, 200), (96, 96, 7, 80)}
    assert T.REPACK == [(5, 3, 2, 4), (1, 1, 1, 1), (64, 3, 7, 7), (7, 64, 1, 1)] and len(set(T.REPACK[0])) == 4
    assert (T.ZN_N, T.ZN_R, T.ZN_D) == (130, 131, 32)
    assert set(T.ZN_QUERY.values()) == {"zero", "underflow"} == set(T.ZN_BANK.values())
    assert any(i >= 128 for i in T.ZN_QUERY) and any(i >= 128 for i in T.ZN_BANK) and any(i < 128 for i in T.ZN_BANK)
    assert {(k, nb) for k, nb in T.KNN_BAD_K} >= {(0, 5), (4, 5), (3, 2)}


@pytest.mark.parametrize("table,cases", [("L2", "L2_CASES"), ("KNN", "KNN_CASES"), ("CAM", "CAM_CASES"), ("BLUR", "BLUR_CASES")])
def test_every_case_is_reached(table, cases):
    rows = getattr(T, table)
    for name, pred in getattr(T, cases).items():
        assert pred(rows), f"{table}: no row reaches: {name}"


# ---- blur: dispatch and the construction of rmax ----
def test_blur_rows_name_their_kernel_and_the_boundary_is_the_lds_rule():
    for r in T.BLUR:
        kernel, lds, tiles, span, rmax = T.blur_geometry(r.h, r.w, r.ks, r.target)
        assert kernel == r.kernel, r.id
        assert r.ks % 2 == 1 and r.ks // 2 < r.h and r.ks // 2 < r.w            # the entry's own argument check
    assert T.blur_geometry(78, 78, 7, 156)[:2] == ("single", (2 * 78 * 78 + 7) * 4) and (2 * 78 * 78 + 7) * 4 <= 48 * 1024
    assert T.blur_geometry(79, 78, 7, 156)[0] == "tiled" and (2 * 79 * 78 + 7) * 4 > 48 * 1024
    assert T.blur_geometry(79, 79, 7, 156)[0] == "tiled"                         # 78 is the largest square map of the single kernel
    assert T.blur_geometry(110, 60, 7, 65) == ("refused", 104068, 2, 64, 111)
    assert T.blur_geometry(80, 80, 7, 40)[2:] == (1, 40, 83)


@pytest.mark.parametrize("r", [r for r in T.BLUR if r.kernel == "tiled"], ids=lambda r: r.id)
def test_tiled_lds_indices_stay_inside_rmax(r):
    """"nr, nc <= rmax by construction (host)": the staged rows and columns of every tile, with the kernel's float32 expressions."""
    _, lds, tiles, span, rmax = T.blur_geometry(r.h, r.w, r.ks, r.target)
    pad = r.ks // 2
    sw = rmax + 2 * pad
    seen_one_wide = False
    for nr, nc, th, tw in T.tile_extents(r.h, r.w, r.target, tiles):
        assert 1 <= nr <= rmax and 1 <= nc <= rmax, (r.id, nr, nc, rmax)
        assert (nr + 2 * pad - 1) * sw + (nc + 2 * pad - 1) < sw * sw           # the last src element staged
        assert (nr - 1) * rmax + (nc - 1) < rmax * rmax                         # the last blr element written
        assert (sw * sw + rmax * rmax + r.ks) * 4 == lds <= 64 * 1024
        seen_one_wide |= tw == 1 or th == 1
    assert seen_one_wide == (r.target % 64 == 1)
    # every bilinear tap of every output pixel falls inside the rows its tile stages
    for extent in (r.h, r.w):
        i0, i1, _ = T.coords(extent, r.target)
        for t in range(tiles):
            a, b = t * 64, min(t * 64 + 64, r.target) - 1
            lo, hi = int(i0[a]), min(int(i0[b]) + 1, extent - 1)
            assert lo <= i0[a:b + 1].min() and i1[a:b + 1].max() <= hi


def test_fused_and_plain_coordinates_take_the_same_source_rows():
    """The bar's coordinate term assumes a fused multiply-add moves lambda, never the integer part; sigma is the same float either way."""
    for r in T.BLUR:
        for extent in (r.h, r.w):
            a, b = T.coords(extent, r.target, False), T.coords(extent, r.target, True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), r.id
            assert np.abs(a[2].astype(np.float64) - b[2].astype(np.float64)).max() <= 2.0 ** -24 * max(extent, 1)
        assert T.sigma_of(r.ks, False) == T.sigma_of(r.ks, True), r.ks
    assert T.blur_c(7) == 87 and T.blur_c(1) == 27


# ---- blur: the reference ----
@pytest.mark.parametrize("r", [r for r in T.BLUR if r.kernel != "refused" and r.ks == 7], ids=lambda r: r.id)
def test_blur_reference_against_the_oracle_in_float64(r):
    """oracle.scoring.upsample restates torchvision's blur and F.interpolate; in float64 its coordinates are exact, the table's are the
    kernel's float32 ones: the two differ by at most two roundings of a coordinate <= max(h, w) times the neighbouring difference."""
    maps, _ = T.blur_case(r)
    want, bar = T.blur_ref(maps, r.ks, r.target)
    ref = osc.upsample(torch.from_numpy(maps).double()[:, None], r.target)[:, 0].numpy()
    b = F.relu(osc.gaussian_blur(torch.from_numpy(maps).double()[:, None], 7))
    assert np.array_equal(ref, F.interpolate(b, (r.target, r.target), mode="bilinear")[:, 0].numpy())      # a scale per axis when h != w
    mag, _, _ = T.blur_op(np.abs(maps.astype(np.float64)), r.ks, r.target, False)
    tol = bar + 4 * T.U * max(r.h, r.w) * mag
    assert (np.abs(want - ref) <= tol).all(), (r.id, float((np.abs(want - ref) / tol).max()))
    assert np.isfinite(bar).all() and (bar > 0).all()


def test_blur_reference_small_cases_against_loops_and_torchvision_taps():
    r = T.BLUR[3]                                                                # 9 x 5, ks = 3
    maps, _ = T.blur_case(r)
    k1 = T.taps(7)
    assert np.abs(k1 - osc.gaussian_kernel1d(7).numpy()).max() < 1e-7 and abs(k1.sum() - 1) < 1e-15
    b = torch.from_numpy(maps).double()[:, None]
    k3 = torch.from_numpy(T.taps(3))
    p = F.pad(b, [1, 1, 1, 1], mode="reflect")
    blurred = F.relu(F.conv2d(p, (k3[:, None] * k3[None, :])[None, None]))[:, 0].numpy()
    want, _ = T.blur_ref(maps, 3, r.target)
    for i in range(r.n):
        loops = osc.bilinear_loops(blurred[i].astype(np.float32), r.target)
        assert np.abs(want[i] - loops).max() < 1e-6
    # the all-negative map: exactly 0; the constant map: the constant within the bar
    _, kinds = T.blur_case(r)
    assert (want[kinds.index("negative")] == 0).all() and np.abs(want[kinds.index("constant")] - np.float32(0.7)).max() < 1e-12


# ---- blur: the bar is not vacuous ----
def _mutants(r, maps):
    k1 = T.taps(r.ks).copy()
    k1[0], k1[1] = k1[1], k1[0]                                                  # one wrong tap (two swapped)
    yield "one wrong tap", T.blur_op(maps.astype(np.float64), r.ks, r.target, True, k1=k1)[0]
    shifted = np.roll(maps, 1, axis=1)                                           # an off-by-one row
    yield "off-by-one row", T.blur_op(shifted.astype(np.float64), r.ks, r.target, True)[0]
    if r.h != r.w:                                                               # h and w swapped in the indexing
        sw = maps.reshape(maps.shape[0], r.w, r.h)
        yield "h and w swapped", T.blur_op(sw.astype(np.float64), r.ks, r.target, True)[0]


@pytest.mark.parametrize("r", [r for r in T.BLUR if r.kernel != "refused" and r.ks > 1], ids=lambda r: r.id)
def test_blur_bar_rejects_wrong_taps_rows_and_swapped_extents(r):
    maps, kinds = T.blur_case(r)
    want, bar = T.blur_ref(maps, r.ks, r.target)
    i = kinds.index("rand")
    names = []
    for name, wrong in _mutants(r, maps):
        err = np.abs(wrong[i] - want[i])
        assert (err > bar[i]).mean() > 0.5, (r.id, name, float((err > bar[i]).mean()))
        assert err.max() > 100 * bar[i].max(), (r.id, name)
        names.append(name)
    assert len(names) == (3 if r.h != r.w else 2)


# ---- l2norm, knn_mean and the zero-norm rows ----
def test_l2_rows_keep_the_bars_assumptions():
    for r in T.L2:
        x = T.l2_case(r)
        assert T.l2_squares_are_normal(x), r.id
        want, bar = T.l2_ref(x)
        zero = T.sum_sq_is_zero(x)
        assert np.isfinite(want).all() and np.isfinite(bar).all()
        live = ~zero
        assert np.abs((want[live] ** 2).sum(axis=1) - 1).max(initial=0) < 1e-12
        assert (bar[live][want[live] != 0] > 0).all()
        for i in range(r.n):
            kind = T.l2_kind(r, i)
            assert zero[i] == (kind in ("zero", "underflow")), (r.id, i)
            if zero[i]:                                                          # the fp32 sum of squares IS 0, in fp32 arithmetic
                assert np.float32((x[i] * x[i]).sum(dtype=np.float32)) == 0 and np.array_equal(want[i], x[i].astype(np.float64))
            if kind == "one":
                assert (x[i] != 0).sum() == 1 and set(np.unique(want[i])) == {-1.0, 0.0} or r.d == 1
        if r.n == 1025:
            assert np.abs(x).max() > 1e14 and 0 < np.abs(x[x != 0]).min() < 1e-29


def test_l2_bar_rejects_a_dropped_element_and_a_wrong_row():
    r = [q for q in T.L2 if (q.n, q.d) == (5, 65)][0]
    x = T.l2_case(r)
    want, bar = T.l2_ref(x)
    dropped = x.astype(np.float64)[:, :64]                                       # the norm without the ragged last element
    wrong = x.astype(np.float64) / np.sqrt((dropped ** 2).sum(axis=1))[:, None]
    assert (np.abs(wrong[0] - want[0]) > bar[0]).any()
    assert (np.abs(np.roll(want, 1, axis=0)[:3] - want[:3]) > bar[:3]).any()


def test_l2norm_then_knn_against_sklearn_zero_rows_included():
    """The two references chained -- rows by l2_ref, distances, knn_ref's selection -- against NearestNeighbors(metric='cosine',
    algorithm='brute') on the zero-norm case: a zero or underflowing row is at distance 1 from every row, on either side."""
    x, bank = T.zero_norm_case()
    ds, mean, bar = T.zero_norm_ref(x, bank)
    sk = T.sklearn_distances(x, bank)
    assert sk.dtype == np.float32 and np.abs(sk.astype(np.float64) - ds).max() <= bar
    for i in T.ZN_QUERY:
        assert (sk[i] == 1).all() and (ds[i] == 1).all()
    xn, bn = T.l2_ref(x)[0], T.l2_ref(bank)[0]
    sim = (xn @ bn.T).astype(np.float32)
    for j in T.ZN_BANK:
        assert (np.abs(sim[:, j]) < 1e-25).all()
    bits, ref, kbar = T.knn_ref(sim, T.ZN_K)
    assert np.abs(bits.astype(np.float64) - sk.astype(np.float64).mean(axis=1)).max() <= 2 * bar
    assert (np.abs(bits.astype(np.float64) - ref) <= kbar).all()
    # before the rule a zero bank row sat at distance 0 (fmax(NaN, 0)) from every query: that answer is outside the bar everywhere
    pulled = np.sort(np.concatenate([ds, np.zeros((T.ZN_N, 1))], axis=1), axis=1)[:, :T.ZN_K].mean(axis=1)
    assert (np.abs(pulled - mean) > 1000 * bar).all()
    # the oracle follows the same rule
    got, dk, _ = osc.cosine_knn_mean(bank, x, T.ZN_K)
    assert np.isfinite(got).all() and np.abs(dk.astype(np.float64) - ds).max() <= 2 * bar and (got[list(T.ZN_QUERY)] == 1).all()


@pytest.mark.parametrize("r", T.KNN, ids=lambda r: r.id)
def test_knn_reference_is_selection_plus_rounded_steps(r):
    sim = T.knn_case(r)
    bits, ref, bar = T.knn_ref(sim, r.k)
    d = torch.from_numpy(sim).double().neg().add(1).clamp(0, 2)
    want = d.topk(r.k, dim=1, largest=False).values.mean(1).numpy()
    assert np.abs(want - ref).max() < 1e-7                                       # 1 - sim in fp32 against float64
    assert (np.abs(bits.astype(np.float64) - ref) <= bar).all() and bits.dtype == np.float32
    if r.kind == "ties" and r.nb >= 63:
        ds = np.sort(np.clip(1 - sim, 0, 2), axis=1)
        assert (ds[:, r.k - 1] == ds[:, r.k]).any() or (ds[:, 0] == ds[:, 1]).any()
    if r.kind == "equal":
        assert (bits == np.clip(np.float32(1) - sim[:, 0], 0, 2)).all() or r.k == 3   # (d + d + d) / 3 may round


# ---- gradcam, repack ----
@pytest.mark.parametrize("r", T.CAM[::3], ids=lambda r: r.id)
def test_gradcam_reference_against_einsum(r):
    act, wide = T.cam_case(r)
    want, bar = T.cam_ref(r, act, wide)
    alpha = torch.from_numpy(wide)[:, r.lead:r.lead + r.c].double()
    ref = torch.einsum("bpc,bc->bp", torch.from_numpy(act).double(), alpha).numpy()
    assert np.allclose(ref, want, rtol=1e-12, atol=1e-12) and (bar > 0).all() and np.isfinite(bar).all()
    if r.b == 3 and r.c > 1:                                                     # the neighbouring image's alpha fails the bar
        other = torch.einsum("bpc,bc->bp", torch.from_numpy(act).double(), alpha.roll(1, 0)).numpy()
        assert (np.abs(other - want) > bar).mean() > 0.9
    if r.stride > r.c:                                                           # the unsliced columns fail it
        off = torch.einsum("bpc,bc->bp", torch.from_numpy(act).double(), torch.from_numpy(wide)[:, :r.c].double()).numpy()
        assert (np.abs(off - want) > bar).mean() > 0.9


def test_repack_shapes_tell_every_axis_apart():
    o, i, kh, kw = T.REPACK[0]
    w = torch.arange(o * i * kh * kw).reshape(o, i, kh, kw)
    perms = {p: w.permute(*p).contiguous().reshape(-1) for p in ((0, 2, 3, 1), (0, 3, 2, 1), (1, 2, 3, 0), (0, 1, 2, 3))}
    assert all(not torch.equal(perms[(0, 2, 3, 1)], v) for p, v in perms.items() if p != (0, 2, 3, 1))
