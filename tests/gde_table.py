"""The GDE table: the seven kernels of csrc/gde.hip behind ssad_gaussian_fit_stats and ssad_mahalanobis_fused, at the smallest shapes that
reach each branch, compared per element against float64 / longdouble on the CPU, over buffers between poisoned guards (Arena, within,
twice of tests/bn_table.py).

Shared by tests/test_gde_table.py (rows, coverage, the references themselves, finite bars: no GPU) and tests/test_hip_gde_paths.py (the
kernels).

Geometry, restated from the documented rules (NOT read back from the library):
  scorer     one workgroup scores 128 queries over all of W; W is walked in tiles of 128 rows, tile t contracts columns
             0 .. min(D, 128 (t + 1)) - 1 in steps of 32: K_j = min(D, 128 ceil((j + 1) / 128)) columns for row j.  Rows of the last tile
             past D and queries past N are out-of-range buffer offsets (zeros).  Inside the diagonal 128 x 128 block the strict upper
             triangle is loaded and replaced by zeros while staging: every scorer, integer and selector row passes it as NaN, and every
             scorer and integer row is run again over the same W with +0 there: the same bits.
  fit        T = ceil(D / 64) tile rows, tiles = T (T + 1) / 2 (64 x 64 tiles of the lower triangle, mirrored);
             scatter:  S = min(ceil(N / 256), max(1, 1024 / tiles)), rows_per = ceil(N / S), S = ceil(N / rows_per); 32 rows per LDS stage;
                       S = 1 writes straight into `scatter`, S > 1 into a workspace that a second launch adds up in split order
             mean:     S1 = min(ceil(N / 128), 2048), rows_per = ceil(N / S1), S1 = ceil(N / rows_per)
             m4:       S3 = min(ceil(N / 64), 2048), rows_per = ceil(N / S3), S3 = ceil(N / rows_per); four waves deal a block's rows
  The D = 1088, N = 3 row has 17 full tile rows (153 tiles against 136 at D = 1024: 1088 = 17 x 64), one more than the scorer's limit
  allows; D = 1120 beside it has 18, the last a partial 64-column tile.  Their S is 1 because N <= 256 (max(1, 1024 / 153) = 6 would
  allow six splits): S = 1 is what every row of at most 256 rows takes.  The cap 1024 / tiles binds at the N = 262 400 row (1025 -> 1024 splits,
  then 1022 of 257 rows, the last of 3), where S1 and S3 are cut to 2048 and become 2035 blocks of 129 rows, the last of 14.

Score bar.  u = 2^-24, first order in u, times SLACK = 1 + 2^-10 for the products of roundings; from the float64 reference alone, no
measured constant.  The reference contracts the kernel's fp32 inputs in float64; for normalize = 1 they are the rows v of
ssad_l2_normalize_rows (the selector rows show, bit for bit, that those are the rows the kernel contracts).
  c_k = fl(fl(v_k - hi_k) - lo_k)      e_c = u |v - hi| + u |c|
  y_j = sum_k W_jk c_k                 e_y = sum_k |W_jk| e_c,k + (2 K_j + 8) u sum_k |W_jk c_k|: a rounded product and a rounded
                                       accumulation per term over the K_j columns the tile contracts (so it holds whether or not the MFMA
                                       fuses; the zeros above the diagonal add nothing)
  ss = sum_j y_j^2 (fmaf)              e_ss = sum_j 2 |y_j| e_y,j + (D + 4) u sum_j y_j^2: at most D / 2 fused steps per lane half (128
                                       register steps per tile), the half merge, the wave merge
  out = sqrtf(ss)                      e_ss / (2 s) + u s, valid where e_ss < ss: asserted per row in tests/test_gde_table.py; the
                                       generators leave no row near it (e_ss <= 2^-9 ss is asserted too: the second order of the square
                                       root, e_ss / (4 ss) of the bar, is then below half of SLACK - 1)
Exact rows, zero tolerance: integer rows (every product and partial sum an integer below 2^24, so exact in fp32 in any order; expected:
float64 sqrt of the integer, rounded once), selector rows (W = e_j e_k^T, mu = 0: out = sqrtf(fl(v_k^2)) = |v_k| -- sqrt(fl(x^2)) = |x|
holds in binary round-to-nearest away from underflow; |v_k| >= 2^-60 or v_k = 0 is asserted), row independence.

Fit bars.  ud = 2^-53; the reference is numpy longdouble (eps <= 2^-63 asserted in tests/test_gde_table.py: its own error is below 2^-10
of every bar) over the fp32 rows the kernels see (ssad_l2_normalize_rows' for normalize = 1).
  mean      (rows_per + S1 + 2) ud sum_i |x_id| / N: a sequential sum per split, the splits in order, one division
  scatter   the centred values carry the mean's error: e_mean,a sum_i |c_ib| + e_mean,b sum_i |c_ia|, plus
            (rows_per + S + 2) ud sum_i |c_ia c_ib|: two centring roundings, a fused step per row, the splits in order
  m4        r_i = sum_d c_id^2:  e_r,i = 2 sum_d |c_id| e_mean,d + (D / 64 + 8) ud r_i  (two centring roundings, D / 64 fused steps per
            lane, six butterfly additions);  m4 = sum_i r_i^2:  sum_i 2 r_i e_r,i + (rows_per + S3 + 2) ud m4
A single row (N = 1) is its own mean: scatter and m4 are exactly 0 and so are their bars.
scatter == scatter^T, both calls of `twice`, and (normalize = 1) ops.gaussian_fit_stats against the entry point: bit for bit.

No comparison skips or masks an element.

Measured on the MI355X on 2026-10-20 (worst error / bar per entry kind over all rows: MEASURED below; for the record, never asserted).
No kind comes near 1: the bars are worst-case sums of K_j (or rows_per) roundings that in fact largely cancel.  The score stays at 0.018
(0.006 on the near-degenerate rows, where the exact first difference leaves e_c almost unused), the mean at 0.001, m4 at 0.034; the
scatter reaches 0.217 at D = 1088, N = 3 (the largest of 1.2 million elements of three addends each, under a bar of (3 + 1 + 2) ud; the
other rows stay below 0.09).  Every integer, selector and independence row was bit-exact, and every scorer and integer row gave the same bits over a
NaN and over a zero upper triangle.
"""
import collections

import numpy as np
import torch

from bn_table import Arena, within as _within, twice, print_worst as _print_worst, _lib, _p, _bits, _seed, U, cdiv

SLACK = 1.0 + 2.0 ** -10
UD = 2.0 ** -53
NAN = float("nan")
BB, BK = 128, 32                                     # the scorer's W tile rows and K step
SCORER_MAX_D, FIT_MAX_D = 1024, 4096
SC_T, SC_K = 64, 32                                  # the scatter tile and its LDS stage
MAX_HOST_BYTES = 40 << 20

# worst error / bar per entry kind, MI355X (from `pytest -s -m gpu tests/test_hip_gde_paths.py`; never asserted)
MEASURED = {"score": 0.018, "score_degenerate": 0.006, "fit_mean": 0.001, "fit_scatter": 0.217, "fit_m4": 0.034}
MEASURED_ON = "2026-10-20"

WORST = {}


def within(rid, kind, got, want, bar):
    _within(rid, kind, got, torch.as_tensor(np.asarray(want, dtype=np.float64)), torch.as_tensor(np.asarray(bar, dtype=np.float64)), worst_of=WORST)


def print_worst():
    _print_worst(WORST)


def _gen(rid):
    return torch.Generator().manual_seed(_seed(rid))


def rows_like_test_hip_gde(n, d, g, spread=1.0):
    """tests/test_hip_gde.py's construction: a base vector plus correlated Gaussian rows."""
    base = torch.randn(d, generator=g) * 2.0
    a = torch.randn(d, d, generator=g) / d ** 0.5
    return (base + spread * (torch.randn(n, d, generator=g) @ a)).float()


def host_normalized(x):
    """x / ||x|| in float64, rounded to fp32: what the tests without a GPU take in place of ssad_l2_normalize_rows' rows (within a few
    ulps of them; only bars and coverage are computed from these, never a comparison with a kernel)."""
    x64 = x.double()
    n = x64.norm(dim=1, keepdim=True)
    return (x64 / torch.where(n == 0, torch.ones_like(n), n)).float()


def device_normalized(x, dev):
    hip, lib, st = _lib()
    xd = x.to(dev).contiguous()
    out = torch.empty_like(xd)
    hip.check(lib.ssad_l2_normalize_rows(_p(xd), _p(out), x.shape[0], x.shape[1], st))
    torch.cuda.synchronize()
    return out.cpu()


class Case:
    pass


# =====================================================================================================================================
# the scorer
# =====================================================================================================================================
ScoreRow = collections.namedtuple("ScoreRow", "id d n normalize kind")        # kind: gen | degenerate
SCORE_D = (32, 96, 128, 160, 256, 1024)
SCORE_N_FULL = (1, 127, 128, 129, 300)


def _score_rows():
    rows = []
    for d in SCORE_D:
        for n in (SCORE_N_FULL if d in (32, 160) else (129,)):
            for nz in (0, 1):
                rows.append(ScoreRow(f"score_{d}x{n}_norm{nz}", d, n, nz, "gen"))
    for nz in (0, 1):
        rows.append(ScoreRow(f"score_degenerate_160x129_norm{nz}", 160, 129, nz, "degenerate"))
    return rows


SCORE = _score_rows()


def w_tiles(d):
    return cdiv(d, BB)


def k_cols(d):
    """K_j for j = 0 .. D - 1: the columns row j's tile contracts."""
    j = np.arange(d)
    return np.minimum(d, BB * ((j + 1 + BB - 1) // BB))


SCORE_CASES = {
    "D less than one W tile": lambda r: r.d < BB and r.d > 32,
    "D = 32: one K step": lambda r: r.d == BK,
    "D exactly one W tile": lambda r: r.d == BB,
    "one W tile plus 32 rows": lambda r: r.d == BB + 32 and w_tiles(r.d) == 2,
    "D exactly two W tiles": lambda r: r.d == 2 * BB,
    "the limit, eight W tiles": lambda r: r.d == SCORER_MAX_D and w_tiles(r.d) == 8,
    "a row whose tile contracts fewer columns than D": lambda r: int(k_cols(r.d).min()) < r.d,
    "one query": lambda r: r.n == 1,
    "one query short of a workgroup": lambda r: r.n == 127,
    "exactly one workgroup": lambda r: r.n == 128,
    "a second workgroup with one query": lambda r: r.n == 129,
    "three workgroups, the last ragged": lambda r: r.n == 300,
    "every N at a short last tile": lambda r: r.d == 160 and r.n in SCORE_N_FULL,
    "raw rows": lambda r: r.normalize == 0,
    "normalised rows": lambda r: r.normalize == 1,
    "near-degenerate rows (the lo half of the mean)": lambda r: r.kind == "degenerate",
}

_FITS = {}


def _factor(rows64):
    """density.ledoit_wolf_factor of float64 rows, on the host."""
    from self_supervised.density import ledoit_wolf_factor
    mean = rows64.mean(0)
    c = rows64 - mean
    r = np.sum(c * c, axis=1)
    mu_hi, mu_lo, w, _ = ledoit_wolf_factor(mean, c.T @ c, float(np.sum(r * r)), rows64.shape[0])
    assert not np.triu(w, 1).any() and not np.signbit(np.triu(w, 1)).any()         # exact +0 above the diagonal
    return torch.from_numpy(mu_hi), torch.from_numpy(mu_lo), torch.from_numpy(w)


def poisoned(w):
    """W with NaN in its strict upper triangle."""
    p = w.clone()
    p[torch.triu(torch.ones_like(w, dtype=torch.bool), 1)] = NAN
    return p


def score_fit(d, normalize, kind="gen"):
    """(mu_hi, mu_lo, W) fp32 from 2 D seeded rows, fitted in float64 on the host (cached per D, normalize, kind)."""
    key = (d, normalize, kind)
    if key not in _FITS:
        g = _gen(f"gde_fit_{kind}_{d}")
        if kind == "degenerate":
            base = torch.randn(d, generator=g)
            fit = (base + 1e-4 * base.norm() / d ** 0.5 * torch.randn(2 * d, d, generator=g)).float()
        else:
            fit = rows_like_test_hip_gde(2 * d, d, g)
        rows = host_normalized(fit) if normalize else fit
        _FITS[key] = _factor(rows.double().numpy())
    return _FITS[key]


def score_case(row):
    c = Case()
    c.row = row
    c.mu_hi, c.mu_lo, c.w = score_fit(row.d, row.normalize, row.kind)
    g = _gen(row.id)
    if row.kind == "degenerate":
        gb = _gen(f"gde_fit_degenerate_{row.d}")
        base = torch.randn(row.d, generator=gb)                                    # the fit's base vector
        c.x = (base + 1e-4 * base.norm() / row.d ** 0.5 * 1.3 * torch.randn(row.n, row.d, generator=g)).float()
    else:
        c.x = rows_like_test_hip_gde(row.n, row.d, g, spread=1.5)
    return c


def score_ref(v, mu_hi, mu_lo, w):
    """v [N][D]: the fp32 rows the kernel contracts.  -> (want [N], bar [N], ss [N], e_ss [N]) in float64 (numpy)."""
    v, hi, lo = v.double().numpy(), mu_hi.double().numpy(), mu_lo.double().numpy()
    wl = np.tril(w.double().numpy())
    d = wl.shape[0]
    d1 = v - hi
    c = d1 - lo
    e_c = U * np.abs(d1) + U * np.abs(c)
    aw = np.abs(wl)
    y = c @ wl.T
    e_y = e_c @ aw.T + (2 * k_cols(d) + 8) * U * (np.abs(c) @ aw.T)
    ss = np.sum(y * y, axis=1)
    e_ss = np.sum(2 * np.abs(y) * e_y, axis=1) + (d + 4) * U * ss
    s = np.sqrt(ss)
    bar = (e_ss / (2 * np.where(s > 0, s, 1.0)) + U * s) * SLACK
    return s, bar, ss, e_ss


def _score_launch(dev, eid, xd, hid, lod, wd, n, d, normalize):
    hip, lib, st = _lib()

    def launch():
        ar = Arena(dev)
        o = {"out": ar.out("out", (n,), torch.float32)}
        hip.check(lib.ssad_mahalanobis_fused(_p(xd), _p(hid), _p(lod), _p(wd), _p(o["out"]), n, d, normalize, st))
        ar.check_outputs(eid)
        return o
    return twice(eid, launch)["out"].cpu()


def run_score_row(row, dev):
    c = score_case(row)
    ia = Arena(dev)
    xd, hid, lod = ia.inp("x", c.x), ia.inp("mu_hi", c.mu_hi), ia.inp("mu_lo", c.mu_lo)
    wp, wz = ia.inp("w, NaN above the diagonal", poisoned(c.w)), ia.inp("w, +0 above the diagonal", c.w)
    assert all(t.data_ptr() % 16 == 0 for t in (xd, hid, lod, wp, wz))
    got = _score_launch(dev, row.id, xd, hid, lod, wp, row.n, row.d, row.normalize)
    v = device_normalized(c.x, dev) if row.normalize else c.x
    want, bar, ss, e_ss = score_ref(v, c.mu_hi, c.mu_lo, c.w)
    assert bool((e_ss < ss).all())
    within(row.id, "score_degenerate" if row.kind == "degenerate" else "score", got, want, bar)
    clean = _score_launch(dev, row.id + " zero upper triangle", xd, hid, lod, wz, row.n, row.d, row.normalize)
    assert torch.equal(_bits(got), _bits(clean)), f"{row.id}: scores over a NaN upper triangle differ from scores over a zero one"
    ia.check_inputs(row.id)


# ---- integer rows ----
IntRow = collections.namedtuple("IntRow", "id d n")
INTEGER = [IntRow(f"int_{d}x129", d, 129) for d in (96, 160, 1024)]
INT_LIMIT = 2 ** 24


def int_case(row):
    """x in -3 .. 3, mu_hi in -1 .. 1, mu_lo = 0, W = +-1 on all of its lower triangle (every element matters), NaN above."""
    g = _gen(row.id)
    c = Case()
    c.x = torch.randint(-3, 4, (row.n, row.d), generator=g).float()
    c.mu_hi = torch.randint(-1, 2, (row.d,), generator=g).float()
    c.mu_lo = torch.zeros(row.d)
    c.w = torch.tril(torch.randint(0, 2, (row.d, row.d), generator=g).float() * 2 - 1)
    return c


def int_ref(c):
    """-> (expected fp32 scores, the largest |partial sum| any order of additions can meet in y, the largest ss), integers in int64."""
    cc = (c.x - c.mu_hi).to(torch.int64)
    wl = c.w.to(torch.int64)
    y = cc @ wl.T
    reach = cc.abs() @ wl.abs().T                     # >= every partial sum of y_j in any order
    ss = (y * y).sum(1)
    want = torch.from_numpy(np.sqrt(ss.numpy().astype(np.float64)).astype(np.float32))
    return want, int(reach.max()), int(ss.max())


def run_int_row(row, dev):
    c = int_case(row)
    want, reach, ssmax = int_ref(c)
    assert reach < INT_LIMIT and ssmax < INT_LIMIT
    ia = Arena(dev)
    xd, hid, lod = ia.inp("x", c.x), ia.inp("mu_hi", c.mu_hi), ia.inp("mu_lo", c.mu_lo)
    wp, wz = ia.inp("w, NaN above the diagonal", poisoned(c.w)), ia.inp("w, +0 above the diagonal", c.w)
    got = _score_launch(dev, row.id, xd, hid, lod, wp, row.n, row.d, 0)
    bad = (_bits(got).view(-1, 4) != _bits(want).view(-1, 4)).any(1).nonzero().flatten()
    assert bad.numel() == 0, (f"{row.id}: {bad.numel()} of {row.n} scores are not sqrt of the exact integer, first at query {int(bad[0])}: got "
                              f"{float(got[bad[0]])!r}, want {float(want[bad[0]])!r}")
    clean = _score_launch(dev, row.id + " zero upper triangle", xd, hid, lod, wz, row.n, row.d, 0)
    assert torch.equal(_bits(got), _bits(clean))
    ia.check_inputs(row.id)


# ---- selector rows ----
SEL_D, SEL_N, SEL_ZERO_ROW = 160, 129, 77
SEL_PAIRS = [(SEL_D - 1, 0), (SEL_D - 1, 31), (SEL_D - 1, 32), (SEL_D - 1, 63), (SEL_D - 1, 64), (SEL_D - 1, SEL_D - 1), (0, 0), (127, 127),
             (128, 0), (128, 128)]
SEL_MIN = 2.0 ** -60


def sel_case():
    x = rows_like_test_hip_gde(SEL_N, SEL_D, _gen("gde_selector"), spread=1.5)
    x[SEL_ZERO_ROW] = 0.0
    return x


def sel_w(j, k):
    w = torch.zeros(SEL_D, SEL_D)
    w[j, k] = 1.0
    return poisoned(w)


def sel_values_ok(v):
    """sqrt(fl(x^2)) = |x| needs x^2 far from underflow: every value 0 or at least 2^-60 in magnitude."""
    a = v.abs()
    return bool(((a == 0) | (a >= SEL_MIN)).all())


def run_selector_rows(dev):
    x = sel_case()
    ia = Arena(dev)
    xd, zd = ia.inp("x", x), ia.inp("zero mean", torch.zeros(SEL_D))
    rows = {0: x, 1: device_normalized(x, dev)}
    assert bool((rows[1][SEL_ZERO_ROW] == 0).all()) and sel_values_ok(rows[0]) and sel_values_ok(rows[1])
    for j, k in SEL_PAIRS:
        wd = ia.inp(f"w = e_{j} e_{k}^T", sel_w(j, k))
        for nz in (0, 1):
            eid = f"selector_{j}_{k}_norm{nz}"
            got = _score_launch(dev, eid, xd, zd, zd, wd, SEL_N, SEL_D, nz)
            want = rows[nz][:, k].abs()
            assert torch.equal(_bits(got), _bits(want)), (f"{eid}: {int((got != want).sum())} of {SEL_N} scores differ from |v_k| of "
                                                          f"{'ssad_l2_normalize_rows' if nz else 'the raw rows'}")
            assert _bits(got[SEL_ZERO_ROW:SEL_ZERO_ROW + 1]).tolist() == [0, 0, 0, 0]                     # +0.0
    ia.check_inputs("selector rows")


# ---- row independence ----
INDEP_D, INDEP_N = 160, 300
INDEP_POSITIONS = (0, 63, 127, 128, INDEP_N - 1)


def run_independence(dev):
    for nz in (0, 1):
        row = ScoreRow(f"score_{INDEP_D}x{INDEP_N}_norm{nz}", INDEP_D, INDEP_N, nz, "gen")
        assert row in SCORE
        c = score_case(row)
        ia = Arena(dev)
        hid, lod, wd = ia.inp("mu_hi", c.mu_hi), ia.inp("mu_lo", c.mu_lo), ia.inp("w", poisoned(c.w))
        full = _score_launch(dev, row.id, ia.inp("x", c.x), hid, lod, wd, row.n, row.d, nz)
        for i in INDEP_POSITIONS:
            one = _score_launch(dev, f"{row.id} row {i} alone", ia.inp("x1", c.x[i:i + 1]), hid, lod, wd, 1, row.d, nz)
            trio = _score_launch(dev, f"{row.id} row {i} first of three", ia.inp("x3", c.x[[i, 5, 77]]), hid, lod, wd, 3, row.d, nz)
            assert torch.equal(_bits(one[0:1]), _bits(full[i:i + 1])) and torch.equal(_bits(trio[0:1]), _bits(full[i:i + 1])), (row.id, i)
        ia.check_inputs(row.id)


# =====================================================================================================================================
# the fit statistics
# =====================================================================================================================================
FitRow = collections.namedtuple("FitRow", "id d n normalize")
FIT_D, FIT_N = (32, 96, 160, 512), (1, 2, 33, 257, 588)
FIT_WIDE, FIT_WIDE_PARTIAL, FIT_LONG = (1088, 3), (1120, 3), (32, 262400)
FIT = ([FitRow(f"fit_{d}x{n}_norm{nz}", d, n, nz) for d in FIT_D for n in FIT_N for nz in (0, 1)]
       + [FitRow(f"fit_{d}x{n}_norm{nz}", d, n, nz) for d, n in (FIT_WIDE, FIT_WIDE_PARTIAL, FIT_LONG) for nz in (0, 1)])

Geometry = collections.namedtuple("Geometry", "tile_rows tiles s sc_rows s1 cs_rows s3 m4_rows")


def fit_geometry(n, d):
    t = cdiv(d, SC_T)
    tiles = t * (t + 1) // 2
    s = min(cdiv(n, 256), max(1, 1024 // tiles))
    sc_rows = cdiv(n, s)
    s = cdiv(n, sc_rows)
    s1 = min(cdiv(n, 128), 2048)
    cs_rows = cdiv(n, s1)
    s1 = cdiv(n, cs_rows)
    s3 = min(cdiv(n, 64), 2048)
    m4_rows = cdiv(n, s3)
    s3 = cdiv(n, m4_rows)
    return Geometry(t, tiles, s, sc_rows, s1, cs_rows, s3, m4_rows)


def _g(r):
    return fit_geometry(r.n, r.d)


FIT_CASES = {
    "one scatter tile": lambda r: _g(r).tiles == 1,
    "a partial 64-column tile beside a full one": lambda r: r.d % SC_T == 32 and _g(r).tile_rows in (2, 3),
    "full tiles only, several": lambda r: r.d % SC_T == 0 and _g(r).tile_rows == 8,
    "more tile rows than the scorer allows": lambda r: r.d > SCORER_MAX_D and _g(r).tiles == 153,
    "more tile rows than the scorer allows, the last partial": lambda r: r.d > SCORER_MAX_D and r.d % SC_T == 32 and _g(r).tile_rows == 18,
    "one row": lambda r: r.n == 1,
    "two rows": lambda r: r.n == 2,
    "one LDS stage and a row": lambda r: r.n == SC_K + 1,
    "single split: straight into scatter": lambda r: _g(r).s == 1,
    "two scatter splits of 129 and 128 rows": lambda r: (_g(r).s, _g(r).sc_rows, r.n - _g(r).sc_rows) == (2, 129, 128),
    "three splits of 196 rows, no multiple of the stage": lambda r: (_g(r).s, _g(r).sc_rows) == (3, 196) and 196 % SC_K != 0 and r.n == 3 * 196,
    "several column-sum and m4 blocks, the last ragged": lambda r: _g(r).s1 > 1 and r.n % _g(r).cs_rows != 0 and _g(r).s3 > 1 and r.n % _g(r).m4_rows != 0,
    "a m4 block with fewer rows than waves": lambda r: r.n < 4,
    "past the column-sum cap: rows_per from the cap": lambda r: cdiv(r.n, 128) > 2048 and _g(r).cs_rows > 128,
    "past the m4 cap: rows_per from the cap": lambda r: cdiv(r.n, 64) > 2048 and _g(r).m4_rows > 64,
    "the scatter split cap binds": lambda r: cdiv(r.n, 256) > max(1, 1024 // _g(r).tiles),
    "raw rows": lambda r: r.normalize == 0,
    "normalised rows": lambda r: r.normalize == 1,
}


def fit_case(row):
    return rows_like_test_hip_gde(row.n, row.d, _gen(f"fit_{row.d}x{row.n}"))


def fit_ref(row, v):
    """v [N][D]: the fp32 rows the statistics are of.  -> {name: (want as float64, bar)}; the values in longdouble, the magnitudes the
    bars are made of in float64."""
    geo = fit_geometry(row.n, row.d)
    n, d = row.n, row.d
    x64 = v.double().numpy()
    xl = x64.astype(np.longdouble)
    mean = xl.sum(0) / np.longdouble(n)
    cl = xl - mean
    scatter = np.einsum("ia,ib->ab", cl, cl) if n > 4 * d else cl.T @ cl        # the same sums; einsum is the faster walk over long x
    rl = (cl * cl).sum(1)
    m4 = (rl * rl).sum()
    c = cl.astype(np.float64)
    ac = np.abs(c)
    e_mean = (geo.cs_rows + geo.s1 + 2) * UD * np.abs(x64).sum(0) / n
    s_abs = ac.sum(0)
    e_sc = np.outer(e_mean, s_abs) + np.outer(s_abs, e_mean) + (geo.sc_rows + geo.s + 2) * UD * (ac.T @ ac)
    r = rl.astype(np.float64)
    e_r = 2 * (ac @ e_mean) + (d // 64 + 8) * UD * r
    e_m4 = np.sum(2 * r * e_r) + (geo.m4_rows + geo.s3 + 2) * UD * float(m4)
    ref = {"mean": (mean.astype(np.float64), e_mean * SLACK), "scatter": (scatter.astype(np.float64), e_sc * SLACK),
           "m4": (np.array([float(m4)]), np.array([e_m4 * SLACK]))}
    ref["_long"] = (xl, mean, scatter, m4)
    return ref


def fit_host_bytes(row):
    return 4 * row.n * row.d + 8 * (row.d * row.d + row.d + 1)


def run_fit_row(row, dev):
    hip, lib, st = _lib()
    from self_supervised import ops
    x = fit_case(row)
    n, d = row.n, row.d
    ia = Arena(dev)
    xd = ia.inp("x", x)
    assert xd.data_ptr() % 16 == 0

    def launch():
        ar = Arena(dev)
        o = {"mean": ar.out("mean", (d,), torch.float64), "scatter": ar.out("scatter", (d, d), torch.float64),
             "m4": ar.out("m4", (1,), torch.float64)}
        hip.check(lib.ssad_gaussian_fit_stats(_p(xd), n, d, row.normalize, _p(o["mean"]), _p(o["scatter"]), _p(o["m4"]), st))
        ar.check_outputs(row.id)
        return o
    o = {k: t.cpu() for k, t in twice(row.id, launch).items()}
    assert torch.equal(_bits(o["scatter"]), _bits(o["scatter"].T.contiguous())), f"{row.id}: scatter differs from its transpose"
    if row.normalize:
        w = ops.gaussian_fit_stats(xd, True)
        for nm, t in zip(("mean", "scatter", "m4"), w):
            assert torch.equal(_bits(t.cpu()), _bits(o[nm])), f"{row.id}: ops.gaussian_fit_stats differs from the entry point in `{nm}`"
    v = device_normalized(x, dev) if row.normalize else x
    ref = fit_ref(row, v)
    for nm in ("mean", "scatter", "m4"):
        within(f"{row.id} {nm}", f"fit_{nm}", o[nm], *ref[nm])
    ia.check_inputs(row.id)


# =====================================================================================================================================
# argument errors
# =====================================================================================================================================
BAD_D_FIT, BAD_D_SCORE = (0, 48, 4128), (0, 48, 1056)


def run_argument_errors(dev):
    """Every refusal returns 2, names its entry point in ssad_last_error() and leaves the poisoned outputs untouched."""
    hip, lib, st = _lib()
    n, d = 5, 32
    ia, ar = Arena(dev), Arena(dev)
    x, mu, w = ia.inp("x", torch.randn(n, d)), ia.inp("mu", torch.zeros(d)), ia.inp("w", torch.eye(d))
    mean, sc, m4 = ar.out("mean", (d,), torch.float64), ar.out("scatter", (d, d), torch.float64), ar.out("m4", (1,), torch.float64)
    out = ar.out("out", (n,), torch.float32)
    fit_ok = dict(x=_p(x), N=n, D=d, normalize=1, mean=_p(mean), scatter=_p(sc), m4=_p(m4))
    fit_bad = {f"null {k}": {k: None} for k in ("x", "mean", "scatter", "m4")}
    fit_bad.update({"N = 0": {"N": 0}, **{f"D = {v}": {"D": v} for v in BAD_D_FIT}})
    for what, change in fit_bad.items():
        assert lib.ssad_gaussian_fit_stats(*{**fit_ok, **change}.values(), st) == 2, what
        assert b"ssad_gaussian_fit_stats" in lib.ssad_last_error(), what
    score_ok = dict(x=_p(x), mu_hi=_p(mu), mu_lo=_p(mu), w=_p(w), out=_p(out), N=n, D=d, normalize=1)
    score_bad = {f"null {k}": {k: None} for k in ("x", "mu_hi", "mu_lo", "w", "out")}
    score_bad.update({"N = 0": {"N": 0}, **{f"D = {v}": {"D": v} for v in BAD_D_SCORE}})
    for what, change in score_bad.items():
        assert lib.ssad_mahalanobis_fused(*{**score_ok, **change}.values(), st) == 2, what
        assert b"ssad_mahalanobis_fused" in lib.ssad_last_error(), what
    torch.cuda.synchronize()
    for name, big, *_ in ar.outs:
        assert bool((big == 255).all()), f"a refused call wrote `{name}` or its guards"
    ia.check_inputs("argument errors")
    assert FIT_MAX_D + 32 in BAD_D_FIT and SCORER_MAX_D + 32 in BAD_D_SCORE
