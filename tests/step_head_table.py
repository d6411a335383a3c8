"""The step-head table: what a training step runs after the trunk and around it -- the small-batch linear kernels (csrc/linear_small.hip, all
three operand roundings), global average pooling (csrc/misc.hip, csrc/train.hip), the plain 3 x 3 / stride 2 max-pool (csrc/stem.hip,
csrc/train.hip), softmax cross-entropy, SGD and the loss scaler (csrc/train.hip) -- at the smallest shapes that reach each branch, compared
per element against float64 on the CPU, over buffers between poisoned guards (Arena, within, twice of tests/bn_table.py).

Shared by tests/test_step_head_table.py (rows, coverage, the references themselves, finite bars: no GPU) and
tests/test_hip_step_head_paths.py (the kernels).

Dispatch, restated from the documented rules (NOT read back from the library):
  linear_small      a 1 x 1 layer over a 1 x 1 map with 0 < M <= 512 rows, contraction % 4 == 0, operands 16-byte aligned; 32 x 32 output
                    tiles; forward / input gradient: 8-float chunks of K dealt over 8 waves, 8 chunks in flight per wave (a trip of the loop
                    is 64 chunks), lane half h supplies k = 8 c + 4 h ..; weight gradient: row pairs (2 q + h) dealt over 4 waves
  gap_fwd           gap_wide_kernel when !hwnc && C % 64 == 0 && HW >= 64 && N C < 256 * 1024, else gap_kernel (eight-wide unrolled loop
                    over HW and a tail); the _h entry: always the wide kernel
  gap_bwd           gap_bwd4_kernel when C % 4 == 0 and dy is 16-byte aligned, else the scalar gap_bwd_kernel; the _h entry: four-wide
  element-wise      min(8192, ceil(n / 256)) workgroups of 256 lanes, grid-stride
  check_finite      n4 = n / 4 float4 pieces when g is 16-byte aligned, else 0; lane i tests pieces i and i + step (step = grid x 256; the
                    second clamped to i when i + step >= n4), strides by 2 step; elements 4 n4 .. n one by one
  softmax_ce        one workgroup of 256 lanes, lane t takes rows t, t + 256, ..

Bars.  u = 2^-24 (one fp32 rounding, relative), uh = 2^-11 (a value stored as a half).  All from the float64 reference, none from a
measurement.  Every bar below is first order in u and is multiplied by 1 + 2^-10 for the products of roundings (SLACK).
  linear z          (2 K + 8) u sum_k |a_k b_k|: a rounded product and a rounded accumulation per term (so it holds whether or not the
                    MFMA fuses), eight partial tiles added.  round 1 / 2: the reference contracts the operands as torch rounds them on the
                    CPU (nearest even); their products are exact in fp32: (K + 8) u sum |a_k b_k|
  epilogue          |scale| bar_z + 3 u (|z scale| + |shift| + |residual|): product, add, add; the ReLU is 1-Lipschitz: same bar
  input gradient    the same with scale 1, no shift
  weight gradient   (2 M + 4) u sum_m |dz_m x_m| ((M + 4) u for round 1 / 2): four partial tiles; accumulate: + u (|old| + |v|)
  statistics        v = the kernel's fp32 z, within bar_z of z.  A row tile leaves fp32 sums of its nt = min(32, M) values of v and of
                    v^2; everything after that is double and rounded once.
                      e_m    = mean bar_z + (nt - 1) u mean (|z| + bar_z)                           mean:   e_m + u (|mean| + e_m)
                      e_var  = 2 std_z rms(bar_z) + mean bar_z^2          (variance of v against variance of z: Cauchy-Schwarz on the
                                                                            centred values, so no |mean| in it)
                             + (nt + 1) u mean (|z| + bar_z)^2            (the single-pass fp32 sum of v^2: the term ~ u E[z^2], all of the
                                                                            bar when |mean| >> std -- the |mean| / std = 30 row)
                             + 2 |mean| e_s + e_s^2,  e_s = (nt - 1) u mean (|z| + bar_z)           (mean^2 from the fp32 sum of v)
                      invstd = (var + eps)^-1/2:   e_var / 2 (var + eps - e_var)^-3/2 + u invstd    (var + eps > e_var asserted per row)
                      running statistics:  momentum x (e_m | e_var R / (R - 1)) + u |ref|
  gap_fwd           (HW + 1) u sum |x| / HW: HW - 1 additions in any order, one division
  gap_bwd           2 u |g / HW| (a division within one ulp), + u |old + g / HW| when accumulating; a stored half: bn_table.half_stored
  softmax_ce        expf within E = 2 ulp, logf within L = 1 ulp (the HIP math API document is not part of this ROCm installation: the
                    issue's fall-back figures); an ulp is at most 2 u relative.  Per row, d_c = fl(p_c - mx) (u |d_c|, so u |d_c| relative
                    in exp), se = sum_c expf(d_c) left to right:
                      eta   = (C - 1 + 2 E) u + u sum_c e^{d_c} |d_c| / se                         relative error of se
                      e_lse = eta + 2 L u |log se| + u |lse|                                       logf, then + mx
                      row   = e_lse + u |lse - p_y|                                                the subtraction; the sum is double
                    loss: mean_b row + u |loss| (absolute).  accuracy: the fp32 quotient count / B, exact (first maximum on ties).
                      dlogits_c: s_c = e^{p_c - lse}; the argument is off by A = e_lse + u |p_c - lse|, expf adds 2 E u:
                      |gscale| (s_c (A + 2 E u) + 2 u |s_c - [c = y]| + 2^-126)                     (- 1, x gscale; 2^-126: a flushed denormal)
                    padding columns C .. ldd: +0.0 bit for bit
  sgd               bar_m = 3 u (|mu m| + |g gs| + |wd p|), + u |g gs| when gs is the fp32 quotient hyper[3] / scaler[0];
                    bar_p = 2 u (|p| + |lr m'|) + |lr| bar_m.  Every step restarts from the fp32 state the kernel left: no compounding
  exact             pooled values, winner slots, routed gradients (the gather adds <= 4 pooled gradients in fp32 in the order oy, ox: the
                    reference does the same), _bwd == _bwd_idx, found_inf, x * loss_scale (one fp32 product), the loss-scaler transitions

Nothing is undecidable: every decision these kernels take (argmax, window winner, finite or not) is taken on the exact fp32 inputs, and
the reference takes it on the same values.  No comparison skips or masks an element; tests/test_step_head_table.py asserts every bar
finite.

Measured on the MI355X on 2026-10-19 (worst error / bar per entry kind over all rows: MEASURED below; for the record, never asserted).
Where one rounding is most of a bar the ratio comes close to 1: gap_bwd into a stored half (0.998: the rounding of the half alone can
use all of its term), the accumulating weight gradient of one or two rows (0.96: u |old + v| against u (|old| + |v|)).  The contraction
bars stay at 0.2 - 0.24, the statistics at 0.74 (running variance of M = 2 rows); the |mean| / std = 30 row measures 0.012 of a bar whose
largest term is the cancellation term.  ssad_sgd_step_dev without a scaler equalled ssad_sgd_step bit for bit in every step of every row.
"""
import collections
import itertools

import torch
import torch.nn.functional as F

from bn_table import Arena, within as _within, twice, print_worst as _print_worst, GUARD_BYTES, half_stored, U, UH, cdiv, _seed, _lib, _p, _bits

SLACK = 1.0 + 2.0 ** -10
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
MOMENTA = (0.1, 0.3)
E_ULP, L_ULP = 2.0, 1.0                     # expf / logf (see the docstring)
EW_MAX_BLOCKS, EW_MAX_LANES = 8192, 8192 * 256
LINEAR_MAX_ROWS = 512
FLT_MAX = 3.4028234663852886e38

# worst error / bar per entry kind, MI355X (from `pytest -s -m gpu tests/test_hip_step_head_paths.py`; never asserted)
MEASURED = {"linear_fwd": 0.236, "linear_dgrad": 0.200, "linear_wgrad": 0.959, "linear_stats": 0.743, "linear_stats_pos": 0.012,
            "gap_fwd": 0.302, "gap_bwd": 0.998, "softmax_loss": 0.239, "softmax_dlogits": 0.769, "sgd": 0.649}
MEASURED_ON = "2026-10-19"

WORST = {}


def within(rid, kind, got, want, bar):
    _within(rid, kind, got, want, bar, worst_of=WORST)


def print_worst():
    _print_worst(WORST)


def f32(x):
    """The float a C `float` argument receives, as a double."""
    return float(torch.tensor(x, dtype=torch.float32))


def _gen(rid):
    return torch.Generator().manual_seed(_seed(rid))


def _sign(n, g, share=0.5):
    return torch.where(torch.rand(n, generator=g) < share, -1.0, 1.0)


def ew_grid(n):
    return max(1, min(EW_MAX_BLOCKS, cdiv(n, 256)))


class Case:
    pass


# =====================================================================================================================================
# linear layers
# =====================================================================================================================================
LinRow = collections.namedtuple("LinRow", "id m k n kind")
_TRIPLES = [(1, 4, 1), (31, 12, 33), (33, 36, 70), (512, 896, 512), (33, 520, 4), (31, 896, 70), (512, 36, 1), (1, 520, 33),
            (512, 12, 4), (33, 4, 70), (1, 896, 4), (2, 36, 33)]
LINEAR = [LinRow(f"lin_{m}x{k}x{n}", m, k, n, "gen") for m, k, n in _TRIPLES]
LINEAR.append(LinRow("lin_pos_512x520x70", 512, 520, 70, "pos"))          # statistics only: per-channel |mean| / std = 30
ROUNDINGS = (0, 1, 2)
ROUND_NAME = {0: "f32", 1: "bf16", 2: "f16"}
POS_RATIO = 30.0
FWD_FORMS = (("full", True, True, True, True), ("scale", True, False, False, False), ("shift", False, True, False, False),
             ("residual", False, False, True, False), ("relu", False, False, False, True))


def linear_small_takes(m, k):
    return 0 < m <= LINEAR_MAX_ROWS and k % 4 == 0


def lin_chunks(k):
    return cdiv(k, 8)


LINEAR_CASES = {
    "one chunk, its h = 1 half outside K": lambda r: r.k == 4,
    "K % 8 == 4 past the first chunk": lambda r: r.k % 8 == 4 and r.k > 8,
    "second trip of the 64-chunk loop with one live chunk": lambda r: lin_chunks(r.k) == 65,
    "the real layer": lambda r: (r.m, r.k, r.n) == (512, 896, 512),
    "the smallest layer": lambda r: (r.m, r.k, r.n) == (1, 4, 1),
    "one lane row": lambda r: r.m == 1,
    "ragged row tile": lambda r: r.m == 31,
    "second row tile": lambda r: r.m == 33,
    "the row limit": lambda r: r.m == LINEAR_MAX_ROWS and linear_small_takes(r.m, r.k) and not linear_small_takes(r.m + 1, r.k),
    "single column": lambda r: r.n == 1,
    "the classifier": lambda r: r.n == 4,
    "ragged column tiles": lambda r: r.n > 32 and r.n % 32 != 0,
    "ragged x ragged": lambda r: r.m % 32 != 0 and r.m > 1 and r.n % 32 != 0 and r.n > 1,
    "wgrad: one row pair": lambda r: r.m == 2,
    "wgrad: last row pair with only h = 0 live": lambda r: r.m % 2 == 1 and r.m > 1,
    "wgrad: a wave with several trips": lambda r: cdiv(r.m, 2) > 32,
    "statistics with |mean| / std = 30": lambda r: r.kind == "pos",
}


def rnd(t, mode):
    """Operands as the kernel's loader rounds them (torch on the CPU: round to nearest even)."""
    return t if mode == 0 else t.bfloat16().float() if mode == 1 else t.half().float()


def lin_case(row):
    g = _gen(row.id)
    m, k, n = row.m, row.k, row.n
    c = Case()
    c.row = row
    if row.kind == "pos":
        s = torch.randn(k, generator=g)
        s = s / s.norm()
        w = torch.randn(n, k, generator=g)
        w = w - (w @ s)[:, None] * s
        w = w / w.norm(dim=1, keepdim=True)
        t = torch.exp2(torch.rand(n, generator=g) * 2 - 1) * _sign(n, g)
        c.b = (t[:, None] * (0.6 * s + 0.8 * w)).float()                              # s . b_n = 0.6 t_n, |b_n| = |t_n|
        c.a = (torch.randn(m, k, generator=g) + (POS_RATIO / 0.6) * s).float()        # mean_n = 30 t_n, std_n = |t_n|
    else:
        c.a = torch.randn(m, k, generator=g)
        c.b = torch.randn(n, k, generator=g) / k ** 0.5
    c.scale = ((0.5 + torch.rand(n, generator=g)) * _sign(n, g, 0.25)).float()
    c.shift = torch.randn(n, generator=g)
    c.res = torch.randn(m, n, generator=g)
    c.dz = torch.randn(m, n, generator=g)
    c.old = torch.randn(n, k, generator=g)
    c.rm0, c.rv0 = torch.randn(n, generator=g) * 0.5, torch.rand(n, generator=g) + 0.5
    return c


class LinRef:
    """float64 contraction of the operands as rounded, and every bar of the linear entries."""

    def __init__(self, c, mode):
        self.c, self.mode = c, mode
        m, k, n = c.row.m, c.row.k, c.row.n
        ar, br = rnd(c.a, mode).double(), rnd(c.b, mode).double()
        self.z = ar @ br.T
        self.bar_z = ((2 * k + 8) if mode == 0 else (k + 8)) * U * (ar.abs() @ br.abs().T) * SLACK

    def fwd(self, scale, shift, res, relu):
        c = self.c
        sc = c.scale.double() if scale else torch.ones(c.row.n, dtype=torch.float64)
        sh = c.shift.double() if shift else torch.zeros(c.row.n, dtype=torch.float64)
        rs = c.res.double() if res else torch.zeros_like(self.z)
        want = self.z * sc + sh + rs
        bar = sc.abs() * self.bar_z + 3 * U * ((self.z * sc).abs() + sh.abs() + rs.abs()) * SLACK
        return (want.clamp(min=0) if relu else want), bar

    def wgrad(self, accumulate):
        c, mode, m = self.c, self.mode, self.c.row.m
        dzr, xr = rnd(c.dz, mode).double(), rnd(c.a, mode).double()
        v = dzr.T @ xr
        bar = ((2 * m + 4) if mode == 0 else (m + 4)) * U * (dzr.abs().T @ xr.abs()) * SLACK
        if accumulate:
            return c.old.double() + v, bar + U * (c.old.double().abs() + v.abs()) * SLACK
        return v, bar

    def stats(self, momentum):
        """-> {name: (want, bar)} for mean, invstd and (momentum not None) the running statistics; `lo` = var + eps - e_var."""
        z, bz, r = self.z, self.bar_z, self.c.row.m
        nt = min(32, r)
        mag = z.abs() + bz
        mean = z.mean(0)
        var = ((z - mean) ** 2).mean(0)
        e_s = (nt - 1) * U * mag.mean(0)
        e_m = bz.mean(0) + e_s
        e_var = (2 * var.sqrt() * (bz ** 2).mean(0).sqrt() + (bz ** 2).mean(0) + (nt + 1) * U * (mag ** 2).mean(0)
                 + 2 * mean.abs() * e_s + e_s ** 2)
        self.lo = var + EPS - e_var * SLACK
        iv = (var + EPS).rsqrt()
        d_iv = 0.5 * e_var * self.lo.clamp(min=1e-300) ** -1.5
        d_iv = torch.where(self.lo > 0, d_iv, torch.full_like(d_iv, float("inf")))
        out = {"mean": (mean, (e_m + U * (mean.abs() + e_m)) * SLACK), "invstd": (iv, (d_iv + U * (iv + d_iv)) * SLACK)}
        self.e_var, self.var = e_var, var
        if momentum is not None:
            mom = f32(momentum)
            unb, k_unb = (var * r / (r - 1), r / (r - 1)) if r > 1 else (var, 1.0)
            rm = (1.0 - mom) * self.c.rm0.double() + mom * mean
            rv = (1.0 - mom) * self.c.rv0.double() + mom * unb
            out["rm"] = (rm, (mom * e_m + U * (rm.abs() + mom * e_m)) * SLACK)
            out["rv"] = (rv, (mom * e_var * k_unb + U * (rv.abs() + mom * e_var * k_unb)) * SLACK)
        return out


def _lin_fn(lib, base, mode):
    return getattr(lib, base + {0: "", 1: "_bf16", 2: "_f16"}[mode])


def run_linear_row(row, dev):
    hip, lib, st = _lib()
    from self_supervised import ops
    c = lin_case(row)
    m, k, n = row.m, row.k, row.n
    assert linear_small_takes(m, k)
    ia = Arena(dev)
    ad, bd, dzd = ia.inp("a", c.a), ia.inp("b", c.b), ia.inp("dz", c.dz)
    scd, shd, rsd = ia.inp("scale", c.scale), ia.inp("shift", c.shift), ia.inp("residual", c.res)
    for mode in ROUNDINGS:
        ref = LinRef(c, mode)
        rid = f"{row.id}[{ROUND_NAME[mode]}]"
        # --- forward + BatchNorm1d statistics ---
        assert ops.igemm_tile(m, 1, 1, k, n, 1, 1, 1, 0, ops.IGEMM_STATS)[0] == ops.LINEAR_SMALL
        for mom in (None,) + MOMENTA:
            eid = f"{rid} fwd_stats{'' if mom is None else f' momentum {mom}'}"

            def launch():
                ar = Arena(dev)
                o = {"z": ar.out("z", (m, n), torch.float32), "mean": ar.out("mean", (n,), torch.float32),
                     "invstd": ar.out("invstd", (n,), torch.float32),
                     "rm": None if mom is None else ar.inp("running_mean", c.rm0, mutable=True),
                     "rv": None if mom is None else ar.inp("running_var", c.rv0, mutable=True)}
                ws = ar.out("workspace", (lib.ssad_conv_stats_workspace(m, 1, 1, n),), torch.float64)
                hip.check(lib.ssad_conv_igemm_fwd_stats(_p(ad), _p(bd), _p(o["z"]), m, 1, 1, k, n, 1, 1, 1, 0, mode, EPS, mom or 0.0, _p(o["mean"]),
                                                        _p(o["invstd"]), _p(o["rm"]), _p(o["rv"]), _p(ws), st))
                ar.check_outputs(eid)
                return o
            o = twice(eid, launch)
            if row.kind != "pos" or mom is None:
                within(f"{eid} z", "linear_fwd", o["z"], ref.z, ref.bar_z)
            for nm, (want, bar) in ref.stats(mom).items():
                within(f"{eid} {nm}", "linear_stats_pos" if row.kind == "pos" else "linear_stats", o[nm], want, bar)
        if row.kind == "pos":
            continue
        # --- forward with the epilogue ---
        assert ops.igemm_tile(m, 1, 1, k, n, 1, 1, 1, 0, ops.IGEMM_FWD)[0] == ops.LINEAR_SMALL
        fwd = _lin_fn(lib, "ssad_conv_igemm_fwd", mode)
        for name, scale, shift, res, relu in FWD_FORMS:
            eid = f"{rid} fwd {name}"

            def launch():
                ar = Arena(dev)
                o = {"y": ar.out("y", (m, n), torch.float32)}
                hip.check(fwd(_p(ad), _p(bd), _p(o["y"]), _p(scd) if scale else None, _p(shd) if shift else None, _p(rsd) if res else None,
                              int(relu), m, 1, 1, k, n, 1, 1, 1, 0, st))
                ar.check_outputs(eid)
                return o
            o = twice(eid, launch)
            within(eid, "linear_fwd", o["y"], *ref.fwd(scale, shift, res, relu))
        # --- input gradient with residual: dx[M][N] = a[M][K] . b[N][K]^T + residual (forward Cout = K, Cin = N) ---
        assert ops.igemm_tile(m, 1, 1, n, k, 1, 1, 1, 0, ops.IGEMM_DGRAD)[0] == ops.LINEAR_SMALL
        dgrad = _lin_fn(lib, "ssad_conv_igemm_dgrad", mode)
        eid = f"{rid} dgrad +residual"

        def launch():
            ar = Arena(dev)
            o = {"dx": ar.out("dx", (m, n), torch.float32)}
            hip.check(dgrad(_p(ad), _p(bd), _p(o["dx"]), _p(rsd), m, 1, 1, k, 1, 1, n, 1, 1, 1, 0, st))
            ar.check_outputs(eid)
            return o
        o = twice(eid, launch)
        within(eid, "linear_dgrad", o["dx"], *ref.fwd(False, False, True, False))
        # --- weight gradient: dw[N][K] (+)= dz[M][N]^T a[M][K] ---
        assert ops.wgrad_path((m, 1, 1, n), (m, 1, 1, k), 1, 1, 1, 0, bf16=mode)[:2] == ("linear_small", ROUND_NAME[mode])
        for acc in (False, True):
            eid = f"{rid} wgrad{' accumulate' if acc else ''}"

            def launch():
                ar = Arena(dev)
                o = {"dw": ar.inp("dw", c.old, mutable=True) if acc else ar.out("dw", (n, k), torch.float32)}
                hip.check(lib.ssad_linear_wgrad_small_r(_p(dzd), _p(ad), _p(o["dw"]), m, k, n, int(acc), mode, st))
                ar.check_outputs(eid)
                return o
            o = twice(eid, launch)
            within(eid, "linear_wgrad", o["dw"], *ref.wgrad(acc))
    ia.check_inputs(row.id)


# =====================================================================================================================================
# global average pooling
# =====================================================================================================================================
GapF = collections.namedtuple("GapF", "id n hw c hwnc half stride offset kernel")
GAP_FWD = [
    GapF("gapf_2x63x64", 2, 63, 64, 0, False, 64, 0, "narrow"),
    GapF("gapf_2x64x64", 2, 64, 64, 0, False, 64, 0, "wide"),
    GapF("gapf_2x64x60", 2, 64, 60, 0, False, 60, 0, "narrow"),
    GapF("gapf_3x65x128", 3, 65, 128, 0, False, 128, 0, "wide"),
    GapF("gapf_4096x64x64", 4096, 64, 64, 0, False, 64, 0, "narrow"),          # N C = 262 144 exactly
    GapF("gapf_4095x64x64", 4095, 64, 64, 0, False, 64, 0, "wide"),            # N C = 262 080
    GapF("gapf_hwnc_2x64x64", 2, 64, 64, 1, False, 64, 0, "narrow"),
    GapF("gapf_hwnc_3x1x20", 3, 1, 20, 1, False, 20, 0, "narrow"),
    GapF("gapf_hwnc_3x7x20", 3, 7, 20, 1, False, 20, 0, "narrow"),
    GapF("gapf_hwnc_3x8x20", 3, 8, 20, 1, False, 20, 0, "narrow"),
    GapF("gapf_hwnc_70x9x20", 70, 9, 20, 1, False, 20, 0, "narrow"),           # 1400 lanes: six workgroups
    GapF("gapf_5x1x64", 5, 1, 64, 0, False, 64, 0, "narrow"),
    GapF("gapf_slice_wide", 3, 65, 128, 0, False, 140, 8, "wide"),
    GapF("gapf_slice_narrow", 3, 9, 20, 0, False, 37, 11, "narrow"),
    GapF("gapf_h_2x65x64", 2, 65, 64, 0, True, 64, 0, "wide"),
    GapF("gapf_h_3x7x128", 3, 7, 128, 0, True, 150, 12, "wide"),
]
GapB = collections.namedtuple("GapB", "id n hw c half stride offset lead kernel")
GAP_BWD = [
    GapB("gapb_3x7x8", 3, 7, 8, False, 8, 0, 0, "four"),
    GapB("gapb_3x7x6", 3, 7, 6, False, 6, 0, 0, "scalar"),
    GapB("gapb_3x7x8_lead4", 3, 7, 8, False, 8, 0, 4, "scalar"),
    GapB("gapb_5x49x64_slice", 5, 49, 64, False, 80, 12, 0, "four"),           # 15 workgroups
    GapB("gapb_9x33x6_slice", 9, 33, 6, False, 11, 3, 0, "scalar"),            # 7 workgroups
    GapB("gapb_h_3x5x64", 3, 5, 64, True, 64, 0, 0, "four"),
    GapB("gapb_h_5x49x128_slice", 5, 49, 128, True, 140, 8, 0, "four"),
]


def gap_fwd_kernel(r):
    if r.half:
        return "wide"
    return "wide" if (not r.hwnc and r.c % 64 == 0 and r.hw >= 64 and r.n * r.c < 256 * 1024) else "narrow"


def gap_bwd_kernel(r):
    if r.half:
        return "four"
    return "four" if (r.c % 4 == 0 and r.lead % 16 == 0) else "scalar"


GAP_CASES = {
    "fwd: HW = 63 narrow / HW = 64 wide at C = 64": lambda rows: {(r.hw, gap_fwd_kernel(r)) for r in rows if isinstance(r, GapF) and r.c == 64
                                                                   and r.n == 2 and not r.hwnc} >= {(63, "narrow"), (64, "wide")},
    "fwd: C = 60 narrow at HW = 64": lambda rows: any(isinstance(r, GapF) and r.c == 60 and r.hw == 64 and gap_fwd_kernel(r) == "narrow" for r in rows),
    "fwd: two channel slabs, ragged pixel lanes": lambda rows: any(isinstance(r, GapF) and r.c == 128 and r.hw == 65 and gap_fwd_kernel(r) == "wide" for r in rows),
    "fwd: N C = 262144 narrow / 262080 wide": lambda rows: {(r.n * r.c, gap_fwd_kernel(r)) for r in rows if isinstance(r, GapF) and r.hw == 64
                                                             and not r.hwnc} >= {(262144, "narrow"), (262080, "wide")},
    "fwd: hwnc keeps a wide shape narrow": lambda rows: any(isinstance(r, GapF) and r.hwnc and r.c % 64 == 0 and r.hw >= 64 for r in rows),
    "fwd: hwnc at HW 1, 7, 8, 9": lambda rows: {r.hw for r in rows if isinstance(r, GapF) and r.hwnc} >= {1, 7, 8, 9},
    "fwd: HW = 1": lambda rows: any(isinstance(r, GapF) and r.hw == 1 and not r.hwnc for r in rows),
    "fwd: a slice of a wider output row, both kernels": lambda rows: {gap_fwd_kernel(r) for r in rows if isinstance(r, GapF) and r.stride > r.c
                                                                      and r.offset > 0 and not r.half} == {"wide", "narrow"},
    "fwd: _h at C = 64 and 128": lambda rows: {r.c for r in rows if isinstance(r, GapF) and r.half} >= {64, 128},
    "bwd: four-wide and scalar": lambda rows: {gap_bwd_kernel(r) for r in rows if isinstance(r, GapB) and not r.half} == {"four", "scalar"},
    "bwd: scalar by C = 6": lambda rows: any(isinstance(r, GapB) and r.c == 6 and gap_bwd_kernel(r) == "scalar" for r in rows),
    "bwd: scalar by a view 4 bytes into its arena": lambda rows: any(isinstance(r, GapB) and r.c == 8 and r.lead == 4 and gap_bwd_kernel(r) == "scalar" for r in rows),
    "bwd: slices, both kernels": lambda rows: {gap_bwd_kernel(r) for r in rows if isinstance(r, GapB) and r.stride > r.c and r.offset > 0
                                               and not r.half} == {"four", "scalar"},
    "bwd: _h": lambda rows: any(isinstance(r, GapB) and r.half for r in rows),
}


def gap_fwd_case(r):
    g = _gen(r.id)
    shape = (r.hw, r.n, r.c) if r.hwnc else (r.n, r.hw, r.c)
    x = torch.randn(shape, generator=g) * torch.exp2(torch.rand(r.c, generator=g) * 2 - 1) + torch.randn(r.c, generator=g)
    return x.half() if r.half else x.float()


def gap_fwd_ref(r, x):
    d = 0 if r.hwnc else 1
    x64 = x.double()
    return x64.mean(d), (r.hw + 1) * U * x64.abs().sum(d) / r.hw * SLACK


def gap_bwd_case(r):
    g = _gen(r.id)
    c = Case()
    c.dpooled = torch.randn(r.n, r.stride, generator=g)
    c.old = torch.randn(r.n, r.hw, r.c, generator=g)
    c.old = c.old.half() if r.half else c.old
    return c


def gap_bwd_ref(r, c, accumulate):
    gq = (c.dpooled[:, r.offset:r.offset + r.c].double() / r.hw)[:, None, :].expand(r.n, r.hw, r.c)
    want, bar = gq, 2 * U * gq.abs()
    if accumulate:
        want = c.old.double() + gq
        bar = bar + U * want.abs()
    bar = bar * SLACK
    return want, half_stored(want, bar) if r.half else bar


def _poisoned(t):
    return bool((_bits(t) == 255).all())


def run_gap_fwd_row(r, dev):
    hip, lib, st = _lib()
    assert gap_fwd_kernel(r) == r.kernel
    x = gap_fwd_case(r)
    ia = Arena(dev)
    xd = ia.inp("x", x)

    def launch():
        ar = Arena(dev)
        o = {"out": ar.out("out", (r.n, r.stride), torch.float32, all_written=False)}
        if r.half:
            hip.check(lib.ssad_gap_fwd_h(_p(xd), _p(o["out"]), r.n, r.hw, r.c, r.stride, r.offset, st))
        else:
            hip.check(lib.ssad_gap_fwd(_p(xd), _p(o["out"]), r.n, r.hw, r.c, r.stride, r.offset, r.hwnc, st))
        ar.check_outputs(r.id)
        return o
    o = twice(r.id, launch)
    out = o["out"].cpu()
    assert _poisoned(out[:, :r.offset]) and _poisoned(out[:, r.offset + r.c:]), f"{r.id}: wrote outside its slice of the output rows"
    within(r.id, "gap_fwd", out[:, r.offset:r.offset + r.c], *gap_fwd_ref(r, x))
    ia.check_inputs(r.id)


def run_gap_bwd_row(r, dev):
    hip, lib, st = _lib()
    assert gap_bwd_kernel(r) == r.kernel
    c = gap_bwd_case(r)
    ia = Arena(dev)
    dpd = ia.inp("dpooled", c.dpooled)
    tdt = torch.float16 if r.half else torch.float32
    for acc in (False, True):
        eid = f"{r.id}{' accumulate' if acc else ''}"

        def launch():
            ar = Arena(dev)
            o = {"dy": ar.inp("dy", c.old, mutable=True, lead=r.lead) if acc else ar.out("dy", (r.n, r.hw, r.c), tdt, lead=r.lead)}
            assert (o["dy"].data_ptr() % 16 == 0) == (r.lead % 16 == 0)
            fn = lib.ssad_gap_bwd_h if r.half else lib.ssad_gap_bwd
            hip.check(fn(_p(dpd), _p(o["dy"]), r.n, r.hw, r.c, r.stride, r.offset, int(acc), st))
            ar.check_outputs(eid)
            return o
        o = twice(eid, launch)
        within(eid, "gap_bwd", o["dy"], *gap_bwd_ref(r, c, acc))
    ia.check_inputs(r.id)


# =====================================================================================================================================
# the plain max-pool
# =====================================================================================================================================
PoolRow = collections.namedtuple("PoolRow", "id n h w c ties")
POOL_HW = ((1, 1), (1, 2), (2, 3), (9, 11), (16, 16))
POOL = [PoolRow(f"pool_{n}x{h}x{w}x{c}{'_ties' if ties else ''}", n, h, w, c, ties)
        for (h, w) in POOL_HW for c in (4, 68) for n in (1, 3) for ties in (False, True)]


def pool_case(r):
    g = _gen(r.id)
    k = Case()
    shape = (r.n, r.h, r.w, r.c)
    if r.ties:
        k.x = torch.randint(-2, 2, shape, generator=g).float()                  # {-2, -1, 0, 1}: many exact ties
    else:
        k.x = -(torch.rand(shape, generator=g) * 4 + 2.0 ** -20)                # strictly negative: a padded 0 would win every border window
    ho, wo = (r.h - 1) // 2 + 1, (r.w - 1) // 2 + 1
    k.dy = torch.randn(r.n, ho, wo, r.c, generator=g)
    return k


class PoolRef:
    """F.max_pool2d on the CPU (first maximum in row-major order) for values and winners; the gather in fp32 in the order oy, ox."""

    def __init__(self, r, k, dtype=torch.float64):
        n, h, w, c = k.x.shape
        pooled, ind = F.max_pool2d(k.x.to(dtype).permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
        self.pooled = pooled.permute(0, 2, 3, 1).contiguous()
        ind = ind.permute(0, 2, 3, 1)
        ho, wo = ind.shape[1:3]
        oy, ox = torch.arange(ho).view(1, ho, 1, 1), torch.arange(wo).view(1, 1, wo, 1)
        self.wy, self.wx = ind // w, ind % w
        self.slot = ((self.wy - (2 * oy - 1)) * 3 + (self.wx - (2 * ox - 1))).to(torch.uint8).contiguous()
        dx = torch.zeros(n, h, w, c, dtype=torch.float32)
        nn_, cc = torch.arange(n).view(n, 1).expand(n, c), torch.arange(c).view(1, c).expand(n, c)
        for y, x in itertools.product(range(ho), range(wo)):                    # fp32, one window after the other: the kernels' order
            dx.index_put_((nn_, self.wy[:, y, x, :], self.wx[:, y, x, :], cc), k.dy[:, y, x, :], accumulate=True)
        self.dx = dx


def run_pool_row(r, dev):
    hip, lib, st = _lib()
    k = pool_case(r)
    ref = PoolRef(r, k)
    n, h, w, c = k.x.shape
    ho, wo = ref.slot.shape[1:3]
    want = ref.pooled.float()
    assert torch.equal(want.double(), ref.pooled)
    ia = Arena(dev)
    xd, dyd, slotd = ia.inp("x", k.x), ia.inp("dy", k.dy), ia.inp("slots", ref.slot)
    xhd = ia.inp("x hwnc", k.x.permute(1, 2, 0, 3).contiguous())
    for name in ("fwd", "fwd hwnc", "fwd_idx"):
        eid = f"{r.id}[{name}]"

        def launch():
            ar = Arena(dev)
            if name == "fwd hwnc":
                o = {"out": ar.out("pooled", (ho, wo, n, c), torch.float32)}
                hip.check(lib.ssad_maxpool3x3s2_fwd(_p(xhd), _p(o["out"]), n, h, w, c, 1, st))
            elif name == "fwd":
                o = {"out": ar.out("pooled", (n, ho, wo, c), torch.float32)}
                hip.check(lib.ssad_maxpool3x3s2_fwd(_p(xd), _p(o["out"]), n, h, w, c, 0, st))
            else:
                o = {"out": ar.out("pooled", (n, ho, wo, c), torch.float32), "idx": ar.out("slots", (n, ho, wo, c), torch.uint8)}
                hip.check(lib.ssad_maxpool3x3s2_fwd_idx(_p(xd), _p(o["out"]), _p(o["idx"]), n, h, w, c, st))
            ar.check_outputs(eid)
            return o
        o = twice(eid, launch)
        got = o["out"].cpu()
        got = got.permute(2, 0, 1, 3).contiguous() if name == "fwd hwnc" else got
        assert torch.equal(_bits(got), _bits(want)), f"{eid}: pooled values differ from max_pool2d's"
        if name == "fwd_idx":
            assert torch.equal(o["idx"].cpu(), ref.slot), f"{eid}: winner slots differ from max_pool2d's"
    dxs = {}
    for name in ("bwd", "bwd_idx"):
        eid = f"{r.id}[{name}]"

        def launch():
            ar = Arena(dev)
            o = {"dx": ar.out("dx", (n, h, w, c), torch.float32)}
            if name == "bwd":
                hip.check(lib.ssad_maxpool3x3s2_bwd(_p(xd), _p(dyd), _p(o["dx"]), n, h, w, c, k.dy.numel(), st))
            else:
                hip.check(lib.ssad_maxpool3x3s2_bwd_idx(_p(slotd), _p(dyd), _p(o["dx"]), n, h, w, c, k.dy.numel(), st))
            ar.check_outputs(eid)
            return o
        dxs[name] = twice(eid, launch)["dx"].cpu()
        assert torch.equal(_bits(dxs[name]), _bits(ref.dx)), f"{eid}: routed gradients differ from the fp32 gather over max_pool2d's winners"
    assert torch.equal(_bits(dxs["bwd"]), _bits(dxs["bwd_idx"]))
    ia.check_inputs(r.id)


# =====================================================================================================================================
# softmax cross-entropy
# =====================================================================================================================================
CeRow = collections.namedtuple("CeRow", "id b c ldd big_scale logits")        # ldd None: no dlogits; logits: n1 | n30 | ties
_CE = [(1, 1, "c", False, "n1"), (255, 2, "c1", False, "n1"), (256, 4, "32", True, "n30"), (257, 7, "c", False, "ties"),
       (600, 4, "c1", True, "n1"), (600, 7, "32", False, "n30"), (257, 4, None, False, "n1"), (1, 7, "32", True, "ties"),
       (256, 2, "c", False, "ties"), (255, 1, "c1", True, "n30"), (600, 2, None, False, "n30"), (257, 4, "c", True, "ties"),
       (1, 4, "c1", False, "n30"), (255, 7, "c1", True, "n1")]
CE = [CeRow(f"ce_{b}x{c}_ldd{l}_{'gs65536' if big else 'gs1'}_{lg}", b, c, {None: None, "c": c, "c1": c + 1, "32": 32}[l], big, lg)
      for b, c, l, big, lg in _CE]


def ce_case(r):
    g = _gen(r.id)
    k = Case()
    if r.logits == "ties":
        k.logits = torch.randint(-1, 2, (r.b, r.c), generator=g).float() * 1.5
    else:
        k.logits = torch.randn(r.b, r.c, generator=g) * (30.0 if r.logits == "n30" else 1.0)
    k.labels = torch.randint(0, r.c, (r.b,), generator=g, dtype=torch.int64)
    k.gscale = f32((65536.0 if r.big_scale else 1.0) / r.b)
    return k


def ce_ref(r, k):
    """-> loss, its bar, accuracy (fp32, exact), dlogits [B][C] and its bar (float64)."""
    p = k.logits.double()
    b, c = p.shape
    mx = p.max(1, keepdim=True).values
    d = p - mx
    ed = d.exp()
    se = ed.sum(1, keepdim=True)
    lse = se.log() + mx
    py = p.gather(1, k.labels[:, None])
    loss = (lse - py).mean()
    eta = (c - 1 + 2 * E_ULP) * U + U * (ed * d.abs()).sum(1, keepdim=True) / se
    e_lse = eta + 2 * L_ULP * U * se.log().abs() + U * lse.abs()
    row = e_lse + U * (lse - py).abs()
    loss_bar = (row.mean() + U * loss.abs()) * SLACK
    first = (p == mx).double().argmax(1)                                        # the first maximum
    acc = torch.tensor(float(int((first == k.labels).sum())), dtype=torch.float32) / torch.tensor(float(b), dtype=torch.float32)
    s = (p - lse).exp()
    onehot = F.one_hot(k.labels, c).double()
    dl = (s - onehot) * k.gscale
    a = e_lse + U * (p - lse).abs()
    dl_bar = abs(k.gscale) * (s * (a + 2 * E_ULP * U) + 2 * U * (s - onehot).abs() + 2.0 ** -126) * SLACK
    return loss, loss_bar, acc, dl, dl_bar


def run_ce_row(r, dev):
    hip, lib, st = _lib()
    k = ce_case(r)
    loss, loss_bar, acc, dl, dl_bar = ce_ref(r, k)
    ia = Arena(dev)
    lgd, lbd = ia.inp("logits", k.logits), ia.inp("labels", k.labels)

    def launch():
        ar = Arena(dev)
        o = {"loss_acc": ar.out("loss_acc", (2,), torch.float32),
             "dlogits": None if r.ldd is None else ar.out("dlogits", (r.b, r.ldd), torch.float32)}
        hip.check(lib.ssad_softmax_ce(_p(lgd), _p(lbd), r.b, r.c, _p(o["loss_acc"]), _p(o["dlogits"]), r.ldd or 0, k.gscale, st))
        ar.check_outputs(r.id)
        return o
    o = twice(r.id, launch)
    la = o["loss_acc"].cpu()
    within(f"{r.id} loss", "softmax_loss", la[0], loss.reshape(()), loss_bar.reshape(()))
    assert torch.equal(_bits(la[1:]), _bits(acc.reshape(1))), f"{r.id}: accuracy {float(la[1])!r}, want {float(acc)!r}"
    if r.ldd is not None:
        got = o["dlogits"].cpu()
        within(f"{r.id} dlogits", "softmax_dlogits", got[:, :r.c], dl, dl_bar)
        assert bool((_bits(got[:, r.c:]) == 0).all()), f"{r.id}: the padding columns of dlogits are not +0.0"
    ia.check_inputs(r.id)


# =====================================================================================================================================
# SGD and the loss scaler
# =====================================================================================================================================
SgdRow = collections.namedtuple("SgdRow", "id n lr mu wd gs")
BIG_N = EW_MAX_LANES + 3                                                      # past one full round of 8192 x 256 lanes
SGD = [SgdRow("sgd_1", 1, 0.1, 0.9, 1e-4, 0.37), SgdRow("sgd_255_plain", 255, 0.1, 0.0, 0.0, 1.0),
       SgdRow("sgd_257_mom", 257, 0.05, 0.9, 0.0, 1.0 / 128), SgdRow("sgd_257_wd", 257, 0.03, 0.0, 1e-4, 0.37),
       SgdRow("sgd_big", BIG_N, 0.05, 0.9, 1e-4, 0.37)]
SGD_STEPS = 3
LOSS_SCALE = 1000.0                                                            # not a power of two: hyper[3] / scaler[0] rounds


def sgd_case(r):
    g = _gen(r.id)
    k = Case()
    k.p0 = torch.randn(r.n, generator=g)
    k.m0 = torch.zeros(r.n)
    k.g = [torch.randn(r.n, generator=g) * 3 for _ in range(SGD_STEPS)]
    k.hyper = torch.tensor([r.lr, r.mu, r.wd, r.gs], dtype=torch.float32)
    return k


def sgd_ref(p, g, m, hyper, loss_scale=None):
    """One step in float64 from the fp32 state -> m', its bar, p', its bar.  hyper: the fp32 vector."""
    lr, mu, wd, gs = (float(v) for v in hyper.double())
    quot = 0.0
    if loss_scale is not None:
        gs, quot = gs / f32(loss_scale), 1.0
    p, g, m = p.double(), g.double(), m.double()
    m1 = mu * m + (g * gs + wd * p)
    bar_m = (3 * U * ((mu * m).abs() + (g * gs).abs() + (wd * p).abs()) + quot * U * (g * gs).abs()) * SLACK
    p1 = p - lr * m1
    bar_p = 2 * U * (p.abs() + (lr * m1).abs()) * SLACK + abs(lr) * bar_m
    return m1, bar_m, p1, bar_p


def run_sgd_row(r, dev):
    """Three steps; each restarts from the fp32 state ssad_sgd_step left.  Per step: ssad_sgd_step; ssad_sgd_step_dev without a scaler (held to
    the same bars, and compared bit for bit: SGD_DEV_DIFF keeps the largest difference); with a scaler, clean and with found_inf set."""
    hip, lib, st = _lib()
    k = sgd_case(r)
    n = r.n
    lr, mu, wd, gs = (float(v) for v in k.hyper)
    ia = Arena(dev)
    hyd = ia.inp("hyper", k.hyper)
    scl = {"clean": ia.inp("scaler", torch.tensor([LOSS_SCALE, 3.0, 0.0])), "found_inf": ia.inp("scaler", torch.tensor([LOSS_SCALE, 3.0, 1.0]))}
    p, m = k.p0, k.m0
    for step in range(SGD_STEPS):
        gd = ia.inp(f"g{step}", k.g[step])
        res = {}
        for form in ("host", "dev", "clean", "found_inf"):
            eid = f"{r.id} step {step} {form}"

            def launch():
                ar = Arena(dev)
                o = {"p": ar.inp("p", p, mutable=True), "m": ar.inp("m", m, mutable=True)}
                if form == "host":
                    hip.check(lib.ssad_sgd_step(_p(o["p"]), _p(gd), _p(o["m"]), n, lr, mu, wd, gs, st))
                else:
                    hip.check(lib.ssad_sgd_step_dev(_p(o["p"]), _p(gd), _p(o["m"]), n, _p(hyd), None if form == "dev" else _p(scl[form]), st))
                ar.check_outputs(eid)
                return o
            o = twice(eid, launch)
            res[form] = (o["p"].cpu(), o["m"].cpu())
            if form == "found_inf":
                assert torch.equal(_bits(res[form][0]), _bits(p)) and torch.equal(_bits(res[form][1]), _bits(m)), f"{eid}: state written while found_inf is set"
                continue
            m1, bar_m, p1, bar_p = sgd_ref(p, k.g[step], m, k.hyper, LOSS_SCALE if form == "clean" else None)
            within(f"{eid} m", "sgd", res[form][1], m1, bar_m)
            within(f"{eid} p", "sgd", res[form][0], p1, bar_p)
        for i, nm in enumerate(("p", "m")):
            diff = float((res["host"][i].double() - res["dev"][i].double()).abs().max())
            SGD_DEV_DIFF[0] = max(SGD_DEV_DIFF[0], diff)
            print(f"   {r.id} step {step}: max |sgd_step_dev - sgd_step| in {nm} = {diff:.3e}", flush=True)
        for i, nm in enumerate(("p", "m")):                                      # include/ssad.h: "Same arithmetic as ssad_sgd_step"
            assert torch.equal(_bits(res["host"][i]), _bits(res["dev"][i])), f"{r.id} step {step}: sgd_step_dev without a scaler differs from sgd_step in {nm}"
        p, m = res["host"]
    ia.check_inputs(r.id)


SGD_DEV_DIFF = [0.0]

# ---- check_finite ----
FinRow = collections.namedtuple("FinRow", "id n lead plants")                 # plants: {name: element index}
FIN_BIG = 4 * (2 * EW_MAX_LANES) + 23                                          # 67 MB: n4 = 2 step + 5, a third grid-stride round; tail of 3
BAD = (float("inf"), float("-inf"), float("nan"))


def fin_geometry(n, lead):
    """(n4, step, rounds of the vector loop, whether a second in-flight piece is live, tail length)."""
    n4 = n // 4 if lead % 16 == 0 else 0
    step = ew_grid(n) * 256
    return n4, step, cdiv(n4, 2 * step), n4 > step, n - 4 * n4


def _fin_rows():
    rows = []
    for n in (1025, 1026, 1027):
        n4 = n // 4
        pl = {"first piece": 2, "last float4": 4 * (n4 - 1) + 3}
        pl.update({f"tail {j}": 4 * n4 + j for j in range(n % 4)})
        rows.append(FinRow(f"fin_{n}", n, 0, pl))
    rows.append(FinRow("fin_1", 1, 0, {"tail 0": 0}))
    rows.append(FinRow("fin_1027_lead4", 1027, 4, {"first": 0, "last": 1026}))
    rows.append(FinRow("fin_big_lead4", BIG_N, 4, {"second round": EW_MAX_LANES + 1, "last": BIG_N - 1}))
    step = EW_MAX_LANES
    n4 = FIN_BIG // 4
    rows.append(FinRow("fin_67MB", FIN_BIG, 0, {"first piece": 4 * 7 + 1, "second in-flight piece": 4 * (step + 7) + 2,
                                                "third round": 4 * (2 * step + 3) + 1, "clamped piece's last float4": 4 * (n4 - 1) + 3,
                                                "second piece's last float4": 4 * (2 * step - 1), "tail 0": 4 * n4, "tail 1": 4 * n4 + 1,
                                                "tail 2": 4 * n4 + 2}))
    return rows


FIN = _fin_rows()
FIN_CASES = {
    "aligned vector pass": lambda r: fin_geometry(r.n, r.lead)[0] > 0,
    "second piece live": lambda r: fin_geometry(r.n, r.lead)[3] and any(fin_geometry(r.n, r.lead)[1] <= i // 4 < 2 * fin_geometry(r.n, r.lead)[1]
                                                                        for i in r.plants.values()),
    "second piece clamped": lambda r: 0 < fin_geometry(r.n, r.lead)[0] <= fin_geometry(r.n, r.lead)[1],
    "third grid-stride round": lambda r: fin_geometry(r.n, r.lead)[2] == 2 and any(i // 4 >= 2 * fin_geometry(r.n, r.lead)[1] and i < 4 * fin_geometry(r.n, r.lead)[0]
                                                                                   for i in r.plants.values()),
    "scalar tail of 1": lambda r: r.lead == 0 and r.n % 4 == 1 and r.n > 1,
    "scalar tail of 2": lambda r: r.lead == 0 and r.n % 4 == 2,
    "scalar tail of 3": lambda r: r.lead == 0 and r.n % 4 == 3,
    "every tail position planted": lambda r: r.lead == 0 and r.n > 4 and {i for i in r.plants.values() if i >= 4 * (r.n // 4)} == set(range(4 * (r.n // 4), r.n)),
    "unaligned fallback n4 = 0, last element": lambda r: r.lead == 4 and fin_geometry(r.n, r.lead)[0] == 0 and r.n - 1 in r.plants.values(),
    "unaligned fallback past one round": lambda r: r.lead == 4 and r.n > EW_MAX_LANES,
    "n = 1": lambda r: r.n == 1,
}


def fin_case(r):
    """Clean values: normal floats, and +-FLT_MAX, subnormals and -0 spread over the tensor (at every planted position's neighbours too)."""
    g = _gen(r.id)
    x = torch.randn(r.n, generator=g)
    special = torch.tensor([FLT_MAX, -FLT_MAX, 2.0 ** -149, -(2.0 ** -130), -0.0, 2.0 ** -126], dtype=torch.float32)
    idx = torch.randint(0, r.n, (min(r.n, 4096),), generator=g)
    x[idx] = special[torch.arange(idx.numel()) % special.numel()]
    for i in r.plants.values():
        for j in (i - 1, i + 1):
            if 0 <= j < r.n:
                x[j] = special[j % special.numel()]
    assert bool(torch.isfinite(x).all())
    return x


def run_fin_row(r, dev):
    hip, lib, st = _lib()
    x = fin_case(r)
    ia = Arena(dev)
    xd = ia.inp("g", x, lead=r.lead)
    assert (xd.data_ptr() % 16 == 0) == (r.lead == 0)

    def run(eid, state, want_flag):
        def launch():
            ar = Arena(dev)
            o = {"scaler": ar.inp("scaler", torch.tensor(state), mutable=True)}
            hip.check(lib.ssad_check_finite(_p(xd), r.n, _p(o["scaler"]), st))
            ar.check_outputs(eid)
            return o
        got = twice(eid, launch)["scaler"].cpu()
        assert got.tolist() == [state[0], state[1], want_flag], f"{eid}: scaler {got.tolist()}, want found_inf = {want_flag}"

    run(f"{r.id} clean", [65536.0, 5.0, 0.0], 0.0)
    run(f"{r.id} clean, flag already set", [65536.0, 5.0, 1.0], 1.0)
    for where, i in r.plants.items():
        keep = x[i].item()
        for bad in BAD:
            xd[i] = bad
            run(f"{r.id} {bad} at {where} ({i})", [65536.0, 5.0, 0.0], 1.0)
        xd[i] = keep
    run(f"{r.id} clean again", [65536.0, 5.0, 0.0], 0.0)
    ia.check_inputs(r.id)                                                      # every planted element restored: the input is as uploaded


# ---- scale_by_loss_scale ----
SCALE = [(n, s) for n in (1, 257, BIG_N) for s in (65536.0, 1234.5677)]


def run_scale_row(n, s, dev):
    hip, lib, st = _lib()
    rid = f"scale_{n}_{s}"
    x = torch.randn(n, generator=_gen(rid)) * 3
    sc = torch.tensor([s, 7.0, 0.0], dtype=torch.float32)
    ia = Arena(dev)
    scd = ia.inp("scaler", sc)

    def launch():
        ar = Arena(dev)
        o = {"x": ar.inp("x", x, mutable=True)}
        hip.check(lib.ssad_scale_by_loss_scale(_p(o["x"]), n, _p(scd), st))
        ar.check_outputs(rid)
        return o
    got = twice(rid, launch)["x"].cpu()
    assert torch.equal(_bits(got), _bits(x * sc[0])), f"{rid}: x * loss_scale is not the fp32 product"
    ia.check_inputs(rid)


# ---- loss_scaler_update ----
def scaler_model(state, growth, backoff, interval):
    """GradScaler's update on [loss_scale, growth_tracker, found_inf], every product in fp32."""
    scale, tracker, found = state
    if found != 0.0:
        scale, tracker = f32(f32(scale) * f32(backoff)), 0.0
    else:
        tracker += 1.0
        if tracker >= interval:
            scale, tracker = f32(f32(scale) * f32(growth)), 0.0
    return [scale, tracker, 0.0]


# (id, growth, backoff, interval, found_inf of each consecutive step)
SCALER = [("interval1", 2.0, 0.5, 1, (0, 0, 1, 0)),
          ("interval3_overflow_on_growth_step", 2.0, 0.5, 3, (0, 0, 1, 0, 0, 0, 0)),
          ("backoff_quarter", 2.0, 0.25, 2, (1, 1, 0, 0, 1)),
          ("growth_1.5", 1.5, 0.5, 2, (0, 0, 0, 0, 1, 0, 0))]
SCALER_START = [1000.0, 0.0]


def run_scaler_row(row, dev):
    hip, lib, st = _lib()
    rid, growth, backoff, interval, founds = row
    state = SCALER_START + [0.0]
    for i, f in enumerate(founds):
        state = [state[0], state[1], float(f)]
        eid = f"scaler_{rid} step {i}"

        def launch():
            ar = Arena(dev)
            o = {"scaler": ar.inp("scaler", torch.tensor(state, dtype=torch.float32), mutable=True)}
            hip.check(lib.ssad_loss_scaler_update(_p(o["scaler"]), growth, backoff, interval, st))
            ar.check_outputs(eid)
            return o
        got = twice(eid, launch)["scaler"].cpu().tolist()
        state = scaler_model(state, growth, backoff, interval)
        assert got == state, f"{eid}: scaler {got}, want {state}"


# =====================================================================================================================================
ROWS = ([("linear", r) for r in LINEAR] + [("gap_fwd", r) for r in GAP_FWD] + [("gap_bwd", r) for r in GAP_BWD] + [("pool", r) for r in POOL]
        + [("ce", r) for r in CE] + [("sgd", r) for r in SGD] + [("fin", r) for r in FIN] + [("scale", r) for r in SCALE]
        + [("scaler", r) for r in SCALER])


def row_id(kr):
    kind, r = kr
    return r.id if hasattr(r, "id") else f"scale_{r[0]}_{r[1]}" if kind == "scale" else f"scaler_{r[0]}"


def run_row(kr, dev):
    kind, r = kr
    if kind == "scale":
        return run_scale_row(r[0], r[1], dev)
    return {"linear": run_linear_row, "gap_fwd": run_gap_fwd_row, "gap_bwd": run_gap_bwd_row, "pool": run_pool_row, "ce": run_ce_row,
            "sgd": run_sgd_row, "fin": run_fin_row, "scaler": run_scaler_row}[kind](r, dev)
