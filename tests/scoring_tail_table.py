"""The scoring-tail table: what every default result passes through after the trunk -- row L2-normalisation, the k-smallest mean of the
three-kernel cosine chain, the Grad-CAM channel contraction, blur + ReLU + bilinear (both kernels) and the weight repacking (all in
csrc/misc.hip) -- at the smallest shapes that reach each case, compared per element against float64 (or bit for bit where every step
is one correctly rounded operation), over buffers between poisoned guards (Arena, within, twice of tests/bn_table.py); and the
zero-norm rows of every cosine path (csrc/misc.hip, csrc/knn.hip) against sklearn's brute-force cosine neighbours.

Shared by tests/test_scoring_tail_table.py (rows, coverage, the references themselves, the mutation checks: no GPU) and
tests/test_hip_scoring_tail_paths.py (the kernels).

Dispatch, restated from the documented rules (NOT read back from the library):
  l2norm / knn_mean / gradcam   one wave per row, four rows per workgroup of 256; lane l takes elements l, l + 64, ..; xor butterfly
  blur_relu_bilinear            the single-workgroup kernel while (2 h w + ks) * 4 <= 48 KiB of LDS; else 64 x 64 output tiles:
                                span = min(64, target), rmax = max over the axes of int(extent / target * span) + 3,
                                LDS = ((rmax + 2 pad)^2 + rmax^2 + ks) * 4 bytes, refused (return 2) above 64 KiB
  repack                        one thread per element

Bars.  u = 2^-24.  All counted from the kernels' operations and computed from the float64 reference, none from a measurement; each is
multiplied by SLACK = 1 + 2^-10 for the products of roundings.
  l2norm     c u |x_e| / ||x||, c = L + 5, L = ceil(D / 64): a lane's sum of squares is L rounded products and L rounded additions
             (or L fused ones), the butterfly 6 additions, all of one sign: (2 L + 6) u relative on the sum, half of that after the
             square root, + u for sqrtf, + u for the division (both correctly rounded: no fast-math).  A row whose fp32 sum of squares
             is exactly 0 -- a zero row, squares that all underflow -- is divided by 1 (sklearn.preprocessing.normalize): x itself,
             bit for bit.  The rows avoid subnormal squares (asserted on the CPU), where a product loses relative precision.
  knn_mean   bit for bit: d = clip(1 - sim, 0, 2), selection, the k smallest added smallest first and the division by float(k) are
             each exact or one correctly rounded fp32 operation, restated in numpy float32.  Against float64 over the same d: k u |ref|
  gradcam    c u sum_k |a_k w_k|, c = L + 7, L = ceil(C / 64): a term passes one product rounding, at most L lane additions and 6
             butterfly additions; a fused multiply-add only removes roundings
  blur       c u A_e + the coordinate term, A_e = the same operator (blur without ReLU, then bilinear) on |maps| in float64.
             The taps: the fp32 argument of expf restated exactly (sigma = 0.15 ks + 0.35 gives the same float fused or not for every
             ks of the table: asserted), exp, the sum and the division in float64; the kernel's expf is within E = 2 ulp (the HIP math
             API document is not part of this ROCm installation: ASSUMED, the figure tests/step_head_table.py uses), an ulp is at most
             2 u: a tap is within (4 E + ks) u relative (its own expf, the sum's expf terms, ks - 1 additions, one division).
             c = 2 (4 E + ks)   the two taps
               + 1              k1[dy] * k1[dx]
               + 1 + ks^2       src * tap and the sequential accumulation (the first addition to 0 is exact; counted anyway)
               + 6              1 - ly, 1 - lx, and product, addition, product, addition of the four-term interpolation
             = 30 + 1 + 50 + 6 = 87 for ks = 7.  The ReLU is 1-Lipschitz.
             Coordinates: sy = max(s (y + 0.5) - 0.5, 0), y0 = int(sy), ly = sy - y0 in np.float32 with the kernel's expressions; the
             compiler may fuse the product and the subtraction, which moves sy by one rounding of the product.  The table computes
             both forms: their integer parts agree on every row (asserted on the CPU) and the bar takes |ly_fused - ly_plain| times the
             |difference| of the two interpolated rows (columns likewise), a quantity known exactly and 0 on most rows.
  repack     equal to permute, bit for bit

Measured on the MI355X on 2026-10-20 (worst error / bar per entry kind over all rows: MEASURED below; for the record, never asserted).
No row exceeds its counted bar.  l2norm 0.419 of c = L + 5 and knn_mean 0.400 of k u (a bar of one to three roundings) are the tight ones;
gradcam 0.123; blur 0.077 (single) and 0.209 (tiled: the 79 x 78 -> 156 row, whose scale 79 / 156 is not a float, so the coordinate
term is live; the other tiled rows stay at 0.07 - 0.14 like the single kernel's); the zero-norm case 0.037 of its distance bar on every
cosine path, the fused, split and both index forms bit-equal to each other.  The tiled rows with 53.9 KiB (96 x 96 -> 80) and 59.2 KiB
(80 x 80 -> 40) of LDS launch and hold their bars.

The shape (110, 60, 7, 65), whose last tile would be one pixel wide, is refused by the host's rule (rmax = 111: 104 068 bytes of LDS): it stays in the table as a
refusal row (return 2, output untouched), next to (120, 120, 7, 64); the last tile one pixel wide runs at (60, 110, 7, 129).
"""
import collections

import numpy as np
import torch

from bn_table import Arena, within as _within, twice, print_worst as _print_worst, U, cdiv, _seed, _lib, _p, _bits

SLACK = 1.0 + 2.0 ** -10
E_ULP = 2.0                                   # expf (see the docstring: assumed)
LDS_SINGLE, LDS_TILED, BLUR_TT = 48 * 1024, 64 * 1024, 64

# worst error / bar per entry kind, MI355X (from `pytest -s -m gpu tests/test_hip_scoring_tail_paths.py`; never asserted)
MEASURED = {"l2norm": 0.419, "knn_mean": 0.400, "gradcam": 0.123, "blur_single": 0.077, "blur_tiled": 0.209, "cosine_paths": 0.037}
MEASURED_ON = "2026-10-20"

WORST = {}


def within(rid, kind, got, want, bar):
    _within(rid, kind, got, torch.as_tensor(want), torch.as_tensor(bar), worst_of=WORST)


def print_worst():
    _print_worst(WORST)


def _rng(rid):
    return np.random.RandomState(_seed(rid) % (2 ** 31))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# =====================================================================================================================================
# ssad_l2_normalize_rows
# =====================================================================================================================================
L2_KINDS = ("gauss", "gauss3", "big", "small", "one", "zero", "underflow")
L2_N = (1, 3, 4, 5, 1025)
L2_D = (1, 32, 63, 64, 65, 100, 512, 2048)
L2Row = collections.namedtuple("L2Row", "id n d first")             # row i of the matrix is of kind L2_KINDS[(first + i) % 7]
L2 = ([L2Row(f"l2_{n}x{d}", n, d, 0) for n in L2_N for d in L2_D]
      + [L2Row(f"l2_1x{d}_{L2_KINDS[f]}", 1, d, f) for d in L2_D for f in range(1, len(L2_KINDS))])


def l2_kind(r, i):
    return L2_KINDS[(r.first + i) % len(L2_KINDS)]


def l2_case(r):
    g = _rng(r.id)
    x = np.zeros((r.n, r.d), np.float32)
    for i in range(r.n):
        kind = l2_kind(r, i)
        sign = np.where(g.rand(r.d) < 0.5, -1.0, 1.0)
        flat = (sign * (0.25 + g.rand(r.d))).astype(np.float32)
        if kind == "gauss":
            x[i] = g.randn(r.d)
        elif kind == "gauss3":
            x[i] = g.randn(r.d) * 3
        elif kind == "big":
            x[i] = flat * np.float32(1e15)
        elif kind == "small":
            x[i] = flat * np.float32(1e-15)
        elif kind == "one":
            x[i, g.randint(r.d)] = np.float32(-2.7)
        elif kind == "underflow":
            x[i] = flat * np.float32(1e-30)
        # the Gaussian rows: no element whose square would be subnormal
        if kind in ("gauss", "gauss3"):
            x[i] = np.where(np.abs(x[i]) < 2.0 ** -40, np.float32(0.5), x[i])
    return x


def sum_sq_is_zero(x):
    """Whether the fp32 sum of squares of each row is exactly 0, in any order: every square rounds to 0 (|x| <= 2^-75)."""
    return (np.abs(x.astype(np.float64)) <= 2.0 ** -75).all(axis=1)


def l2_ref(x):
    """-> (x / ||x|| in float64 with sklearn's rule for a zero sum of squares, the per-element bar)."""
    x64 = x.astype(np.float64)
    zero = sum_sq_is_zero(x)
    nrm = np.sqrt((x64 * x64).sum(axis=1))
    nrm = np.where(zero, 1.0, nrm)
    want = x64 / nrm[:, None]
    c = cdiv(x.shape[1], 64) + 5
    bar = c * U * np.abs(want) * SLACK
    bar[zero] = 0.0                                                 # x / 1: exact
    return want, bar


def l2_squares_are_normal(x):
    """Every non-zero square of a row that is not a zero-sum row is a normal float (the bar's assumption)."""
    sq = x.astype(np.float64) ** 2
    live = ~sum_sq_is_zero(x)
    return bool(((sq[live] == 0) | ((sq[live] >= 2.0 ** -120) & (sq[live] <= 2.0 ** 110))).all())     # x 2048 stays below 2^128


L2_CASES = {
    "one row": lambda rows: any(r.n == 1 for r in rows),
    "ragged workgroup of three rows": lambda rows: any(r.n == 3 for r in rows),
    "one full workgroup": lambda rows: any(r.n == 4 for r in rows),
    "a second workgroup with one row": lambda rows: any(r.n == 5 for r in rows),
    "many workgroups, the last with one row": lambda rows: any(r.n == 1025 for r in rows),
    "D = 1": lambda rows: any(r.d == 1 for r in rows),
    "half a wave": lambda rows: any(r.d == 32 for r in rows),
    "D = 63, 64, 65 around one lane round": lambda rows: {r.d for r in rows} >= {63, 64, 65},
    "ragged second lane round": lambda rows: any(r.d == 100 for r in rows),
    "D = 512 and 2048": lambda rows: {r.d for r in rows} >= {512, 2048},
    "every kind of row at every D, as a matrix of one row": lambda rows: {(r.d, l2_kind(r, 0)) for r in rows if r.n == 1}
    == {(d, k) for d in L2_D for k in L2_KINDS},
    "every kind of row inside a larger matrix": lambda rows: all({l2_kind(r, i) for i in range(r.n)} == set(L2_KINDS)
                                                                 for r in rows if r.n == 1025),
}


def run_l2_row(r, dev):
    hip, lib, st = _lib()
    from self_supervised import ops
    x = l2_case(r)
    want, bar = l2_ref(x)
    ia = Arena(dev)
    xd = ia.inp("x", _t(x))

    def launch():
        ar = Arena(dev)
        o = {"out": ar.out("out", (r.n, r.d), torch.float32)}
        hip.check(lib.ssad_l2_normalize_rows(_p(xd), _p(o["out"]), r.n, r.d, st))
        ar.check_outputs(r.id)
        return o
    o = twice(r.id, launch)
    within(r.id, "l2norm", o["out"], want, bar)
    zero = sum_sq_is_zero(x)
    if zero.any():
        assert torch.equal(_bits(o["out"].cpu()[_t(zero)]), _bits(_t(x)[_t(zero)])), f"{r.id}: a zero-sum row is not x / 1"
    assert torch.equal(_bits(ops.l2_normalize_rows(xd.contiguous())), _bits(o["out"])), f"{r.id}: ops.l2_normalize_rows differs"
    ia.check_inputs(r.id)


# =====================================================================================================================================
# ssad_cosine_knn_mean
# =====================================================================================================================================
KnnRow = collections.namedtuple("KnnRow", "id nq nb k kind")         # kind: rand | ties | equal
KNN_NQ, KNN_NB = (1, 4, 5), (1, 2, 3, 63, 64, 65, 200)
KNN = [KnnRow(f"knn_{nq}x{nb}_k{k}_{kind}", nq, nb, k, kind)
       for nb in KNN_NB for k in (1, 2, 3) if k <= nb
       for nq, kind in ((1, "rand"), (4, "ties"), (5, "rand"), (5, "equal"))]
KNN_BAD_K = ((0, 5), (4, 5), (3, 2), (2, 1))                           # (k, Nb): return 2, output untouched


def knn_case(r):
    g = _rng(r.id)
    if r.kind == "rand":
        sim = (g.rand(r.nq, r.nb) * 2.6 - 1.3).astype(np.float32)
        if r.nb >= 2:                                               # both clip ends in every row
            sim[:, 0], sim[:, -1] = np.float32(1.25), np.float32(-1.25)
    elif r.kind == "ties":
        sim = (g.randint(-5, 6, (r.nq, r.nb)) * 0.25).astype(np.float32)
    else:
        sim = np.repeat((g.rand(r.nq, 1) * 1.6 - 0.8).astype(np.float32), r.nb, axis=1)
    return np.ascontiguousarray(sim)


def knn_ref(sim, k):
    """-> (the kernel's bits restated in numpy float32, the float64 mean over the same d, its bar)."""
    one = np.float32(1)
    d = np.clip(one - sim, np.float32(0), np.float32(2)).astype(np.float32)
    ds = np.sort(d, axis=1)[:, :k]
    s = ds[:, 0].copy()
    for j in range(1, k):
        s = (s + ds[:, j]).astype(np.float32)
    bits = (s / np.float32(k)).astype(np.float32)
    ref = ds.astype(np.float64).mean(axis=1)
    return bits, ref, k * U * np.abs(ref) * SLACK


KNN_CASES = {
    "Nq = 1, 4, 5": lambda rows: {r.nq for r in rows} == {1, 4, 5},
    "Nb = 1, 2, 3, 63, 64, 65, 200": lambda rows: {r.nb for r in rows} == set(KNN_NB),
    "k = 1, 2, 3 wherever k <= Nb": lambda rows: {(r.nb, r.k) for r in rows} == {(nb, k) for nb in KNN_NB for k in (1, 2, 3) if k <= nb},
    "Nb < 3 with k = Nb": lambda rows: {(r.nb, r.k) for r in rows} >= {(1, 1), (2, 2)},
    "sim above 1 and below -1 in a row": lambda rows: any(r.kind == "rand" and r.nb >= 2 and (knn_case(r) > 1).any(axis=1).all()
                                                          and (knn_case(r) < -1).any(axis=1).all() for r in rows),
    "ties among the k smallest": lambda rows: any(r.kind == "ties" and r.nb >= 63 and r.k == 3 for r in rows),
    "all-equal rows": lambda rows: any(r.kind == "equal" and r.nb >= 3 for r in rows),
    "lanes without an element (Nb < 64)": lambda rows: any(r.nb < 64 for r in rows),
    "a lane with four elements (Nb = 200)": lambda rows: any(r.nb == 200 for r in rows),
}


def run_knn_row(r, dev):
    hip, lib, st = _lib()
    from self_supervised import ops
    sim = knn_case(r)
    bits, ref, bar = knn_ref(sim, r.k)
    ia = Arena(dev)
    sd = ia.inp("sim", _t(sim))

    def launch():
        ar = Arena(dev)
        o = {"out": ar.out("out", (r.nq,), torch.float32)}
        hip.check(lib.ssad_cosine_knn_mean(_p(sd), _p(o["out"]), r.nq, r.nb, r.k, st))
        ar.check_outputs(r.id)
        return o
    o = twice(r.id, launch)
    assert torch.equal(_bits(o["out"].cpu()), _bits(_t(bits))), f"{r.id}: not the fp32 mean of the k smallest distances, bit for bit"
    within(r.id, "knn_mean", o["out"], ref, bar)
    assert torch.equal(_bits(ops.cosine_knn_mean(sd.contiguous(), r.k)), _bits(o["out"])), f"{r.id}: ops.cosine_knn_mean differs"
    ia.check_inputs(r.id)


def run_knn_bad_k(dev):
    hip, lib, st = _lib()
    for k, nb in KNN_BAD_K:
        ia, ar = Arena(dev), Arena(dev)
        sd = ia.inp("sim", torch.zeros(3, nb))
        out = ar.out("out", (3,), torch.float32, all_written=False)
        assert lib.ssad_cosine_knn_mean(_p(sd), _p(out), 3, nb, k, st) == 2, f"k = {k}, Nb = {nb}: not refused"
        ar.check_outputs(f"knn k = {k}")
        assert bool((_bits(out) == 255).all()), f"k = {k}, Nb = {nb}: the refused call wrote its output"
        ia.check_inputs(f"knn k = {k}")


# =====================================================================================================================================
# ssad_gradcam_map
# =====================================================================================================================================
CamRow = collections.namedtuple("CamRow", "id b hw c stride lead")     # alpha = columns lead .. lead + C of a [B][stride] matrix
CAM_B, CAM_HW, CAM_C = (1, 3), (1, 3, 4, 5, 49), (1, 63, 64, 65, 512)
CAM = [CamRow(f"cam_{b}x{hw}x{c}{'_slice' if b == 3 else ''}", b, hw, c, c + 9 if b == 3 else c, 4 if b == 3 else 0)
       for b in CAM_B for hw in CAM_HW for c in CAM_C]


def cam_case(r):
    g = _rng(r.id)
    act = g.randn(r.b, r.hw, r.c).astype(np.float32)
    wide = g.randn(r.b, r.stride).astype(np.float32)
    return act, wide


def cam_ref(r, act, wide):
    a = wide[:, r.lead:r.lead + r.c].astype(np.float64)
    prod = act.astype(np.float64) * a[:, None, :]
    c = cdiv(r.c, 64) + 7
    return prod.sum(axis=2), c * U * np.abs(prod).sum(axis=2) * SLACK


CAM_CASES = {
    "B = 1 and 3": lambda rows: {r.b for r in rows} == {1, 3},
    "HW = 1, 3, 4, 5, 49": lambda rows: {r.hw for r in rows} == set(CAM_HW),
    "a position group of four spanning two images": lambda rows: any(r.b == 3 and r.hw % 4 != 0 and r.hw > 1 for r in rows),
    "C = 1, 63, 64, 65, 512": lambda rows: {r.c for r in rows} == set(CAM_C),
    "alpha a column slice of a wider matrix": lambda rows: any(r.stride > r.c and r.lead > 0 for r in rows),
    "alpha_stride = C": lambda rows: any(r.stride == r.c for r in rows),
    "sums that cancel": lambda rows: any(r.c == 512 and (np.abs(cam_ref(r, *cam_case(r))[0])
                                                          < 0.02 * cam_ref(r, *cam_case(r))[1] / (U * 15)).any() for r in rows),
}


def run_cam_row(r, dev):
    hip, lib, st = _lib()
    from self_supervised import ops
    act, wide = cam_case(r)
    want, bar = cam_ref(r, act, wide)
    ia = Arena(dev)
    ad, wd = ia.inp("act", _t(act)), ia.inp("alpha", _t(wide))
    alpha = wd[:, r.lead:r.lead + r.c]

    def launch():
        ar = Arena(dev)
        o = {"out": ar.out("out", (r.b, r.hw), torch.float32)}
        hip.check(lib.ssad_gradcam_map(_p(ad), alpha.data_ptr(), _p(o["out"]), r.b, r.hw, r.c, r.stride, st))
        ar.check_outputs(r.id)
        return o
    o = twice(r.id, launch)
    within(r.id, "gradcam", o["out"], want, bar)
    got = ops.gradcam_map(ad.view(r.b, r.hw, 1, r.c), alpha)
    assert torch.equal(_bits(got), _bits(o["out"])), f"{r.id}: ops.gradcam_map differs"
    ia.check_inputs(r.id)


# =====================================================================================================================================
# ssad_blur_relu_bilinear
# =====================================================================================================================================
BlurRow = collections.namedtuple("BlurRow", "id h w ks target n kernel")        # kernel: single | tiled | refused
BLUR = [
    BlurRow("blur_4x4_k7_t8", 4, 4, 7, 8, 3, "single"),                        # pad = h - 1
    BlurRow("blur_7x7_k7_t16", 7, 7, 7, 16, 3, "single"),
    BlurRow("blur_7x7_k1_t16", 7, 7, 1, 16, 3, "single"),
    BlurRow("blur_9x5_k3_t10", 9, 5, 3, 10, 3, "single"),
    BlurRow("blur_40x100_k7_t64", 40, 100, 7, 64, 3, "single"),
    BlurRow("blur_78x78_k7_t156", 78, 78, 7, 156, 3, "single"),                # the largest square map of the single kernel
    BlurRow("blur_16x16_k5_t8", 16, 16, 5, 8, 3, "single"),                    # down-sampling
    BlurRow("blur_16x16_k7_t16", 16, 16, 7, 16, 3, "single"),                  # identity size
    BlurRow("blur_79x78_k7_t156", 79, 78, 7, 156, 2, "tiled"),                 # the first shape past the boundary
    BlurRow("blur_60x110_k7_t128", 60, 110, 7, 128, 2, "tiled"),
    BlurRow("blur_60x110_k7_t129", 60, 110, 7, 129, 2, "tiled"),               # last tile one pixel wide
    BlurRow("blur_80x80_k7_t40", 80, 80, 7, 40, 2, "tiled"),                   # target below one tile, span = target
    BlurRow("blur_90x90_k7_t200", 90, 90, 7, 200, 2, "tiled"),
    BlurRow("blur_96x96_k7_t80", 96, 96, 7, 80, 2, "tiled"),                   # mild down-sampling
    # its last tile is one pixel wide, but rmax = int(110 / 65 * 64) + 3 = 111 needs 104 068 bytes of LDS: refused by the documented rule
    BlurRow("blur_110x60_k7_t65", 110, 60, 7, 65, 2, "refused"),
    BlurRow("blur_120x120_k7_t64", 120, 120, 7, 64, 2, "refused"),
]
MAP_KINDS = ("rand", "negative", "constant")


def blur_geometry(h, w, ks, target):
    """-> (kernel, LDS bytes, tiles, span, rmax) by the host's rule."""
    lds = (2 * h * w + ks) * 4
    if lds <= LDS_SINGLE:
        return "single", lds, 0, 0, 0
    tiles = cdiv(target, BLUR_TT)
    span = min(BLUR_TT, target)
    rmax = max(int(h / target * span) + 3, int(w / target * span) + 3)
    sw = rmax + 2 * (ks // 2)
    lds = (sw * sw + rmax * rmax + ks) * 4
    return ("tiled" if lds <= LDS_TILED else "refused"), lds, tiles, span, rmax


def coords(extent, target, fused=False):
    """The kernel's source coordinates along one axis in np.float32 -> (i0, i1, lambda) per output index.  fused: the product and the
    subtraction as one fused multiply-add (exact in float64, rounded once)."""
    s = np.float32(extent) / np.float32(target)
    t = (np.arange(target, dtype=np.float32) + np.float32(0.5)).astype(np.float32)
    if fused:
        v = (s.astype(np.float64) * t.astype(np.float64) - 0.5).astype(np.float32)
    else:
        v = ((s * t).astype(np.float32) - np.float32(0.5)).astype(np.float32)
    v = np.maximum(v, np.float32(0))
    i0 = v.astype(np.int32)
    i1 = i0 + (i0 < extent - 1)
    lam = (v - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, lam


def sigma_of(ks, fused=False):
    a, k, b = np.float32(0.15), np.float32(ks), np.float32(0.35)
    if fused:
        return np.float32(np.float64(a) * np.float64(k) + np.float64(b))
    return np.float32(np.float32(a * k) + b)


def taps(ks):
    """The 1-D taps: the fp32 argument of expf as the kernel forms it, then exp, sum and division in float64."""
    sigma = sigma_of(ks)
    half = np.float32(np.float32(ks - 1) * np.float32(0.5))
    x = (-half + np.arange(ks, dtype=np.float32)).astype(np.float32)
    q = (x / sigma).astype(np.float32)
    arg = ((np.float32(-0.5) * q).astype(np.float32) * q).astype(np.float32)
    v = np.exp(arg.astype(np.float64))
    return v / v.sum()


def blur_c(ks):
    return 2 * (4 * E_ULP + ks) + 1 + 1 + ks * ks + 6


def blur_op(m64, ks, target, relu, k1=None):
    """Blur (reflect pad, outer-product taps), optional ReLU, bilinear with the float32 coordinates; float64 otherwise.
    m64 [n][h][w] -> (out [n][T][T], the |d out / d ly| and |d out / d lx| magnitudes)."""
    n, h, w = m64.shape
    k1 = taps(ks) if k1 is None else k1
    pad = ks // 2
    p = np.pad(m64, ((0, 0), (pad, pad), (pad, pad)), mode="reflect") if pad else m64
    b = np.zeros_like(m64)
    for dy in range(ks):
        for dx in range(ks):
            b += p[:, dy:dy + h, dx:dx + w] * (k1[dy] * k1[dx])
    if relu:
        b = np.maximum(b, 0.0)
    y0, y1, ly = coords(h, target)
    x0, x1, lx = coords(w, target)
    ly, lx = ly.astype(np.float64)[None, :, None], lx.astype(np.float64)[None, None, :]
    top = (1 - lx) * b[:, y0][:, :, x0] + lx * b[:, y0][:, :, x1]
    bot = (1 - lx) * b[:, y1][:, :, x0] + lx * b[:, y1][:, :, x1]
    left = (1 - ly) * b[:, y0][:, :, x0] + ly * b[:, y1][:, :, x0]
    right = (1 - ly) * b[:, y0][:, :, x1] + ly * b[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot, np.abs(bot - top), np.abs(right - left)


def blur_ref(maps, ks, target):
    """-> (want, bar) in float64 for maps [n][h][w] float32."""
    m64 = maps.astype(np.float64)
    n, h, w = m64.shape
    want, dly, dlx = blur_op(m64, ks, target, True)
    mag, _, _ = blur_op(np.abs(m64), ks, target, False)
    d_ly = np.abs(coords(h, target, True)[2].astype(np.float64) - coords(h, target)[2].astype(np.float64))[None, :, None]
    d_lx = np.abs(coords(w, target, True)[2].astype(np.float64) - coords(w, target)[2].astype(np.float64))[None, None, :]
    return want, (blur_c(ks) * U * mag + d_ly * dly + d_lx * dlx) * SLACK


def blur_case(r):
    g = _rng(r.id)
    kinds = MAP_KINDS if r.n == 3 else ("rand", MAP_KINDS[1 + BLUR.index(r) % 2])
    maps = np.zeros((r.n, r.h, r.w), np.float32)
    for i, kind in enumerate(kinds):
        if kind == "rand":
            maps[i] = g.rand(r.h, r.w) - 0.3
        elif kind == "negative":
            maps[i] = -(g.rand(r.h, r.w) + 0.01)
        else:
            maps[i] = 0.7
    return maps, kinds


def tile_extents(h, w, target, tiles):
    """(nr, nc) of every output tile of the tiled kernel, with its float32 expressions."""
    out = []
    y0, _, _ = coords(h, target)
    x0, _, _ = coords(w, target)
    for t in range(tiles * tiles):
        ty0, tx0 = (t // tiles) * BLUR_TT, (t % tiles) * BLUR_TT
        ty1, tx1 = min(ty0 + BLUR_TT, target) - 1, min(tx0 + BLUR_TT, target) - 1
        ya, xa = int(y0[ty0]), int(x0[tx0])
        yb, xb = min(int(y0[ty1]) + 1, h - 1), min(int(x0[tx1]) + 1, w - 1)
        out.append((yb - ya + 1, xb - xa + 1, ty1 - ty0 + 1, tx1 - tx0 + 1))
    return out


BLUR_CASES = {
    "a non-square map, both kernels": lambda rows: {r.kernel for r in rows if r.h != r.w} >= {"single", "tiled"},
    "h > w and h < w": lambda rows: any(r.h > r.w for r in rows) and any(r.h < r.w for r in rows),
    "reflect padding at ks / 2 = h - 1": lambda rows: any(r.ks // 2 == r.h - 1 for r in rows),
    "ks = 1, 3, 5, 7": lambda rows: {r.ks for r in rows} >= {1, 3, 5, 7},
    "the dispatch boundary, both sides": lambda rows: any(r.kernel == "single" and blur_geometry(r.h + 1, r.w, r.ks, r.target)[0] != "single"
                                                          and any(q.kernel == "tiled" and (q.h, q.w, q.ks, q.target) == (r.h + 1, r.w, r.ks, r.target)
                                                                  for q in rows) for r in rows),
    "single kernel: down-sampling and identity size": lambda rows: any(r.kernel == "single" and r.target < r.h for r in rows)
    and any(r.kernel == "single" and r.target == r.h == r.w for r in rows),
    "single kernel: n = 3": lambda rows: all(r.n == 3 for r in rows if r.kernel == "single"),
    "tiled kernel: n = 2": lambda rows: all(r.n == 2 for r in rows if r.kernel == "tiled"),
    "tiled: a target below one 64-wide tile, span = target": lambda rows: any(r.kernel == "tiled" and r.target < BLUR_TT for r in rows),
    "tiled: a last tile one pixel wide": lambda rows: any(r.kernel == "tiled" and r.target % BLUR_TT == 1 for r in rows),
    "tiled: rmax sized under down-sampling": lambda rows: any(r.kernel == "tiled" and r.target < r.h and r.target > BLUR_TT for r in rows),
    "tiled: a tile that fills rmax": lambda rows: any(r.kernel == "tiled" and max(max(e[0], e[1]) for e in tile_extents(r.h, r.w, r.target, blur_geometry(r.h, r.w, r.ks, r.target)[2]))
                                                      >= blur_geometry(r.h, r.w, r.ks, r.target)[4] - 1 for r in rows),
    "tiled: more than 48 KiB of LDS": lambda rows: any(r.kernel == "tiled" and blur_geometry(r.h, r.w, r.ks, r.target)[1] > LDS_SINGLE for r in rows),
    "tiled: the refusal above 64 KiB": lambda rows: any(r.kernel == "refused" for r in rows),
    "coordinates that round differently when fused": lambda rows: any(r.kernel != "refused" and (coords(r.h, r.target, True)[2] != coords(r.h, r.target)[2]).any()
                                                                      for r in rows),
    "all-negative and constant maps, both kernels": lambda rows: {(r.kernel, k) for r in rows if r.kernel != "refused" for k in blur_case(r)[1]}
    >= {(kn, k) for kn in ("single", "tiled") for k in MAP_KINDS},
}


def run_blur_row(r, dev):
    hip, lib, st = _lib()
    from self_supervised import ops
    kernel, lds, tiles, span, rmax = blur_geometry(r.h, r.w, r.ks, r.target)
    assert kernel == r.kernel, f"{r.id}: the LDS rule names {kernel}"
    maps, kinds = blur_case(r)
    ia = Arena(dev)
    md = ia.inp("maps", _t(maps))
    if kernel == "refused":
        ar = Arena(dev)
        out = ar.out("out", (r.n, r.target, r.target), torch.float32, all_written=False)
        assert lib.ssad_blur_relu_bilinear(_p(md), _p(out), r.n, r.h, r.w, r.ks, r.target, st) == 2, f"{r.id}: not refused"
        ar.check_outputs(r.id)
        assert bool((_bits(out) == 255).all()), f"{r.id}: the refused call wrote its output"
        ia.check_inputs(r.id)
        return
    want, bar = blur_ref(maps, r.ks, r.target)

    def launch():
        ar = Arena(dev)
        o = {"out": ar.out("out", (r.n, r.target, r.target), torch.float32)}
        hip.check(lib.ssad_blur_relu_bilinear(_p(md), _p(o["out"]), r.n, r.h, r.w, r.ks, r.target, st))
        ar.check_outputs(r.id)
        return o
    o = twice(r.id, launch)
    within(r.id, f"blur_{kernel}", o["out"], want, bar)
    got = o["out"].cpu()
    for i, kind in enumerate(kinds):
        if kind == "negative":
            assert bool((got[i] == 0).all()), f"{r.id}: an all-negative map does not give exactly 0"
    wrapped = ops.blur_relu_bilinear(md.view(r.n, 1, r.h, r.w), r.ks, r.target)
    assert torch.equal(_bits(wrapped), _bits(o["out"])), f"{r.id}: ops.blur_relu_bilinear differs"
    ia.check_inputs(r.id)


# =====================================================================================================================================
# ssad_repack_*
# =====================================================================================================================================
REPACK = [(5, 3, 2, 4), (1, 1, 1, 1), (64, 3, 7, 7), (7, 64, 1, 1)]


def run_repack_row(shape, dev):
    hip, lib, st = _lib()
    from self_supervised import ops
    o_, i_, kh, kw = shape
    rid = "repack_%dx%dx%dx%d" % shape
    w = torch.randn(shape, generator=torch.Generator().manual_seed(_seed(rid)))
    ohwi = w.permute(0, 2, 3, 1).contiguous()
    ia = Arena(dev)
    wd, od = ia.inp("oihw", w), ia.inp("ohwi", ohwi)

    def launch():
        ar = Arena(dev)
        o = {"ohwi": ar.out("ohwi", (o_, kh, kw, i_), torch.float32), "oihw": ar.out("oihw", shape, torch.float32),
             "round": ar.out("round trip", shape, torch.float32)}
        hip.check(lib.ssad_repack_oihw_to_ohwi(_p(wd), _p(o["ohwi"]), o_, i_, kh, kw, st))
        hip.check(lib.ssad_repack_ohwi_to_oihw(_p(od), _p(o["oihw"]), o_, i_, kh, kw, st))
        hip.check(lib.ssad_repack_ohwi_to_oihw(_p(o["ohwi"]), _p(o["round"]), o_, i_, kh, kw, st))
        ar.check_outputs(rid)
        return o
    o = twice(rid, launch)
    assert torch.equal(_bits(o["ohwi"].cpu()), _bits(ohwi)), f"{rid}: oihw -> ohwi is not permute(0, 2, 3, 1)"
    assert torch.equal(_bits(o["oihw"].cpu()), _bits(w)), f"{rid}: ohwi -> oihw is not permute(0, 3, 1, 2)"
    assert torch.equal(_bits(o["round"].cpu()), _bits(w)), f"{rid}: the round trip changes the weights"
    assert torch.equal(_bits(ops.repack_oihw_to_ohwi(wd.contiguous())), _bits(o["ohwi"]))
    assert torch.equal(_bits(ops.repack_ohwi_to_oihw(od.contiguous())), _bits(o["oihw"]))
    ia.check_inputs(rid)


# =====================================================================================================================================
# zero-norm rows through every cosine path
# =====================================================================================================================================
ZN_N, ZN_R, ZN_D, ZN_K = 130, 131, 32, 3                                 # one full and one ragged 128-row tile on each side
ZN_QUERY = {0: "zero", 1: "underflow", 129: "zero"}
ZN_BANK = {5: "zero", 64: "zero", 130: "underflow"}


def zero_norm_case():
    g = _rng("zero_norm")
    x = (g.randn(ZN_N, ZN_D) * 3).astype(np.float32)
    bank = g.randn(ZN_R, ZN_D).astype(np.float32)
    for t, plan in ((x, ZN_QUERY), (bank, ZN_BANK)):
        for i, kind in plan.items():
            t[i] = 0 if kind == "zero" else np.float32(1e-30) * (0.25 + g.rand(ZN_D)).astype(np.float32)
    return x, bank


def zero_norm_ref(x, bank, k=ZN_K):
    """float64 cosine distances with sklearn's rule -> (the k smallest per query, ascending [N][k], their mean, the bar of a distance).
    Bar: both rows normalised within (1 + 5) u per element, so <= 12 u on a dot product of unit rows; the contraction adds a rounded
    product and a rounded addition per term, <= 2 D u sum |a b| <= 2 D u; 1 - sim one more u of at most 2."""
    xn, bn = l2_ref(x)[0], l2_ref(bank)[0]
    d = np.clip(1.0 - xn @ bn.T, 0.0, 2.0)
    ds = np.sort(d, axis=1)[:, :k]
    return ds, ds.mean(axis=1), (2 * ZN_D + 12 + 2) * U * SLACK


def sklearn_distances(x, bank, k=ZN_K):
    from sklearn.neighbors import NearestNeighbors
    return NearestNeighbors(n_neighbors=k, algorithm="brute", metric="cosine").fit(bank).kneighbors(x)[0]


def run_zero_norm(dev):
    """ops.l2_normalize_rows, the three-kernel chain, ssad_cosine_knn_fused, _split, _index (one launch and split) on the zero-norm case:
    every distance within its bar of float64 and of sklearn (twice the bar: sklearn's own fp32 arithmetic), zero-norm queries at exactly 1."""
    hip, lib, st = _lib()
    from self_supervised import ops
    x, bank = zero_norm_case()
    ds, mean, bar = zero_norm_ref(x, bank)
    sk = sklearn_distances(x, bank).astype(np.float64)
    assert np.abs(sk - ds).max() <= bar, "sklearn and the float64 reference disagree"
    ia = Arena(dev)
    xd, bd = ia.inp("x", _t(x)), ia.inp("bank", _t(bank))
    bn = ops.l2_normalize_rows(bd.contiguous())
    within("zero_norm bank rows", "l2norm", bn, *l2_ref(bank))
    xn = ops.l2_normalize_rows(xd.contiguous())
    within("zero_norm query rows", "l2norm", xn, *l2_ref(x))
    for t, src, plan in ((xn, x, ZN_QUERY), (bn, bank, ZN_BANK)):
        for i in plan:
            assert torch.equal(_bits(t[i].cpu()), _bits(_t(src[i]))), f"zero-norm row {i} is not x / 1"
    ib = Arena(dev)
    bnd = ib.inp("normalised bank", bn.cpu())
    n, r, d, k = ZN_N, ZN_R, ZN_D, ZN_K
    full = np.full((n,), bar + 2 * k * U * SLACK)                     # k - 1 additions and the division, of values <= 2
    zq = sorted(ZN_QUERY)
    got = {}
    got["chain"] = ops.cosine_knn_mean(ops.linear_fwd(xn, bnd.contiguous()), k)

    def mean_launch(name, call):
        def launch():
            ar = Arena(dev)
            o = {"out": ar.out("out", (n,), torch.float32)}
            part = ar.out("part", (2, n, 3), torch.float32, all_written=False)
            hip.check(call(_p(o["out"]), _p(part)))
            ar.check_outputs(name)
            return o
        got[name] = twice(name, launch)["out"]

    mean_launch("fused", lambda out, part: lib.ssad_cosine_knn_fused(_p(xd), _p(bnd), out, n, d, r, k, st))
    mean_launch("split", lambda out, part: lib.ssad_cosine_knn_split(_p(xd), _p(bnd), part, out, n, d, r, k, 2, st))
    for name, v in got.items():
        within(f"zero_norm {name} against float64", "cosine_paths", v, mean, full)
        within(f"zero_norm {name} against sklearn", "cosine_paths", v, sk.mean(axis=1), 2 * full)
        assert bool((v.cpu()[zq] == 1.0).all()), f"zero_norm {name}: a zero-norm query does not score exactly 1"
    assert torch.equal(_bits(got["fused"]), _bits(got["split"])), "the split form differs from the fused kernel"
    idx_got = {}
    for name, s in (("index", 1), ("index_split", 2)):
        def launch():
            ar = Arena(dev)
            o = {"dist": ar.out("dist", (n, k), torch.float32), "idx": ar.out("idx", (n, k), torch.int32)}
            part = ar.out("part", (2, n, 3), torch.int64, all_written=False)
            hip.check(lib.ssad_cosine_knn_index(_p(xd), _p(bnd), _p(part), _p(o["dist"]), _p(o["idx"]), n, d, r, k, s, st))
            ar.check_outputs(name)
            return o
        o = twice(name, launch)
        idx_got[name] = o
        within(f"zero_norm {name} against float64", "cosine_paths", o["dist"], ds, np.full(ds.shape, bar))
        within(f"zero_norm {name} against sklearn", "cosine_paths", o["dist"], sk, np.full(ds.shape, 2 * bar))
        dist, idx = o["dist"].cpu(), o["idx"].cpu()
        assert bool((dist[zq] == 1.0).all()) and idx[zq].tolist() == [[0, 1, 2]] * len(zq), f"zero_norm {name}: a zero-norm query is not at 1 from rows 0, 1, 2"
        hit = torch.isin(idx, torch.tensor(sorted(ZN_BANK), dtype=torch.int32))
        assert bool((dist[hit] == 1.0).all()), f"zero_norm {name}: a zero-norm bank row is not at distance exactly 1"
    for nm in ("dist", "idx"):
        assert torch.equal(_bits(idx_got["index"][nm]), _bits(idx_got["index_split"][nm])), f"the split index form differs in {nm}"
    ia.check_inputs("zero_norm")
    ib.check_inputs("zero_norm")


# =====================================================================================================================================
ROWS = ([("l2", r) for r in L2] + [("knn", r) for r in KNN] + [("cam", r) for r in CAM] + [("blur", r) for r in BLUR]
        + [("repack", s) for s in REPACK])


def row_id(kr):
    kind, r = kr
    return r.id if hasattr(r, "id") else "repack_%dx%dx%dx%d" % r


def run_row(kr, dev):
    kind, r = kr
    return {"l2": run_l2_row, "knn": run_knn_row, "cam": run_cam_row, "blur": run_blur_row, "repack": run_repack_row}[kind](r, dev)
