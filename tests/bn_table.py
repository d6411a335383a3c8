"""The BatchNorm table: every BatchNorm entry point of csrc/train.hip (and the fused stem forms of csrc/stem.hip) at the smallest shapes
that reach each launch geometry, compared per element or per channel against float64 on the CPU, over buffers between poisoned guards.

Shared by tests/test_bn_table.py (geometry, coverage, decidability and the references themselves: no GPU) and tests/test_hip_bn_paths.py
(the kernels).

Geometry, restated from the documented rules (NOT read back from the library):
  col_geom(C, E)   a lane owns E = 4 floats / 8 halves; TC = min(16, C / E) lanes along a row, rounded DOWN to a divisor of 256;
                   RL = 256 / TC row lanes; gx = ceil((C / E) / TC) column blocks
  col_blocks(R)    row blocks: ceil(R / (32 RL)), but at least min(256, ceil(R / (4 RL))), at most 2048, at least 1
  launch           rows_per_block = ceil(R / blocks); nblk = ceil(R / rows_per_block) (no empty trailing block)
  workspace        ssad_colreduce_workspace(R, C) = col_blocks of the FLOAT geometry x 2 C doubles, for half launches too
  apply kernels    R C / E lanes, a grid of min(8192, ceil(lanes / 256)) workgroups of 256; the parameter vectors are loaded once when
                   grid * 256 is a multiple of C / E ("fixed"), else per element
Row: (id, kind, R, C, half, launch, ws, ws_rows).  launch / ws = (TC, RL, gx, nblk, rows_per_block) of the launch (E of the row) and of
the float geometry; ws_rows = the workspace's row blocks.  `tiny` and `small` rows carry the name of their route instead.
  kind  gen    every entry (below)            pos   the same on z with per-channel |mean| / std = 100 (float) / 30 (half)
        sums   bn_stats and the plain column sums only (the 236 MB row)
        tiny   plain column sums (col_sum_tiny_kernel, or the general path just past it)
        small  ssad_bn_small_fwd / _bwd
Entries of a gen / pos row, each a launch of its own, each run twice (bit-identical): bn_stats (no running statistics; momentum 0.1;
momentum 0.3), bn_apply_fwd and bn_apply_fwd_mask (plain, +residual, +relu, +residual+relu), bn_bwd_reduce (saved activation; plain
column sums; dbeta only), bn_bwd_reduce_zmask / _mask, bn_apply_bwd (train / eval, with / without dres), bn_apply_bwd_zmask / _mask.

Bars.  u = 2^-24 (one fp32 rounding, relative), uh = 2^-11 (a value stored as a half).  All from the reference, none from a measurement.
  mean, invstd, running statistics   4 u |ref|: double sums, sqrt and division in double, ONE rounding to fp32
  dbeta, column sums                 u |ref| + 2 u max_r |g_r|: the addends are exact in double, one rounding
  dgamma                             u |ref| + 4 u sum_r |g_r xhat_r|: xhat = (z - mean) * invstd in fp32 is two roundings (the
                                     difference of two fp32 values rounds relative to ITSELF: no cancellation), the product is double
  apply forward                      8 u (|(z - mean) invstd gamma| + |beta| + |res|): subtract, two products (3 u on the first term),
                                     two adds (u each on everything before them)
  stored as a half                   the bar b above + max(uh (|ref| + b), 2^-25): the kernel rounds an fp32 value v within b of ref,
                                     by at most uh |v|; below 2^-14 the halves are 2^-24 apart whatever |v| is (uh |ref| alone, the
                                     first derivation, missed both: found at f16_1025x72, a dz of 6e-7 rounded to the subnormal grid)
  apply backward                     8 u |gamma invstd| (|g| + |dbeta| / R + |xhat dgamma| / R): the last term carries
                                     xhat (2 u), * dgamma (u), invR (u) and its product (u), one subtraction (u), gamma * invstd (u) and
                                     the final product (u) = 8 u; the others fewer.  dres = the masked dy bit for bit.
  pooled values                      the apply-forward bar at the winner; winner slots, raw winners and mask bits exact
  pool backward (no winners tensor)  g_r is a sum of up to four pooled gradients IN fp32 (three roundings): the bars above with
                                     + 3 u a_r on |g_r| where a_r = sum of the |pooled gradients| routed to a pixel that gets several
Sign and tie decisions: an element is undecidable when |y_ref| <= 64 x its apply-forward bar, a pooling window when its two largest
values are closer than 64 x the bar of the largest and are not both the ReLU's zero.  The generators redraw such elements (from the same
seeded stream) until none is left, so every row has ZERO undecidable elements (tests/test_bn_table.py asserts it) and no comparison
skips anything.

Measured on the MI355X on 2026-10-19 (worst error / bar per entry kind over all rows: MEASURED below; for the record, never asserted).
The half rows reach 0.999 of the apply bars because the rounding of the stored half alone can use all of its term; the fp32 rows stay
at 0.56.  dbeta reaches 0.95 where |ref| is large against max |g|: the one rounding to fp32 is then the whole bar.
"""
import collections
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "self-supervised-anomaly-detection_amd")

U, UH = 2.0 ** -24, 2.0 ** -11
DECIDE = 64.0
EPS = float(torch.tensor(1e-5, dtype=torch.float32))            # the float the kernels receive, as a double
MOMENTA = (0.1, 0.3)
GUARD_BYTES = 8192                                               # >= 4 KiB on either side of every tensor
TINY_MAX_ROWS, SMALL_MAX_ROWS, PARTIALS_IN_FLIGHT, EW_MAX_LANES = 4096, 512, 1792, 8192 * 256

# worst error / bar per entry kind, MI355X (from `pytest -s -m gpu tests/test_hip_bn_paths.py`; never asserted)
MEASURED = {"stats": 0.248, "dbeta": 0.949, "dgamma": 0.399, "apply_fwd": 0.999, "apply_bwd": 0.999, "pool_fwd": 0.992, "pool_bwd": 0.996}

Row = collections.namedtuple("Row", "id kind r c half launch ws ws_rows")

GENERAL = [
    Row("f32_1x4", "gen", 1, 4, False, (1, 256, 1, 1, 1), (1, 256, 1, 1, 1), 1),
    Row("f16_5x8", "gen", 5, 8, True, (1, 256, 1, 1, 5), (2, 128, 1, 1, 5), 1),
    Row("f32_7x36", "gen", 7, 36, False, (8, 32, 2, 1, 7), (8, 32, 2, 1, 7), 1),
    Row("f32_1025x48", "gen", 1025, 48, False, (8, 32, 2, 9, 114), (8, 32, 2, 9, 114), 9),
    Row("f16_1025x72", "gen", 1025, 72, True, (8, 32, 2, 9, 114), (16, 16, 2, 17, 61), 17),
    Row("f16_2049x136", "gen", 2049, 136, True, (16, 16, 2, 33, 63), (16, 16, 3, 33, 63), 33),
    Row("f32_600x64", "gen", 600, 64, False, (16, 16, 1, 10, 60), (16, 16, 1, 10, 60), 10),
    Row("f16_1890x64", "gen", 1890, 64, True, (8, 32, 1, 15, 126), (16, 16, 1, 30, 63), 30),
    Row("f32_4099x128", "gen", 4099, 128, False, (16, 16, 2, 65, 64), (16, 16, 2, 65, 64), 65),
    Row("f16_4099x128", "gen", 4099, 128, True, (16, 16, 1, 65, 64), (16, 16, 2, 65, 64), 65),
    Row("f32_45x512", "gen", 45, 512, False, (16, 16, 8, 1, 45), (16, 16, 8, 1, 45), 1),
    Row("f16_45x512", "gen", 45, 512, True, (16, 16, 4, 1, 45), (16, 16, 8, 1, 45), 1),
    Row("f32_32770x256", "gen", 32770, 256, False, (16, 16, 4, 255, 129), (16, 16, 4, 255, 129), 256),
    Row("f16_32770x512", "gen", 32770, 512, True, (16, 16, 4, 255, 129), (16, 16, 8, 255, 129), 256),
    Row("f32_14745605x4", "sums", 14745605, 4, False, (1, 256, 1, 1801, 8188), (1, 256, 1, 1801, 8188), 1801),
    Row("f32_pos_1890x64", "pos", 1890, 64, False, (16, 16, 1, 30, 63), (16, 16, 1, 30, 63), 30),
    Row("f16_pos_1890x64", "pos", 1890, 64, True, (8, 32, 1, 15, 126), (16, 16, 1, 30, 63), 30),
    # just outside ssad_bn_small_ok (R = 513): the general entries
    Row("f32_513x32", "gen", 513, 32, False, (8, 32, 1, 5, 103), (8, 32, 1, 5, 103), 5),
]
TINY = [Row(f"tiny_{r}x{c}", "tiny", r, c, False, "col_sum_tiny", None, None) for c in (4, 8, 16, 32) for r in (1, 33, 4096)]
TINY.append(Row("tiny_4097x32", "tiny", 4097, 32, False, (8, 32, 1, 33, 125), (8, 32, 1, 33, 125), 33))
SMALL = [Row(f"small_{r}x{c}", "small", r, c, False, "bn_small", None, None) for r in (1, 8, 45, 512) for c in (32, 96, 512)]
ROWS = GENERAL + TINY + SMALL
STEM = [(n, h, w, half) for (n, h, w) in ((2, 9, 13), (5, 21, 18), (3, 16, 16)) for half in (False, True)]
STEM_C = 64


# ---- the geometry, restated ----
def cdiv(a, b):
    return -(-a // b)


def col_geom(c, e):
    tc = min(16, c // e)
    while 256 % tc:
        tc -= 1
    return tc, 256 // tc


def col_blocks(r, rl):
    nblk = max(cdiv(r, rl * 32), min(cdiv(r, rl * 4), 256))
    return max(1, min(nblk, 2048))


def launch_geometry(r, c, e):
    """(TC, RL, gx, nblk, rows_per_block) of a column reduction over R x C with E channels per lane."""
    tc, rl = col_geom(c, e)
    rpb = cdiv(r, col_blocks(r, rl))
    return tc, rl, cdiv(c // e, tc), cdiv(r, rpb), rpb


def workspace_rows(r, c):
    return col_blocks(r, col_geom(c, 4)[1])


def lanes(row):
    return row.r * (row.c // (8 if row.half else 4))


def apply_fixed(row):
    """Whether the apply kernels load their parameter vectors once per thread."""
    grid = min(8192, max(1, cdiv(lanes(row), 256)))
    return (grid * 256) % (row.c // (8 if row.half else 4)) == 0


def takes_general_path(row):
    return not isinstance(row.launch, str)


# one predicate per case that must be reached (tests/test_bn_table.py): over the restated geometry only
def _e(row):
    return 8 if row.half else 4


CASES = {
    "TC rounded down, float": lambda r: takes_general_path(r) and not r.half and min(16, r.c // 4) != r.launch[0],
    "TC rounded down, half": lambda r: takes_general_path(r) and r.half and min(16, r.c // 8) != r.launch[0],
    "TC = 1, 2 or 4": lambda r: takes_general_path(r) and r.launch[0] in (1, 2, 4),
    "two column blocks, the second ragged": lambda r: takes_general_path(r) and r.launch[2] > 1 and (r.c // _e(r)) % r.launch[0] != 0,
    "apply kernels reload their parameters (!fixed)": lambda r: r.kind in ("gen", "pos") and not apply_fixed(r),
    "second grid-stride round, float": lambda r: r.kind == "gen" and not r.half and lanes(r) > EW_MAX_LANES,
    "second grid-stride round, half": lambda r: r.kind == "gen" and r.half and lanes(r) > EW_MAX_LANES,
    "nblk shrunk after rounding rows_per_block, float": lambda r: takes_general_path(r) and not r.half
    and r.launch[3] < col_blocks(r.r, r.launch[1]),
    "nblk shrunk after rounding rows_per_block, half": lambda r: takes_general_path(r) and r.half
    and r.launch[3] < col_blocks(r.r, r.launch[1]),
    "ragged last row block": lambda r: takes_general_path(r) and r.launch[3] > 1 and r.r % r.launch[4] != 0,
    "R < RL": lambda r: takes_general_path(r) and r.r < r.launch[1],
    "eight partial rows in flight": lambda r: takes_general_path(r) and r.launch[3] > PARTIALS_IN_FLIGHT,
    "half launch with fewer row blocks than the workspace": lambda r: takes_general_path(r) and r.half and r.launch[3] < r.ws_rows,
    "cancellation, float": lambda r: r.kind == "pos" and not r.half,
    "cancellation, half": lambda r: r.kind == "pos" and r.half,
    "tiny route at its last row count": lambda r: r.launch == "col_sum_tiny" and r.r == TINY_MAX_ROWS,
    "general path just past the tiny route": lambda r: r.kind == "tiny" and takes_general_path(r) and r.r == TINY_MAX_ROWS + 1,
    "small route at its last row count": lambda r: r.launch == "bn_small" and r.r == SMALL_MAX_ROWS,
    "general entries just past the small route": lambda r: r.kind == "gen" and r.r == SMALL_MAX_ROWS + 1 and r.c % 32 == 0,
}


# ---- inputs: seeded CPU generators, redrawn until every sign and tie is decidable ----
def _seed(rid):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(rid))


def _st(t, half):
    return t.half() if half else t.float()


def _params(c, g):
    """gamma in +-[0.5, 1.5] (about a quarter negative, gamma[0] always), beta in +-[0.1, 0.5]."""
    gamma = (0.5 + torch.rand(c, generator=g)) * torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0)
    gamma[0] = -gamma[0].abs()
    beta = (0.1 + 0.4 * torch.rand(c, generator=g)) * torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    return gamma.float(), beta.float()


def stats64(z, eps=EPS):
    """float64 mean, biased variance, invstd over the rows of the STORED z."""
    z = z.double().reshape(-1, z.shape[-1])
    m = z.mean(0)
    var = ((z - m) ** 2).mean(0)
    return m, var, (var + eps).rsqrt()


def half_stored(want, bar):
    """The bar of a value stored as a half: the fp32 value v the kernel rounds is within `bar` of `want`, and rounding it to a half
    moves it by at most uh |v| <= uh (|want| + bar), or by half the spacing of the subnormal halves, 2^-25, below 2^-14."""
    return bar + (UH * (want.abs() + bar)).clamp(min=2.0 ** -25)


def fwd_bar(t, beta, res, want, half):
    b = 8 * U * (t.abs() + beta.abs() + (res.abs() if res is not None else 0.0))
    return half_stored(want, b) if half else b


def _undecided(z, res, ch, p, half):
    """-> (plain undecidable, with-residual undecidable) for elements z / res of channels ch (None: z, res are [..][C])."""
    mu, iv, ga, be = (v.double() if ch is None else v.double()[ch] for v in p)
    t = (z.double() - mu) * iv * ga
    yl = t + be
    bad_z = yl.abs() <= DECIDE * fwd_bar(t, be, None, yl, half)
    if res is None:
        return bad_z, None
    yr = yl + res.double()
    return bad_z, yr.abs() <= DECIDE * fwd_bar(t, be, res.double(), yr, half)


class Case:
    pass


def _draw_z(n, ch, k, g):
    return torch.randn(n, generator=g) * k.sc[ch] + k.off[ch]


def make_case(row):
    """The inputs of a gen / pos / small row, as the kernels receive them (stored type; fp32 parameter vectors)."""
    g = torch.Generator().manual_seed(_seed(row.id))
    r, c, half = row.r, row.c, row.half
    k = Case()
    k.row, k.half = row, half
    k.sc = torch.exp2(torch.rand(c, generator=g) * 2 - 1)
    if row.kind == "pos":
        k.off = k.sc * (30.0 if half else 100.0) * torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    else:
        k.off = torch.randn(c, generator=g) * 0.5 * k.sc
    k.z = _st(torch.randn(r, c, generator=g) * k.sc + k.off, half)
    m, _, iv = stats64(k.z)
    k.mean, k.invstd = m.float(), iv.float()
    k.gamma, k.beta = _params(c, g)
    k.res = _st(torch.randn(r, c, generator=g), half)
    k.dy = _st(torch.randn(r, c, generator=g) * torch.exp2(torch.rand(c, generator=g) * 2 - 1), half)
    k.rm0, k.rv0 = torch.randn(c, generator=g) * 0.5, torch.rand(c, generator=g) + 0.5
    p = (k.mean, k.invstd, k.gamma, k.beta)
    zf, rf = k.z.view(-1), k.res.view(-1)
    idx = None                                                   # None: every element; then only the redrawn ones
    for _ in range(64):
        if idx is None:
            bz, br = _undecided(k.z, k.res, None, p, half)
            iz, ir = bz.view(-1).nonzero().flatten(), (br & ~bz).view(-1).nonzero().flatten()
        else:
            bz, br = _undecided(zf[idx], rf[idx], idx % c, p, half)
            iz, ir = idx[bz], idx[br & ~bz]
        if iz.numel() + ir.numel() == 0:
            break
        zf[iz] = _st(_draw_z(iz.numel(), iz % c, k, g), half)
        rf[ir] = _st(torch.randn(ir.numel(), generator=g), half)
        idx = torch.cat([iz, ir])
    else:
        raise AssertionError(f"{row.id}: undecidable elements left after 64 redraws")
    return k


def undecidable_share(k):
    """Share of elements of a case whose ReLU sign (plain or with the residual) the float64 reference cannot decide."""
    bz, br = _undecided(k.z, k.res, None, (k.mean, k.invstd, k.gamma, k.beta), k.half)
    return float((bz | br).double().mean())


def sums_case(row):
    """z of the 236 MB row (bn_stats and the plain column sums share it) and its float64 column sums, once."""
    g = torch.Generator().manual_seed(_seed(row.id))
    k = Case()
    k.row, k.half = row, False
    sc = torch.exp2(torch.rand(row.c, generator=g) * 2 - 1)
    k.z = torch.randn(row.r, row.c, generator=g)
    k.z.mul_(sc).add_(torch.randn(row.c, generator=g) * 0.5)
    k.rm0, k.rv0 = torch.randn(row.c, generator=g) * 0.5, torch.rand(row.c, generator=g) + 0.5
    return k


def tiny_case(row):
    g = torch.Generator().manual_seed(_seed(row.id))
    return torch.randn(row.r, row.c, generator=g) * torch.exp2(torch.rand(row.c, generator=g) * 4 - 2)


# ---- float64 references (vectorised) ----
class Ref:
    """Everything the entries of a gen / pos / small case are compared with, in float64 from the stored inputs."""

    def __init__(self, k):
        d = lambda t: t.double()
        self.k, self.R = k, k.z.shape[0]
        mu, iv, ga, be = d(k.mean), d(k.invstd), d(k.gamma), d(k.beta)
        self.xh = (d(k.z) - mu) * iv
        self.t = self.xh * ga
        self.yl = self.t + be
        self.yr = self.yl + d(k.res)
        self.gi = ga * iv

    def fwd(self, res, relu):
        y = self.yr if res else self.yl
        want = y.clamp(min=0) if relu else y
        return want, fwd_bar(self.t, self.k.beta.double(), self.k.res.double() if res else None, want, self.k.half)

    def reduce(self, g):
        """dbeta, its bar, dgamma, its bar for the masked gradient g (float64 [R][C])."""
        gx = g * self.xh
        db, dg = g.sum(0), gx.sum(0)
        return db, U * db.abs() + 2 * U * g.abs().max(0).values, dg, U * dg.abs() + 4 * U * gx.abs().sum(0)

    def bwd(self, g, dbeta, dgamma, eval_mode, extra=None):
        """dz and its bar from the masked gradient and the fp32 dbeta / dgamma vectors the kernel receives."""
        if eval_mode:
            want, mag = g * self.gi, g.abs()
        else:
            t2, t3 = dbeta.double() / self.R, self.xh * dgamma.double() / self.R
            want, mag = self.gi * (g - t2 - t3), g.abs() + t2.abs() + t3.abs()
        bar = 8 * U * self.gi.abs() * mag
        if extra is not None:
            bar = bar + self.gi.abs() * extra
        return want, half_stored(want, bar) if self.k.half else bar


def stats_ref(k, momentum):
    """mean, invstd and the updated running statistics (None without) in float64; momentum as the float the kernel receives."""
    if not hasattr(k, "stats"):
        k.stats = stats64(k.z)                                   # once per case
    (m, var, iv), rm0, rv0 = k.stats, k.rm0, k.rv0
    rows = k.z.shape[0]
    if momentum is None:
        return m, iv, None, None
    mom = float(torch.tensor(momentum, dtype=torch.float32))
    unb = var * rows / (rows - 1) if rows > 1 else var
    return m, iv, (1.0 - mom) * rm0.double() + mom * m, (1.0 - mom) * rv0.double() + mom * unb


def mask_bytes(pos):
    """[R][C] bool -> the nibble mask [R][C / 4] uint8: bit k of byte q = channel 4 q + k.  A half lane's uint16 word (bits 0-3 and
    8-11 for its eight channels) is, in memory, two such bytes."""
    q = pos.reshape(pos.shape[0], -1, 4).to(torch.uint8)
    return q[..., 0] | (q[..., 1] << 1) | (q[..., 2] << 2) | (q[..., 3] << 3)


def mask_bits(mask, c):
    """The inverse: bytes -> [R][C] float64 of 0 / 1."""
    m = mask.reshape(-1, c // 4, 1).to(torch.int32)
    return ((m >> torch.arange(4, dtype=torch.int32)) & 1).reshape(-1, c).double()


# ---- the stem forms ----
def _windows(y):
    """[N][H][W][C] -> the 3 x 3 / stride 2 / pad 1 windows [N][C][9][Ho Wo], -inf outside the map."""
    n, h, w, c = y.shape
    p = F.pad(y.permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
    return F.unfold(p, kernel_size=3, stride=2).reshape(n, c, 9, -1)


def _stem_bad(k):
    """-> (sign-undecidable pixels [N][H][W][C], flat z index of the winner of every undecidable window)."""
    p = (k.mean, k.invstd, k.gamma, k.beta)
    n, h, w, c = k.z.shape
    bz, _ = _undecided(k.z, None, None, p, k.half)
    mu, iv, ga, be = (v.double() for v in p)
    t = (k.z.double() - mu) * iv * ga
    y = (t + be).clamp(min=0)
    bar = fwd_bar(t, be, None, y, k.half)
    wy, wb = _windows(y), _windows(bar)
    top, arg = wy.topk(2, dim=2)
    gap_bar = DECIDE * wb.gather(2, arg[:, :, :1]).squeeze(2)
    second = torch.where(torch.isinf(top[:, :, 1]), torch.full_like(top[:, :, 1], -1.0), top[:, :, 1])      # a 1 x 1 map: no rival
    bad_w = ((top[:, :, 0] - second) <= gap_bar) & ~((top[:, :, 0] == 0) & (second == 0))
    flat = _windows(torch.arange(n * h * w * c, dtype=torch.float64).reshape(n, h, w, c))
    win = flat.gather(2, arg[:, :, :1]).squeeze(2)[bad_w].long()
    return bz.reshape(n, h, w, c), win


def make_stem_case(n, h, w, half):
    c = STEM_C
    rid = f"stem_{n}x{h}x{w}_{'f16' if half else 'f32'}"
    g = torch.Generator().manual_seed(_seed(rid))
    k = Case()
    k.id, k.half, k.shape = rid, half, (n, h, w, c)
    k.sc = torch.exp2(torch.rand(c, generator=g) * 2 - 1)
    k.off = torch.randn(c, generator=g) * 0.5 * k.sc
    k.z = _st(torch.randn(n, h, w, c, generator=g) * k.sc + k.off, half)
    m, _, iv = stats64(k.z)
    k.mean, k.invstd = m.float(), iv.float()
    k.gamma, k.beta = _params(c, g)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    k.dpool = _st(torch.randn(n, ho, wo, c, generator=g) * torch.exp2(torch.rand(c, generator=g) * 2 - 1), half)
    zf = k.z.view(-1)
    for _ in range(200):
        bz, win = _stem_bad(k)
        i = torch.unique(torch.cat([bz.reshape(-1).nonzero().flatten(), win]))
        if i.numel() == 0:
            break
        zf[i] = _st(_draw_z(i.numel(), i % c, k, g), half)
    else:
        raise AssertionError(f"{rid}: undecidable signs or windows left after 200 redraws")
    return k


def stem_undecidable(k):
    bz, win = _stem_bad(k)
    return int(bz.sum()) + int(win.numel())


class StemRef:
    """float64 max_pool2d over the float64 BatchNorm + ReLU, and its autograd."""

    def __init__(self, k):
        n, h, w, c = k.shape
        mu, iv, ga, be = (v.double() for v in (k.mean, k.invstd, k.gamma, k.beta))
        self.k, self.R = k, n * h * w
        self.xh = (k.z.double() - mu) * iv
        self.t = self.xh * ga
        self.gi = ga * iv
        yl = (self.t + be).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        act = yl.clamp(min=0)
        pooled, ind = F.max_pool2d(act, 3, 2, 1, return_indices=True)
        self.pooled = pooled.detach().permute(0, 2, 3, 1).contiguous()
        ind = ind.permute(0, 2, 3, 1)                                           # [N][Ho][Wo][C] of y * W + x
        ho, wo = ind.shape[1:3]
        oy, ox = torch.arange(ho).view(1, ho, 1, 1), torch.arange(wo).view(1, 1, wo, 1)
        wy, wx = ind // w, ind % w
        self.slot = ((wy - (2 * oy - 1)) * 3 + (wx - (2 * ox - 1))).to(torch.uint8).contiguous()
        nn_, cc = torch.arange(n).view(n, 1, 1, 1), torch.arange(c).view(1, 1, 1, c)
        self.zwin = k.z[nn_, wy, wx, cc].contiguous()                          # the raw z of every winner, as stored
        self.pool_bar = fwd_bar(self.t, be, None, (self.t + be).clamp(min=0), k.half)[nn_, wy, wx, cc]
        dp = k.dpool.double().permute(0, 3, 1, 2)
        (g,) = torch.autograd.grad(pooled, yl, dp, retain_graph=True)           # through the pool AND the ReLU
        self.g = g.permute(0, 2, 3, 1).contiguous()
        # what the fp32 sum of several pooled gradients at one pixel can lose: 3 u x their magnitudes, where there are several
        (a,) = torch.autograd.grad(pooled, act, dp.abs(), retain_graph=True)
        (cnt,) = torch.autograd.grad(pooled, act, torch.ones_like(dp))
        self.a = (3 * U * a * (cnt > 1) * (act.detach() > 0)).permute(0, 2, 3, 1).contiguous()
        # over the pooled cells (the winners form): g = dpool where the winner's activation is positive
        self.g_win = k.dpool.double() * (self.pooled > 0)
        self.xh_win = (self.zwin.double() - mu) * iv

    def reduce(self, pooled_form):
        g, xh = (self.g_win, self.xh_win) if pooled_form else (self.g, self.xh)
        c = g.shape[-1]
        g, xh = g.reshape(-1, c), xh.reshape(-1, c)
        lost = torch.zeros_like(g) if pooled_form else self.a.reshape(-1, c)
        gx = g * xh
        db, dg = g.sum(0), gx.sum(0)
        return (db, U * db.abs() + 2 * U * g.abs().max(0).values + lost.sum(0),
                dg, U * dg.abs() + 4 * U * gx.abs().sum(0) + (lost * xh.abs()).sum(0))

    def bwd(self, dbeta, dgamma):
        t2, t3 = dbeta.double() / self.R, self.xh * dgamma.double() / self.R
        want = self.gi * (self.g - t2 - t3)
        bar = self.gi.abs() * (8 * U * (self.g.abs() + t2.abs() + t3.abs()) + self.a)
        return want, half_stored(want, bar) if self.k.half else bar


# ---- buffers between guards ----
class Arena:
    """Every tensor of a launch is a view in the middle of an allocation of its own: [guard | tensor | guard], all bytes 0xff -- NaN as
    a half, a float or a double, a value no mask byte, mask word or winner slot can take.  Outputs start poisoned: afterwards no
    element may be left so and the guards must be bit-unchanged.  Inputs (checked once per row) must come back bit-unchanged, guards
    included; a read outside one meets NaN and shows in the result."""

    def __init__(self, dev):
        self.dev, self.ins, self.outs = dev, [], []

    def _big(self, nbytes):
        return torch.full((nbytes + 2 * GUARD_BYTES,), 255, dtype=torch.uint8, device=self.dev)

    def inp(self, name, t, mutable=False, lead=0):
        """lead: the view starts `lead` bytes further into its allocation (a tensor that is not 16-byte aligned); those bytes are guard."""
        if t is None:
            return None
        t = t.contiguous()
        nb = t.numel() * t.element_size()
        big = self._big(nb + lead)
        view = big[GUARD_BYTES + lead:GUARD_BYTES + lead + nb].view(t.dtype).view(t.shape)
        view.copy_(t)
        (self.outs if mutable else self.ins).append((name, big, big.clone() if not mutable else None, nb, t.dtype, True, lead))
        return view

    def out(self, name, shape, dtype, all_written=True, lead=0):
        n = 1
        for s in shape:
            n *= s
        nb = n * torch.empty((), dtype=dtype).element_size()
        big = self._big(nb + lead)
        self.outs.append((name, big, None, nb, dtype, all_written, lead))
        return big[GUARD_BYTES + lead:GUARD_BYTES + lead + nb].view(dtype).view(shape)

    def check_outputs(self, rid):
        torch.cuda.synchronize()
        for name, big, _, nb, dtype, all_written, lead in self.outs:
            front = GUARD_BYTES + lead
            assert bool((big[:front] == 255).all()), f"{rid}: the launch wrote in front of `{name}`"
            assert bool((big[front + nb:] == 255).all()), f"{rid}: the launch wrote past the end of `{name}`"
            if not all_written:
                continue
            body = big[front:front + nb].view(dtype)
            left = int((body == 255).sum()) if dtype == torch.uint8 else int(torch.isnan(body).sum())
            assert left == 0, f"{rid}: {left} elements of `{name}` left unwritten or NaN"

    def check_inputs(self, rid):
        torch.cuda.synchronize()
        for name, big, snap, _, _, _, _ in self.ins:
            assert torch.equal(big, snap), f"{rid}: input `{name}` or its guards were written"


# ---- comparisons ----
WORST = {}


def within(rid, kind, got, want, bar, worst_of=None):
    """Prints the worst error / bar of one output, then asserts every element within its bar.  worst_of: the dict that keeps the worst
    ratio per kind (default: this table's WORST)."""
    got = got.detach().cpu().double().reshape(want.shape)
    assert bool(torch.isfinite(got).all()), f"{rid}: non-finite values in the output"
    err = (got - want).abs()
    ratio = torch.where(bar > 0, err / bar.clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    worst = float(ratio.max())
    worst_of = WORST if worst_of is None else worst_of
    worst_of[kind] = max(worst_of.get(kind, 0.0), worst)
    print(f"   {rid}: worst err / bar {worst:.3f}", flush=True)
    if worst > 1.0:
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{rid}: {int((ratio > 1).sum())} of {ratio.numel()} elements outside the bar, worst at flat index {i}: got "
                             f"{got.reshape(-1)[i].item():.9g}, want {want.reshape(-1)[i].item():.9g}, bar {bar.reshape(-1)[i].item():.3e}")


def print_worst(worst_of=None):
    for kind, v in sorted((WORST if worst_of is None else worst_of).items()):
        print(f"worst {kind}: err / bar {v:.3f}", flush=True)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def twice(rid, launch):
    """Runs launch() -> {name: output tensor} twice, each into fresh poisoned buffers: bit-identical; -> the first."""
    a, b = launch(), launch()
    for nm in a:
        if a[nm] is not None:
            assert torch.equal(_bits(a[nm]), _bits(b[nm])), f"{rid}: two launches differ in `{nm}`"
    return a


def _lib():
    for q in (ROOT, PKG):
        if q not in sys.path:
            sys.path.insert(0, q)
    from self_supervised import _hip
    return _hip, _hip.lib(), _hip.stream()


def _p(t):
    return None if t is None else t.data_ptr()


def _tdt(half):
    return torch.float16 if half else torch.float32


def _ws(ar, r, c, lib):
    """The reduction workspace: EXACTLY ssad_colreduce_workspace(R, C) doubles between guards (only nblk rows of it are written)."""
    return ar.out("workspace", (lib.ssad_colreduce_workspace(r, c),), torch.float64, all_written=False)


def _stats_entries(rid, k, zd, dev, sfx):
    hip, lib, st = _lib()
    r, c = k.z.shape
    fn = getattr(lib, "ssad_bn_stats" + sfx)
    for mom in (None,) + MOMENTA:
        eid = f"{rid}[bn_stats{'' if mom is None else f' momentum {mom}'}]"

        def launch():
            ar = Arena(dev)
            o = {"mean": ar.out("mean", (c,), torch.float32), "invstd": ar.out("invstd", (c,), torch.float32),
                 "rm": None if mom is None else ar.inp("running_mean", k.rm0, mutable=True),
                 "rv": None if mom is None else ar.inp("running_var", k.rv0, mutable=True)}
            hip.check(fn(_p(zd), r, c, EPS, mom or 0.0, _p(o["mean"]), _p(o["invstd"]), _p(o["rm"]), _p(o["rv"]), _p(_ws(ar, r, c, lib)), st))
            ar.check_outputs(eid)
            return o
        o = twice(eid, launch)
        m, iv, rm, rv = stats_ref(k, mom)
        for nm, want in (("mean", m), ("invstd", iv), ("rm", rm), ("rv", rv)):
            if want is not None:
                within(f"{eid} {nm}", "stats", o[nm], want, 4 * U * want.abs())


def run_general_row(row, dev):
    hip, lib, st = _lib()
    k = sums_case(row) if row.kind == "sums" else make_case(row)
    r, c, half = row.r, row.c, row.half
    sfx, tdt = ("_h" if half else ""), _tdt(half)
    rid = row.id
    ia = Arena(dev)
    zd = ia.inp("z", k.z)
    _stats_entries(rid, k, zd, dev, sfx)
    red = getattr(lib, "ssad_bn_bwd_reduce" + sfx)

    def reduce_launch(eid, call, want_dgamma):
        def launch():
            ar = Arena(dev)
            o = {"dbeta": ar.out("dbeta", (c,), torch.float32), "dgamma": ar.out("dgamma", (c,), torch.float32) if want_dgamma else None}
            hip.check(call(o, _p(_ws(ar, r, c, lib))))
            ar.check_outputs(eid)
            return o
        return twice(eid, launch)

    if row.kind == "sums":
        o = reduce_launch(f"{rid}[plain column sums]", lambda o, ws: red(_p(zd), None, None, None, None, _p(o["dbeta"]), None, r, c, ws, st), False)
        z64 = k.z.double()
        want = z64.sum(0)
        within(f"{rid}[plain column sums]", "dbeta", o["dbeta"], want, U * want.abs() + 2 * U * z64.abs().max(0).values)
        ia.check_inputs(rid)
        return
    ref = Ref(k)
    vec = {nm: ia.inp(nm, getattr(k, nm)) for nm in ("mean", "invstd", "gamma", "beta")}
    resd, dyd = ia.inp("residual", k.res), ia.inp("dy", k.dy)
    V = [_p(vec[nm]) for nm in ("mean", "invstd", "gamma", "beta")]
    # --- apply forward, plain and with the mask ---
    fwd, fwdm = getattr(lib, "ssad_bn_apply_fwd" + sfx), getattr(lib, "ssad_bn_apply_fwd_mask" + sfx)
    for with_mask in (False, True):
        for res in (False, True):
            for relu in (False, True):
                eid = f"{rid}[bn_apply_fwd{'_mask' if with_mask else ''}{' +residual' if res else ''}{' +relu' if relu else ''}]"

                def launch():
                    ar = Arena(dev)
                    o = {"y": ar.out("y", (r, c), tdt), "mask": ar.out("mask", (r, c // 4), torch.uint8) if with_mask else None}
                    if with_mask:
                        hip.check(fwdm(_p(zd), *V, _p(resd) if res else None, _p(o["y"]), _p(o["mask"]), r, c, int(relu), st))
                    else:
                        hip.check(fwd(_p(zd), *V, _p(resd) if res else None, _p(o["y"]), r, c, int(relu), st))
                    ar.check_outputs(eid)
                    return o
                o = twice(eid, launch)
                want, bar = ref.fwd(res, relu)
                within(eid, "apply_fwd", o["y"], want, bar)
                if with_mask:
                    got = o["mask"].cpu()
                    assert torch.equal(got, mask_bytes(o["y"].cpu().float() > 0)), f"{eid}: the mask is not (y > 0) of the stored output"
                    assert torch.equal(got, mask_bytes((ref.yr if res else ref.yl) > 0)), f"{eid}: mask bits differ from the float64 signs"
    # --- backward reductions ---
    yact = _st(ref.yr.clamp(min=0), half)                       # the saved activation of the +residual +relu form
    maskb = mask_bytes(ref.yr > 0)
    yad, mkd = ia.inp("yact", yact), ia.inp("mask", maskb)
    dy64 = k.dy.double()
    g_act, g_z, g_m = dy64 * (yact.double() > 0), dy64 * (ref.yl > 0), dy64 * mask_bits(maskb, c)
    assert torch.equal(g_act, g_m)
    MU, IV, GA, BE = V
    sums = {}
    forms = [("saved activation", g_act, True, lambda o, ws: red(_p(dyd), _p(yad), _p(zd), MU, IV, _p(o["dbeta"]), _p(o["dgamma"]), r, c, ws, st)),
             ("plain column sums", dy64, False, lambda o, ws: red(_p(dyd), None, None, None, None, _p(o["dbeta"]), None, r, c, ws, st)),
             ("dbeta only", g_act, False, lambda o, ws: red(_p(dyd), _p(yad), None, None, None, _p(o["dbeta"]), None, r, c, ws, st)),
             ("zmask", g_z, True, lambda o, ws: getattr(lib, "ssad_bn_bwd_reduce_zmask" + sfx)(
                 _p(dyd), _p(zd), MU, IV, GA, BE, _p(o["dbeta"]), _p(o["dgamma"]), r, c, ws, st)),
             ("mask", g_m, True, lambda o, ws: getattr(lib, "ssad_bn_bwd_reduce_mask" + sfx)(
                 _p(dyd), _p(mkd), _p(zd), MU, IV, _p(o["dbeta"]), _p(o["dgamma"]), r, c, ws, st))]
    for name, g, with_dg, call in forms:
        eid = f"{rid}[bn_bwd_reduce {name}]"
        o = reduce_launch(eid, call, with_dg)
        db, db_bar, dg, dg_bar = ref.reduce(g)
        within(f"{eid} dbeta", "dbeta", o["dbeta"], db, db_bar)
        if with_dg:
            within(f"{eid} dgamma", "dgamma", o["dgamma"], dg, dg_bar)
        sums[name] = (o["dbeta"], o["dgamma"])
    # --- apply backward: dbeta / dgamma are the fp32 vectors of the matching reduction above (already checked) ---
    bwd = getattr(lib, "ssad_bn_apply_bwd" + sfx)
    db_a, dg_a = sums["saved activation"]
    for eval_mode in (False, True):
        for with_dres in (False, True):
            eid = f"{rid}[bn_apply_bwd {'eval' if eval_mode else 'train'}{' +dres' if with_dres else ''}]"

            def launch():
                ar = Arena(dev)
                o = {"dz": ar.out("dz", (r, c), tdt), "dres": ar.out("dres", (r, c), tdt) if with_dres else None}
                hip.check(bwd(_p(dyd), _p(yad), _p(zd), MU, IV, GA, _p(db_a), _p(dg_a), _p(o["dz"]), _p(o["dres"]), r, c, int(eval_mode), st))
                ar.check_outputs(eid)
                return o
            o = twice(eid, launch)
            want, bar = ref.bwd(g_act, db_a.cpu(), dg_a.cpu(), eval_mode)
            within(eid, "apply_bwd", o["dz"], want, bar)
            if with_dres:
                masked = torch.where(yact.float() > 0, k.dy, torch.zeros_like(k.dy))
                assert torch.equal(_bits(o["dres"].cpu()), _bits(masked)), f"{eid}: dres is not the masked dy bit for bit"
    for name, g, fn_name, extra in (("zmask", g_z, "ssad_bn_apply_bwd_zmask", (BE,)), ("mask", g_m, "ssad_bn_apply_bwd_mask", ())):
        eid = f"{rid}[bn_apply_bwd_{name}]"
        db_v, dg_v = sums[name]
        fn = getattr(lib, fn_name + sfx)

        def launch():
            ar = Arena(dev)
            o = {"dz": ar.out("dz", (r, c), tdt)}
            if name == "zmask":
                hip.check(fn(_p(dyd), _p(zd), MU, IV, GA, BE, _p(db_v), _p(dg_v), _p(o["dz"]), r, c, st))
            else:
                hip.check(fn(_p(dyd), _p(mkd), _p(zd), MU, IV, GA, _p(db_v), _p(dg_v), _p(o["dz"]), r, c, st))
            ar.check_outputs(eid)
            return o
        o = twice(eid, launch)
        want, bar = ref.bwd(g, db_v.cpu(), dg_v.cpu(), False)
        within(eid, "apply_bwd", o["dz"], want, bar)
    ia.check_inputs(rid)


def run_tiny_row(row, dev):
    hip, lib, st = _lib()
    a = tiny_case(row)
    r, c = row.r, row.c
    ia = Arena(dev)
    ad = ia.inp("a", a)
    eid = f"{row.id}[plain column sums]"

    def launch():
        ar = Arena(dev)
        o = {"sums": ar.out("sums", (c,), torch.float32)}
        hip.check(lib.ssad_bn_bwd_reduce(_p(ad), None, None, None, None, _p(o["sums"]), None, r, c, _p(_ws(ar, r, c, lib)), st))
        ar.check_outputs(eid)
        return o
    o = twice(eid, launch)
    want = a.double().sum(0)
    within(eid, "dbeta", o["sums"], want, U * want.abs() + 2 * U * a.double().abs().max(0).values)
    ia.check_inputs(row.id)


def run_small_row(row, dev):
    """ssad_bn_small_fwd / _bwd.  Their apply halves use the kernel's OWN fp32 statistics / sums, which are outputs: those are held to
    their bars first, and the apply is then compared with float64 over exactly those fp32 vectors."""
    hip, lib, st = _lib()
    k = make_case(row)
    r, c = row.r, row.c
    assert lib.ssad_bn_small_ok(r, c) == 1, f"{row.id}: ssad_bn_small_ok refuses the row"
    ia = Arena(dev)
    zd, dyd = ia.inp("z", k.z), ia.inp("dy", k.dy)
    vec = {nm: ia.inp(nm, getattr(k, nm)) for nm in ("mean", "invstd", "gamma", "beta")}
    for relu, mom in ((False, None), (True, 0.1), (False, 0.3)):
        eid = f"{row.id}[bn_small_fwd{' +relu' if relu else ''}{'' if mom is None else f' momentum {mom}'}]"

        def launch():
            ar = Arena(dev)
            o = {"y": ar.out("y", (r, c), torch.float32), "mean": ar.out("mean", (c,), torch.float32), "invstd": ar.out("invstd", (c,), torch.float32),
                 "rm": None if mom is None else ar.inp("running_mean", k.rm0, mutable=True),
                 "rv": None if mom is None else ar.inp("running_var", k.rv0, mutable=True)}
            hip.check(lib.ssad_bn_small_fwd(_p(zd), _p(vec["gamma"]), _p(vec["beta"]), _p(o["y"]), _p(o["mean"]), _p(o["invstd"]), _p(o["rm"]),
                                            _p(o["rv"]), r, c, EPS, mom or 0.0, int(relu), st))
            ar.check_outputs(eid)
            return o
        o = twice(eid, launch)
        m, iv, rm, rv = stats_ref(k, mom)
        for nm, want in (("mean", m), ("invstd", iv), ("rm", rm), ("rv", rv)):
            if want is not None:
                within(f"{eid} {nm}", "stats", o[nm], want, 4 * U * want.abs())
        k2 = Case()
        k2.__dict__.update(k.__dict__)
        k2.mean, k2.invstd = o["mean"].cpu(), o["invstd"].cpu()
        want, bar = Ref(k2).fwd(False, relu)
        within(f"{eid} y", "apply_fwd", o["y"], want, bar)
    ref = Ref(k)
    dy64 = k.dy.double()
    for zmask, with_dbias in ((False, True), (True, False), (True, True)):
        eid = f"{row.id}[bn_small_bwd{' zmask' if zmask else ''}{' +dbias' if with_dbias else ''}]"

        def launch():
            ar = Arena(dev)
            o = {"dbeta": ar.out("dbeta", (c,), torch.float32), "dgamma": ar.out("dgamma", (c,), torch.float32),
                 "dbias": ar.out("dbias", (c,), torch.float32) if with_dbias else None, "dz": ar.out("dz", (r, c), torch.float32)}
            hip.check(lib.ssad_bn_small_bwd(_p(dyd), _p(zd), _p(vec["mean"]), _p(vec["invstd"]), _p(vec["gamma"]), _p(vec["beta"]) if zmask else None,
                                            _p(o["dbeta"]), _p(o["dgamma"]), _p(o["dbias"]), _p(o["dz"]), r, c, st))
            ar.check_outputs(eid)
            return o
        o = twice(eid, launch)
        g = dy64 * (ref.yl > 0) if zmask else dy64
        db, db_bar, dg, dg_bar = ref.reduce(g)
        within(f"{eid} dbeta", "dbeta", o["dbeta"], db, db_bar)
        within(f"{eid} dgamma", "dgamma", o["dgamma"], dg, dg_bar)
        want, bar = ref.bwd(g, o["dbeta"].cpu(), o["dgamma"].cpu(), False)
        within(f"{eid} dz", "apply_bwd", o["dz"], want, bar)
        if with_dbias:
            dz64 = o["dz"].cpu().double()
            want = dz64.sum(0)
            within(f"{eid} dbias", "dbeta", o["dbias"], want, U * want.abs() + 2 * U * dz64.abs().max(0).values)
    ia.check_inputs(row.id)


def run_stem_case(n, h, w, half, dev):
    hip, lib, st = _lib()
    k = make_stem_case(n, h, w, half)
    ref = StemRef(k)
    c, rid, tdt, sfx = STEM_C, k.id, _tdt(half), ("_h" if half else "")
    ho, wo = ref.slot.shape[1:3]
    ia = Arena(dev)
    zd, dpd = ia.inp("z", k.z), ia.inp("dpool", k.dpool)
    V = [_p(ia.inp(nm, getattr(k, nm))) for nm in ("mean", "invstd", "gamma", "beta")]
    slotd, zwd = ia.inp("winner slots", ref.slot), ia.inp("zwin", ref.zwin)
    for winners in (False, True):
        eid = f"{rid}[bn_relu_maxpool_fwd{' +winners' if winners else ''}]"

        def launch():
            ar = Arena(dev)
            o = {"out": ar.out("pooled", (n, ho, wo, c), tdt), "idx": ar.out("slots", (n, ho, wo, c), torch.uint8),
                 "zwin": ar.out("zwin", (n, ho, wo, c), tdt) if winners else None}
            if winners:
                hip.check(getattr(lib, "ssad_bn_relu_maxpool_fwd_win" + sfx)(_p(zd), *V, _p(o["out"]), _p(o["idx"]), _p(o["zwin"]), n, h, w, c, st))
            else:
                hip.check(getattr(lib, "ssad_bn_relu_maxpool_fwd" + sfx)(_p(zd), *V, _p(o["out"]), _p(o["idx"]), n, h, w, c, st))
            ar.check_outputs(eid)
            return o
        o = twice(eid, launch)
        within(eid, "pool_fwd", o["out"], ref.pooled, ref.pool_bar)
        assert torch.equal(o["idx"].cpu(), ref.slot), f"{eid}: winner slots differ from max_pool2d's"
        if winners:
            assert torch.equal(_bits(o["zwin"].cpu()), _bits(ref.zwin)), f"{eid}: the raw winners are not z at max_pool2d's winners"
    for pooled_form in (False, True):
        eid = f"{rid}[pool_bn_relu_bwd{' +zwin' if pooled_form else ''}]"

        def launch():
            ar = Arena(dev)
            o = {"dbeta": ar.out("dbeta", (c,), torch.float32), "dgamma": ar.out("dgamma", (c,), torch.float32),
                 "dz": ar.out("dz", (n, h, w, c), tdt)}
            if pooled_form:
                rp = n * ho * wo
                hip.check(getattr(lib, "ssad_bn_bwd_reduce_zmask" + sfx)(_p(dpd), _p(zwd), *V, _p(o["dbeta"]), _p(o["dgamma"]), rp, c,
                                                                        _p(_ws(ar, rp, c, lib)), st))
                hip.check(getattr(lib, "ssad_pool_bn_relu_bwd_apply" + sfx)(_p(slotd), _p(dpd), _p(zd), *V, _p(o["dbeta"]), _p(o["dgamma"]),
                                                                           _p(o["dz"]), n, h, w, c, k.dpool.numel(), st))
            else:
                hip.check(getattr(lib, "ssad_pool_bn_relu_bwd" + sfx)(_p(slotd), _p(dpd), _p(zd), *V, _p(o["dbeta"]), _p(o["dgamma"]), _p(o["dz"]),
                                                                     n, h, w, c, k.dpool.numel(), _p(_ws(ar, n * h * w, c, lib)), st))
            ar.check_outputs(eid)
            return o
        o = twice(eid, launch)
        db, db_bar, dg, dg_bar = ref.reduce(pooled_form)
        within(f"{eid} dbeta", "dbeta", o["dbeta"], db, db_bar)
        within(f"{eid} dgamma", "dgamma", o["dgamma"], dg, dg_bar)
        want, bar = ref.bwd(o["dbeta"].cpu(), o["dgamma"].cpu())
        within(f"{eid} dz", "pool_bwd", o["dz"], want, bar)
    ia.check_inputs(rid)


def run_row(row, dev):
    if row.kind == "tiny":
        return run_tiny_row(row, dev)
    if row.kind == "small":
        return run_small_row(row, dev)
    return run_general_row(row, dev)
