"""The stem forward table: every kernel of csrc/stem.hip and csrc/stem16.hip -- stem_conv7x7_kernel, stem_patch_fused_kernel,
stem_patch_border_kernel, stem_conv7x7_16_kernel and the five weight packers -- at the smallest shapes that reach each loader form, each
epilogue form and the several-tile / several-window walk of the four persistent kernels, every written element compared with float64
torch on the CPU, over buffers that sit between guards and start out poisoned.

Shared by tests/test_stem_table.py (geometry, coverage and the sensitivity of the inputs; no GPU) and tests/test_hip_stem_paths.py
(the kernels).

Row: (id, entry, geometry, forms, claims, reason, launch).
  entry  stem   ssad_stem_fwd / ssad_stem_fwd_stats (fp32).  geometry (B, H, W, patch_dim, patch_stride, rs); rs = 1: resize_to = (2 H, 2 W)
         patch  ssad_stem_patch_pool_fwd_ring / ssad_stem_patch_border_fwd.  geometry (B, H, W, patch_stride): 32 x 32 windows
         s16    ssad_stem_fwd_stats16 / ssad_stem_fwd_stats16_h.  geometry (B, H, W)
  forms, joined by "+", each a launch (or a group of launches) of its own --
     stem:  A  scale, shift, ReLU, NHWC        Ap  the same, position-major [Ho][Wo][N][64]
            R  raw: NULL scale and shift, relu = 0 (negative values pass)        Rp  raw, position-major
            C  scale only: NULL shift, relu = 0, NHWC                             Cp  scale only, position-major
            S  raw + statistics (ssad_stem_fwd_stats): z bit-equal to R; mean, invstd, the running statistics from non-trivial values;
               and once more with NULL running pointers
     patch: full / fullp  the whole 16 x 16 map, NHWC / position-major;  rLO_HI / rLO_HIp  the ring form skipping LO <= py, px <= HI;
            border  ssad_stem_patch_border_fwd (position-major only);  a row whose id ends in _null passes NULL scale and shift
     s16:   f16 / bf16  fp16 / bf16 operands, fp32 z;  f16h  fp16 operands, z stored as halves.  Each from the OIHW and from the OHWI
            filter (bit-equal), with running statistics and with NULL
  claims: what the row is the smallest shape for, as tags that tests/test_stem_table.py checks against geometry() -- see CLAIMS.
  launch: (N windows, Hv, Wv, Ho, Wo, tiles_y, tiles_x, total tiles, grid, the most tiles one workgroup walks), written out; for the
         patch kernels a tile is a window.  geometry() derives the same from the constants below, restated from the kernels' comments (the 8 x 32 output tile, 4096 persistent workgroups of the conv kernels,
         2048 of the patch kernels, the to-64 rule of models.py:217-219), not read back from the library.

Reference: float64 on the CPU from the same fp32 inputs.  Window and nearest resize by the integer rule the kernel documents, source index
= origin + floor(v * window / Hv); F.conv2d(stride 2, pad 3) in float64; scale, shift, ReLU; F.max_pool2d(3, 2, 1) where the kernel
pools.  16-bit rows: the fp16- / bf16-rounded image and filter, exact in float64.  Only the subtraction |got - want| runs on the device
(in float64, chunk by chunk); every written element is compared, on every row.

Inputs: images randn + a per-channel offset (0.6, 0.4, 0.5), a seed per geometry; filter randn / sqrt(147) + a per-channel mean of
magnitude 0.007 .. 0.02 with either sign -- a zero-mean image would cancel the filter's mean, so the offset is what makes the raw outputs'
|mean| / std of order 1 (printed by every statistics form); scale of magnitude 0.5 .. 1.5 with either sign; shift randn.

Bars (DESIGN s.2, TOL of tests/igemm_tile_table.py): every element within 2e-5 of the row's largest reference magnitude -- the fp32 stem,
the folded patch kernels (the group-summed filter is the same real number rounded differently) and the 16-bit-operand kernels (products
exact in fp32) alike.  out_half: the stored half within one spacing of halves at the float64 reference -- plus, see below, 4 x the
yardstick's absolute error.  Statistics (the bars of
tests/test_hip_training.py, its rel_err = max |err| / max |want|): mean 1e-5 absolute, invstd 1e-5, running statistics 1e-4 -- against
float64 statistics of the float64 reference (of the stored halves for out_half: the wrapper documents that).  The folded packer: float64
group sums within 4 * 2^-24 of the group's sum of magnitudes (three fp32 additions).

Measured on the MI355X (worst over the rows of a family, as a fraction of the row's largest reference magnitude; beside it the fp32-CPU
yardstick: the same reference computed in fp32 on the CPU against float64, over the first 64 samples of a row):
  family          err / max|want|   fp32-CPU yardstick   mean err    invstd err   running err
  stem fp32       6.35e-07          6.35e-07             9.70e-08    6.12e-08     4.39e-08
  folded patch    2.67e-07          5.64e-07             (0.013 of the 2e-5 bar: the group-summed filter costs nothing measurable)
  stem16 f16      2.30e-07          5.41e-07             1.16e-07    6.93e-08     4.25e-08
  stem16 bf16     2.61e-07          2.41e-07             9.33e-08    8.23e-08     4.03e-08
  stem16 f16h     (below)           5.41e-07             1.16e-07    1.41e-07     5.90e-08
  folded packer   1.15e-07 of the group's sum of magnitudes (bar 2.38e-07)
out_half: "within one spacing of halves of the float64 reference" cannot be met by a correct kernel.  The kernel rounds its fp32
accumulator, which carries the fp32 summation error of terms of order 1 (the yardstick: up to 5.4e-07 of max |want|, 3.6e-06 absolute),
while halves near zero are 6e-08 apart: where a sum cancels to |z| < 2^-10 that error alone is several spacings.  Measured: up to 5.89
spacings (at |z| of order 1e-4), on 1025 x 64 x 64; 5.6e-04 of the stored halves are not the correctly rounded half of the float64
value at all.  The f16h bar is therefore a spacing + HALF_MARGIN = 4 x the largest absolute error of the row's own fp32-CPU yardstick
(a different summation order of the same products; 4 covers the spread between orders) -- set from the yardstick, not from the kernel.
"""
import functools
import math

import torch
import torch.nn.functional as F

# ---- constants restated from the kernels' comments ----
TOH, TOW = 8, 32                    # output tile of stem_conv7x7_kernel and stem_conv7x7_16_kernel
CONV_GRID_CAP = 4096                # their persistent workgroups = rows of the statistics partials (ssad_stem_stats_rows)
PATCH_GRID_CAP = 2048               # persistent workgroups of stem_patch_fused_kernel and stem_patch_border_kernel
PATCH_WINDOW = 32                   # the patch kernels' window; exact 2x upsample to 64
TOL = 2e-5                          # TOL[""] of tests/igemm_tile_table.py
HALF_MARGIN = 4                     # out_half: a half spacing + HALF_MARGIN x the fp32-CPU yardstick's largest absolute error (docstring)
MEAN_TOL, INVSTD_TOL, RUNNING_TOL = 1e-5, 1e-5, 1e-4
EPS, MOMENTUM = 1e-5, 0.1
POISON = 1e30                       # float outputs (tests/scoring_trunk_table.py): finite, survives ReLU and any mask
RINGS = ((4, 12), (0, 15), (7, 7), (0, 0), (15, 15))
_ALL_PATCH = "full+fullp+" + "+".join(f"r{a}_{b}+r{a}_{b}p" for a, b in RINGS) + "+border"
_SMALL, _SMALL_S = "A+Ap+R+Rp", "A+Ap+R+Rp+S"

STEM = [
    ("img_1x64x64", "stem", (1, 64, 64, 0, 0, 0), _SMALL_S, "direct whole one_column",
     "one whole tile column, 4 tiles, one sample",
     (1, 64, 64, 32, 32, 4, 1, 4, 4, 1)),
    ("img_3x64x128", "stem", (3, 64, 128, 0, 0, 0), _SMALL_S + "+C+Cp", "direct whole two_columns",
     "Wo = 64: two whole tile columns",
     (3, 64, 128, 32, 64, 4, 2, 24, 24, 1)),
    ("img_2x70x74", "stem", (2, 70, 74, 0, 0, 0), _SMALL_S + "+C+Cp", "direct whole ragged odd_ho",
     "Ho = 35, Wo = 37: a whole and a ragged tile in the same row; Ho odd, a wave's second row is absent in the last tile",
     (2, 70, 74, 35, 37, 5, 2, 20, 20, 1)),
    ("img_2x65x97", "stem", (2, 65, 97, 0, 0, 0), _SMALL_S, "direct whole ragged single_last_row",
     "Ho = 33: the last tile row has a single output row",
     (2, 65, 97, 33, 49, 5, 2, 20, 20, 1)),
    ("img_1x101x77", "stem", (1, 101, 77, 0, 0, 0), _SMALL_S, "direct whole ragged odd_ho", "Wo = 39",
     (1, 101, 77, 51, 39, 7, 2, 14, 14, 1)),
    ("img_4x40x56", "stem", (4, 40, 56, 0, 0, 0), _SMALL_S, "to64 both_below whole",
     "both sides below 64: ratios 0.625 and 0.875",
     (4, 64, 64, 32, 32, 4, 1, 16, 16, 1)),
    ("img_2x48x200", "stem", (2, 48, 200, 0, 0, 0), _SMALL_S, "to64 one_below whole",
     "one side below 64, so the other is downsampled by 3.125",
     (2, 64, 64, 32, 32, 4, 1, 8, 8, 1)),
    ("img_2x32x32", "stem", (2, 32, 32, 0, 0, 0), _SMALL_S, "to64 both_below exact2x whole", "exact 2x",
     (2, 64, 64, 32, 32, 4, 1, 8, 8, 1)),
    ("patch_2x64x56_pd32_ps8", "stem", (2, 64, 56, 32, 8, 0), _SMALL, "windows to64 exact2x whole",
     "windows of 32 resized to 64",
     (40, 64, 64, 32, 32, 4, 1, 160, 160, 1)),
    ("patch_1x70x70_pd32_ps3", "stem", (1, 70, 70, 32, 3, 0), _SMALL, "windows to64 odd_stride whole", "odd stride",
     (169, 64, 64, 32, 32, 4, 1, 676, 676, 1)),
    ("patch_1x96x80_pd64_ps16", "stem", (1, 96, 80, 64, 16, 0), _SMALL, "windows direct whole",
     "direct windows: no resize in patch mode",
     (6, 64, 64, 32, 32, 4, 1, 24, 24, 1)),
    ("patch_1x80x80_pd48_ps16", "stem", (1, 80, 80, 48, 16, 0), _SMALL, "windows to64 whole", "ratio 0.75",
     (9, 64, 64, 32, 32, 4, 1, 36, 36, 1)),
    ("rs_2x33x36", "stem", (2, 33, 36, 0, 0, 1), _SMALL, "resize2x whole ragged single_last_row",
     "resize_to = (2h, 2w), the dense per-image map of the shared-layer1 scoring pass: odd and non-square",
     (2, 66, 72, 33, 36, 5, 2, 20, 20, 1)),
    ("rs_1x50x34", "stem", (1, 50, 34, 0, 0, 1), _SMALL, "resize2x whole ragged", "resize_to = (2h, 2w): non-square, Wo = 34",
     (1, 100, 68, 50, 34, 7, 2, 14, 14, 1)),
    ("loop_img_1025_S", "stem", (1025, 64, 64, 0, 0, 0), "S", "direct whole walk2 next_tile_other_sample",
     "4100 tiles on 4096 workgroups: four workgroups walk two tiles, the prefetched tile belongs to another sample; statistics",
     (1025, 64, 64, 32, 32, 4, 1, 4100, 4096, 2)),
    ("loop_img_1025_A", "stem", (1025, 64, 64, 0, 0, 0), "A", "direct whole walk2 next_tile_other_sample",
     "the same walk through the affine + ReLU epilogue",
     (1025, 64, 64, 32, 32, 4, 1, 4100, 4096, 2)),
    ("loop_patch_1089", "stem", (1, 64, 64, 32, 1, 0), "Ap", "windows to64 exact2x whole walk2 next_tile_other_sample",
     "1089 windows, 4356 tiles: 260 workgroups walk two tiles; position-major",
     (1089, 64, 64, 32, 32, 4, 1, 4356, 4096, 2)),
]
PATCH = [
    ("pp_2x64x56_ps8", "patch", (2, 64, 56, 8), _ALL_PATCH, "", "baseline, 40 windows",
     (40, 64, 64, 32, 32, 1, 1, 40, 40, 1)),
    ("pp_3x32x32_ps1", "patch", (3, 32, 32, 1), _ALL_PATCH, "one_window_per_image", "one window per image: the image-level use",
     (3, 64, 64, 32, 32, 1, 1, 3, 3, 1)),
    ("pp_1x72x66_ps2", "patch", (1, 72, 66, 2), _ALL_PATCH, "even_stride", "even stride, many overlapping windows",
     (378, 64, 64, 32, 32, 1, 1, 378, 378, 1)),
    ("pp_1x70x70_ps3", "patch", (1, 70, 70, 3), _ALL_PATCH, "odd_stride", "odd stride",
     (169, 64, 64, 32, 32, 1, 1, 169, 169, 1)),
    ("pp_2x64x56_ps8_null", "patch", (2, 64, 56, 8), "full+fullp+r4_12p+border", "", "NULL scale and shift",
     (40, 64, 64, 32, 32, 1, 1, 40, 40, 1)),
    ("pp_loop_2x64x64_ps1", "patch", (2, 64, 64, 1), "full+r4_12p+border", "walk2 prefetch_crosses_image",
     "2178 windows on 2048 workgroups: 130 walk two windows; the prefetch crosses the image boundary at window 1089",
     (2178, 64, 64, 32, 32, 1, 1, 2178, 2048, 2)),
]
S16 = [
    ("s16_1x64x64", "s16", (1, 64, 64), "f16+bf16+f16h", "whole", "base case",
     (1, 64, 64, 32, 32, 4, 1, 4, 4, 1)),
    ("s16_3x70x74", "s16", (3, 70, 74), "f16+bf16+f16h", "whole ragged odd_ho", "ragged",
     (3, 70, 74, 35, 37, 5, 2, 30, 30, 1)),
    ("s16_5x65x97", "s16", (5, 65, 97), "f16+bf16+f16h", "whole ragged single_last_row", "ragged, a single last row",
     (5, 65, 97, 33, 49, 5, 2, 50, 50, 1)),
    ("s16_loop_1025_f16", "s16", (1025, 64, 64), "f16", "whole walk2 next_tile_other_sample", "the persistent loop, fp16",
     (1025, 64, 64, 32, 32, 4, 1, 4100, 4096, 2)),
    ("s16_loop_1025_bf16", "s16", (1025, 64, 64), "bf16", "whole walk2 next_tile_other_sample", "the persistent loop, bf16",
     (1025, 64, 64, 32, 32, 4, 1, 4100, 4096, 2)),
    ("s16_loop_1025_f16h", "s16", (1025, 64, 64), "f16h", "whole walk2 next_tile_other_sample", "the persistent loop, half output",
     (1025, 64, 64, 32, 32, 4, 1, 4100, 4096, 2)),
]
ROWS = STEM + PATCH + S16


# ---- geometry ----
def geometry(entry, geo):
    """dict(P, n, wh, ww, hv, wv, ho, wo, ty, tx, total, grid, walk) of a row from the restated constants."""
    if entry == "patch":
        b, h, w, ps = geo
        prow, pcol = (h - PATCH_WINDOW) // ps + 1, (w - PATCH_WINDOW) // ps + 1
        n = b * prow * pcol
        grid = min(n, PATCH_GRID_CAP)
        return dict(P=prow * pcol, pcol=pcol, n=n, wh=32, ww=32, hv=64, wv=64, ho=32, wo=32, ty=1, tx=1, total=n, grid=grid,
                    walk=-(-n // grid))
    b, h, w, pd, ps, rs = geo if entry == "stem" else geo + (0, 0, 0)
    if pd:
        prow, pcol = (h - pd) // ps + 1, (w - pd) // ps + 1
        wh = ww = pd
    else:
        prow = pcol = 1
        wh, ww = h, w
    if rs:
        hv, wv = 2 * h, 2 * w
    else:
        hv, wv = (64, 64) if (wh < 64 or ww < 64) else (wh, ww)          # models.py:217-219
    ho, wo = (hv - 1) // 2 + 1, (wv - 1) // 2 + 1
    ty, tx = -(-ho // TOH), -(-wo // TOW)
    n = b * prow * pcol
    total = n * ty * tx
    grid = min(total, CONV_GRID_CAP)
    return dict(P=prow * pcol, pcol=pcol, n=n, wh=wh, ww=ww, hv=hv, wv=wv, ho=ho, wo=wo, ty=ty, tx=tx, total=total, grid=grid,
                walk=-(-total // grid))


# tag -> predicate over (geometry dict, the row's geometry tuple): what "the smallest shape for" means in numbers
CLAIMS = {
    "whole": lambda g, t: g["wo"] >= TOW,                                          # some tile has all 32 columns
    "ragged": lambda g, t: g["wo"] % TOW != 0 and g["wo"] > TOW,                   # ... and some tile in the same row has not
    "one_column": lambda g, t: g["tx"] == 1 and g["wo"] == TOW,
    "two_columns": lambda g, t: g["tx"] == 2 and g["wo"] == 2 * TOW,
    "odd_ho": lambda g, t: g["ho"] % 2 == 1,
    "single_last_row": lambda g, t: g["ho"] % TOH == 1,
    "direct": lambda g, t: (g["wh"], g["ww"]) == (g["hv"], g["wv"]),
    "to64": lambda g, t: (g["hv"], g["wv"]) == (64, 64) and (g["wh"] < 64 or g["ww"] < 64),
    "both_below": lambda g, t: g["wh"] < 64 and g["ww"] < 64,
    "one_below": lambda g, t: (g["wh"] < 64) != (g["ww"] < 64),
    "exact2x": lambda g, t: (g["hv"], g["wv"]) == (2 * g["wh"], 2 * g["ww"]),
    "resize2x": lambda g, t: t[5] == 1 and (g["hv"], g["wv"]) == (2 * t[1], 2 * t[2]) and (t[1] % 2 == 1 or t[1] != t[2]),
    "windows": lambda g, t: t[3] > 0 and g["P"] > 1,
    "odd_stride": lambda g, t: t[-2 if len(t) == 6 else -1] % 2 == 1 and g["P"] > 1,
    "even_stride": lambda g, t: t[-1] % 2 == 0 and g["P"] > 1,
    "one_window_per_image": lambda g, t: g["P"] == 1 and t[0] > 1,
    "walk2": lambda g, t: g["walk"] == 2 and g["total"] > g["grid"],
    # tile t + grid lies in another sample than tile t for every walking workgroup (tiles per sample < grid)
    "next_tile_other_sample": lambda g, t: g["ty"] * g["tx"] < g["grid"] and g["total"] > g["grid"],
    # some walking workgroup's second window is in the next image: first windows 0 .. total - grid - 1 are all in image 0
    "prefetch_crosses_image": lambda g, t: g["total"] - g["grid"] <= g["P"] < g["grid"] and g["P"] < g["total"],
}


def cells(row):
    """The (whole / ragged, epilogue form, layout) cells of stem_conv7x7_kernel a stem row runs."""
    g = geometry(row[1], row[2])
    tiles = (["whole"] if CLAIMS["whole"](g, row[2]) else []) + (["ragged"] if g["wo"] % TOW else [])
    out = set()
    for f in row[3].split("+"):
        form = {"A": "affine_relu", "R": "raw", "S": "raw_stats", "C": "scale_only"}[f[0]]
        out |= {(t, form, "pm" if f.endswith("p") else "nhwc") for t in tiles}
    return out


ALL_CELLS = {(t, f, l) for t in ("whole", "ragged") for f in ("affine_relu", "raw", "raw_stats", "scale_only") for l in ("nhwc", "pm")
             if not (f == "raw_stats" and l == "pm")}               # ssad_stem_fwd_stats writes NHWC only


# ---- inputs ----
def seed_of(row):
    return sum(map(ord, row[1] + repr(row[2])))          # per geometry: rows that split one geometry by form share their reference


def make_inputs(row):
    """(img fp32 [B][3][H][W], filter OIHW fp32, scale, shift) of a row."""
    g = torch.Generator().manual_seed(seed_of(row))
    b, h, w = row[2][:3]
    img = torch.randn(b, 3, h, w, generator=g) + torch.tensor([0.6, 0.4, 0.5]).view(1, 3, 1, 1)
    sign = lambda n: torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    wt = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5 + (sign(64) * (0.007 + 0.013 * torch.rand(64, generator=g))).view(64, 1, 1, 1)
    sc = sign(64) * (0.5 + torch.rand(64, generator=g))
    sh = torch.randn(64, generator=g)
    sh[sh.abs() < 0.05] = 0.25
    return img, wt, sc, sh


def running_start(row):
    g = torch.Generator().manual_seed(seed_of(row) + 1)
    return torch.randn(64, generator=g) * 0.5, torch.rand(64, generator=g) + 0.5


# ---- the float64 reference ----
def select(img, pd, ps, hv, wv, dy=0, dx=0):
    """Windows and nearest resize by the documented integer rule -> [N][3][hv][wv], sample n = b * P + pr * pcol + pc.
    dy / dx: the window-origin defect of the sensitivity test (indices clamped to the image)."""
    b, _, h, w = img.shape
    wh, ww = (pd, pd) if pd else (h, w)
    prow, pcol = ((h - pd) // ps + 1, (w - pd) // ps + 1) if pd else (1, 1)
    iy, ix = (torch.arange(hv) * wh) // hv, (torch.arange(wv) * ww) // wv
    out = []
    for pr in range(prow):
        for pc in range(pcol):
            yy, xx = (ps * pr + dy + iy).clamp(0, h - 1), (ps * pc + dx + ix).clamp(0, w - 1)
            out.append(img[:, :, yy][:, :, :, xx])
    return torch.stack(out, 1).reshape(b * prow * pcol, 3, hv, wv)


def conv_nhwc(x, wt, chunk=64):
    """F.conv2d(stride 2, pad 3) in the dtype of x, sample chunks -> NHWC [N][Ho][Wo][64]."""
    return torch.cat([F.conv2d(x[i:i + chunk], wt, None, 2, 3).permute(0, 2, 3, 1) for i in range(0, x.shape[0], chunk)]).contiguous()


def rounded(t, mode):
    """The operand as the 16-bit kernels multiply it (exact in float64)."""
    return t.half().float() if mode.startswith("f16") else t.bfloat16().float() if mode == "bf16" else t


def raw_reference(row, mode="", dtype=torch.float64, limit=None, defect=None):
    """The raw convolution of a row, NHWC [N][Ho][Wo][64] in `dtype` on the CPU (limit: the first samples only -- the yardstick).
    defect: None, or one of the deliberate errors of the sensitivity test: "origin", "swap", "kx6"."""
    img, wt, _, _ = make_inputs(row)
    g = geometry(row[1], row[2])
    pd, ps = (row[2][3], row[2][4]) if row[1] == "stem" else (PATCH_WINDOW, row[2][3]) if row[1] == "patch" else (0, 0)
    if pd == 0 and (g["hv"], g["wv"]) == (g["wh"], g["ww"]) and defect != "origin":
        x = rounded(img, mode).to(dtype)
    else:
        x = select(rounded(img, mode).to(dtype), pd, ps, g["hv"], g["wv"], *((1, 1) if defect == "origin" else (0, 0)))
    if limit is not None:
        x = x[:limit]
    wt = rounded(wt, mode).to(dtype)
    if defect == "kx6":
        wt = wt.clone()
        wt[:, :, :, 6] = 0
    z = conv_nhwc(x, wt)
    if defect == "swap":
        idx = torch.arange(z.shape[0])
        idx[:z.shape[0] // 2 * 2] ^= 1                        # samples n and n + 1 change places
        z = z[idx]
    return z


@functools.lru_cache(maxsize=1)
def _raw64(entry, geo, mode):
    """The float64 raw map of a geometry, kept for the next row or form that shares it (inputs depend on entry and geometry only)."""
    return raw_reference((None, entry, geo), mode)


def epilogue(z, sc, sh, relu, pool=False, left_dropped=False):
    """scale, shift, ReLU, max-pool on an NHWC raw map, in z's dtype (None: absent)."""
    if sc is not None:
        z = z * sc.to(z.dtype)
    if sh is not None:
        z = z + sh.to(z.dtype)
    if relu:
        z = z.clamp(min=0)
    if pool:
        zc = z.permute(0, 3, 1, 2)
        # left_dropped: the sensitivity test's defect -- columns 2 px, 2 px + 1 only
        zc = F.max_pool2d(zc, (3, 2), 2, (1, 0)) if left_dropped else F.max_pool2d(zc, 3, 2, 1)
        z = zc.permute(0, 2, 3, 1).contiguous()
    return z


def reference_stats(z):
    """mean, biased variance, row count over an NHWC float64 map."""
    zz = z.reshape(-1, 64).double()
    m = zz.mean(0)
    return m, ((zz - m) ** 2).mean(0), zz.shape[0]


# ---- buffers between guards ----
GUARD = 1 << 16


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Arena:
    """Every tensor of a launch in an allocation of its own, [GUARD | tensor | GUARD].  Inputs sit between NaN guards (a read outside
    meets NaN and shows in the result) and must come back bit-unchanged, guards included.  Outputs and their guards start as poison --
    1e30 for fp32, NaN for the fp64 workspace and for halves --: afterwards the guards must be bit-unchanged, no poison may be left
    where the kernel is documented to write, and every element it is documented to skip must still hold it."""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def inp(self, name, t, mutable=False):
        if t is None:
            return None
        big = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=t.dtype, device=self.dev)
        big[GUARD:GUARD + t.numel()] = t.reshape(-1).to(self.dev)
        self.items.append((name, big, None if mutable else big.clone(), (big[:GUARD].clone(), big[GUARD + t.numel():].clone()), t.numel(), None))
        return big[GUARD:GUARD + t.numel()].view(t.shape)

    def out(self, name, shape, dtype, skip=None, partial=False):
        """skip: bool tensor broadcastable to shape, True where the kernel is documented NOT to write.  partial: only the guards are
        checked (the statistics workspace: rows past the grid are nobody's)."""
        n = math.prod(shape)
        big = torch.full((n + 2 * GUARD,), POISON if dtype == torch.float32 else float("nan"), dtype=dtype, device=self.dev)
        self.items.append((name, big, None, (big[:GUARD].clone(), big[GUARD + n:].clone()), n, (shape, skip, partial)))
        return big[GUARD:GUARD + n].view(shape)

    def check(self, rid):
        torch.cuda.synchronize()
        for name, big, snap, (g0, g1), n, spec in self.items:
            assert torch.equal(_bits(big[:GUARD]), _bits(g0)), f"{rid}: the launch wrote in front of `{name}`"
            assert torch.equal(_bits(big[GUARD + n:]), _bits(g1)), f"{rid}: the launch wrote past the end of `{name}`"
            if spec is None:
                assert snap is None or torch.equal(_bits(big), _bits(snap)), f"{rid}: input `{name}` was written"
                continue
            shape, skip, partial = spec
            if partial:
                continue
            t = big[GUARD:GUARD + n].view(shape)
            poisoned = (t == POISON) if t.dtype == torch.float32 else torch.isnan(t)
            if skip is None:
                left = int(poisoned.sum())
                assert left == 0, f"{rid}: {left} of {n} elements of `{name}` left unwritten"
            else:
                skip = skip.to(self.dev).expand(shape)
                left = int((poisoned & ~skip).sum())
                assert left == 0, f"{rid}: {left} elements of `{name}` the kernel is documented to write left unwritten"
                hit = int((~poisoned & skip).sum())
                assert hit == 0, f"{rid}: {hit} elements of `{name}` the kernel is documented to skip were written"


# ---- comparison ----
WORST = {}                  # family -> {figure: worst}


def note(family, key, v):
    d = WORST.setdefault(family, {})
    d[key] = max(d.get(key, 0.0), float(v))


def compare(rid, family, got, want, keep=None, half=False, slack=0.0):
    """Every element of `got` (device, viewed [N][..][64] like `want`, CPU float64) against `want`, chunk by chunk, the subtraction in
    float64 on the device.  keep: bool [1][Y][X][1], the positions the kernel writes.  fp32: |err| <= TOL * max |want|.
    half: |err| <= the spacing of halves at |want| (2^-24 below 2^-14) + slack (HALF_MARGIN x the yardstick's absolute error: see the
    docstring) -> also the share of elements that are not the correctly rounded half.
    -> worst error as a fraction of max |want| (fp32) or of the spacing (half, before the slack)."""
    assert tuple(got.shape) == tuple(want.shape), f"{rid}: shape {tuple(got.shape)} against {tuple(want.shape)}"
    dev = got.device
    wmax = want.abs().max().item()
    step = max(1, (1 << 23) // max(1, want[0].numel()))
    k = None if keep is None else keep.to(dev)
    worst, off, total = 0.0, 0, 0
    for i in range(0, want.shape[0], step):
        w = want[i:i + step].to(dev)
        gq = got[i:i + step]
        if k is not None:
            gq = torch.where(k, gq, torch.zeros((), dtype=gq.dtype, device=dev))
            w = torch.where(k, w, torch.zeros((), dtype=w.dtype, device=dev))
        e = (gq.double() - w).abs()
        if half:
            ex = torch.frexp(w.abs())[1].clamp(min=-13)            # |w| = m 2^ex, 0.5 <= m < 1: halves there are 2^(ex - 11) apart
            sp = torch.exp2((ex - 11).double())
            e, over = e / sp, e > sp + slack
            off += int((gq != w.half()).sum())
            total += e.numel()
        bar = f"a half spacing + {slack:.3e}" if half else TOL * wmax
        m = e.max().item()
        bad = (over | torch.isnan(e)) if half else ~(e <= bar)
        if bad.any():
            j = int(bad.reshape(-1).nonzero()[0])
            raise AssertionError(f"{rid}: {int(bad.sum())} elements over the bar {bar} in samples {i}.., first flat index {j}: got "
                                 f"{gq.reshape(-1)[j].item():.9g}, want {w.reshape(-1)[j].item():.9g} (max |want| {wmax:.3e})")
        worst = max(worst, m)
    if half:
        note(family, "half err / spacing", worst)
        note(family, "share not correctly rounded", off / max(total, 1))
        return worst
    note(family, "err / max|want|", worst / wmax)
    return worst / wmax


def yardstick(rid, family, row, mode, chain):
    """The same reference in fp32 on the CPU against float64, over the first 64 samples; chain(z) applies the form's epilogue."""
    z32, z64 = chain(raw_reference(row, mode, torch.float32, 64)), chain(raw_reference(row, mode, torch.float64, 64))
    ya = (z32.double() - z64).abs().max().item()
    y = ya / z64.abs().max().item()
    note(family, "fp32-CPU yardstick", y)
    return y, ya


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-12)


def check_stats(rid, family, z64, mean, invstd, run0, run1):
    """mean, invstd and the running statistics against float64 statistics of z64 (the reference; the stored halves for out_half)."""
    assert torch.isfinite(mean).all() and torch.isfinite(invstd).all(), f"{rid}: a NaN of the workspace reached the statistics"
    m, v, n = reference_stats(z64)
    em = (mean.cpu().double() - m).abs().max().item()
    ei = _rel(invstd, (v + EPS).rsqrt())
    print(f"   {rid}: mean err {em:.2e}, invstd err {ei:.2e}, |mean| / std {float((m.abs() / v.sqrt()).min()):.2f} .. "
          f"{float((m.abs() / v.sqrt()).max()):.2f}", flush=True)
    assert em < MEAN_TOL, f"{rid}: mean off by {em:.3e}"
    assert ei < INVSTD_TOL, f"{rid}: invstd off by {ei:.3e}"
    note(family, "mean err", em)
    note(family, "invstd err", ei)
    if run1 is not None:
        mom = float(torch.tensor(MOMENTUM, dtype=torch.float32))
        want_m = (1 - mom) * run0[0].double() + mom * m
        want_v = (1 - mom) * run0[1].double() + mom * v * n / max(n - 1, 1)
        er = max(_rel(run1[0], want_m), _rel(run1[1], want_v))
        assert torch.isfinite(run1[0]).all() and torch.isfinite(run1[1]).all() and er < RUNNING_TOL, f"{rid}: running statistics off by {er:.3e}"
        note(family, "running err", er)


# ---- packers ----
def pack_rule(wt):
    """ssad_pack_stem_weight in numpy: wk[k][co], k = ((ky*4+q)*3+c)*2+h, kx = 2q+h; the kx = 7 rows are zeros."""
    import numpy as np
    w = wt.numpy()
    wk = np.zeros((168, 64), np.float32)
    for ky in range(7):
        for q in range(4):
            for c in range(3):
                for h in range(2):
                    if 2 * q + h < 7:
                        wk[((ky * 4 + q) * 3 + c) * 2 + h] = w[:, c, ky, 2 * q + h]
    return torch.from_numpy(wk)


def pack16_rule(wt, dtype):
    """ssad_pack_stem_weight16 from the comment in stem16.hip: wk16[ky][kk][co][16], k = 16 kk + j <-> (kx = k / 4, c = k % 4);
    kx = 7 and c = 3 are zeros."""
    wk = torch.zeros(7, 2, 64, 16, dtype=dtype)
    for ky in range(7):
        for k in range(32):
            kx, c = k // 4, k % 4
            if kx < 7 and c < 3:
                wk[ky, k // 16, :, k % 16] = wt[:, c, ky, kx].to(dtype)
    return wk


def folded_rule(wt):
    """ssad_pack_stem_weight_folded in float64: wf[(a*2+q)*3+c][h][co], b = 2q+h, tap groups {0}, {1,2}, {3,4}, {5,6} in ky (a) and
    kx (b) -> (group sums, group sums of magnitudes)."""
    grp = ((0,), (1, 2), (3, 4), (5, 6))
    w = wt.double()
    wf, wa = torch.zeros(24, 2, 64, dtype=torch.float64), torch.zeros(24, 2, 64, dtype=torch.float64)
    for a in range(4):
        for q in range(2):
            for c in range(3):
                for h in range(2):
                    sub = w[:, c][:, list(grp[a])][:, :, list(grp[2 * q + h])]
                    wf[(a * 2 + q) * 3 + c, h], wa[(a * 2 + q) * 3 + c, h] = sub.sum((1, 2)), sub.abs().sum((1, 2))
    return wf, wa


def _P(t):
    return None if t is None else t.data_ptr()


def run_packers(dev):
    """Every packer into a poisoned destination between guards: exact against the index rule (float64 group sums for the folded one);
    the padded rows are zeros the packer wrote itself."""
    from self_supervised import _hip
    lib, st = _hip.lib(), _hip.stream()
    wt = make_inputs(STEM[0])[1]
    ohwi = wt.permute(0, 2, 3, 1).contiguous()
    want = pack_rule(wt)
    assert int((want == 0).all(1).sum()) == 7 * 3, "21 of the 168 K rows are the kx = 7 padding"
    for fn, src in ((lib.ssad_pack_stem_weight, wt), (lib.ssad_pack_stem_weight_ohwi, ohwi)):
        ar = Arena(dev)
        s, d = ar.inp("filter", src), ar.out("wk", (168, 64), torch.float32)
        _hip.check(fn(_P(s), _P(d), st))
        ar.check("pack_stem_weight")
        assert torch.equal(_bits(d.cpu()), _bits(want)), "ssad_pack_stem_weight(_ohwi): not the index rule"
    for f16, dt in ((1, torch.float16), (0, torch.bfloat16)):
        want16 = pack16_rule(wt, dt)
        for fn, src in ((lib.ssad_pack_stem_weight16, wt), (lib.ssad_pack_stem_weight16_ohwi, ohwi)):
            ar = Arena(dev)
            s, d = ar.inp("filter", src), ar.out("wk16", (7, 2, 64, 16), dt)
            _hip.check(fn(_P(s), _P(d), f16, st))
            ar.check("pack_stem_weight16")
            assert torch.equal(_bits(d.cpu()), _bits(want16)), f"ssad_pack_stem_weight16(_ohwi) {dt}: not the documented layout"
    wf, wa = folded_rule(wt)
    ar = Arena(dev)
    s, d = ar.inp("filter", wt), ar.out("wf", (24, 2, 64), torch.float32)
    _hip.check(lib.ssad_pack_stem_weight_folded(_P(s), _P(d), st))
    ar.check("pack_stem_weight_folded")
    err = (d.cpu().double() - wf).abs()
    assert (err <= 4 * 2.0 ** -24 * wa).all(), f"ssad_pack_stem_weight_folded: off by {(err / wa).max().item():.3e} of the group's magnitudes"
    note("packers", "folded err / sum|w|", (err / wa).max().item())


# ---- the rows ----
def _pm(t):
    """position-major [Y][X][N][64] -> a view [N][Y][X][64]."""
    return t.permute(2, 0, 1, 3)


def run_stem_row(row, dev):
    from self_supervised import _hip, ops
    lib, st = _hip.lib(), _hip.stream()
    rid, _, (b, h, w, pd, ps, rs), forms = row[:4]
    g = geometry("stem", row[2])
    n, ho, wo = g["n"], g["ho"], g["wo"]
    img, wt, sc, sh = make_inputs(row)
    z64 = _raw64("stem", row[2], "")
    assert (z64 < 0).any()
    wk = ops.pack_stem_weight(wt.to(dev))

    def launch(fid, scale, shift, relu, hwnc):
        ar = Arena(dev)
        t = dict(img=ar.inp("img", img), wk=ar.inp("wk", wk), sc=ar.inp("scale", scale), sh=ar.inp("shift", shift))
        t["out"] = ar.out("out", (ho, wo, n, 64) if hwnc else (n, ho, wo, 64), torch.float32)
        _hip.check(lib.ssad_stem_fwd(_P(t["img"]), b, h, w, pd, ps, g["hv"], g["wv"], _P(t["wk"]), _P(t["sc"]), _P(t["sh"]), int(relu),
                                     int(hwnc), _P(t["out"]), st))
        ar.check(fid)
        return t["out"]

    def launch_stats(fid, run):
        ar = Arena(dev)
        t = dict(img=ar.inp("img", img), wk=ar.inp("wk", wk))
        t["out"] = ar.out("out", (n, ho, wo, 64), torch.float32)
        t["ws"] = ar.out("statistics workspace", (CONV_GRID_CAP * 128,), torch.float64, partial=True)
        t["mean"], t["invstd"] = ar.out("mean", (64,), torch.float32), ar.out("invstd", (64,), torch.float32)
        t["rm"], t["rv"] = (ar.inp("running_mean", run[0], True), ar.inp("running_var", run[1], True)) if run else (None, None)
        _hip.check(lib.ssad_stem_fwd_stats(_P(t["img"]), b, h, w, g["hv"], g["wv"], _P(t["wk"]), _P(t["out"]), EPS, MOMENTUM, _P(t["mean"]),
                                           _P(t["invstd"]), _P(t["rm"]), _P(t["rv"]), _P(t["ws"]), st))
        ar.check(fid)
        ws = t["ws"].view(CONV_GRID_CAP, 128)
        assert not torch.isnan(ws[:g["grid"]]).any(), f"{fid}: a workgroup left its row of the statistics partials unwritten"
        return t

    for f in forms.split("+"):
        fid, hwnc = f"{rid}[{f}]", f.endswith("p")
        if f[0] == "S":
            assert not (pd or rs), "ssad_stem_fwd_stats takes whole images"
            run0 = running_start(row)
            t = launch_stats(fid, run0)
            raw = launch(fid + " without statistics", None, None, False, False)
            assert torch.equal(_bits(t["out"]), _bits(raw)), f"{fid}: z with and without statistics differ"
            e = compare(fid, "stem fp32", t["out"], z64)
            check_stats(fid, "stem fp32", z64, t["mean"], t["invstd"], run0, (t["rm"], t["rv"]))
            t2 = launch_stats(fid + " (NULL running statistics)", None)
            for k in ("out", "mean", "invstd"):
                assert torch.equal(_bits(t2[k]), _bits(t[k])), f"{fid}: `{k}` depends on the running-statistics pointers"
            y = yardstick(fid, "stem fp32", row, "", lambda z: z)[0]
        else:
            scale, shift, relu = {"A": (sc, sh, True), "R": (None, None, False), "C": (sc, None, False)}[f[0]]
            want = epilogue(z64, scale, shift, relu)
            out = launch(fid, scale, shift, relu, hwnc)
            e = compare(fid, "stem fp32", _pm(out) if hwnc else out, want)
            y = yardstick(fid, "stem fp32", row, "", lambda z: epilogue(z, scale, shift, relu))[0]
            if f == "A" and n * ho * wo * 64 <= 1 << 22:       # the wrapper, where it can pass the arguments: bit-equal
                for hw_ in (False, True):
                    wr = ops.stem_fwd(img.to(dev), wk, sc.to(dev), sh.to(dev), True, pd, ps, hwnc=hw_, resize_to=(2 * h, 2 * w) if rs else None)
                    assert torch.equal(_pm(wr) if hw_ else wr, out), f"{fid}: the C call into poisoned buffers differs from ops.stem_fwd"
        print(f"ok {fid}: err / max|want| {e:.2e} (fp32 on the CPU {y:.2e})", flush=True)


def _patch_form(f):
    """-> (border, hwnc, lo, hi)."""
    if f == "border":
        return True, True, 1, 0
    hwnc = f.endswith("p")
    if f.startswith("full"):
        return False, hwnc, 1, 0
    lo, hi = f.rstrip("p")[1:].split("_")
    return False, hwnc, int(lo), int(hi)


def run_patch_row(row, dev):
    from self_supervised import _hip, ops
    lib, st = _hip.lib(), _hip.stream()
    rid, _, (b, h, w, ps), forms = row[:4]
    n = geometry("patch", row[2])["n"]
    img, wt, sc, sh = make_inputs(row)
    if rid.endswith("_null"):
        sc = sh = None
    want = epilogue(_raw64("patch", row[2], ""), sc, sh, True, pool=True)
    wf = ops.pack_stem_weight_folded(wt.to(dev))
    edge = torch.zeros(16, 16, dtype=torch.bool)
    edge[[0, 1, 15], :] = True
    edge[:, [0, 1, 15]] = True
    full = {}
    for f in forms.split("+"):                               # ("full" / "fullp" come first)
        fid = f"{rid}[{f}]"
        border, hwnc, lo, hi = _patch_form(f)
        if border:
            skip = ~edge
        else:
            skip = torch.zeros(16, 16, dtype=torch.bool)
            skip[lo:hi + 1, lo:hi + 1] = lo <= hi
        ar = Arena(dev)
        t = dict(img=ar.inp("img", img), wf=ar.inp("wf", wf), sc=ar.inp("scale", sc), sh=ar.inp("shift", sh))
        out = ar.out("out", (16, 16, n, 64) if hwnc else (n, 16, 16, 64), torch.float32, skip=skip.view(16, 16, 1, 1) if hwnc else skip.view(1, 16, 16, 1))
        if border:
            _hip.check(lib.ssad_stem_patch_border_fwd(_P(t["img"]), b, h, w, ps, _P(t["wf"]), _P(t["sc"]), _P(t["sh"]), _P(out), st))
        else:
            _hip.check(lib.ssad_stem_patch_pool_fwd_ring(_P(t["img"]), b, h, w, ps, _P(t["wf"]), _P(t["sc"]), _P(t["sh"]), int(hwnc), lo, hi,
                                                         _P(out), st))
        ar.check(fid)
        got = _pm(out) if hwnc else out
        keep = (~skip).view(1, 16, 16, 1)
        e = compare(fid, "folded patch", got, want, keep=keep) if keep.any() else 0.0
        if f.startswith("full"):
            full[hwnc] = got
        elif hwnc in full:                                   # the identities of test_fused_patch_stem, bit for bit
            kd = keep.to(dev).expand(got.shape)
            assert torch.equal(got[kd], full[hwnc][kd]), f"{fid}: differs from the full form where both write"
    y = yardstick(rid, "folded patch", row, "", lambda z: epilogue(z, sc, sh, True, pool=True))[0]
    print(f"ok {rid}: uses {WORST['folded patch']['err / max|want|'] / TOL:.3f} of the bar so far (fp32 on the CPU {y:.2e})", flush=True)


def run_s16_row(row, dev):
    from self_supervised import _hip
    lib, st = _hip.lib(), _hip.stream()
    rid, _, (b, h, w), forms = row[:4]
    g = geometry("s16", row[2])
    ho, wo = g["ho"], g["wo"]
    img, wt, _, _ = make_inputs(row)
    ohwi = wt.permute(0, 2, 3, 1).contiguous()
    for mode in forms.split("+"):
        fid, half, f16 = f"{rid}[{mode}]", mode == "f16h", int(mode != "bf16")
        fam = "stem16 " + mode
        z64 = _raw64("s16", row[2], "f16" if half else mode)
        res = []
        for layout, src, run in (("OIHW", wt, True), ("OHWI", ohwi, True), ("OIHW, NULL running statistics", wt, False)):
            ar = Arena(dev)
            s = ar.inp("filter", src)
            wk = ar.out("wk16", (7, 2, 64, 16), torch.float16 if f16 else torch.bfloat16)
            _hip.check((lib.ssad_pack_stem_weight16_ohwi if layout == "OHWI" else lib.ssad_pack_stem_weight16)(_P(s), _P(wk), f16, st))
            t = dict(img=ar.inp("img", img))
            t["out"] = ar.out("out", (b, ho, wo, 64), torch.float16 if half else torch.float32)
            t["ws"] = ar.out("statistics workspace", (CONV_GRID_CAP * 128,), torch.float64, partial=True)
            t["mean"], t["invstd"] = ar.out("mean", (64,), torch.float32), ar.out("invstd", (64,), torch.float32)
            run0 = running_start(row)
            t["rm"], t["rv"] = (ar.inp("running_mean", run0[0], True), ar.inp("running_var", run0[1], True)) if run else (None, None)
            args = (_P(t["img"]), b, h, w, _P(wk), _P(t["out"]), EPS, MOMENTUM, _P(t["mean"]), _P(t["invstd"]), _P(t["rm"]), _P(t["rv"]), _P(t["ws"]))
            _hip.check(lib.ssad_stem_fwd_stats16_h(*args, st) if half else lib.ssad_stem_fwd_stats16(*args, f16, st))
            ar.check(f"{fid} {layout}")
            assert not torch.isnan(t["ws"].view(CONV_GRID_CAP, 128)[:g["grid"]]).any(), f"{fid}: statistics partials left unwritten"
            res.append(t)
        for k in ("out", "mean", "invstd", "rm", "rv"):
            assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), f"{fid}: `{k}` from the OIHW and the OHWI filter differ"
        for k in ("out", "mean", "invstd"):
            assert torch.equal(_bits(res[0][k]), _bits(res[2][k])), f"{fid}: `{k}` depends on the running-statistics pointers"
        t = res[0]
        y, ya = yardstick(fid, fam, row, "f16" if half else mode, lambda z: z)
        e = compare(fid, fam, t["out"], z64, half=half, slack=HALF_MARGIN * ya)
        zs = t["out"].cpu().double() if half else z64          # out_half: the statistics of the halves the kernel stored
        check_stats(fid, fam, zs, t["mean"], t["invstd"], running_start(row), (t["rm"], t["rv"]))
        print(f"ok {fid}: {'err / half spacing' if half else 'err / max|want|'} {e:.2e} (fp32 on the CPU {y:.2e})", flush=True)


def run_row(row, dev):
    {"stem": run_stem_row, "patch": run_patch_row, "s16": run_s16_row}[row[1]](row, dev)


def print_worst():
    """The worst measured figures per family so far (the figures of the docstring): `pytest -s -m gpu tests/test_hip_stem_paths.py`
    prints them when the module ends."""
    for fam, d in sorted(WORST.items()):
        print(f"worst {fam}: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(d.items())), flush=True)
