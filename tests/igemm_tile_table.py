"""The implicit-GEMM tile table: every entry point of csrc/conv_igemm.hip, at shapes that land on every tile its dispatch can pick,
with the tile each row must select and the comparison of every output element against float64 torch on the CPU.

Shared by tests/test_igemm_tile_table.py (tile selection only, no GPU) and tests/test_hip_igemm_tiles.py (the kernels).  The tile
switches (SSAD_CONV64_VARIANT, ...) are read once per process, so each switch set runs in a child process of its own:

    python tests/igemm_tile_table.py SET [--tiles-only]

runs SET's rows, prints one JSON line {"set": ..., "tiles": [[row id, entry, tile], ...]} and exits non-zero on the first mismatch.

Row: (id, entry, (n, h, w, cin, cout, k, stride, pad), epilogue, expected tile).  The shape is always the FORWARD conv's: x [n][h][w][cin],
filter [cout][k][k][cin]; an input-gradient row computes dx of that conv (dx channels = cin, contraction over cout).  Entries:
  fwd, hwnc, ring, stats, dgrad, dgrad_masked   exact fp32: expected tile = an ops.IGEMM_TILES name, "pos:" when position-major
  fwd:M, hwnc:M, dgrad:M (M = bf16, f16, x3, x6), stats:h16, dgrad:h16
                                                the 16-bit / split-bf16 dispatchers, whose one choice is whether the launch's output
                                                channels are <= 64 (the 256 x 64 tile, "c64") or not (128 x 128, "c128")
Epilogue letters: a = scale / shift, r = residual, R = ReLU (absent: null pointers); ring rows carry (skip_lo, skip_hi) and the full
epilogue instead.
"""
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "self-supervised-anomaly-detection_amd")

# ---- the default selection (no switch set) ----
DEFAULT = [
    # pixel-major forward convs
    ("f_64x64", "fwd", (3, 9, 7, 32, 70, 3, 1, 1), "arR", "64x64"),                 # ragged M (189), Cout 70: not a multiple of 4
    ("f_64x64_ds", "fwd", (5, 16, 16, 64, 96, 1, 2, 0), "a", "64x64"),              # 1 x 1 / stride 2 downsample
    ("f_64x64_2x2", "fwd", (100, 2, 2, 32, 128, 3, 1, 1), "R", "64x64"),            # 2 x 2 map, < 128 samples: pixel-major
    ("f_128x64", "fwd", (103, 15, 15, 32, 160, 3, 1, 1), "ar", "128x64"),           # M = 23175, Cout 160 = 2.5 BN
    ("f_128x128", "fwd", (257, 32, 32, 32, 130, 1, 2, 0), "aR", "128x128"),         # 514 row tiles, Cout 130
    ("f_128x256", "fwd", (129, 16, 16, 64, 256, 1, 1, 0), "arR", "128x256_K16"),    # 258 row tiles x 1
    ("f_256x64", "fwd", (7, 9, 9, 32, 42, 3, 2, 1), "R", "256x64_K16"),             # Cout 42, ragged M (175)
    ("f_256x64_1x1", "fwd", (3, 1, 1, 64, 64, 3, 1, 1), "a", "256x64_K16"),         # 1 x 1 map: only the centre tap is in bounds
    # NHWC tensors, position-major rows (>= 128 samples on a padded map of <= 4 positions)
    ("fp_256x64", "fwd", (130, 2, 2, 64, 64, 3, 1, 1), "arR", "pos:256x64_K16"),
    ("fp_128x128", "fwd", (200, 2, 2, 32, 100, 3, 1, 1), "aR", "pos:128x128_K16"),  # N = 200: ragged sample group, Cout 100
    ("fp_128x128_1x1", "fwd", (129, 1, 1, 32, 96, 3, 1, 1), "a", "pos:128x128_K16"),
    ("fp_128x256", "fwd", (4100, 2, 2, 32, 512, 3, 1, 1), "ar", "pos:128x256_K16"),  # 33 sample groups x 4 positions x 2
    # [H][W][N][C] tensors
    ("h_256x64", "hwnc", (150, 8, 8, 32, 40, 3, 2, 1), "ar", "pos:256x64_K16"),
    ("h_128x128_ds", "hwnc", (300, 4, 4, 32, 128, 1, 2, 0), "aR", "pos:128x128_K16"),
    ("h_128x128_2x2", "hwnc", (70, 2, 2, 64, 192, 3, 1, 1), "", "pos:128x128_K16"),
    # 33 sample groups (the last one 104 samples) over 2 x 2 positions of 4 and 6 taps: heaviest-first order in chunks of 32 groups
    ("h_128x256", "hwnc", (4200, 4, 4, 32, 512, 3, 2, 1), "arR", "pos:128x256_K16"),
    # ring launches (the patch-scoring pass's layer1): only the positions outside the skipped square
    ("r_128x64", "ring", (200, 8, 8, 32, 64, 3, 1, 1), (2, 5), "pos:128x64_K16"),
    ("r_128x64_c38", "ring", (130, 6, 6, 64, 38, 3, 1, 1), (1, 4), "pos:128x64_K16"),
    # conv + BatchNorm statistics: pixel-major rows only
    ("s_64x64", "stats", (3, 9, 7, 32, 70, 3, 1, 1), "", "64x64"),
    ("s_64x64_2x2", "stats", (200, 2, 2, 32, 128, 3, 1, 1), "", "64x64"),           # >= 128 samples on 2 x 2: still pixel-major
    ("s_128x64", "stats", (103, 15, 15, 32, 160, 3, 1, 1), "", "128x64"),
    ("s_256x64", "stats", (7, 9, 9, 32, 42, 3, 2, 1), "", "256x64_K16"),
    ("s_128x128", "stats", (257, 32, 32, 32, 130, 1, 2, 0), "", "128x128"),
    ("s_128x256", "stats", (129, 16, 16, 64, 256, 1, 1, 0), "", "128x256_K16"),
    # input gradients, stride 1 and the parity-class stride-2 form
    ("d1_64x64", "dgrad", (3, 9, 7, 70, 32, 3, 1, 1), "r", "64x64"),                # dx channels 70, ragged M
    ("d2_64x64", "dgrad", (5, 15, 15, 96, 64, 3, 2, 1), "", "64x64"),               # odd map: parity classes of 64 / 56 / 56 / 49
    ("d2_64x64_ds", "dgrad", (4, 16, 16, 96, 64, 1, 2, 0), "r", "64x64"),
    ("d1_64x64_2x2", "dgrad", (200, 2, 2, 128, 64, 3, 1, 1), "", "64x64"),          # >= 128 samples on 2 x 2: pixel-major
    ("d1_128x64", "dgrad", (103, 15, 15, 160, 32, 3, 1, 1), "r", "128x64"),
    ("d2_128x64", "dgrad", (103, 15, 15, 160, 32, 3, 2, 1), "", "128x64"),
    ("d1_128x128", "dgrad", (257, 16, 16, 130, 32, 1, 1, 0), "", "128x128"),
    ("d2_128x128", "dgrad", (250, 16, 16, 128, 32, 3, 2, 1), "r", "128x128"),
    ("d1_128x256", "dgrad", (129, 16, 16, 256, 32, 1, 1, 0), "r", "128x256_K16"),
    ("d2_128x256", "dgrad", (129, 16, 16, 256, 32, 3, 2, 1), "r", "128x256_K16"),
    ("d1_256x64_2x2", "dgrad", (6, 2, 2, 64, 64, 3, 1, 1), "", "256x64_K16"),
    ("d1_256x64_1x1", "dgrad", (3, 1, 1, 64, 32, 3, 1, 1), "r", "256x64_K16"),
    ("d2_256x64", "dgrad", (7, 9, 9, 48, 64, 3, 2, 1), "r", "256x64_K16"),
    ("m1_64x64", "dgrad_masked", (3, 9, 7, 96, 32, 3, 1, 1), "r", "64x64"),
    ("m1_256x64", "dgrad_masked", (5, 8, 8, 64, 64, 3, 1, 1), "r", "256x64_K16"),
    ("m2_128x256", "dgrad_masked", (129, 16, 16, 256, 64, 1, 2, 0), "r", "128x256_K16"),
    ("m2_128x64", "dgrad_masked", (103, 15, 15, 160, 32, 3, 2, 1), "r", "128x64"),
]
_SPLIT_FWD = [("fwd", (3, 9, 7, 32, 44, 3, 1, 1), "arR", "c64"), ("fwd", (5, 9, 9, 64, 200, 3, 2, 1), "ar", "c128"),
              ("dgrad", (3, 9, 7, 64, 32, 3, 1, 1), "r", "c64"), ("dgrad", (4, 9, 9, 136, 64, 3, 1, 1), "", "c128"),
              ("dgrad", (3, 15, 15, 48, 64, 3, 2, 1), "", "c64"), ("dgrad", (5, 16, 16, 132, 32, 1, 2, 0), "r", "c128")]
_SPLIT_POS = [("hwnc", (140, 2, 2, 32, 64, 3, 1, 1), "aR", "c64"), ("hwnc", (300, 3, 3, 64, 256, 3, 1, 1), "ar", "c128")]


def _split_rows(modes, shapes, tag=""):
    return [(f"{e}{'s' + str(shape[6]) if e == 'dgrad' else ''}_{m}{tag}_{c}_{i}", f"{e}:{m}", shape, epi, c)
            for m in modes for i, (e, shape, epi, c) in enumerate(shapes)]


DEFAULT += _split_rows(("bf16", "f16", "x3", "x6"), _SPLIT_FWD) + _split_rows(("x3", "x6"), _SPLIT_POS)
DEFAULT += [
    ("s_h16_c64", "stats:h16", (3, 9, 7, 32, 44, 3, 1, 1), "", "c64"),
    ("s_h16_c128", "stats:h16", (5, 9, 9, 64, 200, 3, 2, 1), "", "c128"),
] + _split_rows(("h16",), _SPLIT_FWD[2:])

# the tiles the default selection can return, per exact-fp32 entry point
REACHABLE = {
    "fwd": {"64x64", "128x64", "128x128", "128x256_K16", "256x64_K16", "pos:256x64_K16", "pos:128x128_K16", "pos:128x256_K16"},
    "hwnc": {"pos:256x64_K16", "pos:128x128_K16", "pos:128x256_K16"},
    "ring": {"pos:128x64_K16"},
    "stats": {"64x64", "128x64", "128x128", "128x256_K16", "256x64_K16"},
    "dgrad": {"64x64", "128x64", "128x128", "128x256_K16", "256x64_K16"},
}

# ---- switch sets: together they reach every tile the default selection never picks.  Setting SSAD_CONV64_VARIANT at all turns
# the ring special case off, so the ring variants run in sets without it; SSAD_CONV128_VARIANT = 1 / 2 / 7 return before the
# wide-tile test; 256 x 256 is position-major only ----
SWITCH_SETS = {
    "conv64_sb_conv128_256x128_split0": (
        {"SSAD_CONV64_VARIANT": "2", "SSAD_CONV128_VARIANT": "1", "SSAD_X3_VARIANT": "0", "SSAD_X6_VARIANT": "0"}, [
            ("f_256x64_sb", "fwd", (7, 9, 9, 32, 42, 3, 2, 1), "arR", "256x64_SB"),
            ("h_256x64_sb", "hwnc", (150, 4, 4, 32, 64, 3, 1, 1), "ar", "pos:256x64_SB"),
            ("r_256x64_sb", "ring", (200, 8, 8, 32, 64, 3, 1, 1), (2, 5), "pos:256x64_SB"),   # no ring special case
            ("d2_256x64_sb", "dgrad", (7, 9, 9, 48, 64, 3, 2, 1), "r", "256x64_SB"),
            ("f_256x128", "fwd", (103, 15, 15, 32, 160, 3, 1, 1), "aR", "256x128"),
            ("h_256x128", "hwnc", (300, 2, 2, 32, 256, 3, 1, 1), "arR", "pos:256x128"),
            ("d2_256x128", "dgrad", (103, 15, 15, 160, 32, 3, 2, 1), "r", "256x128"),
            ("s_256x128", "stats", (129, 16, 16, 64, 256, 1, 1, 0), "", "256x128"),
        ] + _split_rows(("x3", "x6"), _SPLIT_FWD + _SPLIT_POS, "v0")),
    "conv64_128x64_conv128_w4": (
        {"SSAD_CONV64_VARIANT": "0", "SSAD_CONV128_VARIANT": "2"}, [
            ("f_128x64_c64", "fwd", (7, 9, 9, 32, 42, 3, 2, 1), "arR", "128x64"),
            ("fp_128x64", "fwd", (130, 2, 2, 64, 64, 3, 1, 1), "ar", "pos:128x64"),
            ("d1_128x64_c64", "dgrad", (6, 2, 2, 64, 64, 3, 1, 1), "r", "128x64"),
            ("f_256x128_w4", "fwd", (257, 32, 32, 32, 130, 1, 2, 0), "aR", "256x128_W4"),
            ("h_256x128_w4", "hwnc", (200, 2, 2, 32, 100, 3, 1, 1), "ar", "pos:256x128_W4"),
            ("d2_256x128_w4", "dgrad", (250, 16, 16, 128, 32, 3, 2, 1), "", "256x128_W4"),
            ("m1_256x128_w4", "dgrad_masked", (103, 15, 15, 160, 32, 3, 1, 1), "r", "256x128_W4"),
        ]),
    "ring_sb_conv128_256x256": (
        {"SSAD_CONV_RING_VARIANT": "1", "SSAD_CONV128_VARIANT": "6"}, [
            ("r_128x64_sb", "ring", (200, 8, 8, 32, 64, 3, 1, 1), (2, 5), "pos:128x64_SB"),
            ("r_128x64_sb_c38", "ring", (130, 6, 6, 64, 38, 3, 1, 1), (1, 4), "pos:128x64_SB"),
            # 4 sample groups of 256 (the last one 132 samples) x 64 positions, 1 x 1 filters
            ("h_256x256", "hwnc", (900, 8, 8, 32, 256, 1, 1, 0), "arR", "pos:256x256"),
            ("f_256x256_fallback", "fwd", (129, 16, 16, 64, 256, 1, 1, 0), "a", "128x256_K16"),   # pixel-major: never 256 x 256
        ]),
    "ring_k32_wide_k32_pos_k32": (
        {"SSAD_CONV_RING_VARIANT": "3", "SSAD_CONV256_K16": "0", "SSAD_CONV128_K16": "0"}, [
            ("r_128x64_k32", "ring", (200, 8, 8, 32, 64, 3, 1, 1), (2, 5), "pos:128x64"),
            ("f_128x256_k32", "fwd", (129, 16, 16, 64, 256, 1, 1, 0), "arR", "128x256"),
            ("h_128x256_k32", "hwnc", (4200, 4, 4, 32, 512, 3, 2, 1), "ar", "pos:128x256"),
            ("d2_128x256_k32", "dgrad", (129, 16, 16, 256, 32, 3, 2, 1), "r", "128x256"),
            ("h_128x128_k32", "hwnc", (300, 4, 4, 32, 128, 1, 2, 0), "aR", "pos:128x128"),
            ("fp_128x128_k32", "fwd", (200, 2, 2, 32, 100, 3, 1, 1), "R", "pos:128x128"),
        ]),
    "conv128_k16": (
        {"SSAD_CONV128_VARIANT": "7"}, [
            ("f_128x128_k16", "fwd", (257, 32, 32, 32, 130, 1, 2, 0), "arR", "128x128_K16"),
            ("f_128x128_k16_small", "fwd", (3, 9, 7, 32, 96, 3, 1, 1), "a", "128x128_K16"),   # before the small-grid tests
            ("d2_128x128_k16", "dgrad", (129, 16, 16, 256, 32, 3, 2, 1), "r", "128x128_K16"),
            ("s_128x128_k16", "stats", (103, 15, 15, 32, 160, 3, 1, 1), "", "128x128_K16"),
        ]),
}
SWITCHES = ("SSAD_CONV64_VARIANT", "SSAD_CONV128_VARIANT", "SSAD_CONV128_K16", "SSAD_CONV256_K16", "SSAD_CONV_RING_VARIANT",
            "SSAD_CONV_WIDE_GRID", "SSAD_CONV_SMALL_GRID", "SSAD_CONV_TINY_GRID", "SSAD_X3_VARIANT", "SSAD_X6_VARIANT",
            "SSAD_POS_LPT", "SSAD_POS_CHUNK", "SSAD_POS_XCD_WGS", "SSAD_CONV_LDS_PAD_64", "SSAD_CONV_LDS_PAD_128")


def rows_of(name):
    return DEFAULT if name == "default" else SWITCH_SETS[name][1]


def child_env(name):
    """The environment of a child process running switch set `name`: every tile switch cleared, then the set's own."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if name != "default":
        env.update(SWITCH_SETS[name][0])
    return env


def run_child(name, tiles_only, timeout):
    """One switch set in a fresh interpreter -> (returncode, stdout + stderr, [[row id, entry, tile], ...] or None)."""
    args = [sys.executable, os.path.abspath(__file__), name] + (["--tiles-only"] if tiles_only else [])
    r = subprocess.run(args, env=child_env(name), cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    tiles = None
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            tiles = json.loads(line)["tiles"]
    return r.returncode, r.stdout + r.stderr, tiles


# ---- tile selection ----
def selected_tile(row):
    """The tile the row's launch selects: ssad_conv_igemm_tile_id for the exact-fp32 entry points; for the 16-bit / split-bf16 forms
    the dispatcher's branch on the launch's output channels (Cout of a forward conv, Cin of an input gradient)."""
    from self_supervised import ops
    rid, entry, (n, h, w, cin, cout, k, s, p), epi, want = row
    if ":" in entry:
        return "c64" if (cin if entry.startswith("dgrad") else cout) <= 64 else "c128"
    mode = {"fwd": ops.IGEMM_FWD, "hwnc": ops.IGEMM_HWNC, "ring": ops.IGEMM_RING, "stats": ops.IGEMM_STATS,
            "dgrad": ops.IGEMM_DGRAD, "dgrad_masked": ops.IGEMM_DGRAD}[entry]
    name, pos = ops.igemm_tile(n, h, w, cin, cout, k, k, s, p, mode)
    return ("pos:" if pos else "") + name


def check_tile(row):
    got = selected_tile(row)
    assert got == row[4], f"row {row[0]} ({row[1]} {row[2]}): expected tile {row[4]}, the dispatch selects {got}"
    return got


# ---- the GPU comparison ----
# relative to max|want| (h16: absolute, 2e-3 * max(1, max|want|): one half ulp of the largest value, twice -- test_hip_half.py).
# exact fp32 2e-5 and split bf16x3 2e-5 / bf16x6 5e-6 are the bars of test_hip_parity.py / test_hip_x3.py.  bf16 / fp16 operands
# are compared with float64 over the SAME rounded operands (their products are exact in fp32), so they hold the fp32 bar too.
# Measured on the MI355X over the default rows: exact fp32 <= 9.6e-7, bf16 / fp16 operands <= 3.8e-7, bf16x3 <= 4.9e-6,
# bf16x6 <= 6.7e-7, half tensors <= 1.9e-3 absolute.
TOL = {"": 2e-5, "bf16": 2e-5, "f16": 2e-5, "x3": 2e-5, "x6": 5e-6, "h16": 2e-3}
STATS_TOL = 1e-5                    # the bar of test_large_grid_conv_dgrad_wgrad
GUARD = 1 << 16                     # elements of the guard region behind every tensor
SENTINEL = -12288.0                 # (exact in fp16 too)


def _guarded(t, fill=float("nan")):
    """t copied into the front of a larger allocation whose tail (GUARD elements) holds `fill`: reads past the end of t land there."""
    big = torch.full((t.numel() + GUARD,), fill, dtype=t.dtype, device=t.device)
    big[:t.numel()] = t.reshape(-1)
    return big[:t.numel()].view(t.shape)


def _poisoned(shape, dtype, dev):
    """(output view filled with NaN, the guard region behind it, holding SENTINEL)."""
    numel = 1
    for d in shape:
        numel *= d
    big = torch.full((numel + GUARD,), float("nan"), dtype=dtype, device=dev)
    big[numel:] = SENTINEL
    return big[:numel].view(shape), big[numel:]


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-12)


def _rounded(t, mode):
    """The operand values the kernel multiplies: bf16 / fp16 modes round them while loading, h16 stores them as halves."""
    return t.bfloat16().double() if mode == "bf16" else t.half().double() if mode in ("f16", "h16") else t.double()


def run_row(row, dev):
    """Run one row through the ops wrapper and through the C entry point into a poisoned buffer; compare with float64."""
    import torch.nn.functional as F
    from self_supervised import ops, _hip
    lib = _hip.lib()
    rid, entry, (n, h, w, cin, cout, k, s, p), epi, _ = row
    base, _, mode = entry.partition(":")
    ring, dgrad, hw = base == "ring", base.startswith("dgrad"), base in ("hwnc", "ring")
    has_a, has_r, relu = (True, True, True) if ring else ("a" in epi, "r" in epi, "R" in epi)
    g = torch.Generator().manual_seed(sum(map(ord, rid)))
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    x = torch.randn(n, h, w, cin, generator=g)                                  # NHWC
    wt = torch.randn(cout, k, k, cin, generator=g) / (cin * k * k) ** 0.5        # OHWI
    oihw = lambda t: t.permute(0, 3, 1, 2)
    if not dgrad:
        want = F.conv2d(oihw(_rounded(x, mode)), oihw(_rounded(wt, mode)), None, s, p).permute(0, 2, 3, 1)
        oshape = (n, ho, wo, cout)
    else:
        dy = torch.randn(n, ho, wo, cout, generator=g)
        want = torch.nn.grad.conv2d_input((n, cin, h, w), oihw(_rounded(wt, mode)), oihw(_rounded(dy, mode)), s, p).permute(0, 2, 3, 1)
        oshape = (n, h, w, cin)
    sc = torch.rand(cout, generator=g) + 0.5 if has_a else None
    sh = torch.randn(cout, generator=g) if has_a else None
    res = torch.randn(oshape, generator=g) if has_r else None
    mask = torch.randint(0, 16, oshape[:3] + (oshape[3] // 4,), generator=g, dtype=torch.uint8) if base == "dgrad_masked" else None
    if has_a:
        want = want * sc.double() + sh.double()
    if has_r:
        r = _rounded(res, mode) if mode == "h16" else res.double()
        if mask is not None:
            r = r * torch.stack([(mask >> b) & 1 for b in range(4)], -1).reshape(oshape).double()
        want = want + r
    if relu:
        want = want.relu()
    tdt = torch.float16 if mode == "h16" else torch.float32
    lay = (lambda t: t.permute(1, 2, 0, 3)) if hw else (lambda t: t)          # NHWC -> [H][W][N][C]
    G = lambda t: None if t is None else _guarded(lay(t).contiguous().to(dev, tdt))
    P = lambda t: None if t is None else t.data_ptr()
    wd = _guarded(wt.to(dev, tdt))
    st = _hip.stream()
    if base in ("fwd", "hwnc", "ring"):
        xd, rd = G(x), G(res)
        scd, shd = (_guarded(sc.to(dev)), _guarded(sh.to(dev))) if has_a else (None, None)
        if ring:
            lo, hi = epi
            got = ops.conv_fwd_hwnc_ring(xd, wd, scd, shd, rd, relu, lo, hi)
        elif hw:
            got = ops.conv_fwd_hwnc(xd, wd, scd, shd, rd, relu, s, p, x3={"": False, "x3": 3, "x6": 6}[mode])
        else:
            got = ops.conv_fwd(xd, wd, scd, shd, rd, relu, s, p, {"": False, "bf16": True, "f16": 2, "x3": 3, "x6": 6}[mode])
        out, guard = _poisoned(tuple(got.shape), torch.float32, dev)
        args = (P(xd), P(wd), P(out), P(scd), P(shd), P(rd), int(relu), n, h, w, cin, cout, k, k, s, p)
        if ring:
            _hip.check(lib.ssad_conv_igemm_fwd_hwnc_ring(*args, lo, hi, st))
        elif mode in ("x3", "x6"):
            _hip.check(getattr(lib, "ssad_conv_igemm_fwd_" + mode)(*args, int(hw), st))
        else:
            fn = {"": lib.ssad_conv_igemm_fwd_hwnc if hw else lib.ssad_conv_igemm_fwd, "bf16": lib.ssad_conv_igemm_fwd_bf16,
                  "f16": lib.ssad_conv_igemm_fwd_f16}[mode]
            _hip.check(fn(*args, st))
        torch.cuda.synchronize()
        got_n, out_n = got.cpu(), out.cpu()
        if hw:
            got_n, out_n = got_n.permute(2, 0, 1, 3), out_n.permute(2, 0, 1, 3)
        if ring:
            inner = torch.zeros(h, w, dtype=torch.bool)
            inner[lo:hi + 1, lo:hi + 1] = True
            assert torch.isnan(out_n[:, inner]).all(), f"{rid}: the ring launch wrote inside the skipped square"
            got_n, out_n, want = got_n[:, ~inner], out_n[:, ~inner], want[:, ~inner]
    elif base == "stats":
        h16 = mode == "h16"
        xd = G(x)
        rm, rv = torch.randn(cout, generator=g).to(dev), (torch.rand(cout, generator=g) + 0.5).to(dev)
        rm0, rv0 = rm.cpu().double(), rv.cpu().double()
        rm2, rv2 = rm.clone(), rv.clone()
        got, mean, invstd = ops.conv_fwd_stats(xd, wd, 1e-5, 0.1, rm, rv, s, p, bf16=2 if h16 else False)
        out, guard = _poisoned(tuple(got.shape), tdt, dev)
        mean2, inv2 = torch.full_like(mean, float("nan")), torch.full_like(invstd, float("nan"))
        ws = torch.full((lib.ssad_conv_stats_workspace(n, ho, wo, cout),), float("nan"), device=dev, dtype=torch.float64)
        geo = (n, h, w, cin, cout, k, k, s, p)
        if h16:
            _hip.check(lib.ssad_conv_igemm_fwd_stats_h(P(xd), P(wd), P(out), *geo, 1e-5, 0.1, P(mean2), P(inv2), P(rm2), P(rv2),
                                                       P(ws), st))
        else:
            _hip.check(lib.ssad_conv_igemm_fwd_stats(P(xd), P(wd), P(out), *geo, 0, 1e-5, 0.1, P(mean2), P(inv2), P(rm2), P(rv2),
                                                     P(ws), st))
        torch.cuda.synchronize()
        assert torch.equal(mean2, mean) and torch.equal(inv2, invstd) and torch.equal(rm2, rm) and torch.equal(rv2, rv), \
            f"{rid}: statistics differ between the wrapper and the direct call"
        # statistics of the conv output (of the STORED halves in the half-tensor form) against float64
        zc = (got.cpu().double() if h16 else want).reshape(-1, cout)
        m64, v64, cnt, zmax = zc.mean(0), zc.var(0, unbiased=False), zc.shape[0], max(1.0, zc.abs().max().item())
        em = (mean.cpu().double() - m64).abs().max().item()
        assert em < STATS_TOL * zmax, f"{rid}: mean off by {em:.3e}"
        assert _rel(invstd, (v64 + 1e-5).rsqrt()) < STATS_TOL, f"{rid}: invstd"
        erm = (rm.cpu().double() - (0.9 * rm0 + 0.1 * m64)).abs().max().item()
        assert erm < STATS_TOL * zmax, f"{rid}: running mean off by {erm:.3e}"
        assert _rel(rv, 0.9 * rv0 + 0.1 * v64 * cnt / (cnt - 1)) < STATS_TOL, f"{rid}: running var"
        got_n, out_n = got.cpu(), out.cpu()
    else:
        dyd, rd = G(dy), G(res)
        wf = _guarded(ops.flip_transpose_weight(wt.to(dev)).to(tdt))
        md = _guarded(mask.to(dev), 0) if mask is not None else None
        got = ops.conv_dgrad(dyd, wf, (n, h, w, cin), s, p, rd, {"": False, "bf16": True, "f16": 2, "x3": 3, "x6": 6, "h16": 2}[mode],
                             md)
        out, guard = _poisoned(tuple(got.shape), tdt, dev)
        geo = (n, ho, wo, cout, h, w, cin, k, k, s, p)
        if mask is not None:
            _hip.check(lib.ssad_conv_igemm_dgrad_masked(P(dyd), P(wf), P(out), P(rd), P(md), *geo, st))
        else:
            fn = {"": lib.ssad_conv_igemm_dgrad, "bf16": lib.ssad_conv_igemm_dgrad_bf16, "f16": lib.ssad_conv_igemm_dgrad_f16,
                  "x3": lib.ssad_conv_igemm_dgrad_x3, "x6": lib.ssad_conv_igemm_dgrad_x6, "h16": lib.ssad_conv_igemm_dgrad_h}[mode]
            _hip.check(fn(P(dyd), P(wf), P(out), P(rd), *geo, st))
        torch.cuda.synchronize()
        got_n, out_n = got.cpu(), out.cpu()
    assert not torch.isnan(out_n).any(), f"{rid}: {int(torch.isnan(out_n).sum())} output elements left unwritten (NaN)"
    assert torch.equal(out_n, got_n), f"{rid}: the direct call into a poisoned buffer differs from the wrapper's result"
    assert (guard.cpu().float() == SENTINEL).all(), f"{rid}: the launch wrote past the end of its output"
    if mode == "h16":
        err = (got_n.double() - want).abs().max().item()
        assert err <= TOL[mode] * max(1.0, want.abs().max().item()), f"{rid}: max err {err:.3e} (half outputs)"
        return err
    e = _rel(got_n, want)
    assert e < TOL[mode], f"{rid}: relative error {e:.3e} >= {TOL[mode]} against float64"
    return e


def _main(argv):
    name, tiles_only = argv[0], "--tiles-only" in argv
    for q in (ROOT, PKG):
        if q not in sys.path:
            sys.path.insert(0, q)
    if not tiles_only:
        assert torch.cuda.is_available(), "the kernel rows need the MI355X"
    seen = []
    for row in rows_of(name):
        seen.append([row[0], row[1], check_tile(row)])
        if not tiles_only:
            print(f"ok {row[0]} err {run_row(row, torch.device('cuda:0')):.2e}", flush=True)
    print(json.dumps({"set": name, "tiles": seen}), flush=True)


if __name__ == "__main__":
    _main(sys.argv[1:])
