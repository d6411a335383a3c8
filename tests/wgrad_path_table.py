"""The weight-gradient path table: every kernel and instantiation ops.conv_wgrad and ops.stem_wgrad can launch, at shapes that land on
each of them, with the path, instantiation and split count each row must select, and the comparison of every element of the
gradient against float64 torch on the CPU.

Shared by tests/test_wgrad_path_table.py (selection only, no GPU) and tests/test_hip_wgrad_paths.py (the kernels).  Most switches
(SSAD_WGRAD_HALO_S2, SSAD_WGRAD_G16, ...) are read once per process, so each switch set runs in a child process of its own:

    python tests/wgrad_path_table.py SET [--tiles-only]

runs SET's rows, prints one JSON line {"set": ..., "tiles": [[row id, entry, [path, instantiation, splits]], ...]} and exits non-zero on
the first mismatch (the protocol of tests/igemm_tile_table.py).

Row: (id, entry, shape, mode, flags, expected path, expected instantiation, expected splits).
  entry "conv": ops.conv_wgrad, shape = the FORWARD conv's (n, h, w, cin, cout, k, stride, pad): x [n][h][w][cin], dy [n][ho][wo][cout]
  entry "stem": ops.stem_wgrad, shape = (b, h, w) of the NCHW images
  mode: f32, bf16 / f16 (fp32 tensors, operands rounded while staged), x3, x6 (force_x6), x6t (bf16x6 training: no force_x6, so the
        exact fp32 kernels), h16 (dy / x -- the stem's dz -- stored as halves)
  flags: a = accumulate into a prefilled gradient, o = to_oihw
Paths and instantiations: ops.wgrad_path / ops.stem_wgrad_path.  splits = the slab count the reduction sums (0: linear_small writes
the gradient directly).
"""
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "self-supervised-anomaly-detection_amd")


def _resnet18_rows(tag, n, size, mode="f32"):
    """The conv layers of a ResNet-18 training step on n images of size x size (after the stem and the max-pool: size / 4)."""
    s = size // 4
    rows = [(f"{tag}_l1", (n, s, s, 64, 64, 3, 1, 1))]
    for i, c in enumerate((128, 256, 512)):
        h = s >> i
        rows += [(f"{tag}_l{i + 2}_s2", (n, h, h, c // 2, c, 3, 2, 1)), (f"{tag}_l{i + 2}_ds", (n, h, h, c // 2, c, 1, 2, 0)),
                 (f"{tag}_l{i + 2}", (n, h // 2, h // 2, c, c, 3, 1, 1))]
    return [(rid, "conv", shape, mode, "") for rid, shape in rows]


# ---- the default selection (no switch set); the expected (path, instantiation, splits) follow each row ----
DEFAULT = [
    # generic split kernel, exact fp32: BT 64 / 128, both choose_splits branches (max_splits = ceil(M / 256) < 16: the "tiny" branch)
    ("g_f32_c32_ragged", "conv", (3, 9, 7, 32, 96, 3, 1, 1), "f32", "", "generic_f32", "BT64", 1),       # M = 189, Cin 32
    ("g_f32_c160", "conv", (4, 12, 12, 160, 160, 3, 1, 1), "f32", "o", "generic_f32", "BT128", 3),       # Cin / Cout 160: ragged tiles
    ("g_f32_c96_s2_odd", "conv", (5, 15, 15, 96, 64, 3, 2, 1), "f32", "a", "generic_f32", "BT64", 2),
    ("g_f32_cost_c96", "conv", (20, 16, 16, 96, 32, 3, 1, 1), "f32", "", "generic_f32", "BT64", 8),      # cost model (max_splits 20)
    ("g_f32_cost_c160", "conv", (64, 16, 16, 160, 192, 3, 2, 1), "f32", "", "generic_f32", "BT128", 16),   # cost model, stride 2
    # M = 4100, 16 splits of 288 pixels (257 rounded up to 32): split 15 starts past M, an empty split
    ("g_f32_empty_split", "conv", (41, 10, 10, 32, 64, 3, 1, 1), "f32", "", "generic_f32", "BT64", 16),
    ("g_f32_ds", "conv", (8, 16, 16, 64, 128, 1, 2, 0), "f32", "o", "generic_f32", "BT64", 2),             # 1 x 1 stride-2 downsample
    ("g_f32_ds_odd", "conv", (6, 15, 15, 160, 192, 1, 2, 0), "f32", "", "generic_f32", "BT128", 2),
    ("g_f32_1x1map", "conv", (6, 1, 1, 64, 96, 3, 1, 1), "f32", "", "generic_f32", "BT64", 1),            # only the centre tap sees x
    ("g_f32_2x2map", "conv", (8, 2, 2, 160, 128, 3, 1, 1), "f32", "a", "generic_f32", "BT128", 1),
    ("g_f32_h5w11", "conv", (3, 5, 11, 32, 64, 3, 1, 1), "f32", "", "generic_f32", "BT64", 1),            # H != W
    ("g_f32_n1", "conv", (1, 9, 9, 32, 32, 3, 1, 1), "f32", "o", "generic_f32", "BT64", 1),
    ("g_f32_head_m513", "conv", (513, 1, 1, 512, 512, 1, 1, 0), "f32", "", "generic_f32", "BT128", 3),     # just past linear_small
    ("g_f32_cls_m513", "conv", (513, 1, 1, 512, 4, 1, 1, 0), "f32", "a", "generic_f32", "BT64", 3),        # the classifier, Cout 4
    ("g_x6t_c96", "conv", (3, 9, 7, 32, 96, 3, 1, 1), "x6t", "", "generic_f32", "BT64", 1),
    # the 16-bit and split-bf16 forms of the generic kernel, both channel tiles
    ("g_bf16_64", "conv", (3, 9, 7, 32, 96, 3, 1, 1), "bf16", "", "generic_bf16", "BT64", 1),
    ("g_bf16_128", "conv", (4, 6, 6, 160, 192, 1, 1, 0), "bf16", "o", "generic_bf16", "BT128", 1),
    ("g_bf16_s2", "conv", (64, 16, 16, 96, 128, 3, 2, 1), "bf16", "", "generic_bf16", "BT128", 16),
    ("g_f16_64", "conv", (3, 9, 7, 32, 96, 3, 1, 1), "f16", "a", "generic_f16", "BT64", 1),
    ("g_f16_128", "conv", (4, 6, 6, 160, 192, 1, 1, 0), "f16", "", "generic_f16", "BT128", 1),
    ("g_x3_64", "conv", (3, 9, 7, 32, 96, 3, 1, 1), "x3", "", "generic_x3", "BT64", 1),
    ("g_x3_128", "conv", (4, 6, 6, 160, 192, 1, 1, 0), "x3", "o", "generic_x3", "BT128", 1),
    ("g_x3_s2_odd", "conv", (5, 15, 15, 96, 64, 3, 2, 1), "x3", "", "generic_x3", "BT64", 2),
    ("g_x3_halo_shape", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "x3", "", "generic_x3", "BT64", 2),      # no halo form for x3
    ("g_x6_64", "conv", (3, 9, 7, 32, 96, 3, 1, 1), "x6", "a", "generic_x6", "BT64", 1),
    ("g_x6_128", "conv", (4, 6, 6, 160, 192, 1, 1, 0), "x6", "", "generic_x6", "BT128", 1),
    ("g_x6_halo_shape", "conv", (2, 9, 9, 128, 128, 3, 1, 1), "x6", "", "generic_x6", "BT128", 1),
    # fp32 halo tiles: stride 1 (4 x 16 when W > 8, else 8 x 8), stride 2 (4 x 8)
    ("halo_s1_4x16", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "4x16", 1),
    ("halo_s1_w9", "conv", (2, 9, 9, 128, 64, 3, 1, 1), "f32", "o", "halo_s1", "4x16", 1),             # W = 9: the 4 x 16 side
    ("halo_s1_8x8", "conv", (3, 8, 8, 64, 128, 3, 1, 1), "f32", "a", "halo_s1", "8x8", 1),              # W = 8: the 8 x 8 side
    ("halo_s1_h6w20", "conv", (2, 6, 20, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "4x16", 2),
    ("halo_s1_1x1", "conv", (5, 1, 1, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "8x8", 1),
    ("halo_s1_2x2_n1", "conv", (1, 2, 2, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "8x8", 1),
    ("halo_s1_many", "conv", (48, 16, 16, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "4x16", 48),
    ("halo_s2_even", "conv", (4, 16, 16, 64, 128, 3, 2, 1), "f32", "", "halo_s2", "4x8", 1),
    ("halo_s2_odd", "conv", (3, 15, 15, 128, 128, 3, 2, 1), "f32", "o", "halo_s2", "4x8", 1),
    ("halo_s2_h17w10", "conv", (2, 17, 10, 64, 64, 3, 2, 1), "f32", "a", "halo_s2", "4x8", 1),
    ("halo_s2_2x2", "conv", (6, 2, 2, 64, 64, 3, 2, 1), "f32", "", "halo_s2", "4x8", 1),
    # 16-bit operands on fp32 tensors, halo tiles (stride 1)
    ("halo16_bf16_4x16", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "bf16", "", "halo16_bf16", "4x16", 1),
    ("halo16_bf16_8x8", "conv", (3, 8, 8, 64, 128, 3, 1, 1), "bf16", "a", "halo16_bf16", "8x8", 1),
    ("halo16_f16_4x16", "conv", (2, 9, 9, 128, 64, 3, 1, 1), "f16", "o", "halo16_f16", "4x16", 1),
    ("halo16_f16_8x8", "conv", (5, 1, 1, 64, 64, 3, 1, 1), "f16", "", "halo16_f16", "8x8", 1),
    ("g_bf16_s2_halo_shape", "conv", (4, 16, 16, 64, 128, 3, 2, 1), "bf16", "", "generic_bf16", "BT64", 1),   # stride 2: no halo16
    # half tensors: g16 (3 x 3 / pad 1, stride 1 and 2), generic f16_h otherwise
    ("g16_s1_4x16", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "h16", "", "g16_s1", "4x16", 1),
    ("g16_s1_8x8", "conv", (3, 8, 8, 64, 128, 3, 1, 1), "h16", "a", "g16_s1", "8x8", 1),
    ("g16_s1_many", "conv", (40, 16, 16, 64, 64, 3, 1, 1), "h16", "", "g16_s1", "4x16", 40),
    ("g16_s2_2x16", "conv", (2, 20, 20, 64, 128, 3, 2, 1), "h16", "o", "g16_s2", "2x16", 2),
    ("g16_s2_4x8", "conv", (3, 15, 15, 64, 64, 3, 2, 1), "h16", "", "g16_s2", "4x8", 1),
    ("g16_s2_h17w10", "conv", (2, 17, 10, 128, 64, 3, 2, 1), "h16", "", "g16_s2", "4x8", 1),
    ("f16h_64", "conv", (3, 9, 7, 32, 96, 3, 1, 1), "h16", "", "generic_f16_h", "BT64", 1),
    ("f16h_128", "conv", (4, 6, 6, 160, 192, 1, 1, 0), "h16", "a", "generic_f16_h", "BT128", 1),
    ("f16h_ds", "conv", (8, 16, 16, 64, 128, 1, 2, 0), "h16", "", "generic_f16_h", "BT64", 2),
    # linear layers over 1 x 1 maps: the small-batch kernel up to ssad_linear_small_max_rows() rows, rounding modes 0 / 1 / 2
    ("lin_m1", "conv", (1, 1, 1, 512, 512, 1, 1, 0), "f32", "", "linear_small", "f32", 0),
    ("lin_m5_acc", "conv", (5, 1, 1, 512, 512, 1, 1, 0), "f32", "a", "linear_small", "f32", 0),
    ("lin_m33_bf16", "conv", (33, 1, 1, 512, 512, 1, 1, 0), "bf16", "", "linear_small", "bf16", 0),
    ("lin_m33_f16_acc", "conv", (33, 1, 1, 512, 512, 1, 1, 0), "f16", "a", "linear_small", "f16", 0),
    ("lin_m512", "conv", (512, 1, 1, 512, 512, 1, 1, 0), "f32", "", "linear_small", "f32", 0),
    ("lin_cls_m5", "conv", (5, 1, 1, 512, 4, 1, 1, 0), "f32", "a", "linear_small", "f32", 0),
    ("lin_m513_bf16", "conv", (513, 1, 1, 512, 512, 1, 1, 0), "bf16", "", "generic_bf16", "BT128", 3),
    # the stem (7 x 7 / 2 from the NCHW image; below 64 px through the nearest resize)
    ("stem_64", "stem", (4, 64, 64), "f32", "", "stem", "float", 32),
    ("stem_256", "stem", (2, 256, 256), "f32", "o", "stem", "float", 256),
    ("stem_70x90", "stem", (3, 70, 90), "f32", "a", "stem", "float", 54),
    ("stem_48x40", "stem", (2, 48, 40), "f32", "", "stem", "float", 16),
    ("stem_h16_64", "stem", (4, 64, 64), "h16", "", "stem", "f16", 32),
    ("stem_h16_70x90", "stem", (3, 70, 90), "h16", "oa", "stem", "f16", 54),
    ("stem_h16_32", "stem", (3, 32, 32), "h16", "", "stem", "f16", 24),
]

# The ResNet-18 layers of the 64 px and 256 px training steps (the exact fp32 step and the precision-16 step with half tensors), and
# the projection head at batch 256: every real layer's path pinned
REAL_ROWS = []
for _tag, _n, _size, _mode in (("r64", 64, 64, "f32"), ("r256", 256, 256, "f32"), ("r64h", 64, 64, "h16"), ("r256h", 256, 256, "h16")):
    REAL_ROWS += _resnet18_rows(_tag, _n, _size, _mode)
REAL_ROWS += [("r256_stem", "stem", (256, 256, 256), "f32", ""), ("r256h_stem", "stem", (256, 256, 256), "h16", ""),
              ("r256_head", "conv", (256, 1, 1, 512, 512, 1, 1, 0), "f32", ""), ("r256_cls", "conv", (256, 1, 1, 512, 4, 1, 1, 0), "f32", ""),
              ("r256h_head", "conv", (256, 1, 1, 512, 512, 1, 1, 0), "f16", "")]
# expected (path, instantiation, splits) of each real layer
REAL_EXPECT = {
    "r64_l1": ('halo_s1', '4x16', 64), "r64_l2_s2": ('halo_s2', '4x8', 16), "r64_l2_ds": ('generic_f32', 'BT64', 16),
    "r64_l2": ('halo_s1', '8x8', 16), "r64_l3_s2": ('halo_s2', '4x8', 16), "r64_l3_ds": ('generic_f32', 'BT128', 4),
    "r64_l3": ('halo_s1', '8x8', 16), "r64_l4_s2": ('halo_s2', '4x8', 8), "r64_l4_ds": ('generic_f32', 'BT128', 1),
    "r64_l4": ('halo_s1', '8x8', 4), "r256_l1": ('halo_s1', '4x16', 512), "r256_l2_s2": ('halo_s2', '4x8', 256),
    "r256_l2_ds": ('generic_f32', 'BT64', 128), "r256_l2": ('halo_s1', '4x16', 128), "r256_l3_s2": ('halo_s2', '4x8', 64),
    "r256_l3_ds": ('generic_f32', 'BT128', 128), "r256_l3": ('halo_s1', '4x16', 32), "r256_l4_s2": ('halo_s2', '4x8', 16),
    "r256_l4_ds": ('generic_f32', 'BT128', 32), "r256_l4": ('halo_s1', '8x8', 8), "r64h_l1": ('g16_s1', '4x16', 64),
    "r64h_l2_s2": ('g16_s2', '4x8', 32), "r64h_l2_ds": ('generic_f16_h', 'BT64', 16), "r64h_l2": ('g16_s1', '8x8', 16),
    "r64h_l3_s2": ('g16_s2', '4x8', 16), "r64h_l3_ds": ('generic_f16_h', 'BT128', 4), "r64h_l3": ('g16_s1', '8x8', 16),
    "r64h_l4_s2": ('g16_s2', '4x8', 16), "r64h_l4_ds": ('generic_f16_h', 'BT128', 1), "r64h_l4": ('g16_s1', '8x8', 8),
    "r256h_l1": ('g16_s1', '4x16', 512), "r256h_l2_s2": ('g16_s2', '2x16', 256), "r256h_l2_ds": ('generic_f16_h', 'BT64', 128),
    "r256h_l2": ('g16_s1', '4x16', 128), "r256h_l3_s2": ('g16_s2', '2x16', 64), "r256h_l3_ds": ('generic_f16_h', 'BT128', 128),
    "r256h_l3": ('g16_s1', '4x16', 32), "r256h_l4_s2": ('g16_s2', '4x8', 16), "r256h_l4_ds": ('generic_f16_h', 'BT128', 32),
    "r256h_l4": ('g16_s1', '8x8', 8), "r256_stem": ('stem', 'float', 512), "r256h_stem": ('stem', 'f16', 512),
    "r256_head": ('linear_small', 'f32', 0), "r256_cls": ('linear_small', 'f32', 0), "r256h_head": ('linear_small', 'f16', 0),
}
DEFAULT += [r + REAL_EXPECT[r[0]] for r in REAL_ROWS]

# every (path, instantiation) the default selection can give
REACHABLE = {
    ("generic_f32", "BT64"), ("generic_f32", "BT128"), ("generic_bf16", "BT64"), ("generic_bf16", "BT128"), ("generic_f16", "BT64"),
    ("generic_f16", "BT128"), ("generic_x3", "BT64"), ("generic_x3", "BT128"), ("generic_x6", "BT64"), ("generic_x6", "BT128"),
    ("generic_f16_h", "BT64"), ("generic_f16_h", "BT128"),
    ("halo_s1", "4x16"), ("halo_s1", "8x8"), ("halo_s2", "4x8"),
    ("halo16_bf16", "4x16"), ("halo16_bf16", "8x8"), ("halo16_f16", "4x16"), ("halo16_f16", "8x8"),
    ("g16_s1", "4x16"), ("g16_s1", "8x8"), ("g16_s2", "2x16"), ("g16_s2", "4x8"),
    ("linear_small", "f32"), ("linear_small", "bf16"), ("linear_small", "f16"),
    ("stem", "float"), ("stem", "f16"),
}
# ... and the ones only a switch set reaches
SWITCHED = {("halo_s2", "4x16"), ("halo_s2", "8x8"), ("halo16_h", "4x16"), ("halo16_h", "8x8"), ("stem", "hf")}

# ---- switch sets ----
_WGS = ("SSAD_WGRAD_HALO_WGS", "SSAD_WGRAD_G16_WGS", "SSAD_WGRAD_HALO16_WGS", "SSAD_STEM_WGRAD_BLOCKS")
SWITCH_SETS = {
    "halo_s2_tile64": ({"SSAD_WGRAD_HALO_S2_TILE": "64"}, [
        ("halo_s2_4x16", "conv", (2, 20, 20, 64, 64, 3, 2, 1), "f32", "", "halo_s2", "4x16", 1),
        ("halo_s2_4x16_odd", "conv", (3, 19, 23, 64, 128, 3, 2, 1), "f32", "a", "halo_s2", "4x16", 2),
        ("halo_s2_8x8", "conv", (3, 15, 15, 64, 128, 3, 2, 1), "f32", "o", "halo_s2", "8x8", 1),
        ("halo_s2_8x8_2x2", "conv", (6, 2, 2, 64, 64, 3, 2, 1), "f32", "", "halo_s2", "8x8", 1),
        ("halo_s1_tile64", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "4x16", 1),
    ]),
    "halo_s2_off": ({"SSAD_WGRAD_HALO_S2": "0"}, [
        ("s2off_64", "conv", (4, 16, 16, 64, 128, 3, 2, 1), "f32", "", "generic_f32", "BT64", 1),
        ("s2off_128", "conv", (3, 15, 15, 128, 128, 3, 2, 1), "f32", "o", "generic_f32", "BT128", 1),
        ("s2off_s1", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "4x16", 1),
    ]),
    "halo_off": ({"SSAD_WGRAD_HALO": "0"}, [
        ("halo_off_s1", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "f32", "a", "generic_f32", "BT64", 2),
        ("halo_off_s2", "conv", (3, 15, 15, 128, 128, 3, 2, 1), "f32", "", "generic_f32", "BT128", 1),
    ]),
    "halo16_off": ({"SSAD_WGRAD_HALO16": "0"}, [
        ("h16off_bf16", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "bf16", "", "generic_bf16", "BT64", 2),
        ("h16off_f16", "conv", (2, 8, 8, 128, 128, 3, 1, 1), "f16", "o", "generic_f16", "BT128", 1),
        ("h16off_g16", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "h16", "", "g16_s1", "4x16", 1),
    ]),
    "g16_off": ({"SSAD_WGRAD_G16": "0"}, [
        ("g16off_h16_4x16", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "h16", "", "halo16_h", "4x16", 1),
        ("g16off_h16_8x8", "conv", (3, 8, 8, 64, 128, 3, 1, 1), "h16", "a", "halo16_h", "8x8", 1),
        ("g16off_s2_64", "conv", (3, 15, 15, 64, 64, 3, 2, 1), "h16", "o", "generic_f16_h", "BT64", 1),
        ("g16off_s2_128", "conv", (2, 20, 20, 128, 128, 3, 2, 1), "h16", "", "generic_f16_h", "BT128", 1),
    ]),
    "stem16_off": ({"SSAD_STEM_WGRAD16": "0"}, [
        ("stem_hf_64", "stem", (4, 64, 64), "h16", "", "stem", "hf", 32),
        ("stem_hf_70x90", "stem", (3, 70, 90), "h16", "oa", "stem", "hf", 54),
        ("stem_hf_48x40", "stem", (2, 48, 40), "h16", "", "stem", "hf", 16),
        ("stem_f32_16off", "stem", (3, 70, 90), "f32", "", "stem", "float", 54),
    ]),
    "linear_small_off": ({"SSAD_LINEAR_SMALL": "0"}, [
        ("linoff_m1", "conv", (1, 1, 1, 512, 512, 1, 1, 0), "f32", "", "generic_f32", "BT128", 1),
        ("linoff_m5", "conv", (5, 1, 1, 512, 4, 1, 1, 0), "f32", "a", "generic_f32", "BT64", 1),
        ("linoff_m33_bf16", "conv", (33, 1, 1, 512, 512, 1, 1, 0), "bf16", "", "generic_bf16", "BT128", 1),
        ("linoff_m512_f16", "conv", (512, 1, 1, 512, 512, 1, 1, 0), "f16", "", "generic_f16", "BT128", 2),
    ]),
    # one split over all of M (generic kernels only: the halo / g16 / stem counts have switches of their own)
    "splits_1": ({"SSAD_WGRAD_SPLITS": "1"}, [
        ("sp1_f32", "conv", (41, 10, 10, 32, 64, 3, 1, 1), "f32", "", "generic_f32", "BT64", 1),
        ("sp1_f32_128", "conv", (64, 16, 16, 160, 192, 3, 2, 1), "f32", "o", "generic_f32", "BT128", 1),
        ("sp1_x3", "conv", (20, 16, 16, 96, 32, 3, 1, 1), "x3", "", "generic_x3", "BT64", 1),
        ("sp1_f16h", "conv", (8, 16, 16, 64, 128, 1, 2, 0), "h16", "a", "generic_f16_h", "BT64", 1),
        ("sp1_halo", "conv", (2, 12, 12, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "4x16", 1),
    ]),
    # a split count far above the cap: max_splits = ceil(M / 256)
    "splits_max": ({"SSAD_WGRAD_SPLITS": "100000"}, [
        ("spmax_f32", "conv", (41, 10, 10, 32, 64, 3, 1, 1), "f32", "", "generic_f32", "BT64", 17),
        ("spmax_bf16", "conv", (64, 16, 16, 96, 128, 3, 2, 1), "bf16", "", "generic_bf16", "BT128", 16),
        ("spmax_x6", "conv", (1, 181, 181, 32, 32, 1, 1, 0), "x6", "a", "generic_x6", "BT64", 128),
    ]),
    # one workgroup / slab per launch
    "wgs_1": (dict.fromkeys(_WGS, "1"), [
        ("wgs1_halo_s1", "conv", (48, 16, 16, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "4x16", 1),
        ("wgs1_halo_s2", "conv", (4, 16, 16, 64, 128, 3, 2, 1), "f32", "o", "halo_s2", "4x8", 1),
        ("wgs1_halo16", "conv", (6, 16, 16, 64, 64, 3, 1, 1), "bf16", "", "halo16_bf16", "4x16", 1),
        ("wgs1_g16_s1", "conv", (40, 16, 16, 64, 64, 3, 1, 1), "h16", "", "g16_s1", "4x16", 1),
        ("wgs1_g16_s2", "conv", (4, 20, 20, 64, 128, 3, 2, 1), "h16", "a", "g16_s2", "2x16", 1),
        ("wgs1_stem", "stem", (3, 70, 90), "f32", "", "stem", "float", 1),
        ("wgs1_stem_h16", "stem", (4, 64, 64), "h16", "", "stem", "f16", 1),
    ]),
    # split counts that are no multiple of 8, or capped by ntiles / 4 -- many trailing splits then hold no tile
    "wgs_13_max": ({"SSAD_WGRAD_HALO_WGS": "100000", "SSAD_WGRAD_G16_WGS": "13", "SSAD_WGRAD_HALO16_WGS": "100000",
                    "SSAD_STEM_WGRAD_BLOCKS": "13"}, [
        ("wgsmax_halo_s1", "conv", (13, 124, 16, 64, 64, 3, 1, 1), "f32", "", "halo_s1", "4x16", 100),   # 403 tiles of 5: 19 empty
        ("wgsmax_halo_s2", "conv", (7, 30, 30, 64, 64, 3, 2, 1), "f32", "a", "halo_s2", "4x8", 7),
        ("wgsmax_halo16", "conv", (13, 124, 16, 64, 64, 3, 1, 1), "f16", "o", "halo16_f16", "4x16", 100),
        ("wgs13_g16_s1", "conv", (40, 16, 16, 64, 64, 3, 1, 1), "h16", "", "g16_s1", "4x16", 13),
        ("wgs13_g16_s2", "conv", (5, 15, 15, 64, 64, 3, 2, 1), "h16", "", "g16_s2", "4x8", 2),        # capped: 10 tiles / 4
        ("wgs13_stem", "stem", (3, 70, 90), "f32", "a", "stem", "float", 13),
        ("wgs13_stem_small", "stem", (1, 32, 32), "h16", "", "stem", "f16", 8),                      # 8 tiles < 13
    ]),
}
SWITCHES = ("SSAD_WGRAD_HALO", "SSAD_WGRAD_HALO_S2", "SSAD_WGRAD_HALO_S2_TILE", "SSAD_WGRAD_HALO16", "SSAD_WGRAD_G16",
            "SSAD_STEM_WGRAD16", "SSAD_LINEAR_SMALL", "SSAD_WGRAD_SPLITS", "SSAD_WGRAD_BLOCKS") + _WGS

# modes -> (conv_wgrad's bf16 argument, force_x6)
MODE_ARGS = {"f32": (False, False), "bf16": (True, False), "f16": (2, False), "x3": (3, False), "x6": (6, True), "x6t": (6, False),
             "h16": (2, False)}


def rows_of(name):
    return DEFAULT if name == "default" else SWITCH_SETS[name][1]


def child_env(name):
    """The environment of a child process running switch set `name`: every wgrad switch cleared, then the set's own."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if name != "default":
        env.update(SWITCH_SETS[name][0])
    return env


def run_child(name, tiles_only, timeout):
    """One switch set in a fresh interpreter -> (returncode, stdout + stderr, [[row id, entry, [path, inst, splits]], ...] or None)."""
    args = [sys.executable, os.path.abspath(__file__), name] + (["--tiles-only"] if tiles_only else [])
    r = subprocess.run(args, env=child_env(name), cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    tiles = None
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            tiles = json.loads(line)["tiles"]
    return r.returncode, r.stdout + r.stderr, tiles


# ---- path selection ----
def conv_geometry(shape):
    n, h, w, cin, cout, k, s, p = shape
    return n, h, w, cin, cout, k, s, p, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def selected_path(row):
    """(path, instantiation, splits) the row's launch selects: ops.wgrad_path / ops.stem_wgrad_path, which the wrappers branch on."""
    from self_supervised import ops
    rid, entry, shape, mode = row[:4]
    if entry == "stem":
        b, h, w = shape
        return list(ops.stem_wgrad_path((b, 3, h, w), half=mode == "h16"))
    n, h, w, cin, cout, k, s, p, ho, wo = conv_geometry(shape)
    bf16, force = MODE_ARGS[mode]
    return list(ops.wgrad_path((n, ho, wo, cout), (n, h, w, cin), k, k, s, p, bf16=bf16, half=mode == "h16", force_x6=force))


def check_path(row):
    got = selected_path(row)
    assert got == list(row[5:8]), f"row {row[0]} ({row[1]} {row[2]} {row[3]}): expected {row[5:8]}, the dispatch selects {got}"
    return got


# ---- the GPU comparison ----
# Two bars per element, both must hold: the global one of test_hip_parity.py, |err| <= 2e-5 * max|want|, and a per-element one,
# |err_e| <= TAU * A_e with A = conv2d_weight(|x|, |dy|) in float64 (the sum of the magnitudes of the products that make up element e).
# Inputs carry per-channel scales 2^-6 .. 2^6 on dy and x, so the per-element bar holds small elements (border taps, ragged channel
# blocks, quiet channels) to their own scale.  bf16 / fp16 operands and half tensors are compared with float64 over the SAME rounded or
# stored operands (their products are exact in fp32).  Accumulate rows add the rounding of the final add: 2^-24 |prefill + want|.
TOL = 2e-5
TAU = {"f32": 1e-5, "x6t": 1e-5, "x6": 1e-5, "bf16": 1e-5, "f16": 1e-5, "h16": 1e-5, "x3": 4e-5}
GUARD = 1 << 16                     # elements of the guard region behind every tensor
SENTINEL = -12288.0


def _guarded(t, fill=float("nan")):
    """t copied into the front of a larger allocation whose tail (GUARD elements) holds `fill`: reads past the end of t land there."""
    big = torch.full((t.numel() + GUARD,), fill, dtype=t.dtype, device=t.device)
    big[:t.numel()] = t.reshape(-1)
    return big[:t.numel()].view(t.shape)


def _poisoned(numel, dev, prefill=None):
    """(flat output of numel floats -- NaN, or a copy of prefill -- , the guard region behind it, holding SENTINEL)."""
    big = torch.full((numel + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    big[numel:] = SENTINEL
    if prefill is not None:
        big[:numel] = prefill.reshape(-1)
    return big[:numel], big[numel:]


def _scaled(shape, g, cdim=-1):
    """randn with a per-channel scale 2^u, u uniform in [-6, 6] (channels along cdim)."""
    t = torch.randn(shape, generator=g)
    c = shape[cdim]
    sc = torch.exp2(torch.rand(c, generator=g) * 12 - 6)
    view = [1] * len(shape)
    view[cdim] = c
    return t * sc.view(view)


def _rounded(t, mode):
    """The operand values the kernel multiplies."""
    if mode == "bf16":
        return t.bfloat16().double()
    if mode in ("f16", "h16"):
        return t.half().double()
    return t.double()


def reference(x64, dy64, k, s, p):
    """float64 conv2d_weight of NHWC x / dy -> OHWI [cout][k][k][cin], and the same over |x|, |dy| (the per-element scale A)."""
    oihw = lambda t: t.permute(0, 3, 1, 2)
    n, h, w, cin = x64.shape
    cout = dy64.shape[-1]
    want = torch.nn.grad.conv2d_weight(oihw(x64), (cout, cin, k, k), oihw(dy64), s, p).permute(0, 2, 3, 1)
    a = torch.nn.grad.conv2d_weight(oihw(x64.abs()), (cout, cin, k, k), oihw(dy64.abs()), s, p).permute(0, 2, 3, 1)
    return want, a


def stem_reference(img64, dz64):
    import torch.nn.functional as F
    b, _, h, w = img64.shape
    src = F.interpolate(img64, (64, 64), mode="nearest") if (h < 64 or w < 64) else img64
    want, a = reference(src.permute(0, 2, 3, 1), dz64, 7, 2, 3)
    return want, a


def compare(rid, got, want, a, mode, prefill=None):
    """Both bars; -> (max |err| / max|want|, max |err_e| / A_e over elements with A_e > 0)."""
    got = got.detach().cpu().double().reshape(want.shape)
    if prefill is not None:
        pre = prefill.detach().cpu().double().reshape(want.shape)
        want = want + pre
        slack = (2.0 ** -24) * want.abs()
    else:
        slack = torch.zeros_like(want)
    assert not torch.isnan(got).any(), f"{rid}: NaN in the gradient"
    err = (got - want).abs()
    wmax = max(want.abs().max().item(), 1e-300)
    e_glob = err.max().item() / wmax
    assert e_glob <= TOL, f"{rid}: max |err| {e_glob:.3e} of max|want| > {TOL}"
    bad = err > TAU[mode] * a + slack
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{rid}: {int(bad.sum())} elements over {TAU[mode]} * A, first flat index {i}: got "
                             f"{got.reshape(-1)[i].item():.9g}, want {want.reshape(-1)[i].item():.9g}, A {a.reshape(-1)[i].item():.3e}")
    pos = a > 0
    e_el = ((err - slack).clamp(min=0)[pos] / a[pos]).max().item() if pos.any() else 0.0
    return e_glob, e_el


def _lib_call(path, mode, lib, dyd, xd, slab_p, splits, shape, st):
    """The C entry point of a slab path, as ops.conv_wgrad calls it."""
    n, h, w, cin, cout, k, s, p, ho, wo = conv_geometry(shape)
    ptr = lambda t: t.data_ptr()
    if path.startswith("g16_"):
        return lib.ssad_conv_wgrad3x3_g16_h(ptr(dyd), ptr(xd), slab_p, splits, n, ho, wo, h, w, cin, cout, s, dyd.numel(), st)
    if path == "halo16_h":
        return lib.ssad_conv_wgrad3x3_halo16_h(ptr(dyd), ptr(xd), slab_p, splits, n, h, w, cin, cout, dyd.numel(), st)
    if path == "generic_f16_h":
        return lib.ssad_conv_wgrad_f16_h(ptr(dyd), ptr(xd), slab_p, splits, n, h, w, cin, cout, k, k, s, p, dyd.numel(), st)
    if path == "halo_s1":
        return lib.ssad_conv_wgrad3x3_halo(ptr(dyd), ptr(xd), slab_p, splits, n, h, w, cin, cout, dyd.numel(), st)
    if path == "halo_s2":
        return lib.ssad_conv_wgrad3x3s2_halo(ptr(dyd), ptr(xd), slab_p, splits, n, ho, wo, h, w, cin, cout, dyd.numel(), st)
    if path.startswith("halo16_"):
        return lib.ssad_conv_wgrad3x3_halo16(ptr(dyd), ptr(xd), slab_p, splits, n, h, w, cin, cout, int(mode == "f16"), dyd.numel(),
                                             st)
    fn = {"generic_f32": lib.ssad_conv_wgrad, "generic_bf16": lib.ssad_conv_wgrad_bf16, "generic_f16": lib.ssad_conv_wgrad_f16,
          "generic_x3": lib.ssad_conv_wgrad_x3, "generic_x6": lib.ssad_conv_wgrad_x6}[path]
    return fn(ptr(dyd), ptr(xd), slab_p, splits, n, h, w, cin, cout, k, k, s, p, dyd.numel(), st)


def check_reducers(rid, slab, splits, cout, kpad, kh, kw, cin, want_ohwi, dev):
    """wgrad_reduce (forced by a dw offset by one float) == wgrad_reduce4 == wgrad_reduce_batch, bit for bit, on the same slab."""
    import ctypes
    from self_supervised import _hip
    lib, st = _hip.lib(), _hip.stream()
    kreal = kh * kw * cin
    total = cout * kreal
    big = torch.full((total + 4 + GUARD,), float("nan"), device=dev)
    one = big[1:1 + total]                                   # 4-byte aligned only: the one-float kernel
    _hip.check(lib.ssad_wgrad_reduce(slab.data_ptr(), one.data_ptr(), splits, cout, kpad, kh, kw, cin, 0, 0, st))
    outs = {"reduce1": one}
    if kreal % 4 == 0 and kpad % 4 == 0:
        four, _ = _poisoned(total, dev)
        _hip.check(lib.ssad_wgrad_reduce(slab.data_ptr(), four.data_ptr(), splits, cout, kpad, kh, kw, cin, 0, 0, st))
        bat, _ = _poisoned(total, dev)
        desc = (ctypes.c_int64 * 6)(slab.data_ptr(), bat.data_ptr(), splits, cout, kpad, kreal)
        _hip.check(lib.ssad_wgrad_reduce_batch(desc, 1, st))
        outs.update(reduce4=four, batch=bat)
    torch.cuda.synchronize()
    assert big[0].isnan() and torch.isnan(big[1 + total:]).all(), f"{rid}: the one-float reduction wrote outside its output"
    ref = outs["reduce1"].cpu()
    assert not torch.isnan(ref).any(), f"{rid}: the one-float reduction left elements unwritten"
    for name, o in outs.items():
        assert torch.equal(o.cpu(), ref), f"{rid}: {name} differs from the one-float reduction"
    if want_ohwi is not None:
        assert torch.equal(ref, want_ohwi.reshape(-1).cpu()), f"{rid}: the reducers differ from the wrapper's gradient"


def run_row(row, dev):
    """Run one row through the ops wrapper and through the C entry point into NaN slabs and a poisoned gradient; compare with float64.
    -> (max |err| / max|want|, max |err_e| / A_e)."""
    from self_supervised import ops, _hip
    lib, st = _hip.lib(), _hip.stream()
    rid, entry, shape, mode, flags, path, inst, splits = row
    acc, oihw = "a" in flags, "o" in flags
    g = torch.Generator().manual_seed(sum(map(ord, rid)))
    tdt = torch.float16 if mode == "h16" else torch.float32
    if entry == "stem":
        b, h, w = shape
        img = _scaled((b, 3, h, w), g, 1)
        _, _, _, ho, wo = ops.stem_geometry(h, w, 0, 0)
        dz = _scaled((b, ho, wo, 64), g)
        kern = row[6]
        img64 = img.half().double() if kern == "f16" else img.double()
        want, a = stem_reference(img64, _rounded(dz, mode))
        cout, k, cin, kpad = 64, 7, 3, 160
        imgd, dzd = _guarded(img.to(dev)), _guarded(dz.to(dev, tdt))
        wrapper = lambda out, o, ac: ops.stem_wgrad(imgd, dzd, out, to_oihw=o, accumulate=ac)
    else:
        n, h, w, cin, cout, k, s, p, ho, wo = conv_geometry(shape)
        x, dy = _scaled((n, h, w, cin), g), _scaled((n, ho, wo, cout), g)
        want, a = reference(_rounded(x, mode), _rounded(dy, mode), k, s, p)
        xd, dyd = _guarded(x.to(dev, tdt)), _guarded(dy.to(dev, tdt))
        bf16, force = MODE_ARGS[mode]
        wrapper = lambda out, o, ac: ops.conv_wgrad(dyd, xd, out, k, k, s, p, to_oihw=o, accumulate=ac, bf16=bf16, force_x6=force)
    total = want.numel()
    prefill = (torch.randn(total, generator=g) * want.abs().max().item()).float() if acc else None
    to_layout = (lambda t: t.permute(0, 3, 1, 2)) if oihw else (lambda t: t)
    # the wrapper, twice (determinism), and in the other layout
    got = prefill.clone().to(dev) if acc else torch.empty(total, device=dev)
    wrapper(got, oihw, acc)
    got2 = prefill.clone().to(dev) if acc else torch.empty(total, device=dev)
    wrapper(got2, oihw, acc)
    other = prefill.clone().to(dev) if acc else torch.empty(total, device=dev)
    wrapper(other, not oihw, acc)
    torch.cuda.synchronize()
    assert torch.equal(got, got2), f"{rid}: two runs differ"
    shp_ohwi, shp_oihw = (cout, k, k, cin), (cout, cin, k, k)
    if acc:      # the prefill is a flat buffer: compare gradients, i.e. the same prefill element by element in either layout
        pass
    else:
        g_ohwi = (other if oihw else got).view(shp_ohwi)
        g_oihw = (got if oihw else other).view(shp_oihw)
        assert torch.equal(g_ohwi.permute(0, 3, 1, 2), g_oihw), f"{rid}: to_oihw is not the permuted OHWI result"
    want_l = to_layout(want).contiguous()
    a_l = to_layout(a).contiguous()
    e = compare(rid, got, want_l, a_l, mode, prefill)
    if acc:
        want_o = (want if oihw else want.permute(0, 3, 1, 2)).contiguous()
        compare(rid + " (other layout)", other, want_o, (a if oihw else a.permute(0, 3, 1, 2)).contiguous(), mode, prefill)
    # the C entry point into a NaN slab, reduced into a poisoned gradient
    out, guard = _poisoned(total, dev, prefill.to(dev) if acc else None)
    slab = None
    if entry == "stem":
        ws = torch.full((lib.ssad_stem_wgrad_workspace(b, h, w),), float("nan"), device=dev)
        assert ws.numel() == splits * 64 * kpad
        fn = lib.ssad_stem_wgrad_h if mode == "h16" else lib.ssad_stem_wgrad
        _hip.check(fn(imgd.data_ptr(), dzd.data_ptr(), out.data_ptr(), b, h, w, dzd.numel(), int(oihw), int(acc), ws.data_ptr(), st))
        slab = ws
    elif path == "linear_small":
        m = n
        _hip.check(lib.ssad_linear_wgrad_small_r(dyd.data_ptr(), xd.data_ptr(), out.data_ptr(), m, cin, cout, int(acc),
                                                 {"f32": 0, "bf16": 1, "f16": 2}[mode], st))
    else:
        slab = torch.full((splits, cout, k * k * cin), float("nan"), device=dev)
        _hip.check(_lib_call(path, mode, lib, dyd, xd, slab.data_ptr(), splits, shape, st))
        _hip.check(lib.ssad_wgrad_reduce(slab.data_ptr(), out.data_ptr(), splits, cout, k * k * cin, k, k, cin, int(oihw), int(acc), st))
    torch.cuda.synchronize()
    if slab is not None:
        assert not torch.isnan(slab).any(), f"{rid}: {int(torch.isnan(slab).sum())} slab elements left unwritten (NaN)"
    assert not torch.isnan(out).any(), f"{rid}: {int(torch.isnan(out).sum())} gradient elements left unwritten (NaN)"
    assert (guard.cpu() == SENTINEL).all(), f"{rid}: the launch wrote past the end of the gradient"
    assert torch.equal(out, got), f"{rid}: the direct call into poisoned buffers differs from the wrapper's result"
    if slab is not None:
        kpad_ = kpad if entry == "stem" else k * k * cin
        check_reducers(rid, slab, splits, cout, kpad_, k, k, cin, None if (acc or oihw) else got, dev)
        # the collected reductions (ops.PENDING_REDUCE + flush_reductions) where the training step would use them
        if entry == "conv" and not acc and not oihw:
            pend = torch.empty(total, device=dev)
            ops.PENDING_REDUCE = []
            try:
                wrapper(pend, False, False)
                assert len(ops.PENDING_REDUCE) == 1, f"{rid}: the reduction was not deferred"
                ops.flush_reductions()
            finally:
                ops.PENDING_REDUCE = None
            torch.cuda.synchronize()
            assert torch.equal(pend, got), f"{rid}: the batched reduction differs from the direct one"
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
        seen.append([row[0], row[1], check_path(row)])
        if not tiles_only:
            eg, ee = run_row(row, torch.device("cuda:0"))
            print(f"ok {row[0]} {row[5]} {row[6]} err/max {eg:.2e} err/A {ee:.2e}", flush=True)
    print(json.dumps({"set": name, "tiles": seen}), flush=True)


if __name__ == "__main__":
    _main(sys.argv[1:])
