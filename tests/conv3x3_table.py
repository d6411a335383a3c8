"""The 3 x 3 / stride 1 / pad 1 convolution table: every entry point and instantiation of csrc/conv_c64.hip, csrc/conv16.hip and
csrc/conv16w.hip at the smallest shapes that reach each case, with the launch geometry each row must get (ssad_conv3x3_geometry: what
the launchers themselves compute) and the comparison of every output element against float64 torch on the CPU, over buffers that sit
between NaN guards.

Shared by tests/test_conv3x3_table.py (geometry only, no GPU) and tests/test_hip_conv3x3_paths.py (the kernels).  SSAD_CONV16W_WGS and
SSAD_CONV16_WGS are read once per process, so each switch set runs in a child process of its own:

    python tests/conv3x3_table.py SET [--geometry-only]

runs SET's rows, prints one JSON line {"set": ..., "geometry": [[row id, entry, [inst, ntiles, gx, gy, chunks, last, walk]], ...]} and
exits non-zero on the first mismatch (the protocol of tests/igemm_tile_table.py).

Row: (id, entry, (n, h, w, cin, cout), epilogue, expected geometry).
  entry  c64 / c64_bf16 / c64_f16: ssad_conv3x3_c64_op with op 0 / 1 / 2 (fp32 tensors);  c64_h: ssad_conv3x3_c64_h (half tensors);
         c64_eval: ssad_conv3x3_c64_eval;  h16: ssad_conv3x3_h;  w16 / w32: ssad_conv3x3_hw / _fw THROUGH THE C ENTRY POINT (no minimum
         amount of work there);  w32_eval: ssad_conv3x3_fw_pack_scaled + ssad_conv3x3_fw_eval
  epilogue, training entries: forms joined by "+", each a launch of its own --
         plain  conv + statistics (momentum 0.1, running statistics from non-trivial values)
         res    + residual                     mask  + residual behind a random nibble mask (one byte per channel quad)
         tr     producer BatchNorm + ReLU on load, with emit and statistics (momentum 0.3), then without emit (z bit-equal)
         dgrad  the input-gradient use: the flipped filter, Cin and Cout swapped, the identity-branch gradient as residual
         pos    plain, on non-negative inputs and a filter with a non-zero mean: |mean| / std of z about 3
     c64_eval: letters I / O / R (position-major input / output / residual), s (scale + shift), r (residual), a (ReLU)
     w32_eval: O (position-major output), s (a scale for the packer, else NULL), r (residual), a (ReLU); the shift is always there
  geometry: (instantiation id, ntiles, gx, gy, input chunks per tile, maps present in the last tile, most tiles one workgroup walks)
            -- include/ssad.h, ssad_conv3x3_geometry; written out from the documented rules, not read back from the library
"""
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "self-supervised-anomaly-detection_amd")

DEFAULT = [
    ('c64_f32_1x1x1', 'c64', (1, 1, 1, 64, 64), 'plain+mask', (816, 1, 1, 1, 1, 1, 1)),
    ('c64_f32_3x5x7', 'c64', (3, 5, 7, 64, 64), 'plain+res+mask+tr+dgrad', (816, 3, 3, 1, 1, 1, 1)),
    ('c64_f32_1x8x16', 'c64', (1, 8, 16, 64, 64), 'plain+mask', (816, 1, 1, 1, 1, 1, 1)),
    ('c64_f32_3x9x17', 'c64', (3, 9, 17, 64, 64), 'plain+res+mask+tr+dgrad', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_f32_1x12x20', 'c64', (1, 12, 20, 64, 64), 'plain+mask', (816, 4, 4, 1, 1, 1, 1)),
    ('c64_f32_3x24x24', 'c64', (3, 24, 24, 64, 64), 'tr+dgrad', (816, 18, 18, 1, 1, 1, 1)),
    ('c64_bf16_3x9x17', 'c64_bf16', (3, 9, 17, 64, 64), 'plain+res+mask+tr+dgrad', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_bf16_1x1x1', 'c64_bf16', (1, 1, 1, 64, 64), 'plain+tr', (816, 1, 1, 1, 1, 1, 1)),
    ('c64_bf16_1x12x20', 'c64_bf16', (1, 12, 20, 64, 64), 'res+mask+dgrad', (816, 4, 4, 1, 1, 1, 1)),
    ('c64_f16_3x9x17', 'c64_f16', (3, 9, 17, 64, 64), 'plain+res+mask+tr+dgrad', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_f16_1x8x16', 'c64_f16', (1, 8, 16, 64, 64), 'plain+tr', (816, 1, 1, 1, 1, 1, 1)),
    ('c64_f16_3x5x7', 'c64_f16', (3, 5, 7, 64, 64), 'res+mask+dgrad', (816, 3, 3, 1, 1, 1, 1)),
    ('c64_f32_pos', 'c64', (3, 9, 17, 64, 64), 'pos', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_h_pos', 'c64_h', (3, 9, 17, 64, 64), 'pos', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_h_1x1x1', 'c64_h', (1, 1, 1, 64, 64), 'plain+res', (816, 1, 1, 1, 1, 1, 1)),
    ('c64_h_3x5x7', 'c64_h', (3, 5, 7, 64, 64), 'plain+res+tr+dgrad', (816, 3, 3, 1, 1, 1, 1)),
    ('c64_h_1x8x16', 'c64_h', (1, 8, 16, 64, 64), 'plain+res', (816, 1, 1, 1, 1, 1, 1)),
    ('c64_h_3x9x17', 'c64_h', (3, 9, 17, 64, 64), 'plain+res+tr+dgrad', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_h_1x12x20', 'c64_h', (1, 12, 20, 64, 64), 'plain+res', (816, 4, 4, 1, 1, 1, 1)),
    ('c64_h_3x24x24', 'c64_h', (3, 24, 24, 64, 64), 'tr+dgrad', (816, 18, 18, 1, 1, 1, 1)),
    ('c64_eval_nnn_0', 'c64_eval', (3, 9, 17, 64, 64), 'sra', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_eval_nnR_1', 'c64_eval', (5, 16, 16, 64, 64), 'Rr', (816, 10, 10, 1, 1, 1, 1)),
    ('c64_eval_nOn_2', 'c64_eval', (3, 9, 17, 64, 64), 'Osra', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_eval_nOR_3', 'c64_eval', (5, 16, 16, 64, 64), 'ORra', (816, 10, 10, 1, 1, 1, 1)),
    ('c64_eval_Inn_4', 'c64_eval', (3, 9, 17, 64, 64), 'Isr', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_eval_InR_5', 'c64_eval', (5, 16, 16, 64, 64), 'IRra', (816, 10, 10, 1, 1, 1, 1)),
    ('c64_eval_IOn_6', 'c64_eval', (3, 9, 17, 64, 64), 'IOsr', (816, 12, 12, 1, 1, 1, 1)),
    ('c64_eval_IOR_7', 'c64_eval', (5, 16, 16, 64, 64), 'IORsra', (816, 10, 10, 1, 1, 1, 1)),
    ('c64_eval_bare', 'c64_eval', (5, 16, 16, 64, 64), '', (816, 10, 10, 1, 1, 1, 1)),
    ('c64_eval_no_residual', 'c64_eval', (3, 9, 17, 64, 64), 'IOsa', (816, 12, 12, 1, 1, 1, 1)),
    ('h16_64_tw8_odd', 'h16', (3, 5, 7, 64, 64), 'plain+res+tr+dgrad', (641, 2, 2, 1, 1, 1, 1)),
    ('h16_64_tw8_h13', 'h16', (1, 13, 8, 128, 192), 'plain+res+tr+dgrad', (641, 1, 1, 3, 2, 2, 1)),
    ('h16_64_tw8_n1', 'h16', (1, 8, 8, 64, 64), 'plain+tr', (641, 1, 1, 1, 1, 1, 1)),
    ('h16_128_tw8_odd', 'h16', (5, 8, 8, 128, 256), 'plain+res+tr+dgrad', (1281, 3, 3, 2, 2, 1, 1)),
    ('h16_128_tw8_h9', 'h16', (1, 9, 5, 64, 128), 'plain+res+tr+dgrad', (1281, 1, 1, 1, 1, 2, 1)),
    ('h16_64_ragged', 'h16', (2, 13, 21, 64, 64), 'plain+res+tr+dgrad', (640, 8, 8, 1, 1, 1, 1)),
    ('h16_64_c192', 'h16', (1, 9, 17, 128, 192), 'plain+res+tr+dgrad', (640, 4, 4, 3, 2, 1, 1)),
    ('h16_128_ragged', 'h16', (2, 13, 21, 128, 128), 'plain+res+tr+dgrad', (1280, 8, 8, 1, 2, 1, 1)),
    ('h16_128_c256', 'h16', (1, 9, 17, 64, 256), 'plain+res+tr', (1280, 4, 4, 2, 1, 1, 1)),
    ('h16_64_cin1024', 'h16', (1, 3, 5, 1024, 64), 'plain+tr', (641, 1, 1, 1, 16, 1, 1)),
    ('h16_128_cin1024', 'h16', (1, 9, 10, 1024, 128), 'plain+tr', (1280, 2, 2, 1, 16, 1, 1)),
    ('h16_64_pos', 'h16', (2, 13, 21, 64, 64), 'pos', (640, 8, 8, 1, 1, 1, 1)),
    ('h16_128_pos', 'h16', (3, 8, 8, 64, 128), 'pos', (1281, 2, 2, 1, 1, 1, 1)),
    ('w16_blk_1x16x32', 'w16', (1, 16, 32, 64, 128), 'plain+res+mask+tr+dgrad', (20064, 2, 2, 1, 1, 1, 1)),
    ('w16_blk_2x32x16', 'w16', (2, 32, 16, 128, 128), 'plain+res+mask+tr', (20064, 4, 4, 1, 2, 1, 1)),
    ('w16_blk_1x32x32_2slabs', 'w16', (1, 32, 32, 64, 256), 'plain+mask+tr', (20064, 4, 4, 2, 1, 1, 1)),
    ('w16_blk_2x16x32_c256', 'w16', (2, 16, 32, 256, 128), 'plain+tr+dgrad', (20064, 4, 4, 1, 4, 1, 1)),
    ('w16_blk_cin1024', 'w16', (1, 16, 16, 1024, 128), 'plain+tr', (20064, 1, 1, 1, 16, 1, 1)),
    ('w16_8x8_n1', 'w16', (1, 8, 8, 128, 128), 'plain+res+mask+tr+dgrad', (21064, 1, 1, 1, 2, 1, 1)),
    ('w16_8x8_n2', 'w16', (2, 8, 8, 128, 128), 'plain+mask+tr', (21064, 1, 1, 1, 2, 2, 1)),
    ('w16_8x8_n3', 'w16', (3, 8, 8, 64, 256), 'plain+res+mask+tr', (21064, 1, 1, 2, 1, 3, 1)),
    ('w16_8x8_n4', 'w16', (4, 8, 8, 64, 128), 'plain+tr', (21064, 1, 1, 1, 1, 4, 1)),
    ('w16_8x8_n5', 'w16', (5, 8, 8, 256, 128), 'plain+res+mask+tr+dgrad', (21064, 2, 2, 1, 4, 1, 1)),
    ('w16_8x8_n7', 'w16', (7, 8, 8, 128, 256), 'plain+res+mask+tr+dgrad', (21064, 2, 2, 2, 2, 3, 1)),
    ('w16_8x8_cin1024', 'w16', (5, 8, 8, 1024, 128), 'plain+tr', (21064, 2, 2, 1, 16, 1, 1)),
    ('w16_t32_1x16x32', 'w16', (1, 16, 32, 64, 64), 'plain+res+mask+tr+dgrad', (10032, 1, 1, 1, 2, 1, 1)),
    ('w16_t32_1x16x64_c192', 'w16', (1, 16, 64, 128, 192), 'plain+res+mask+tr', (10032, 2, 2, 3, 4, 1, 1)),
    ('w16_t32_2x32x32', 'w16', (2, 32, 32, 64, 64), 'plain+mask+tr+dgrad', (10032, 4, 4, 1, 2, 1, 1)),
    ('w16_t32_1x32x32_c256', 'w16', (1, 32, 32, 256, 64), 'plain+tr', (10032, 2, 2, 1, 8, 1, 1)),
    ('w16_t32_cin1024', 'w16', (1, 16, 32, 1024, 64), 'plain+tr', (10032, 1, 1, 1, 32, 1, 1)),
    ('w16_2map_n1', 'w16', (1, 16, 16, 64, 64), 'plain+res+mask+tr+dgrad', (10132, 1, 1, 1, 2, 1, 1)),
    ('w16_2map_n2', 'w16', (2, 16, 16, 128, 64), 'plain+mask+tr', (10132, 1, 1, 1, 4, 2, 1)),
    ('w16_2map_n3', 'w16', (3, 16, 16, 64, 64), 'plain+res+mask+tr+dgrad', (10132, 2, 2, 1, 2, 1, 1)),
    ('w16_2map_n5', 'w16', (5, 16, 16, 256, 64), 'plain+res+mask+tr', (10132, 3, 3, 1, 8, 1, 1)),
    ('w16_2map_n3_c192', 'w16', (3, 16, 16, 64, 192), 'plain+res+mask+tr', (10132, 2, 2, 3, 2, 1, 1)),
    ('w16_2map_cin1024', 'w16', (3, 16, 16, 1024, 64), 'plain+tr', (10132, 2, 2, 1, 32, 1, 1)),
    ('w16_blk_pos', 'w16', (1, 16, 32, 64, 128), 'pos', (20064, 2, 2, 1, 1, 1, 1)),
    ('w16_8x8_pos', 'w16', (3, 8, 8, 64, 128), 'pos', (21064, 1, 1, 1, 1, 3, 1)),
    ('w16_t32_pos', 'w16', (1, 16, 32, 64, 64), 'pos', (10032, 1, 1, 1, 2, 1, 1)),
    ('w16_2map_pos', 'w16', (3, 16, 16, 64, 64), 'pos', (10132, 2, 2, 1, 2, 1, 1)),
    ('w32_blk_1x16x32', 'w32', (1, 16, 32, 64, 128), 'plain+res+mask+tr+dgrad', (20032, 2, 2, 1, 2, 1, 1)),
    ('w32_blk_2x32x16', 'w32', (2, 32, 16, 128, 128), 'plain+res+mask+tr', (20032, 4, 4, 1, 4, 1, 1)),
    ('w32_blk_1x32x32_2slabs', 'w32', (1, 32, 32, 64, 256), 'plain+mask+tr', (20032, 4, 4, 2, 2, 1, 1)),
    ('w32_blk_2x16x32_c256', 'w32', (2, 16, 32, 256, 128), 'plain+tr', (20032, 4, 4, 1, 8, 1, 1)),
    ('w32_blk_cin1024', 'w32', (1, 16, 16, 1024, 128), 'plain+tr', (20032, 1, 1, 1, 32, 1, 1)),
    ('w32_8x8_n1', 'w32', (1, 8, 8, 128, 128), 'plain+res+mask+tr+dgrad', (21032, 1, 1, 1, 4, 1, 1)),
    ('w32_8x8_n2', 'w32', (2, 8, 8, 128, 128), 'plain+mask+tr', (21032, 1, 1, 1, 4, 2, 1)),
    ('w32_8x8_n3', 'w32', (3, 8, 8, 64, 256), 'plain+res+mask+tr', (21032, 1, 1, 2, 2, 3, 1)),
    ('w32_8x8_n4', 'w32', (4, 8, 8, 64, 128), 'plain+tr', (21032, 1, 1, 1, 2, 4, 1)),
    ('w32_8x8_n5', 'w32', (5, 8, 8, 256, 128), 'plain+res+mask+tr+dgrad', (21032, 2, 2, 1, 8, 1, 1)),
    ('w32_8x8_n7', 'w32', (7, 8, 8, 128, 256), 'plain+res+mask+tr+dgrad', (21032, 2, 2, 2, 4, 3, 1)),
    ('w32_8x8_cin1024', 'w32', (5, 8, 8, 1024, 128), 'plain+tr', (21032, 2, 2, 1, 32, 1, 1)),
    ('w32_t32_1x16x32', 'w32', (1, 16, 32, 64, 64), 'plain+res+mask+tr+dgrad', (10016, 1, 1, 1, 4, 1, 1)),
    ('w32_t32_1x16x64_c192', 'w32', (1, 16, 64, 128, 192), 'plain+res+mask+tr', (10016, 2, 2, 3, 8, 1, 1)),
    ('w32_t32_2x32x32', 'w32', (2, 32, 32, 64, 64), 'plain+mask+tr+dgrad', (10016, 4, 4, 1, 4, 1, 1)),
    ('w32_t32_1x32x32_c256', 'w32', (1, 32, 32, 256, 64), 'plain+tr', (10016, 2, 2, 1, 16, 1, 1)),
    ('w32_t32_cin1024', 'w32', (1, 16, 32, 1024, 64), 'plain+tr', (10016, 1, 1, 1, 64, 1, 1)),
    ('w32_2map_n1', 'w32', (1, 16, 16, 64, 64), 'plain+res+mask+tr+dgrad', (10116, 1, 1, 1, 4, 1, 1)),
    ('w32_2map_n2', 'w32', (2, 16, 16, 128, 64), 'plain+mask+tr', (10116, 1, 1, 1, 8, 2, 1)),
    ('w32_2map_n3', 'w32', (3, 16, 16, 64, 64), 'plain+res+mask+tr+dgrad', (10116, 2, 2, 1, 4, 1, 1)),
    ('w32_2map_n5', 'w32', (5, 16, 16, 256, 64), 'plain+res+mask+tr', (10116, 3, 3, 1, 16, 1, 1)),
    ('w32_2map_n3_c192', 'w32', (3, 16, 16, 64, 192), 'plain+res+mask+tr', (10116, 2, 2, 3, 4, 1, 1)),
    ('w32_2map_cin1024', 'w32', (3, 16, 16, 1024, 64), 'plain+tr', (10116, 2, 2, 1, 64, 1, 1)),
    ('w32_blk_pos', 'w32', (1, 16, 32, 64, 128), 'pos', (20032, 2, 2, 1, 2, 1, 1)),
    ('w32_8x8_pos', 'w32', (3, 8, 8, 64, 128), 'pos', (21032, 1, 1, 1, 2, 3, 1)),
    ('w32_t32_pos', 'w32', (1, 16, 32, 64, 64), 'pos', (10016, 1, 1, 1, 4, 1, 1)),
    ('w32_2map_pos', 'w32', (3, 16, 16, 64, 64), 'pos', (10116, 2, 2, 1, 4, 1, 1)),
    ('w32_eval_2map_n3', 'w32_eval', (3, 16, 16, 64, 64), 'sra', (10116, 2, 2, 1, 4, 1, 1)),
    ('w32_eval_2map_n3_pm', 'w32_eval', (3, 16, 16, 64, 64), 'Osr', (10116, 2, 2, 1, 4, 1, 1)),
    ('w32_eval_2map_n5_shift', 'w32_eval', (5, 16, 16, 128, 64), 'a', (10116, 3, 3, 1, 8, 1, 1)),
    ('w32_eval_2map_n1_pm', 'w32_eval', (1, 16, 16, 64, 64), 'Ora', (10116, 1, 1, 1, 4, 1, 1)),
    ('w32_eval_blk_n3', 'w32_eval', (3, 16, 32, 64, 128), 'sra', (20032, 6, 6, 1, 2, 1, 1)),
    ('w32_eval_blk_n3_pm', 'w32_eval', (3, 32, 16, 64, 128), 'Os', (20032, 6, 6, 1, 2, 1, 1)),
    ('w32_eval_blk_n1_shift', 'w32_eval', (1, 16, 16, 128, 128), 'r', (20032, 1, 1, 1, 4, 1, 1)),
    ('w32_eval_blk_n5_pm', 'w32_eval', (5, 16, 16, 64, 256), 'Oa', (20032, 5, 5, 2, 2, 1, 1)),
]
_WGS1 = [
    ('wgs1_w16_8x8_n19', 'w16', (19, 8, 8, 64, 128), 'plain+res+mask+tr', (21064, 5, 1, 1, 1, 3, 5)),
    ('wgs1_w32_8x8_n18', 'w32', (18, 8, 8, 64, 128), 'plain+mask+tr', (21032, 5, 1, 1, 2, 2, 5)),
    ('wgs1_w16_blk_6', 'w16', (1, 32, 48, 64, 128), 'plain+tr', (20064, 6, 1, 1, 1, 1, 6)),
    ('wgs1_w32_blk_6', 'w32', (3, 16, 32, 64, 128), 'plain+res+tr', (20032, 6, 1, 1, 2, 1, 6)),
    ('wgs1_w16_t32_6', 'w16', (1, 32, 96, 64, 64), 'plain+mask+tr', (10032, 6, 1, 1, 2, 1, 6)),
    ('wgs1_w32_t32_5', 'w32', (5, 16, 32, 64, 64), 'plain+tr', (10016, 5, 1, 1, 4, 1, 5)),
    ('wgs1_w16_2map_n11', 'w16', (11, 16, 16, 64, 64), 'plain+res+tr', (10132, 6, 1, 1, 2, 1, 6)),
    ('wgs1_w32_2map_n13', 'w32', (13, 16, 16, 64, 64), 'plain+mask+tr', (10116, 7, 1, 1, 4, 1, 7)),
    ('wgs1_h16_tw8_n11', 'h16', (11, 5, 7, 64, 64), 'plain+res+tr', (641, 6, 1, 1, 1, 1, 6)),
    ('wgs1_h16_128_tw8_n13', 'h16', (13, 8, 8, 64, 128), 'plain+tr', (1281, 7, 1, 1, 1, 1, 7)),
    ('wgs1_h16_64_6', 'h16', (1, 9, 40, 64, 64), 'plain+tr', (640, 6, 1, 1, 1, 1, 6)),
    ('wgs1_h16_128_8', 'h16', (2, 13, 21, 64, 128), 'plain+res+tr', (1280, 8, 1, 1, 1, 1, 8)),
]
_WGS3 = [
    ('wgs3_w16_8x8_n25', 'w16', (25, 8, 8, 64, 128), 'plain+res+mask+tr', (21064, 7, 3, 1, 1, 1, 3)),
    ('wgs3_w32_8x8_n18', 'w32', (18, 8, 8, 64, 128), 'plain+mask+tr', (21032, 5, 3, 1, 2, 2, 2)),
    ('wgs3_w16_blk_8', 'w16', (2, 32, 32, 64, 128), 'plain+tr', (20064, 8, 3, 1, 1, 1, 3)),
    ('wgs3_w32_blk_7', 'w32', (7, 16, 16, 64, 128), 'plain+res+tr', (20032, 7, 3, 1, 2, 1, 3)),
    ('wgs3_w16_blk_2slabs', 'w16', (5, 16, 16, 64, 256), 'plain+tr', (20064, 5, 1, 2, 1, 1, 5)),
    ('wgs3_w16_t32_7', 'w16', (7, 16, 32, 64, 64), 'plain+mask+tr', (10032, 7, 3, 1, 2, 1, 3)),
    ('wgs3_w32_t32_6', 'w32', (1, 32, 96, 64, 64), 'plain+tr', (10016, 6, 3, 1, 4, 1, 2)),
    ('wgs3_w16_2map_n13', 'w16', (13, 16, 16, 64, 64), 'plain+res+tr', (10132, 7, 3, 1, 2, 1, 3)),
    ('wgs3_w32_2map_n15', 'w32', (15, 16, 16, 64, 64), 'plain+mask+tr', (10116, 8, 3, 1, 4, 1, 3)),
    ('wgs3_w32_2map_c192', 'w32', (9, 16, 16, 64, 192), 'plain+tr', (10116, 5, 1, 3, 4, 1, 5)),
    ('wgs3_h16_tw8_n13', 'h16', (13, 5, 7, 64, 64), 'plain+res+tr', (641, 7, 3, 1, 1, 1, 3)),
    ('wgs3_h16_128_tw8_n15', 'h16', (15, 8, 8, 64, 128), 'plain+tr', (1281, 8, 3, 1, 1, 1, 3)),
    ('wgs3_h16_64_6', 'h16', (1, 9, 40, 64, 64), 'plain+tr', (640, 6, 3, 1, 1, 1, 2)),
    ('wgs3_h16_128_8', 'h16', (2, 13, 21, 64, 128), 'plain+res+tr', (1280, 8, 3, 1, 1, 1, 3)),
    ('wgs3_h16_c192', 'h16', (1, 9, 40, 64, 192), 'plain+tr', (640, 6, 1, 3, 1, 1, 6)),
]

SWITCH_SETS = {
    # one workgroup per channel slab walks every tile
    "wgs_1": ({"SSAD_CONV16W_WGS": "1", "SSAD_CONV16_WGS": "1"}, _WGS1),
    # three workgroup slots: with one slab, workgroups walk 3 / 2 / 2 tiles and the ragged last tile is the LAST of a walk of several;
    # with two or three slabs, one workgroup per slab again
    "wgs_3": ({"SSAD_CONV16W_WGS": "3", "SSAD_CONV16_WGS": "3"}, _WGS3),
}
SWITCHES = ("SSAD_CONV16W_WGS", "SSAD_CONV16_WGS", "SSAD_CONV16W_MIN", "SSAD_CONV16W", "SSAD_CONV16", "SSAD_CONV32W", "SSAD_CONV32W_MIN")

# every instantiation of every kernel (ids: include/ssad.h)
INSTANTIATIONS = {
    "c64": {816}, "c64_bf16": {816}, "c64_f16": {816}, "c64_h": {816}, "c64_eval": {816},
    "h16": {640, 641, 1280, 1281},
    "w16": {20064, 21064, 10032, 10132},        # 16 x 16 blocks, four 8 x 8 maps, 16 x 32 tiles, two 16 x 16 maps
    "w32": {20032, 21032, 10016, 10116},
    "w32_eval": {10116, 20032},
}
TRAINING = ("c64", "c64_bf16", "c64_f16", "c64_h", "h16", "w16", "w32")
MASKED = ("c64", "c64_bf16", "c64_f16", "w16", "w32")
HALF_TENSORS = ("c64_h", "h16", "w16")
PACKED = ("w16", "w32")
C64_OP = {"c64": 0, "c64_bf16": 1, "c64_f16": 2}


def rows_of(name):
    return DEFAULT if name == "default" else SWITCH_SETS[name][1]


def child_env(name):
    """The environment of a child process running switch set `name`: every conv switch cleared, then the set's own."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if name != "default":
        env.update(SWITCH_SETS[name][0])
    return env


def run_child(name, geometry_only, timeout):
    """One switch set in a fresh interpreter -> (returncode, stdout + stderr, [[row id, entry, geometry], ...] or None)."""
    args = [sys.executable, os.path.abspath(__file__), name] + (["--geometry-only"] if geometry_only else [])
    r = subprocess.run(args, env=child_env(name), cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    geo = None
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            geo = json.loads(line)["geometry"]
    return r.returncode, r.stdout + r.stderr, geo


# ---- geometry ----
def path_of(entry):
    return 0 if entry.startswith("c64") else 1 if entry == "h16" else 2


def geometry_of(entry, shape):
    """[inst, ntiles, gx, gy, chunks, last, walk] of the launch, from the library (ops.conv3x3_geometry)."""
    from self_supervised import ops
    g = ops.conv3x3_geometry(path_of(entry), *shape, f32=entry.startswith("w32"))
    assert g is not None, f"{entry} {shape}: the entry point refuses the shape"
    return [g[k] for k in ("inst", "ntiles", "gx", "gy", "chunks", "last", "walk")]


def check_geometry(row):
    got = geometry_of(row[1], row[2])
    assert got == list(row[4]), f"row {row[0]} ({row[1]} {row[2]}): expected geometry {row[4]}, the launcher computes {got}"
    return got


# ---- buffers between guards ----
# Elements of the guard region on EITHER side of every tensor.  The missing maps of a last multi-map tile at the widest tensor of the
# table (1024 channels: the emitted activation of the Cin = 1024 rows) are three 8 x 8 maps = 196 608 elements or one 16 x 16 map =
# 262 144: a store to, or a load from, a missing image lands wholly inside the guard.
GUARD = 1 << 18


class Arena:
    """Every tensor of a launch in the middle of an allocation of its own: [GUARD | tensor | GUARD], guards NaN (0xff for bytes).
    Inputs must come back bit-unchanged, guards included; outputs start as NaN, must hold no NaN afterwards, and their guards must be
    bit-unchanged.  A read outside an input meets NaN (or set mask bits) and shows in the result."""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def _big(self, numel, dtype):
        fill = 255 if dtype == torch.uint8 else float("nan")
        return torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=self.dev)

    def inp(self, name, t, mutable=False):
        if t is None:
            return None
        big = self._big(t.numel(), t.dtype)
        big[GUARD:GUARD + t.numel()] = t.reshape(-1).to(self.dev)
        self.items.append((name, big, big.clone(), t.numel() if mutable else None))
        return big[GUARD:GUARD + t.numel()].view(t.shape)

    def out(self, name, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        big = self._big(n, dtype)
        self.items.append((name, big, big.clone(), n))
        return big[GUARD:GUARD + n].view(shape)

    def check(self, rid):
        torch.cuda.synchronize()
        for name, big, snap, n in self.items:
            b, s, e = big.view(torch.uint8), snap.view(torch.uint8), big.element_size()
            if n is None:
                assert torch.equal(b, s), f"{rid}: input `{name}` or its guards were written"
                continue
            lo, hi = GUARD * e, (GUARD + n) * e
            assert torch.equal(b[:lo], s[:lo]), f"{rid}: the launch wrote in front of `{name}`"
            assert torch.equal(b[hi:], s[hi:]), f"{rid}: the launch wrote past the end of `{name}`"
            left = int(torch.isnan(big[GUARD:GUARD + n]).sum())
            assert left == 0, f"{rid}: {left} of {n} elements of `{name}` left unwritten or NaN"


# ---- bars ----
# Per element: |err_e| <= TAU * A_e (+ 2^-11 |want_e| + 2^-25 where the element is stored as a half), A = conv2d(|x|, |w|) + |residual|
# in float64 over the operands as the kernel sees them -- the value of tests/wgrad_path_table.py.  Global: the bars the existing tests
# hold, 2e-5 max|want| (fp32 tensors) and 2e-3 max(1, max|want|) (half tensors).
TAU = 1e-5
U32, U16 = 2.0 ** -24, 2.0 ** -11
# Emitted activation relu((x - mean) * invstd * gamma + beta), evaluated in fp32 as written: four roundings (subtract, two products,
# add; fewer where the compiler contracts), each at most 2^-24 of B = (|x| + |mean|) invstd |gamma| + |beta|, the total doubled.
EMIT_BAR = 2 * 4 * U32
# Statistics: the sums over a tile are taken in fp32 before they go to double -- per lane and tile at most 32 values (float form of
# conv16w.hip), at most 128 (half forms of conv16w.hip and conv16.hip, v_dot2 / fp32 adds), none in conv_c64.hip (double per value) --
# so a sum of n values carries at most n 2^-24 of the sum of their magnitudes; both sums enter the variance (E z^2 - mean^2, where
# |mean| mean|z| <= (E z^2 + mean^2) / 2 ... bounded by the same scale), hence the factor 2; + 2 for the final fp32 roundings.
STAT_N32 = {"c64": 0, "c64_bf16": 0, "c64_f16": 0, "c64_h": 0, "h16": 128, "w16": 128, "w32": 32}
WORST = {}                          # entry -> [worst err / A, worst emit err / B, worst var err / (E z^2 + mean^2)]


def tau_s(entry):
    return 2 * (STAT_N32[entry] + 2) * U32


def _note(entry, k, v):
    w = WORST.setdefault(entry, [0.0, 0.0, 0.0])
    w[k] = max(w[k], v)


def compare(rid, entry, got, want, a, half_tensors):
    """Both bars over every element -> worst err_e / A_e (after the half-storage allowance)."""
    got = got.detach().cpu().double().reshape(want.shape)
    assert not torch.isnan(got).any(), f"{rid}: NaN in the output"
    err = (got - want).abs()
    wmax = want.abs().max().item()
    glob = 2e-3 * max(1.0, wmax) if half_tensors else 2e-5 * wmax
    assert err.max().item() <= glob, f"{rid}: max |err| {err.max().item():.3e} > {glob:.3e} (max|want| {wmax:.3e})"
    slack = U16 * want.abs() + 2.0 ** -25 if half_tensors else torch.zeros_like(want)
    bad = err > TAU * a + slack
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{rid}: {int(bad.sum())} of {bad.numel()} elements over {TAU} * A, first flat index {i}: got "
                             f"{got.reshape(-1)[i].item():.9g}, want {want.reshape(-1)[i].item():.9g}, A {a.reshape(-1)[i].item():.3e}")
    pos = a > 0
    r = ((err - slack).clamp(min=0)[pos] / a[pos]).max().item() if pos.any() else 0.0
    _note(entry, 0, r)
    return r


def check_emit(rid, entry, em, x_st, tr, half_tensors):
    """The emitted activation against float64 relu((x - mean) * invstd * gamma + beta); ReLU is continuous: nothing excluded."""
    mu, iv, ga, be = (t.double().cpu() for t in tr)
    x = x_st.double().cpu()
    want = ((x - mu) * iv * ga + be).clamp(min=0)
    b = (x.abs() + mu.abs()) * iv * ga.abs() + be.abs()
    bar = EMIT_BAR * b + ((U16 * want + 2.0 ** -25) if half_tensors else 0.0)
    err = (em.double().cpu() - want).abs()
    bad = err > bar
    assert not bad.any(), f"{rid}: {int(bad.sum())} emitted elements outside the float64 bar, worst err / B {(err / b).max().item():.3e}"
    slack = (U16 * want + 2.0 ** -25) if half_tensors else 0.0
    _note(entry, 1, ((err - slack).clamp(min=0) / b).max().item())


def check_stats(rid, entry, z, mean, invstd, eps, mom, run0, run1):
    """mean / invstd / running statistics against float64 over the STORED z [rows][C]."""
    z = z.double().cpu().reshape(-1, z.shape[-1])
    rows = z.shape[0]
    zm, ex2 = z.mean(0), (z * z).mean(0)
    var = ((z - zm) ** 2).mean(0)
    zmax = max(1.0, z.abs().max().item())
    mean, invstd = mean.double().cpu(), invstd.double().cpu()
    assert (mean - zm).abs().max().item() < 1e-5 * zmax, f"{rid}: mean off by {(mean - zm).abs().max().item():.3e}"
    want_i = (var + eps).rsqrt()
    ri = ((invstd - want_i).abs() / want_i).max().item()
    assert ri < 1e-5, f"{rid}: invstd off by {ri:.3e} (relative)"
    scale = ex2 + zm * zm
    verr = (invstd ** -2 - eps - var).abs() - 4 * U32 * (var + eps)          # the fp32 rounding of invstd itself
    ts = tau_s(entry)
    print(f"   {rid}: var err / (E z^2 + mean^2) {(verr.clamp(min=0) / scale).max().item():.3e} (bar {ts:.3e}), "
          f"|mean| / std up to {(zm.abs() / var.sqrt().clamp(min=1e-30)).max().item():.2f}", flush=True)
    assert (verr <= ts * scale).all(), f"{rid}: variance off by {(verr / scale).max().item():.3e} of E z^2 + mean^2 (bar {ts:.3e})"
    _note(entry, 2, (verr.clamp(min=0) / scale).max().item())
    # running statistics: (1 - m) old + m new in double, rounded once; the unbiased n / (n - 1)
    m = float(torch.tensor(mom, dtype=torch.float32))
    unb = var * rows / (rows - 1) if rows > 1 else var
    for name, old, new, stat, bar in (("running_mean", run0[0], run1[0], zm, 1e-5 * zmax),
                                      ("running_var", run0[1], run1[1], unb, ts * scale * (rows / max(rows - 1, 1)))):
        want = (1.0 - m) * old.double().cpu() + m * stat
        err = (new.double().cpu() - want).abs()
        lim = m * bar + 2 * U32 * want.abs()
        assert (err <= lim).all(), f"{rid}: {name} off by {err.max().item():.3e} (momentum {mom})"


# ---- operands and references ----
def _scaled(shape, g, span):
    """randn with a per-channel (last dimension) scale 2^u, u uniform in [-span, span]: small elements are held to their own scale."""
    return torch.randn(shape, generator=g) * torch.exp2(torch.rand(shape[-1], generator=g) * 2 * span - span)


def _operand(entry, t):
    """The values the kernel multiplies: rounded to bf16 / half where the operand mode rounds."""
    if entry == "c64_bf16":
        return t.float().bfloat16().double()
    if entry in ("c64_f16", "c64_h", "h16", "w16"):
        return t.float().half().double()
    return t.double()


def conv64(x, w):
    """float64 conv2d, 3 x 3 / stride 1 / pad 1, NHWC x and OHWI w -> NHWC."""
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, 1, 1).permute(0, 2, 3, 1).contiguous()


def flip_transpose(w):
    """[Cout][3][3][Cin] -> the input gradient's filter [Cin][3][3][Cout]."""
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


def unpack(packed, cout, cin):
    """A packed filter back to OHWI [Cout][3][3][Cin] from the documented fragment order [Cout/32][tap][Cin/(2 E)][2][32][E], E = 8
    halves / 4 floats: element (ct, tap, kb, kh, n, j) is w[32 ct + n][tap][2 E kb + E kh + j]."""
    e = 8 if packed.dtype == torch.float16 else 4
    return packed.reshape(cout // 32, 9, cin // (2 * e), 2, 32, e).permute(0, 4, 1, 2, 3, 5).reshape(cout, 3, 3, cin)


def _pack(entry, w32, cout, cin, flip, dev, scale=None):
    """The packed filter of a w16 / w32 row through the C packer, between guards -> device tensor."""
    import ctypes
    from self_supervised import _hip
    lib, st = _hip.lib(), _hip.stream()
    ar = Arena(dev)
    src = ar.inp("filter", w32.float())
    dt = torch.float16 if entry == "w16" else torch.float32
    dst = ar.out("packed filter", (cout * 9 * cin,), dt)
    if scale is not None or entry == "w32_eval":
        sc = ar.inp("scale", scale)
        _hip.check(lib.ssad_conv3x3_fw_pack_scaled(src.data_ptr(), None if sc is None else sc.data_ptr(), dst.data_ptr(), cout, cin, st))
    else:
        desc = (ctypes.c_int64 * 5)(0, 0, cout, cin, int(flip))
        fn = lib.ssad_conv3x3_hw_pack_batch if entry == "w16" else lib.ssad_conv3x3_fw_pack_batch
        _hip.check(fn(src.data_ptr(), dst.data_ptr(), desc, 1, st))
    ar.check("pack")
    return dst.clone()


def _launch(entry, shape, t, eps, mom):
    """The C entry point of a training row over the tensors of dict t (None where absent)."""
    from self_supervised import _hip
    lib, st = _hip.lib(), _hip.stream()
    n, h, w, cin, cout = shape
    P = lambda k: None if t.get(k) is None else t[k].data_ptr()
    tr = [None] * 4 if t.get("tr") is None else [v.data_ptr() for v in t["tr"]]
    tail = (P("ws"), eps, mom, P("mean"), P("invstd"), P("rm"), P("rv"))
    if entry in C64_OP:
        return lib.ssad_conv3x3_c64_op(P("x"), P("w"), P("out"), P("res"), P("mask"), *tr, P("emit"), n, h, w, *tail, C64_OP[entry], st)
    if entry == "c64_h":
        return lib.ssad_conv3x3_c64_h(P("x"), P("w"), P("out"), P("res"), *tr, P("emit"), n, h, w, *tail, st)
    if entry == "h16":
        return lib.ssad_conv3x3_h(P("x"), P("w"), P("out"), P("res"), *tr, P("emit"), n, h, w, cin, cout, *tail, st)
    fn = lib.ssad_conv3x3_hw if entry == "w16" else lib.ssad_conv3x3_fw
    return fn(P("x"), P("w"), P("out"), P("res"), P("mask"), *tr, P("emit"), n, h, w, cin, cout, *tail, st)


def _call(rid, entry, shape, dev, x, wk, res=None, mask=None, tr=None, emit=False, stats=None):
    """One launch through the C entry point, every tensor between guards -> dict of results (device tensors)."""
    from self_supervised import _hip
    n, h, w, cin, cout = shape
    ar = Arena(dev)
    t = {"x": ar.inp("in", x), "w": ar.inp("filter", wk), "res": ar.inp("residual", res), "mask": ar.inp("res_mask", mask)}
    if tr is not None:
        t["tr"] = [ar.inp(nm, v) for nm, v in zip(("tr_mean", "tr_invstd", "tr_gamma", "tr_beta"), tr)]
    t["out"] = ar.out("out", (n, h, w, cout), x.dtype)
    if emit:
        t["emit"] = ar.out("emit", (n, h, w, cin), x.dtype)
    eps = mom = 0.0
    if stats is not None:
        eps, mom, rm, rv = stats
        gx = geometry_of(entry, shape)[2]
        t["ws"] = ar.out("statistics workspace", (gx * 2 * cout,), torch.float64)
        t["mean"], t["invstd"] = ar.out("mean", (cout,), torch.float32), ar.out("invstd", (cout,), torch.float32)
        t["rm"], t["rv"] = ar.inp("running_mean", rm, mutable=True), ar.inp("running_var", rv, mutable=True)
    _hip.check(_launch(entry, shape, t, eps, mom))
    ar.check(rid)
    return t


def _wrapper(entry, shape, x, wk, res=None, mask=None, tr=None, emit=False, stats=None):
    """The ops wrapper of the entry where it accepts the shape (the register-fed forms ask for a chip-filling launch), else None."""
    from self_supervised import ops
    n, h, w, cin, cout = shape
    if entry in C64_OP or entry == "c64_h":
        r = ops.conv3x3_c64(x, wk, residual=res, transform=tr, emit=emit, stats=stats, res_mask=mask, bf16=C64_OP.get(entry, 2))
    elif entry == "h16":
        r = ops.conv3x3_h(x, wk, residual=res, transform=tr, emit=emit, stats=stats)
    elif ops.conv3x3_hw_ok(n, h, w, cin, cout, entry == "w32"):
        r = ops.conv3x3_hw(x, wk, cout, residual=res, transform=tr, emit=emit, stats=stats, res_mask=mask)
    else:
        return None
    return r if isinstance(r, tuple) else (r,)


def _same_as_wrapper(rid, entry, shape, t, **kw):
    """The C result into poisoned buffers == the wrapper's, bit for bit (z, the emitted activation, mean / invstd, running statistics)."""
    stats = kw.get("stats")
    if stats is not None:
        kw = dict(kw, stats=(stats[0], stats[1], stats[2].clone(), stats[3].clone()))
    r = _wrapper(entry, shape, **kw)
    if r is None:
        return
    torch.cuda.synchronize()
    names = ["out"] + (["emit"] if kw.get("emit") else []) + (["mean", "invstd"] if stats is not None else [])
    for nm, v in zip(names, r):
        assert torch.equal(v.reshape(-1).view(torch.int16 if v.dtype == torch.float16 else torch.int32),
                           t[nm].reshape(-1).view(torch.int16 if v.dtype == torch.float16 else torch.int32)), \
            f"{rid}: `{nm}` of the C call into poisoned buffers differs from the wrapper's"
    if stats is not None:
        assert torch.equal(kw["stats"][2], t["rm"]) and torch.equal(kw["stats"][3], t["rv"]), f"{rid}: running statistics differ from the wrapper's"


def run_training_row(row, dev):
    from self_supervised import ops
    rid, entry, shape, epilogue, _ = row
    n, h, w, cin, cout = shape
    half = entry in HALF_TENSORS
    tdt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(sum(map(ord, rid)))
    forms = epilogue.split("+")
    pos = forms == ["pos"]
    if pos:      # z with |mean| / std about 3: E|x| = 0.8, a filter mean of 3.75 / (9 Cin) on a spread of 1 / sqrt(9 Cin)
        x = torch.randn((n, h, w, cin), generator=g).abs()
        w32 = torch.randn((cout, 3, 3, cin), generator=g) / (9 * cin) ** 0.5 + 3.75 / (9 * cin)
        forms = ["plain"]
    else:
        x = _scaled((n, h, w, cin), g, 3)
        w32 = _scaled((cin, 3, 3, cout), g, 2).permute(3, 1, 2, 0).contiguous() / (9 * cin) ** 0.5       # scale per OUTPUT channel
    res = _scaled((n, h, w, cout), g, 3)
    x_st, res_st = x.to(tdt), res.to(tdt)                          # as stored
    w_ref = _operand(entry, w32)
    if entry in PACKED:
        wk = _pack(entry, w32, cout, cin, False, dev)
        got_w = unpack(wk.cpu(), cout, cin).double()
        assert torch.equal(got_w, w_ref), f"{rid}: the packed filter, unpacked from the documented fragment order, is not the source"
    else:
        wk = (w32.half() if entry == "h16" else w32).to(dev)
    xd, resd = x_st.to(dev), res_st.to(dev)
    worst = 0.0
    want0 = a0 = None
    if {"plain", "res", "mask"} & set(forms):
        xe = _operand(entry, x_st)
        want0, a0 = conv64(xe, w_ref), conv64(xe.abs(), w_ref.abs())
    for form in forms:
        fid = f"{rid}[{form}]"
        if form == "plain":
            rm0, rv0 = (torch.randn(cout, generator=g) * 0.5).to(dev), (torch.rand(cout, generator=g) + 0.5).to(dev)
            kw = dict(x=xd, wk=wk, stats=(1e-5, 0.1, rm0, rv0))
            t = _call(fid, entry, shape, dev, **kw)
            worst = max(worst, compare(fid, entry, t["out"], want0, a0, half))
            check_stats(fid, entry, t["out"], t["mean"], t["invstd"], 1e-5, 0.1, (rm0, rv0), (t["rm"], t["rv"]))
        elif form in ("res", "mask"):
            assert form == "res" or entry in MASKED, f"{rid}: {entry} has no residual mask"
            mask = bits = None
            r64 = res_st.double()
            if form == "mask":
                mask = torch.randint(0, 16, (n, h, w, cout // 4), generator=g, dtype=torch.uint8)
                bits = torch.stack([(mask >> k) & 1 for k in range(4)], -1).reshape(n, h, w, cout).double()
                r64 = r64 * bits                                    # "add the residual where the bit is set"
                mask = mask.to(dev)
            kw = dict(x=xd, wk=wk, res=resd, mask=mask)
            t = _call(fid, entry, shape, dev, **kw)
            worst = max(worst, compare(fid, entry, t["out"], want0 + r64, a0 + r64.abs(), half))
        elif form == "tr":
            tr = [(torch.randn(cin, generator=g) * 0.2).to(dev), (torch.rand(cin, generator=g) + 0.5).to(dev),
                  (torch.rand(cin, generator=g) + 0.5).to(dev), (torch.randn(cin, generator=g) * 0.3).to(dev)]
            rm0, rv0 = (torch.randn(cout, generator=g) * 0.5).to(dev), (torch.rand(cout, generator=g) + 0.5).to(dev)
            kw = dict(x=xd, wk=wk, tr=tr, emit=True, stats=(1e-5, 0.3, rm0, rv0))
            t = _call(fid, entry, shape, dev, **kw)
            act = ops.bn_apply_fwd(xd, tr[0], tr[1], tr[2], tr[3], None, True)
            torch.cuda.synchronize()
            assert torch.equal(t["emit"], act), f"{fid}: the emitted activation is not bit-equal to ops.bn_apply_fwd"
            check_emit(fid, entry, t["emit"], x_st, tr, half)
            ae = _operand(entry, t["emit"].cpu())                  # the kernel's own activation, checked above
            worst = max(worst, compare(fid, entry, t["out"], conv64(ae, w_ref), conv64(ae.abs(), w_ref.abs()), half))
            check_stats(fid, entry, t["out"], t["mean"], t["invstd"], 1e-5, 0.3, (rm0, rv0), (t["rm"], t["rv"]))
            t_ne = _call(fid + " without emit", entry, shape, dev, x=xd, wk=wk, tr=tr)
            assert torch.equal(t_ne["out"], t["out"]), f"{fid}: z with and without emit differ"
        elif form == "dgrad":       # in = dz [n][h][w][cout], the flipped filter [cin][3][3][cout], residual [n][h][w][cin]
            dshape = (n, h, w, cout, cin)
            assert geometry_of(entry, dshape) is not None
            wf = flip_transpose(w32)
            wkd = _pack(entry, w32, cin, cout, True, dev) if entry in PACKED else (wf.half() if entry == "h16" else wf).to(dev)
            if entry in PACKED:
                assert torch.equal(wkd, _pack(entry, wf, cin, cout, False, dev)), f"{fid}: flipped pack != plain pack of the flip-transpose"
            ge = _operand(entry, res_st)
            wfr = _operand(entry, wf)
            kw = dict(x=resd, wk=wkd, res=xd)
            t = _call(fid, entry, dshape, dev, **kw)
            worst = max(worst, compare(fid, entry, t["out"], conv64(ge, wfr) + x_st.double(), conv64(ge.abs(), wfr.abs()) + x_st.double().abs(),
                                       half))
        else:
            raise AssertionError(f"{rid}: unknown epilogue form {form}")
        # the wrapper where it takes the shape, and a second call: bit-equal
        _same_as_wrapper(fid, entry, dshape if form == "dgrad" else shape, t, **kw)
        if "stats" in kw:
            kw = dict(kw, stats=kw["stats"][:2] + (kw["stats"][2].clone(), kw["stats"][3].clone()))
        t2 = _call(fid + " (second call)", entry, dshape if form == "dgrad" else shape, dev, **kw)
        for nm in ("out", "emit", "mean", "invstd", "rm", "rv"):
            if t.get(nm) is not None:
                assert torch.equal(t2[nm].reshape(-1).view(torch.uint8), t[nm].reshape(-1).view(torch.uint8)), f"{fid}: two calls differ in `{nm}`"
    return worst


def run_eval_row(row, dev):
    """c64_eval: act(conv * scale + shift + residual) in any of the eight layouts; w32_eval: act(conv(packed-and-scaled filter) + shift +
    residual), NHWC or position-major output."""
    from self_supervised import ops, _hip
    lib, st = _hip.lib(), _hip.stream()
    rid, entry, shape, flags, _ = row
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(sum(map(ord, rid)))
    x = _scaled((n, h, w, cin), g, 3)
    w32 = _scaled((cin, 3, 3, cout), g, 2).permute(3, 1, 2, 0).contiguous() / (9 * cin) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5 if "s" in flags else None
    sh = torch.randn(cout, generator=g) if ("s" in flags or entry == "w32_eval") else None
    res = _scaled((n, h, w, cout), g, 3) if "r" in flags else None
    relu, i_pm, o_pm, r_pm = "a" in flags, "I" in flags, "O" in flags, "R" in flags
    pm = lambda t, on: t.permute(1, 2, 0, 3).contiguous() if (on and t is not None) else t         # NHWC -> [H][W][N][C]
    x64, r64 = x.double(), (res.double() if res is not None else torch.zeros(n, h, w, cout, dtype=torch.float64))
    if entry == "c64_eval":
        s64 = sc.double() if sc is not None else torch.ones(cout, dtype=torch.float64)
        b64 = sh.double() if sh is not None else torch.zeros(cout, dtype=torch.float64)
        want = conv64(x64, w32.double()) * s64 + b64 + r64
        a = conv64(x64.abs(), w32.double().abs()) * s64.abs() + b64.abs() + r64.abs()
        wk = w32
    else:
        wk = _pack(entry, w32, cout, cin, False, dev, scale=sc.to(dev) if sc is not None else None)
        w_eff = (w32 * sc.view(-1, 1, 1, 1)) if sc is not None else w32                               # one fp32 product per element
        assert torch.equal(unpack(wk.cpu(), cout, cin), w_eff), f"{rid}: the packed-and-scaled filter, unpacked, is not w * scale"
        want = conv64(x64, w_eff.double()) + sh.double() + r64
        a = conv64(x64.abs(), w_eff.double().abs()) + sh.double().abs() + r64.abs()
    if relu:
        want = want.clamp(min=0)
    outs = []
    for rep in range(2):
        ar = Arena(dev)
        xd, wd, rd = ar.inp("in", pm(x, i_pm)), ar.inp("filter", wk), ar.inp("residual", pm(res, r_pm))
        scd, shd = ar.inp("scale", sc), ar.inp("shift", sh)
        out = ar.out("out", (h, w, n, cout) if o_pm else (n, h, w, cout), torch.float32)
        P = lambda t: None if t is None else t.data_ptr()
        if entry == "c64_eval":
            _hip.check(lib.ssad_conv3x3_c64_eval(P(xd), P(wd), P(out), P(scd), P(shd), P(rd), int(relu), n, h, w, int(i_pm), int(o_pm),
                                                 int(r_pm), st))
        else:
            _hip.check(lib.ssad_conv3x3_fw_eval(P(xd), P(wd), P(out), P(shd), P(rd), int(relu), n, h, w, cin, cout, int(o_pm), st))
        ar.check(rid)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), f"{rid}: two calls differ"
    xg, rg = pm(x, i_pm).to(dev), (pm(res, r_pm).to(dev) if res is not None else None)
    if entry == "c64_eval":
        wr = ops.conv3x3_c64_eval(xg, w32.to(dev), sc.to(dev) if sc is not None else None, sh.to(dev) if sh is not None else None, rg, relu,
                                  in_hwnc=i_pm, out_hwnc=o_pm, res_hwnc=r_pm)
    else:
        wr = ops.conv3x3_fw_eval(xg, wk, cout, sh.to(dev), rg, relu, out_hwnc=o_pm)
    torch.cuda.synchronize()
    assert torch.equal(wr, outs[0]), f"{rid}: the C call into poisoned buffers differs from the wrapper's result"
    got = outs[0].permute(2, 0, 1, 3) if o_pm else outs[0]
    return compare(rid, entry, got, want, a, False)


def run_packers(dev):
    """ssad_conv3x3_hw_pack_batch / _fw_pack_batch: three filters in one table, one of them flipped, at unequal offsets with gaps
    between them; unpacked on the host from the documented fragment order they are the source (rounded to half for _hw), the gaps stay
    untouched, and the flipped pack of a filter is the plain pack of its flip-transpose."""
    import ctypes
    from self_supervised import _hip
    lib, st = _hip.lib(), _hip.stream()
    g = torch.Generator().manual_seed(77)
    # (Cout, Cin of the conv that RUNS on the pack, flip): the source of a flipped entry is [Cin][3][3][Cout]
    spec = [(64, 128, 0), (128, 64, 1), (192, 64, 0)]
    srcs = [torch.randn((i, 3, 3, o) if f else (o, 3, 3, i), generator=g) for o, i, f in spec]
    for fn, dt in ((lib.ssad_conv3x3_hw_pack_batch, torch.float16), (lib.ssad_conv3x3_fw_pack_batch, torch.float32)):
        flat, desc, so, do = [], [], 0, 0
        for (o, i, f), s in zip(spec, srcs):
            so += 24                                            # a gap in front of every source filter
            flat += [torch.full((24,), float("nan")), s.reshape(-1)]
            do += 40                                            # ... and in front of every packed one (a multiple of 8 elements)
            desc += [so, do, o, i, f]
            so += s.numel()
            do += s.numel()
        ar = Arena(dev)
        src = ar.inp("filters", torch.cat(flat))
        dst = torch.full((do + 2 * GUARD,), float("nan"), dtype=dt, device=dev)
        before = dst.clone()
        _hip.check(fn(src.data_ptr(), dst[GUARD:].data_ptr(), (ctypes.c_int64 * len(desc))(*desc), len(spec), st))
        ar.check("packers")
        written = torch.zeros(do + 2 * GUARD, dtype=torch.bool)
        for k, ((o, i, f), s) in enumerate(zip(spec, srcs)):
            off = GUARD + desc[5 * k + 1]
            written[off:off + s.numel()] = True
            got = unpack(dst[off:off + s.numel()].cpu(), o, i)
            want = flip_transpose(s) if f else s
            assert torch.equal(got, want.to(dt)), f"packers: filter {k} ({o} x {i}, flip {f}, {dt}) unpacked is not its source"
            plain = _pack("w16" if dt == torch.float16 else "w32", want, o, i, False, dev)
            assert torch.equal(plain, dst[off:off + s.numel()]), f"packers: filter {k}: the batched (flipped) pack != the plain pack of its flip-transpose"
        same = dst.cpu().view(torch.int16 if dt == torch.float16 else torch.int32) == before.cpu().view(torch.int16 if dt == torch.float16 else torch.int32)
        assert same[~written].all(), "packers: wrote outside the packed filters"


def run_row(row, dev):
    """Geometry, then the kernels: -> worst err_e / A_e of the row."""
    check_geometry(row)
    if row[1] in TRAINING:
        return run_training_row(row, dev)
    return run_eval_row(row, dev)


def _main(argv):
    name, geometry_only = argv[0], "--geometry-only" in argv
    for q in (ROOT, PKG):
        if q not in sys.path:
            sys.path.insert(0, q)
    if not geometry_only:
        assert torch.cuda.is_available(), "the kernel rows need the MI355X"
    seen = []
    for row in rows_of(name):
        seen.append([row[0], row[1], check_geometry(row)])
        if not geometry_only:
            e = run_row(row, torch.device("cuda:0"))
            print(f"ok {row[0]} {row[1]} {row[4][0]} err/A {e:.2e}", flush=True)
    print_worst()
    print(json.dumps({"set": name, "geometry": seen}), flush=True)


def print_worst():
    """The worst measured ratios per entry so far (the figures of DESIGN.md): `python tests/conv3x3_table.py default` prints them, and so
    does `pytest -s -m gpu tests/test_hip_conv3x3_paths.py` when the module ends."""
    for ent, wv in sorted(WORST.items()):
        print(f"worst {ent}: err/A {wv[0]:.3e} emit err/B {wv[1]:.3e} var err/(Ez^2+mean^2) {wv[2]:.3e}", flush=True)


if __name__ == "__main__":
    _main(sys.argv[1:])
