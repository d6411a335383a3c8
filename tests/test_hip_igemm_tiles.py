"""Every implicit-GEMM tile the conv dispatch can pick, against float64 (the table: tests/igemm_tile_table.py).

Each row first asserts the tile its launch selects, then runs through the ops wrapper and once more through the C entry point into
a NaN-filled output followed by a guard region: no NaN may be left, the result must be bit-equal to the wrapper's and the guard
untouched.  Inputs, filters, scale / shift and residuals sit in front of NaN guards of their own, so a load past their end that
reached a result would show.  Every element is compared with float64 torch on the CPU (F.conv2d / conv2d_input, the epilogue and
the BatchNorm statistics in float64) at the bars of test_hip_parity.py (exact fp32, 2e-5 of max|want|), test_hip_x3.py (bf16x3 2e-5,
bf16x6 5e-6) and test_hip_half.py (half tensors, 2e-3 * max(1, max|want|)); the bf16 / fp16-operand rows are compared with float64
over the same rounded operands, whose products are exact in fp32, and hold the fp32 bar.

The non-default tiles are reached through the switches of the README's run-time table, which are read once per process: each switch
set runs in a fresh child interpreter, one at a time, and the first failing child stops the sequence."""
import pytest
import torch

import igemm_tile_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    return torch.device("cuda:0")


@pytest.mark.parametrize("row", T.DEFAULT, ids=[r[0] for r in T.DEFAULT])
def test_default_tile_against_fp64(dev, row):
    T.check_tile(row)
    T.run_row(row, dev)


def test_switch_sets_against_fp64(dev):
    for name in T.SWITCH_SETS:
        rc, out, tiles = T.run_child(name, tiles_only=False, timeout=600)
        assert rc == 0, f"switch set {name} {T.SWITCH_SETS[name][0]}: exit status {rc}\n{out[-4000:]}"
        assert tiles is not None and len(tiles) == len(T.rows_of(name)), out[-4000:]
