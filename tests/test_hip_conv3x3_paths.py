"""Every entry point and instantiation of the three 3 x 3 / stride 1 / pad 1 kernels against float64 (the table: tests/conv3x3_table.py).

Each row first asserts its launch geometry, then runs every epilogue form it lists through the C entry point with every tensor between
NaN guards -- inputs in front of AND behind one, outputs prefilled with NaN -- : no NaN may be left in an output, every guard and every
input must come back bit-unchanged, the result must be bit-equal to the ops wrapper's where the wrapper takes the shape and to a second
call, and z must not depend on emit.  Every element is held to the global bar of the existing tests and to |err_e| <= 1e-5 A_e
(+ half storage), the emitted activation to ops.bn_apply_fwd bit for bit and to float64, the statistics to float64 over the stored z.

SSAD_CONV16W_WGS / SSAD_CONV16_WGS are read once per process: each switch set runs in a fresh child interpreter, one at a time, and the
first failing child stops the sequence.

The worst measured ratios per entry are printed when the module ends (`pytest -s`), and by `python tests/conv3x3_table.py default`."""
import pytest
import torch

import conv3x3_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    yield torch.device("cuda:0")
    T.print_worst()          # the worst err / A, emit and variance ratios per entry over the rows that ran (shown under pytest -s)


@pytest.mark.parametrize("row", T.DEFAULT, ids=[r[0] for r in T.DEFAULT])
def test_default_row_against_fp64(dev, row):
    T.run_row(row, dev)


def test_packers(dev):
    T.run_packers(dev)


def test_switch_sets_against_fp64(dev):
    for name in T.SWITCH_SETS:
        rc, out, geo = T.run_child(name, geometry_only=False, timeout=600)
        assert rc == 0, f"switch set {name} {T.SWITCH_SETS[name][0]}: exit status {rc}\n{out[-4000:]}"
        assert geo is not None and len(geo) == len(T.rows_of(name)), out[-4000:]
