"""Every BatchNorm entry point of csrc/train.hip, and the fused stem forms of csrc/stem.hip, against float64 (the table: tests/bn_table.py).

One test per row.  Every tensor of every launch is a view between poisoned guards, the reduction workspace is exactly
ssad_colreduce_workspace(R, C) doubles (half launches too); after each launch no output element may be left poisoned and every guard
must be bit-unchanged, and after the row every input.  Every launch runs twice into fresh buffers: bit-identical.  Every output element
(or channel) is held to a bar derived from the arithmetic and computed from the float64 reference (the table's docstring); mask bits,
winner slots, raw winners and dres are exact.

The worst error / bar per output is printed before it is asserted (`pytest -s`), and per entry kind when the module ends."""
import pytest
import torch

import bn_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    yield torch.device("cuda:0")
    T.print_worst()


@pytest.mark.parametrize("row", T.ROWS, ids=[r.id for r in T.ROWS])
def test_row_against_fp64(dev, row):
    T.run_row(row, dev)


@pytest.mark.parametrize("stem", T.STEM, ids=lambda s: "x".join(map(str, s[:3])) + ("_f16" if s[3] else "_f32"))
def test_stem_form_against_fp64(dev, stem):
    T.run_stem_case(*stem, dev)
