"""Every stem forward kernel form against float64 (the table: tests/stem_table.py).

Each row runs every form it lists through the C entry point with every tensor between guards -- inputs between NaN, outputs and the
statistics workspace prefilled with poison --: no poison may be left where the kernel is documented to write, every element it is
documented to skip (the ring form's square, the border form's interior) must still hold it, every guard and every input must come back
bit-unchanged.  Every written element is held to 2e-5 of the row's largest float64 reference magnitude (a stored half: to the spacing of
halves), the statistics to float64 statistics of the reference.  The loop rows launch more tiles (windows) than persistent workgroups.

The worst measured figures per family are printed when the module ends (`pytest -s`)."""
import pytest
import torch

import stem_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    yield torch.device("cuda:0")
    T.print_worst()
    T._raw64.cache_clear()


@pytest.mark.parametrize("row", T.ROWS, ids=[r[0] for r in T.ROWS])
def test_row_against_fp64(dev, row):
    T.run_row(row, dev)


def test_packers(dev):
    T.run_packers(dev)
