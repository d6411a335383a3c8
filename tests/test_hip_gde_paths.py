"""The kernels of csrc/gde.hip against float64 / longdouble (the table: tests/gde_table.py): ssad_mahalanobis_fused at every W-tile and
workgroup edge over a W whose strict upper triangle is NaN, its exact rows (integers, selectors, row independence), and
ssad_gaussian_fit_stats at every split geometry.

Everything goes through the C entry points on views between poisoned guards; every launch runs twice into fresh buffers: bit-identical;
after each launch no output element may be left poisoned and every guard must be bit-unchanged, and after a row every input.  Every output
element is held to a bar derived from the arithmetic and computed from the reference (the table's docstring).

The worst error / bar per output is printed before it is asserted (`pytest -s`), and per entry kind when the module ends."""
import pytest
import torch

import gde_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    yield torch.device("cuda:0")
    T.print_worst()


def test_scorer_rows_against_fp64(dev):
    for row in T.SCORE:
        T.run_score_row(row, dev)
    T.print_worst()


def test_exact_rows(dev):
    for row in T.INTEGER:
        T.run_int_row(row, dev)
    T.run_selector_rows(dev)
    T.run_independence(dev)
    T.print_worst()


def test_fit_rows_against_longdouble(dev):
    for row in T.FIT:
        T.run_fit_row(row, dev)
    T.print_worst()


def test_argument_errors(dev):
    T.run_argument_errors(dev)
    T.print_worst()
