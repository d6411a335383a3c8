"""The tail of the default scoring path against exact references (the table: tests/scoring_tail_table.py): row L2-normalisation, the
k-smallest mean of the cosine chain, the Grad-CAM contraction, blur + ReLU + bilinear in both kernels, the weight repacking, and the
zero-norm rows of every cosine path against sklearn.

One test per row.  Everything goes through the C entry points; every tensor of every launch is a view between poisoned guards; every
launch runs twice into fresh buffers: bit-identical; after each launch no output element may be left poisoned and every guard must be
bit-unchanged, and after the row every input; where the ops wrapper takes the shape its result is bit-equal.  Every output element is
held to a bar counted from the kernel's operations and computed from the float64 reference (the table's docstring); the k-smallest
mean, the repacking, zero-sum rows and all-negative maps are exact.

The worst error / bar per output is printed before it is asserted (`pytest -s`), and per entry kind when the module ends."""
import pytest
import torch

import scoring_tail_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    yield torch.device("cuda:0")
    T.print_worst()


@pytest.mark.parametrize("row", T.ROWS, ids=[T.row_id(kr) for kr in T.ROWS])
def test_row_against_reference(dev, row):
    T.run_row(row, dev)


def test_knn_mean_refuses_k_outside_1_to_3_or_above_the_bank(dev):
    T.run_knn_bad_k(dev)


def test_zero_norm_rows_are_at_distance_one_on_every_cosine_path(dev):
    T.run_zero_norm(dev)
