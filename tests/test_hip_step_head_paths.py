"""The head, loss and optimiser kernels of a training step against float64 (the table: tests/step_head_table.py): the small-batch
linear kernels in all three operand roundings, global average pooling forward and backward, the plain max-pool, softmax cross-entropy,
SGD, check_finite, the loss scale and its update.

One test per row.  Everything goes through the C entry points (the linear kernels through ssad_conv_igemm_fwd / _fwd_stats / _dgrad and
ssad_linear_wgrad_small_r, after asserting that ops.igemm_tile / ops.wgrad_path name the small kernel for the row).  Every tensor of
every launch is a view between poisoned guards; every launch runs twice into fresh buffers: bit-identical; after each launch no output
element may be left poisoned and every guard must be bit-unchanged, and after the row every input.  Every output element is held to a
bar derived from the arithmetic and computed from the float64 reference (the table's docstring); pooled values, winner slots, routed
gradients, the accuracy, padding columns, found_inf, x * loss_scale and the scaler transitions are exact.

The worst error / bar per output is printed before it is asserted (`pytest -s`), and per entry kind when the module ends."""
import pytest
import torch

import step_head_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    yield torch.device("cuda:0")
    T.print_worst()
    print(f"largest |sgd_step_dev(scaler = NULL) - sgd_step|: {T.SGD_DEV_DIFF[0]:.3e}", flush=True)


@pytest.mark.parametrize("row", T.ROWS, ids=[T.row_id(kr) for kr in T.ROWS])
def test_row_against_fp64(dev, row):
    T.run_row(row, dev)

