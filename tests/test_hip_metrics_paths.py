"""Every entry point of csrc/auroc.hip -- AUROC, the PRO curve, the F1-optimal threshold, the confusion counts -- against exact
references (the table: tests/metrics_table.py).

One test per row.  The C entry points are called directly; every device buffer is a view between poisoned guards (inputs between
bytes that read as a huge finite score and as label 1), the workspace is exactly ssad_*_workspace(n) bytes and is filled with 0xA5 for
the first of two launches and 0x5A for the second: bit-identical outputs, guards bit-unchanged after each launch, inputs after the row,
and the wrappers of metrics.py return what the direct call returned.  Every comparison is an equality except `pros` of the
general-weights row, whose worst error / bar is printed (`pytest -s`) before it is asserted."""
import pytest
import torch

import metrics_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    yield torch.device("cuda:0")
    for kind, v in sorted(T.WORST.items()):
        print(f"worst {kind}: err / bar {v:.3e}", flush=True)


@pytest.mark.parametrize("row", T.ROWS, ids=[r.id for r in T.ROWS])
def test_row_against_exact_reference(dev, row):
    T.run_row(row, dev)


def test_refusals_leave_the_outputs_untouched(dev):
    T.run_argument_checks(dev)
