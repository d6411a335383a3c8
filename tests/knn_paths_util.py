"""What the tests of the kNN detector's bank kinds share."""
import torch


def fp32_rows_held(det):
    """Names of the attributes of `det` through which a float32 tensor of two dimensions and the bank's width can be reached:
    the attribute itself, or one level into a dict, a tuple, a list or an object's own attributes.  [] for a detector whose bank is
    fp16 or int8 states that no fp32 copy of the bank outlived ``fit``."""
    width = int(det.bank.shape[1])
    held = []
    for name, value in vars(det).items():
        if isinstance(value, dict):
            inner = list(value.values())
        elif isinstance(value, (tuple, list)):
            inner = list(value)
        else:
            inner = list(getattr(value, "__dict__", {}).values())
        if any(torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == width for t in [value] + inner):
            held.append(name)
    return held
