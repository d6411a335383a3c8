"""float64 yardsticks of the greedy k-center coreset (csrc/coreset.hip ssad_coreset_greedy), shared by the coreset tests."""
import numpy as np
import torch


def greedy64(p, m, start=0):
    """numpy float64 farthest-point selection: sel[0] = start, sel[t] = argmax_r min_{s<t} |p_r - p_sel[s]|^2 (np.argmax: ties to the
    smallest row), rad[t] = that maximum (rad[0] = inf); stops when the maximum is 0."""
    p = np.asarray(p, dtype=np.float64)
    mind = ((p - p[start]) ** 2).sum(1)
    sel, rad = [int(start)], [np.inf]
    for _ in range(1, min(int(m), p.shape[0])):
        i = int(np.argmax(mind))
        if mind[i] == 0.0:
            break
        sel.append(i)
        rad.append(float(mind[i]))
        np.minimum(mind, ((p - p[i]) ** 2).sum(1), out=mind)
    return np.array(sel, dtype=np.int64), np.array(rad)


def replay64(p, sel, chunk=8192):
    """Replays a selection in float64 on p's device.  For every step t >= 1 returns (max_r mind64_t[r], mind64_t[sel[t]]), mind64_t[r]
    being the distance of row r to its nearest centre among sel[:t].  Squared distances are formed as |x|^2 + |c|^2 - 2 x.c in
    float64: their error is ~1e-13 of the values, far below the checks' 1e-5."""
    x = p.double()
    sel = sel.to(x.device)
    m = sel.numel()
    c = x.index_select(0, sel)
    cn = (c * c).sum(1)
    col_max = torch.full((m,), -1.0, dtype=torch.float64, device=x.device)
    at_sel = torch.empty(m, dtype=torch.float64, device=x.device)
    steps = torch.arange(m, device=x.device)
    for i in range(0, x.shape[0], chunk):
        xb = x[i:i + chunk]
        dist = ((xb * xb).sum(1, keepdim=True) + cn[None, :] - 2.0 * (xb @ c.t())).clamp_min_(0.0)
        cm = torch.cummin(dist, dim=1).values                   # cm[r, t] = distance to the nearest of centres 0..t
        col_max = torch.maximum(col_max, cm.max(0).values)
        t_in = steps[(sel >= i) & (sel < i + xb.shape[0]) & (steps >= 1)]
        at_sel[t_in] = cm[sel[t_in] - i, t_in - 1]
    return col_max[:-1].cpu().numpy(), at_sel[1:].cpu().numpy()
