"""Reference of the stage-pyramid rows (csrc/pyramid_features.hip, ops.stage_pyramid_rows): integer index arithmetic on the CPU.

out[(n, i, j)][k] = m_s[n][(i H_s) // H_0][(j W_s) // W_0][c] for the stage s and channel c of column sel[k] of the concatenation.  A
copy has no error bar: the tests compare with torch.equal."""
import torch

# (N; (H, W, C) per stage, finest first)
CASES = {
    "2;8x8x8,4x4x16,2x2x32": (2, ((8, 8, 8), (4, 4, 16), (2, 2, 32))),
    "1;9x9x8,5x5x8,3x3x12": (1, ((9, 9, 8), (5, 5, 8), (3, 3, 12))),                    # non-integer ratios
    "2;6x10x4,3x5x8,2x3x8": (2, ((6, 10, 4), (3, 5, 8), (2, 3, 8))),                    # non-square
    "3;16x16x64,8x8x128,4x4x256": (3, ((16, 16, 64), (8, 8, 128), (4, 4, 256))),        # a 64-pixel image
    "2;8x8x8,4x4x16": (2, ((8, 8, 8), (4, 4, 16))),                                     # two maps only
    "4;64x64x64,32x32x128,16x16x256": (4, ((64, 64, 64), (32, 32, 128), (16, 16, 256))),  # full size
}


def maps(n, stages, seed=0):
    """Seeded NHWC fp32 stage maps [n][H][W][C]; every element distinct within a map, so a wrong source shows."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((n, h, w, c), generator=g, dtype=torch.float32) for h, w, c in stages]


def selections(stages, position_channels=None):
    """name -> sel (None or an int64 vector): the selections of the issue for the widths `stages` gives."""
    widths = [c for _, _, c in stages]
    D = sum(widths)
    starts = [sum(widths[:s]) for s in range(len(widths))]
    out = {"none": None, "single": torch.tensor([D // 2 + 1]),
           "first-and-last-of-every-stage": torch.tensor(sorted({v for a, c in zip(starts, widths) for v in (a, a + c - 1)})),
           "coarsest-only": torch.arange(starts[-1] + 1, D, 2), "finest-only": torch.arange(0, widths[0], 3)}
    if D == 448 and position_channels is not None:
        out["padim-96"] = position_channels(448, 96, 0)
    return out


def reference(ms, sel=None):
    """ms: NHWC maps, finest first (any float dtype, on the CPU) -> [N * H_0 * W_0][d], bit copies of the sources."""
    n, h0, w0, _ = ms[0].shape
    i, j = torch.arange(h0), torch.arange(w0)
    parts = []
    for m in ms:
        _, h, w, _ = m.shape
        src_i, src_j = (i * h) // h0, (j * w) // w0
        parts.append(m[:, src_i][:, :, src_j])
    rows = torch.cat(parts, dim=3).reshape(n * h0 * w0, -1)
    return rows if sel is None else rows[:, torch.as_tensor(sel).long()]
