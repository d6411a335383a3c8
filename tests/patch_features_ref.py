"""The float64 reference of the locally aware patch features (csrc/patch_features.hip), the shapes and the error bar its tests share.

Reference: the library calls themselves -- F.avg_pool2d(3, 1, 1) of both stage maps, F.interpolate(bilinear, align_corners=False) of the
coarser one to the finer grid, torch.cat -- in float64 on the CPU (anomalib's PatchCore feature construction), not a restatement of the
kernel.

Bar, per element: |out - ref| <= 40 * 2^-24 * A(|x|) (about 2.4e-6 of A), A(|x|) = the same reference applied to the absolute values of
the inputs -- every weight is non-negative, so that is the sum of the |terms| of the element.  Derived: an output is at most 9 adds and
one multiply for a pool, four corner weights of at most three roundings each and four more adds, about 20 roundings in any order; 40
leaves a factor 2 for another association.  A plain fp32 torch evaluation on the CPU stays within 5 of these units on every shape."""
import functools

import torch
import torch.nn.functional as F

UNIT = 2.0 ** -24
BAR_UNITS = 40.0

# (N, Hf, Wf, Cf, Hc, Wc, Cc): each the smallest shape at which one failure mode shows
SHAPES = [
    (1, 1, 1, 4, 1, 1, 4),              # every tap is padding
    (3, 5, 7, 8, 3, 4, 12),             # odd sizes, ratio not 2, non-square, n > 0 offsets
    (1, 6, 6, 8, 2, 2, 8),              # ratio 3, clamped at both edges
    (1, 4, 6, 8, 4, 6, 8),              # ratio 1
    (2, 9, 9, 32, 5, 5, 32),            # ratio (2k-1):k
    (2, 12, 12, 128, 6, 6, 256),        # the end-to-end test's geometry
    (2, 32, 32, 128, 16, 16, 256),      # the workload's geometry
    # the kernel's own thresholds: two pooled coarse rows leave the LDS room for fewer channels than the map has
    (1, 3, 5, 4, 2, 700, 12),           # channel chunks of 8 + 4, the coarse map wider than the fine one (downsampling)
    (1, 2, 3, 4, 2, 2048, 8),           # the widest coarse map: chunks of 4 channels
    (1, 7, 3, 4, 20, 2, 4),             # more coarse rows than fine ones: the rows in the LDS are never reused
]
ROWS_PER_BLOCK = (1, 3, 8)              # explicit row bands beside the automatic one; the bits may not depend on them


def reference(fine, coarse):
    """fine [N][Hf][Wf][Cf], coarse [N][Hc][Wc][Cc] (NHWC, any float type) -> float64 [N * Hf * Wf][Cf + Cc]."""
    f = fine.detach().cpu().double().permute(0, 3, 1, 2)
    c = coarse.detach().cpu().double().permute(0, 3, 1, 2)
    pf = F.avg_pool2d(f, 3, 1, 1)
    pc = F.interpolate(F.avg_pool2d(c, 3, 1, 1), size=tuple(f.shape[-2:]), mode='bilinear', align_corners=False)
    return torch.cat([pf, pc], 1).permute(0, 2, 3, 1).reshape(-1, f.shape[1] + c.shape[1]).contiguous()


@functools.lru_cache(maxsize=None)
def case(shape):
    """(fine, coarse, ref, bar) of one shape, computed once: N(0, 1) inputs, the fine map scaled by 100 u^4 per element so that
    neighbouring values differ by orders of magnitude; ref = reference(fine, coarse); bar = BAR_UNITS * UNIT * reference(|fine|,
    |coarse|).  Nobody writes to them."""
    n, hf, wf, cf, hc, wc, cc = shape
    g = torch.Generator().manual_seed(1000 + sum((k + 1) * v for k, v in enumerate(shape)))
    fine = torch.randn(n, hf, wf, cf, generator=g) * (100.0 * torch.rand(n, hf, wf, cf, generator=g) ** 4)
    coarse = torch.randn(n, hc, wc, cc, generator=g)
    return fine, coarse, reference(fine, coarse), BAR_UNITS * UNIT * reference(fine.abs(), coarse.abs())


def worst_units(out, shape):
    """The largest |out - ref| of the shape's case in units of UNIT * A(|x|) (the bar is BAR_UNITS)."""
    _, _, ref, bar = case(shape)
    return ((out.detach().cpu().double() - ref).abs() / (bar / BAR_UNITS)).max().item()
