"""Time of the GDE kernels (csrc/gde.hip) against the cosine k-NN kernel at the ResNet-18 patch-scoring size, in one process:
N = 256 x 841 = 215 296 queries, D = 512; the k-NN scores against a 588-row bank (the 70 % of one image's 841 patches).
Fraction of the fp32-MFMA peak (157.3 TFLOP/s) counts 2 N D^2 FLOP for the Mahalanobis kernel (dense W; the kernel skips W's zero
upper blocks, 62.5 % of the dense MFMAs at D = 512) and 2 N D R for the k-NN.
   python tools/gde_probe.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch
from self_supervised import ops
from self_supervised.density import ledoit_wolf_factor

PEAK = 157.3e12
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
N, D, R = 256 * 841, 512, 588


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


x = torch.randn((N, D), generator=g).to(dev)
fit = torch.randn((R, D), generator=g).to(dev)
bank = ops.l2_normalize_rows(fit)
mean, scatter, m4 = ops.gaussian_fit_stats(fit, True)
mu_hi, mu_lo, w, s = ledoit_wolf_factor(mean.cpu().numpy(), scatter.cpu().numpy(), m4.item(), R)
mu_hi, mu_lo, w = (torch.from_numpy(a).to(dev) for a in (mu_hi, mu_lo, w))

res = {}
ms, out = timed(lambda: ops.cosine_knn_fused(x, bank, 3))
res["knn_fused"] = {"N": N, "D": D, "R": R, "ms": round(ms, 4), "gflop": 2.0 * N * D * R / 1e9,
                    "frac_peak": round(2.0 * N * D * R / (ms * 1e-3) / PEAK, 3)}
ms, out = timed(lambda: ops.mahalanobis_fused(x, mu_hi, mu_lo, w, True))
res["mahalanobis_fused"] = {"N": N, "D": D, "ms": round(ms, 4), "gflop_dense": 2.0 * N * D * D / 1e9,
                            "frac_peak_dense": round(2.0 * N * D * D / (ms * 1e-3) / PEAK, 3),
                            "frac_peak_issued": round(2.0 * N * D * D * 0.625 / (ms * 1e-3) / PEAK, 3),
                            "finite": bool(torch.isfinite(out).all().item())}
res["mahalanobis_vs_knn"] = round(res["mahalanobis_fused"]["ms"] / res["knn_fused"]["ms"], 3)
ms, _ = timed(lambda: ops.gaussian_fit_stats(x, True), reps=5)
res["gaussian_fit_stats"] = {"N": N, "D": D, "ms": round(ms, 4), "gflop_fp64_lower": N * D * (D + 1) / 1e9}
ms, _ = timed(lambda: ops.gaussian_fit_stats(fit, True), reps=20)
res["gaussian_fit_stats_588"] = {"N": R, "D": D, "ms": round(ms, 4)}
print(json.dumps(res), flush=True)
