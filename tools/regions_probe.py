"""Time of the defect-region kernels, medians of ONE run, the candidates taking turns inside one loop:
(a) ops.label_regions + ops.region_stats on 83 x 256 x 256, event-timed: thresholded blob maps (the workload) against one
    one-pixel-wide spiral per image (the longest path an image of that size holds) -- the design goal is that the time does not
    grow with the path length, so the ratio spiral / blobs is reported -- with ops.bn_apply_fwd over the same byte count as the
    byte-bound yardstick;
(b) metrics.compute_pro_gpu(labelling='device') beside labelling='host' on the same maps and ground truths, WALL time (the host
    loop is CPU time: events do not see it).
   python tools/regions_probe.py"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import regions_ref as ref
from self_supervised import metrics, ops

dev = torch.device("cuda", 0)
N, SIDE = 83, 256


def alternate(fns, reps=15, warm=2, wall=False):
    """Median time (ms) of each callable of `fns` (a dict), the callables taking turns inside one loop; events, or the wall clock
    around a synchronised call."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            if wall:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append(1e3 * (time.perf_counter() - t0))
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def label_and_stats():
    blobs = torch.from_numpy(ref.blobs(N, SIDE, seed=1)).to(dev)
    spiral = torch.from_numpy(np.repeat(ref.spiral(SIDE)[None], N, 0).astype(np.float32)).to(dev)
    thr = 0.62
    c = 128
    z = torch.randn((N * SIDE * SIDE // c, c), device=dev)                      # 4 bytes read + 4 written per pixel
    mean, invstd, gamma, beta = torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.ones(c, device=dev), torch.zeros(c, device=dev)

    def run(x, stats=True):
        labels, _, offsets = ops.label_regions(x, thr)
        if stats:
            ops.region_stats(labels, offsets, x)                               # reads offsets[n] back: one synchronisation

    ms = alternate({"bn_apply_fwd_same_pixels": lambda: ops.bn_apply_fwd(z, mean, invstd, gamma, beta, None, True),
                    "blobs_label": lambda: run(blobs, False), "spiral_label": lambda: run(spiral, False),
                    "blobs_label_stats": lambda: run(blobs), "spiral_label_stats": lambda: run(spiral)})
    regions = {k: int(ops.label_regions(x, thr)[2][-1].item()) for k, x in (("blobs", blobs), ("spiral", spiral))}
    print(json.dumps({"label_regions_83x256x256_ms": ms, "regions": regions,
                      "spiral_over_blobs_label": round(ms["spiral_label"] / ms["blobs_label"], 3),
                      "spiral_over_blobs_label_stats": round(ms["spiral_label_stats"] / ms["blobs_label_stats"], 3)}), flush=True)


def pro_curve():
    maps = torch.from_numpy(ref.blobs(N, SIDE, seed=2)).to(dev)
    gts = torch.from_numpy((ref.blobs(N, SIDE, seed=3) >= 0.75).astype(np.uint8))
    gts[:20] = 0                                                               # the good test images of a category
    f0, p0 = metrics.compute_pro_gpu(maps, gts)
    f1, p1 = metrics.compute_pro_gpu(maps, gts, labelling="device")
    ms = alternate({"host": lambda: metrics.compute_pro_gpu(maps, gts),
                    "device": lambda: metrics.compute_pro_gpu(maps, gts, labelling="device")}, reps=7, warm=1, wall=True)
    print(json.dumps({"compute_pro_gpu_wall_ms": ms, "equal_bits": bool(np.array_equal(f0, f1) and np.array_equal(p0, p1)),
                      "curve_points": int(len(f0)), "ground_truth_regions": int(ref.label_batch(gts.numpy(), 8)[2][-1])}), flush=True)


if __name__ == "__main__":
    label_and_stats()
    pro_curve()
