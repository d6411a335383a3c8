"""Times the inverted-file search of the Euclidean kNN beside the flat search: event-timed medians, the two taking
turns in one loop on the same inputs.  Rows are a seeded Gaussian mixture (real features do not exist offline): `--blobs` centres,
unit spread.  Prints one JSON line per setting.

    python tools/knn_ivf_probe.py --d 384 --images 83 --bank-images 146 --p 1024 --nprobe 1 8 32 --reps 7
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


def mixture(n, d, blobs, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn((blobs, d), generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float32) * 2.0
    which = torch.randint(0, blobs, (n,), generator=g)
    return (centres[which] + torch.randn((n, d), generator=g, dtype=torch.float32)).to(device).contiguous()


def timed(fns, reps):
    """Median milliseconds of every callable, the callables taking turns in one loop."""
    ms = [[] for _ in fns]
    for _ in range(reps + 1):                                       # the first round warms up
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [float(np.median(m[1:])) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--images", type=int, nargs="+", default=[83, 1])
    ap.add_argument("--bank-images", type=int, default=146)
    ap.add_argument("--p", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from self_supervised import ops
    from self_supervised.models import ivf_nlist
    dev = torch.device("cuda")
    r = a.bank_images * a.p
    bank = mixture(r, a.d, a.blobs, 2, dev)
    nlist = ivf_nlist(None, r)
    torch.cuda.synchronize()
    # fit: k-means, and the assignment search's share of it
    fit = lambda: ops.kmeans_l2(bank, nlist)
    (fit_ms,) = timed([fit], 2)
    ops.PROFILE = []
    fit()
    recs = ops.drain_profile()
    ops.PROFILE = None
    share = sum(x["ms"] for x in recs if x["kernel"].startswith("l2_knn_index")) / max(sum(x["ms"] for x in recs), 1e-9)
    cent, assign = fit()
    sorted_cells, perm = torch.sort(assign, stable=True)
    bank_s = bank.index_select(0, perm).contiguous()
    bsq_s, bsq = ops.row_sqnorms(bank_s), ops.row_sqnorms(bank)
    offsets, perm32, csq = ops.cell_offsets(sorted_cells, nlist), perm.to(torch.int32), ops.row_sqnorms(cent)
    sizes = (offsets[1:] - offsets[:-1]).cpu().numpy()
    print(json.dumps({"fit": True, "d": a.d, "rows": r, "nlist": nlist, "kmeans_ms": round(fit_ms, 2),
                      "assignment_share_of_kernel_time": round(share, 3), "cells_min_median_max": [int(sizes.min()), int(np.median(sizes)),
                                                                                                 int(sizes.max())],
                      "empty": int((sizes == 0).sum())}), flush=True)
    for q in a.images:
        n = q * a.p
        x = mixture(n, a.d, a.blobs, 3, dev)
        flat_i = ops.l2_knn_index(x, bank, bsq, 3)
        flat_o = ops.l2_knn_fused(x, bank, bsq, 3)
        for nprobe in a.nprobe:
            nprobe = min(nprobe, nlist)
            probes = ops.ivf_probes(x, cent, csq, nprobe)
            search = lambda: ops.l2_knn_ivf(x, bank_s, bsq_s, offsets, probes, perm32, 3)
            coarse = lambda: ops.ivf_probes(x, cent, csq, nprobe)
            sched = lambda: ops.ivf_schedule(probes, nlist)
            flat = lambda: ops.l2_knn_fused(x, bank, bsq, 3)
            t_search, t_coarse, t_sched, t_flat = timed([search, coarse, sched, flat], a.reps)
            _, idx = ops.l2_knn_ivf_index(x, bank_s, bsq_s, offsets, probes, perm32, 3)
            out = search()
            rel = ((out - flat_o) / flat_o)
            arith = (nlist + nprobe * r / nlist) / r
            total = t_search + t_coarse
            print(json.dumps({"d": a.d, "queries": n, "rows": r, "nlist": nlist, "nprobe": nprobe, "flat_ms": round(t_flat, 3),
                              "ivf_search_ms": round(t_search, 3), "of_which_schedule_ms": round(t_sched, 3),
                              "coarse_ms": round(t_coarse, 3), "ivf_total_ms": round(total, 3), "ivf_over_flat": round(total / t_flat, 4),
                              "arithmetic_ratio": round(arith, 5), "ratio_over_arithmetic": round(total / t_flat / arith, 2),
                              "recall_at_1": round(float((idx[:, 0] == flat_i[1][:, 0]).float().mean()), 4),
                              "map_rel_change_max": float(rel.max()), "map_rel_change_mean": float(rel.mean())}), flush=True)


if __name__ == "__main__":
    main()
