"""Times of the stage-pyramid rows (PaDiM's / SPADE's embedding), event-timed medians of one run, the candidates taking
turns in one loop.
(a) the kernel (csrc/pyramid_features.hip) at 256 images of 256 x 256 pixels -- maps 64 x 64 x 64, 32 x 32 x 128, 16 x 16 x 256 -- with
    all 448 columns and with PaDiM's 96, beside ops.bn_apply_fwd over the same byte count (the project's byte-bound yardstick) and the
    torch composition on the same inputs (F.interpolate nearest + cat + index_select);
(b) ops.position_gaussian_fit_stats (146 images) and ops.position_mahalanobis (83 images) at P = 4096, d = 96, on preselected rows
    (96 columns, identity selection) and on the full 448-column rows;
with --inference, (c) the wall time of tools.inference(bank='train', localization='dense', detector='padim') on the synthetic 209 /
    83-image category of §4.8 (seeded weights) with dense_features='pyramid' beside 'local', second round.
   python tools/pyramid_probe.py [--inference]"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ.setdefault("SSAD_ALLOW_RANDOM_BACKBONE", "1")
import numpy as np
import torch
import torch.nn.functional as F
from self_supervised import ops
from self_supervised.density import position_channels, position_gaussian_factor

dev = torch.device("cuda", 0)
STAGES = ((64, 64, 64), (32, 32, 128), (16, 16, 256))
N_IMG, N_FIT, N_QUERY, P, D, d = 256, 146, 83, 4096, 448, 96


def alternate(fns, reps=15, warm=2):
    """Median event time (ms) of each callable of `fns` (a dict), the callables taking turns inside one loop."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in times.items()}


def yardstick(nbytes, g):
    c = 128
    z = torch.randn((nbytes // 8 // c, c), device=dev, generator=g)
    bn = (torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.ones(c, device=dev), torch.zeros(c, device=dev))
    return (lambda: ops.bn_apply_fwd(z, *bn, None, True)), 8 * z.numel()


def kernel():
    g = torch.Generator(device=dev).manual_seed(0)
    maps = [torch.randn((N_IMG, h, w, c), device=dev, generator=g) for h, w, c in STAGES]
    sel = position_channels(D, d, 0)
    sel_dev = ops.pyramid_sel(sel, D, dev)
    idx = sel.to(dev)
    nchw = [m.permute(0, 3, 1, 2) for m in maps]                      # torch's layout for interpolate (views: no copy is timed)

    def torch_form(pick):
        up = torch.cat([nchw[0]] + [F.interpolate(m, size=STAGES[0][:2], mode='nearest') for m in nchw[1:]], dim=1)
        rows = up.permute(0, 2, 3, 1).reshape(N_IMG * P, D)
        return rows.index_select(1, idx) if pick else rows.contiguous()
    for name, s, width in (("all_448", None, D), ("padim_96", sel_dev, d)):
        out = torch.empty((N_IMG * P, width), device=dev)
        nbytes = 4 * (sum(m.numel() for m in maps) + out.numel())
        bn, bn_bytes = yardstick(nbytes, g)
        ms = alternate({"bn_apply_fwd": bn, "stage_pyramid_rows": lambda: ops.stage_pyramid_rows(maps, out=out, sel_dev=s),
                        "torch": lambda: torch_form(s is not None)}, reps=11)
        row = {"columns": width, "images": N_IMG, "bytes": nbytes, "yardstick_bytes": bn_bytes,
               "equals_torch": bool(torch.equal(out, torch_form(s is not None)))}
        for k, v in ms.items():
            row[k + "_ms"] = round(v, 4)
        row["stage_pyramid_rows_GBps"] = round(nbytes / ms["stage_pyramid_rows"] / 1e6, 1)
        row["bn_apply_fwd_GBps"] = round(bn_bytes / ms["bn_apply_fwd"] / 1e6, 1)
        print(json.dumps({"kernel": {name: row}}), flush=True)
        del out, bn


def gaussians():
    g = torch.Generator(device=dev).manual_seed(1)
    base = torch.randn((1, P, D), device=dev, generator=g) * 2.0
    fit = (base + torch.randn((N_FIT, P, D), device=dev, generator=g)).reshape(N_FIT * P, D).contiguous()
    q = (base + 1.5 * torch.randn((N_QUERY, P, D), device=dev, generator=g)).reshape(N_QUERY * P, D).contiguous()
    sel = position_channels(D, d, 0)
    full_sel = ops.position_sel(sel, D, dev)
    ident = ops.position_sel(torch.arange(d), d, dev)
    fit_pre, q_pre = fit.index_select(1, sel.to(dev)).contiguous(), q.index_select(1, sel.to(dev)).contiguous()
    ms = alternate({"fit_stats_preselected": lambda: ops.position_gaussian_fit_stats(fit_pre, None, N_FIT, P, sel_dev=ident),
                    "fit_stats_448": lambda: ops.position_gaussian_fit_stats(fit, None, N_FIT, P, sel_dev=full_sel)}, reps=5, warm=1)
    a, b = ops.position_gaussian_fit_stats(fit_pre, None, N_FIT, P, sel_dev=ident), ops.position_gaussian_fit_stats(fit, None, N_FIT, P,
                                                                                                                   sel_dev=full_sel)
    row = {k + "_ms": round(v, 3) for k, v in ms.items()}
    row.update(images=N_FIT, P=P, d=d, mean_bit_equal=bool(torch.equal(a[0], b[0])), scatter_bit_equal=bool(torch.equal(a[1], b[1])),
               rows_bytes_preselected=4 * fit_pre.numel(), rows_bytes_448=4 * fit.numel())
    print(json.dumps({"fit_stats": row}), flush=True)
    mu_hi, mu_lo, w = ops.position_gaussian_factor(a[0], a[1].clone(), N_FIT, 0.01)
    del fit, fit_pre, a, b
    o1, o2 = torch.empty(N_QUERY * P, device=dev), torch.empty(N_QUERY * P, device=dev)
    ms = alternate({"mahalanobis_preselected": lambda: ops.position_mahalanobis(q_pre, None, mu_hi, mu_lo, w, N_QUERY, P, sel_dev=ident,
                                                                                out=o1),
                    "mahalanobis_448": lambda: ops.position_mahalanobis(q, None, mu_hi, mu_lo, w, N_QUERY, P, sel_dev=full_sel, out=o2)},
                   reps=11)
    row = {k + "_ms": round(v, 3) for k, v in ms.items()}
    row.update(images=N_QUERY, P=P, d=d, scores_bit_equal=bool(torch.equal(o1, o2)), w_bytes=4 * w.numel(),
               rows_bytes_preselected=4 * q_pre.numel(), rows_bytes_448=4 * q.numel())
    print(json.dumps({"mahalanobis": row}), flush=True)


def inference_wall():
    from fake_mvtec import make_tree
    from oracle import weights
    from self_supervised import datasets, tools
    tmp = tempfile.mkdtemp()
    root = make_tree(os.path.join(tmp, "data"), categories=("bottle",), n_train=209, n_test_good=20, n_test_bad=63, size=256)
    ck = os.path.join(tmp, "seeded.ckpt")
    torch.save({"state_dict": weights.seeded_state_dict(0), "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    datasets._DataModule.num_workers = 0
    out = {}
    os.environ["SSAD_TIMELINE"] = "1"
    for _ in range(2):                                                # second round: warm caches
        for feats in ("local", "pyramid"):
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                                  localization='dense', detector='padim', dense_features=feats)
            torch.cuda.synchronize()
            out["padim_96_" + feats] = round(time.perf_counter() - t0, 3)
            out["padim_96_" + feats + "_map"] = list(res.anomaly_maps.shape)
            t = tools.TIMELINE
            out["padim_96_" + feats + "_phases"] = {b[0]: round(b[1] - a[1], 3) for a, b in zip(t, t[1:])}
    print(json.dumps({"inference_wall_s": out, "bank": "train", "localization": "dense", "train_images": 209, "test_images": 83}),
          flush=True)


if __name__ == "__main__":
    kernel()
    gaussians()
    if "--inference" in sys.argv:
        inference_wall()
