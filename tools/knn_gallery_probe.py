"""Time of the gallery kNN kernel (csrc/knn_gallery.hip ssad_l2_knn_gallery) beside the exact Euclidean search of the whole bank
(csrc/knn_l2.hip ssad_l2_knn_fused) at the shapes of DESIGN §4.16: T = 146 bank images, P = 1024 and 841 rows per image,
D = 384, Q = 1 and 83 query images, K = 10 and 50, k = 3.  With --parent-lib PATH the exact side is the library built from the PARENT
commit (through ctypes) -- the kernel a user ran before the gallery existed; without it, this build's.  The sides of a row alternate
inside one loop and the medians of the per-call event times are reported, with the stage-1 prologue (group_means, l2_direct, sort)
timed in the same loop.  With --inference, also the wall time of tools.inference(patch_localization=True, bank='train',
localization='dense', metric='euclidean') with the exact bank, coreset=0.01 and gallery=50 on a synthetic 209 / 83-image category
(seeded weights), second round.
   python tools/knn_gallery_probe.py [--parent-lib PATH] [--inference | --inference-only]"""
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
from self_supervised import _hip, ops

dev = torch.device("cuda", 0)


def alternate(fns, reps=15):
    """Median event time (ms) of each callable of `fns` (a dict), the callables taking turns inside one loop."""
    for fn in fns.values():
        for _ in range(2):
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


def exact_kernel(path):
    """ssad_l2_knn_fused of a build of the library (the parent commit's, or this one's): fn(x, bank, bsq, s)."""
    lib = ctypes.CDLL(path) if path else _hip.lib()
    lib.ssad_l2_knn_fused.argtypes = _hip.SIGNATURES["ssad_l2_knn_fused"]

    def mean(x, bank, bsq, s):
        n, d = x.shape
        out = torch.empty(n, device=dev)
        part = torch.empty((s, n, 3), device=dev) if s > 1 else None
        rc = lib.ssad_l2_knn_fused(x.data_ptr(), bank.data_ptr(), bsq.data_ptr(), _hip.ptr(part, True), out.data_ptr(), n, d, bank.shape[0],
                                   3, s, _hip.stream())
        assert rc == 0
    return mean


def kernels(exact, which):
    g = torch.Generator(device=dev).manual_seed(0)
    t, d = 146, 384
    for p in (1024, 841):
        bank = torch.randn((t * p, d), device=dev, generator=g)
        bsq = ops.row_sqnorms(bank)
        desc = ops.group_means(bank, p)
        x_all = torch.randn((83 * p, d), device=dev, generator=g)
        for q in (1, 83):
            x = x_all[:q * p]
            s_exact = ops.knn_splits(q * p, t * p)

            def stage1(kk):
                d2 = ops.l2_direct(ops.group_means(x, p), desc)
                return torch.sort(d2, dim=1, stable=True)[1][:, :kk].to(torch.int32).contiguous()
            for kk in (10, 50):
                gal = stage1(kk)
                s = ops.gallery_splits(q, p, kk)
                row = {"T": t, "P": p, "D": d, "Q": q, "K": kk, "rule_S": s, "exact_S": s_exact, "exact_side": which}
                row.update(alternate({"exact_ms": lambda: exact(x, bank, bsq, s_exact),
                                      "gallery_ms": lambda: ops.l2_knn_gallery(x, bank, bsq, gal, p, 3),
                                      "gallery_S1_ms": lambda: ops.l2_knn_gallery(x, bank, bsq, gal, p, 3, splits=1),
                                      "stage1_ms": lambda: stage1(kk)}))
                row["gallery_over_exact"] = row["gallery_ms"] / row["exact_ms"]
                row["K_over_T"] = kk / t
                row["ratio_over_K_over_T"] = row["gallery_over_exact"] / row["K_over_T"]
                print(json.dumps(row), flush=True)


def inference_wall():
    from fake_mvtec import make_tree
    from oracle import weights
    from self_supervised import datasets, tools
    os.environ.setdefault("SSAD_ALLOW_RANDOM_BACKBONE", "1")
    tmp = tempfile.mkdtemp()
    root = make_tree(os.path.join(tmp, "data"), categories=("bottle",), n_train=209, n_test_good=20, n_test_bad=63, size=256)
    ck = os.path.join(tmp, "seeded.ckpt")
    torch.save({"state_dict": weights.seeded_state_dict(0), "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    datasets._DataModule.num_workers = 0
    out = {}
    for _ in range(2):                                                # second round: warm caches
        for name, kw in (("exact", {}), ("coreset_0.01", {"coreset": 0.01}), ("gallery_50", {"gallery": 50})):
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                            localization='dense', metric='euclidean', **kw)
            torch.cuda.synchronize()
            out[name] = time.perf_counter() - t0
    print(json.dumps({"inference_wall_s": out, "bank": "train", "localization": "dense", "metric": "euclidean", "train_images": 209,
                      "test_images": 83}), flush=True)


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    if "--inference-only" not in sys.argv:
        kernels(exact_kernel(path), "parent" if path else "this build")
    if "--inference" in sys.argv or "--inference-only" in sys.argv:
        inference_wall()
