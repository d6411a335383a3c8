"""Time of the bank-split cosine k-NN (csrc/knn.hip ssad_cosine_knn_split) against the one-launch kernel for banks the size of a whole
training set: R = 123 000 rows (70 % of bottle's 209 images x 841 patches), D = 512, N = 841 (one image), 13 456 (16 images) and
70 000 queries; every split count of a sweep, the rule's pick (ops.knn_splits) and the fraction of the fp32-MFMA peak (157.3 TFLOP/s)
by 2 N R D.  With --inference, also the wall time of tools.inference(patch_localization=True) with the default and the whole-training-set
bank on a synthetic 209-image category (seeded weights).
   python tools/knn_split_probe.py [--inference]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
from self_supervised import ops

PEAK = 157.3e12
dev = torch.device("cuda", 0)
R, D = 123000, 512


def timed(fn, reps=10):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels():
    g = torch.Generator(device=dev).manual_seed(0)
    bank = ops.l2_normalize_rows(torch.randn((R, D), device=dev, generator=g))
    x_all = torch.randn((70000, D), device=dev, generator=g)
    res = []
    for n in (841, 13456, 70000):
        x = x_all[:n]
        flop = 2.0 * n * R * D
        pick = ops.knn_splits(n, R)
        row = {"N": n, "R": R, "D": D, "rule_S": pick}
        os.environ["SSAD_KNN_SPLIT"] = "0"
        row["fused_ms"] = timed(lambda: ops.cosine_knn_fused(x, bank, 3))
        del os.environ["SSAD_KNN_SPLIT"]
        sweep = {}
        for s in sorted({1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 30, 48, pick}):
            sweep[s] = timed(lambda: ops.cosine_knn_split(x, bank, 3, s))
        row["split_ms"] = sweep
        row["rule_ms"] = timed(lambda: ops.cosine_knn_fused(x, bank, 3))
        row["speedup_rule_vs_fused"] = row["fused_ms"] / row["rule_ms"]
        row["peak_frac_fused"] = flop / (row["fused_ms"] * 1e-3) / PEAK
        row["peak_frac_rule"] = flop / (row["rule_ms"] * 1e-3) / PEAK
        row["peak_frac_best_split"] = flop / (min(sweep.values()) * 1e-3) / PEAK
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


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
    for bank in ("reference", "train", "reference", "train"):         # second round: warm caches
        np.random.seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank=bank)
        torch.cuda.synchronize()
        out[bank] = time.perf_counter() - t0
    print(json.dumps({"inference_wall_s": out, "train_images": 209, "test_images": 83}), flush=True)


if __name__ == "__main__":
    kernels()
    if "--inference" in sys.argv:
        inference_wall()
