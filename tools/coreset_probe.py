"""Time of the greedy k-center coreset selection (csrc/coreset.hip ssad_coreset_greedy) for banks the size of a whole training set:
R = 123 000 rows (70 % of bottle's 209 images x 841 patches), d = 128 (the projected rows the detector selects on) and d = 512 (the
unprojected rows), m = 1 % and 10 % of R; per step, and the bytes one step streams (R d 4) over its time.  Then the cosine 3-NN of
841 (one image) and 69 803 (83 images) queries against the exact 512-wide bank and against the 1 % and 10 % coresets.  With
--inference, also the wall time of tools.inference(bank='train', patch_localization=True) with coreset None / 0.1 / 0.01 on a
synthetic 209 / 83-image category (seeded weights).
   python tools/coreset_probe.py [--inference]"""
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

dev = torch.device("cuda", 0)
R, D = 123000, 512


def timed(fn, reps=5):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def selection():
    g = torch.Generator(device=dev).manual_seed(0)
    bank = ops.l2_normalize_rows(torch.randn((R, D), device=dev, generator=g))
    res = []
    for d in (128, 512):
        p = bank[:, :d].contiguous() if d < D else bank
        for frac in (0.01, 0.1):
            m = int(np.ceil(frac * R))
            n_sel = ops.coreset_greedy(p, m)[0].numel()
            ms = timed(lambda: ops.coreset_greedy(p, m), reps=3 if frac > 0.05 else 5)
            row = {"R": R, "d": d, "m": m, "selected": n_sel, "wgs": ops.coreset_workgroups(R), "select_ms": ms,
                   "us_per_step": 1e3 * ms / m, "step_TBps": R * d * 4 / (1e-3 * ms / m) / 1e12}
            res.append(row)
            print(json.dumps(row), flush=True)
    return bank


def knn(bank):
    g = torch.Generator(device=dev).manual_seed(1)
    x_all = torch.randn((69803, D), device=dev, generator=g)
    banks = {"exact": bank}
    for frac in (0.1, 0.01):
        sel, _ = ops.coreset_greedy(bank, int(np.ceil(frac * R)))
        banks[f"coreset_{frac}"] = bank.index_select(0, sel).contiguous()
    for n in (841, 69803):
        x = x_all[:n]
        row = {"N": n}
        for name, b in banks.items():
            row[name + "_rows"] = int(b.shape[0])
            row[name + "_ms"] = timed(lambda: ops.cosine_knn_fused(x, b, 3), reps=10)
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
    for cs in (None, 0.1, 0.01, None, 0.1, 0.01):          # second round: warm caches
        np.random.seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train', coreset=cs)
        torch.cuda.synchronize()
        out[str(cs)] = time.perf_counter() - t0
    print(json.dumps({"inference_wall_s": out, "train_images": 209, "test_images": 83}), flush=True)


if __name__ == "__main__":
    knn(selection())
    if "--inference" in sys.argv:
        inference_wall()
