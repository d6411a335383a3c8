"""Time of the dense feature-map localisation, event-timed medians of one run:
(a) the kernel alone (csrc/patch_features.hip) at the workload's size -- N = 256 maps of 32 x 32 x 128 / 16 x 16 x 256, 604 MB read and
    written -- for every row band and the automatic one, as GB/s, beside ops.bn_apply_fwd on a tensor of the same byte count (the
    project's byte-bound yardstick) inside the same loop;
(b) model(x) for 256 images of 256 x 256 in dense mode against patch mode, taking turns;
with --inference, also the wall time of tools.inference(patch_localization=True, bank='train', coreset=0.01) on the synthetic 209 / 83-image
category of §4.8 (seeded weights) with localization='patches' and 'dense', second round.
   python tools/dense_probe.py [--inference]"""
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
from self_supervised import ops

dev = torch.device("cuda", 0)


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


def kernel_alone(n=256):
    g = torch.Generator(device=dev).manual_seed(0)
    fine = torch.randn((n, 32, 32, 128), device=dev, generator=g)
    coarse = torch.randn((n, 16, 16, 256), device=dev, generator=g)
    out = torch.empty((n * 1024, 384), device=dev)
    nbytes = 4 * (fine.numel() + coarse.numel() + out.numel())
    # the yardstick: y = relu(z * a + b) over as many bytes (half read, half written)
    c = 128
    z = torch.randn((nbytes // 8 // c, c), device=dev, generator=g)
    mean, invstd, gamma, beta = (torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.ones(c, device=dev),
                                 torch.zeros(c, device=dev))
    fns = {"bn_apply_fwd": lambda: ops.bn_apply_fwd(z, mean, invstd, gamma, beta, None, True)}
    for rb in (0, 1, 2, 4, 8, 16, 32):
        fns[f"rows_per_block_{rb}"] = (lambda rb=rb: ops.local_patch_features(fine, coarse, out=out, rows_per_block=rb))
    ms = alternate(fns)
    row = {"N": n, "bytes": nbytes, "yardstick_bytes": 8 * z.numel()}
    for k, v in ms.items():
        row[k + "_ms"] = round(v, 4)
        row[k + "_GBps"] = round((8 * z.numel() if k == "bn_apply_fwd" else nbytes) / v / 1e6, 1)
    print(json.dumps({"kernel_alone": row}), flush=True)


def forward_256():
    from oracle import weights
    from self_supervised.models import PeraNet
    m = PeraNet()
    m.load_state_dict(weights.seeded_state_dict(0))
    m.eval().to(dev)
    x = weights.synthetic_images(256, 256, seed=7).to(dev)

    def run(dense):
        (m.disable_patch_level_mode if dense else m.disable_dense_mode)()
        (m.enable_dense_mode if dense else m.enable_patch_level_mode)()
        with torch.no_grad():
            m(x)
    ms = alternate({"patches": lambda: run(False), "dense": lambda: run(True)}, reps=7, warm=1)
    print(json.dumps({"model_forward_256_images_ms": {k: round(v, 3) for k, v in ms.items()},
                      "rows": {"patches": [256 * 841, 512], "dense": [256 * 1024, 384]}}), flush=True)


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
    for _ in range(2):                                                # second round: warm caches
        for name in ("patches", "dense"):
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                                  coreset=0.01, localization=name)
            torch.cuda.synchronize()
            out[name] = round(time.perf_counter() - t0, 3)
            out[name + "_map"] = list(res.anomaly_maps.shape)
    print(json.dumps({"inference_wall_s": out, "bank": "train", "coreset": 0.01, "train_images": 209, "test_images": 83}), flush=True)


if __name__ == "__main__":
    kernel_alone()
    forward_256()
    if "--inference" in sys.argv:
        inference_wall()
