"""Time of the Euclidean k-NN kernels (csrc/knn_l2.hip ssad_l2_knn_fused / _index) against the cosine kernel of
the same shape (csrc/knn.hip), at the shapes of DESIGN §4.10: N = 841 / 13 456 / 70 000 queries, R = 588 / 12 300 / 123 000 bank rows,
D = 384 and 512, k = 3.  With --parent-lib PATH the cosine side is the library built from the PARENT commit (through ctypes) -- the
kernel a user ran before this metric existed; without it, this build's.  The sides of a row alternate inside one loop and the
medians of the per-call event times are reported.  Where the N x R matrix fits in memory the torch formulation
torch.cdist(x, bank).topk(3, largest=False) is timed in the same loop.  With --inference, also the wall time of
tools.inference(patch_localization=True, bank='train', localization='dense', coreset=0.01) with metric='cosine' and 'euclidean' on a
synthetic 209 / 83-image category (seeded weights), second round.
   python tools/knn_l2_probe.py [--parent-lib PATH] [--inference]"""
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
CDIST_MAX_BYTES = 8 << 30          # the N x R fp32 matrix torch.cdist writes


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


def cosine_kernels(path):
    """The three cosine entry points of a build of the library (the parent commit's, or this one's): name -> fn(x, bank, s)."""
    lib = ctypes.CDLL(path) if path else _hip.lib()
    for name in ("ssad_cosine_knn_fused", "ssad_cosine_knn_split", "ssad_cosine_knn_index"):
        getattr(lib, name).argtypes = _hip.SIGNATURES[name]

    def mean(x, bank, s):
        n, d = x.shape
        out = torch.empty(n, device=dev)
        if s == 1:
            rc = lib.ssad_cosine_knn_fused(x.data_ptr(), bank.data_ptr(), out.data_ptr(), n, d, bank.shape[0], 3, _hip.stream())
        else:
            part = torch.empty((s, n, 3), device=dev)
            rc = lib.ssad_cosine_knn_split(x.data_ptr(), bank.data_ptr(), part.data_ptr(), out.data_ptr(), n, d, bank.shape[0], 3, s,
                                           _hip.stream())
        assert rc == 0

    def index(x, bank, s):
        n, d = x.shape
        dist = torch.empty((n, 3), device=dev)
        idx = torch.empty((n, 3), device=dev, dtype=torch.int32)
        part = torch.empty((s, n, 3), device=dev, dtype=torch.int64) if s > 1 else None
        rc = lib.ssad_cosine_knn_index(x.data_ptr(), bank.data_ptr(), _hip.ptr(part, True, torch.int64), dist.data_ptr(), idx.data_ptr(), n,
                                       d, bank.shape[0], 3, s, _hip.stream())
        assert rc == 0
    return mean, index


def kernels(cos_mean, cos_index, which):
    g = torch.Generator(device=dev).manual_seed(0)
    for d in (384, 512):
        raw_all = torch.randn((123000, d), device=dev, generator=g)
        unit_all = ops.l2_normalize_rows(raw_all)
        sq_all = ops.row_sqnorms(raw_all)
        x_all = torch.randn((70000, d), device=dev, generator=g)
        for r in (588, 12300, 123000):
            raw, unit, sq = raw_all[:r], unit_all[:r], sq_all[:r]
            for n in (841, 13456, 70000):
                x = x_all[:n]
                s = ops.knn_splits(n, r)
                fns = {"cosine_mean_ms": lambda: cos_mean(x, unit, s), "l2_mean_ms": lambda: ops.l2_knn_fused(x, raw, sq, 3, splits=s),
                       "cosine_index_ms": lambda: cos_index(x, unit, s), "l2_index_ms": lambda: ops.l2_knn_index(x, raw, sq, 3, splits=s)}
                if 4 * n * r <= CDIST_MAX_BYTES:
                    fns["torch_cdist_topk_ms"] = lambda: torch.cdist(x, raw).topk(3, largest=False)
                row = {"N": n, "R": r, "D": d, "rule_S": s, "cosine_side": which}
                row.update(alternate(fns))
                row["l2_over_cosine_mean"] = row["l2_mean_ms"] / row["cosine_mean_ms"]
                row["l2_over_cosine_index"] = row["l2_index_ms"] / row["cosine_index_ms"]
                if "torch_cdist_topk_ms" in row:
                    row["torch_over_l2_mean"] = row["torch_cdist_topk_ms"] / row["l2_mean_ms"]
                print(json.dumps(row), flush=True)
        row = alternate({"row_sqnorms_123000_ms": lambda: ops.row_sqnorms(raw_all), "l2_normalize_123000_ms": lambda: ops.l2_normalize_rows(raw_all)})
        row["D"] = d
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
        for metric in ("cosine", "euclidean"):
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                            localization='dense', coreset=0.01, metric=metric)
            torch.cuda.synchronize()
            out[metric] = time.perf_counter() - t0
    print(json.dumps({"inference_wall_s": out, "bank": "train", "localization": "dense", "coreset": 0.01, "train_images": 209,
                      "test_images": 83}), flush=True)


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    kernels(*cosine_kernels(path), "parent" if path else "this build")
    if "--inference" in sys.argv:
        inference_wall()
