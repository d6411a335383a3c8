"""Time of the flat Euclidean search with half-precision operands (csrc/knn_l2_half.hip, ops.l2h_knn_fused / l2h_knn_index) against the
fp32 kernels of the same shape (csrc/knn_l2.hip ssad_l2_knn_fused / _index), at the 18 shapes of DESIGN §4.13:
N = 841 / 13 456 / 70 000 queries, R = 588 / 12 300 / 123 000 bank rows, D = 384 and 512, k = 3, and at the pyramid shape (340 000 x
598 000 rows, D = 448; --pyramid, fewer repetitions).  With --parent-lib PATH the fp32 side is the library built from the PARENT commit
(through ctypes) -- the kernel a user ran before this option existed; without it, this build's.  The sides of a row alternate inside
one loop and the medians of the per-call event times are reported.  The half side INCLUDES rounding the queries (ops.rows_to_half per
call); rounding the bank happens once at fit time and is reported on a line of its own.  Also recall@1 / recall@3 of the half search
against the fp32 flat search on the seeded Gaussian mixture of tools/knn_ivf_probe.py (real features do not exist offline).  With
--inference, the wall time of tools.inference(patch_localization=True, bank='train', localization='dense', metric='euclidean') with
either bank_dtype on a synthetic 209 / 83-image category (seeded weights), second round.
   python tools/knn_l2_half_probe.py [--parent-lib PATH] [--pyramid] [--inference]"""
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


def fp32_kernels(path):
    """The two fp32 Euclidean entry points of a build of the library (the parent commit's, or this one's): mean / index fn(x, bank, sq, s)."""
    lib = ctypes.CDLL(path) if path else _hip.lib()
    for name in ("ssad_l2_knn_fused", "ssad_l2_knn_index"):
        getattr(lib, name).argtypes = _hip.SIGNATURES[name]
    P = lambda t: None if t is None else t.data_ptr()

    def mean(x, bank, sq, s):
        n, d = x.shape
        out = torch.empty(n, device=dev)
        part = torch.empty((s, n, 3), device=dev) if s > 1 else None
        rc = lib.ssad_l2_knn_fused(P(x), P(bank), P(sq), P(part), P(out), n, d, bank.shape[0], 3, s, _hip.stream())
        assert rc == 0
        return out

    def index(x, bank, sq, s):
        n, d = x.shape
        dist = torch.empty((n, 3), device=dev)
        idx = torch.empty((n, 3), device=dev, dtype=torch.int32)
        part = torch.empty((s, n, 3), device=dev, dtype=torch.int64) if s > 1 else None
        rc = lib.ssad_l2_knn_index(P(x), P(bank), P(sq), P(part), P(dist), P(idx), n, d, bank.shape[0], 3, s, _hip.stream())
        assert rc == 0
        return dist, idx
    return mean, index


def one_shape(f32_mean, f32_index, x, raw, sq, bh, bhsq, which, reps):
    n, d = x.shape
    r = raw.shape[0]
    s = ops.knn_splits(n, r)
    fns = {"f32_mean_ms": lambda: f32_mean(x, raw, sq, s), "half_mean_ms": lambda: ops.l2h_knn_fused(x, bh, bhsq, 3, splits=s),
           "f32_index_ms": lambda: f32_index(x, raw, sq, s), "half_index_ms": lambda: ops.l2h_knn_index(x, bh, bhsq, 3, splits=s),
           "round_queries_ms": lambda: ops.rows_to_half(x)}
    row = {"N": n, "R": r, "D": d, "rule_S": s, "f32_side": which, "reps": reps}
    row.update(alternate(fns, reps))
    row["f32_over_half_mean"] = row["f32_mean_ms"] / row["half_mean_ms"]
    row["f32_over_half_index"] = row["f32_index_ms"] / row["half_index_ms"]
    row["half_mean_tflops"] = 2.0 * n * r * d / (row["half_mean_ms"] - row["round_queries_ms"]) * 1e-9
    row["f32_mean_tflops"] = 2.0 * n * r * d / row["f32_mean_ms"] * 1e-9
    print(json.dumps(row), flush=True)


def kernels(f32_mean, f32_index, which):
    g = torch.Generator(device=dev).manual_seed(0)
    for d in (384, 512):
        raw_all = torch.randn((123000, d), device=dev, generator=g)
        sq_all = ops.row_sqnorms(raw_all)
        bh_all, bhsq_all = ops.rows_to_half(raw_all)
        x_all = torch.randn((70000, d), device=dev, generator=g)
        for r in (588, 12300, 123000):
            for n in (841, 13456, 70000):
                one_shape(f32_mean, f32_index, x_all[:n], raw_all[:r], sq_all[:r], bh_all[:r], bhsq_all[:r], which, 15)
        row = alternate({"round_bank_123000_ms": lambda: ops.rows_to_half(raw_all), "row_sqnorms_123000_ms": lambda: ops.row_sqnorms(raw_all)})
        row["D"] = d
        print(json.dumps(row), flush=True)


def pyramid(f32_mean, f32_index, which):
    g = torch.Generator(device=dev).manual_seed(0)
    raw = torch.randn((598000, 448), device=dev, generator=g)
    x = torch.randn((340000, 448), device=dev, generator=g)
    bh, bhsq = ops.rows_to_half(raw)
    one_shape(f32_mean, f32_index, x, raw, ops.row_sqnorms(raw), bh, bhsq, which, 3)


def recall():
    """recall@1 / recall@3 of the half search against the fp32 flat search of this build, rows of the seeded mixture of §4.18."""
    def mixture(n, d, blobs, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        centres = torch.randn((blobs, d), generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float32) * 2.0
        which = torch.randint(0, blobs, (n,), generator=g)
        return (centres[which] + torch.randn((n, d), generator=g, dtype=torch.float32)).to(dev).contiguous()
    d = 384
    bank, x = mixture(146 * 1024, d, 64, 2), mixture(83 * 1024, d, 64, 3)
    _, want = ops.l2_knn_index(x, bank, ops.row_sqnorms(bank), 3)
    bh, bhsq = ops.rows_to_half(bank)
    _, got = ops.l2h_knn_index(x, bh, bhsq, 3)
    r1 = float((got[:, 0] == want[:, 0]).float().mean())
    r3 = float((got.unsqueeze(2) == want.unsqueeze(1)).any(2).float().mean())
    so, sw = ops.l2h_knn_fused(x, bh, bhsq, 3), ops.l2_knn_fused(x, bank, ops.row_sqnorms(bank), 3)
    print(json.dumps({"recall_at_1": r1, "recall_at_3": r3, "N": int(x.shape[0]), "R": int(bank.shape[0]), "D": d, "blobs": 64,
                      "max_rel_score_diff": float(((so - sw).abs() / sw).max())}), flush=True)


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
        for dtype in ("float32", "float16"):
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                            localization='dense', metric='euclidean', bank_dtype=dtype)
            torch.cuda.synchronize()
            out[dtype] = time.perf_counter() - t0
    print(json.dumps({"inference_wall_s": out, "bank": "train", "localization": "dense", "metric": "euclidean", "train_images": 209,
                      "test_images": 83}), flush=True)


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    side = fp32_kernels(path) + ("parent" if path else "this build",)
    kernels(*side)
    recall()
    if "--pyramid" in sys.argv:
        pyramid(*side)
    if "--inference" in sys.argv:
        inference_wall()
