"""Time of the index-returning cosine k-NN (csrc/knn.hip ssad_cosine_knn_index) against the mean kernels it shares its tile
with (ssad_cosine_knn_fused / _split) at the shapes of DESIGN §4.8: N = 841 / 13 456 / 70 000 queries, R = 588 / 12 300 / 123 000 bank
rows, D = 512, k = 3 -- the one-launch forms against each other, and what the ops.knn_splits rule picks for each.  The two sides
of a pair alternate inside one loop and the medians of the per-call event times are reported.  Then the whole image-score step
(AnomalyDetector.image_scores on raw maps that exist already) for 83 images of 841 patches against the 123 000-row bank, stage by
stage.  With --parent-lib PATH the mean kernels of a library built from another commit are timed in the same loop (through
ctypes).  With --inference, also the wall time of tools.inference(patch_localization=True, bank='train') on a synthetic 209 / 83-image
category (seeded weights) without and with image_scores='reweighted', second round.
   python tools/knn_index_probe.py [--parent-lib PATH] [--inference]"""
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
D = 512


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


def parent_kernels(path):
    """The mean kernels of another build of the library: (fused(x, bank, out), split(x, bank, part, out, s))."""
    lib = ctypes.CDLL(path)
    sig = _hip.SIGNATURES
    lib.ssad_cosine_knn_fused.argtypes = sig["ssad_cosine_knn_fused"]
    lib.ssad_cosine_knn_split.argtypes = sig["ssad_cosine_knn_split"]

    def fused(x, bank, out):
        assert lib.ssad_cosine_knn_fused(x.data_ptr(), bank.data_ptr(), out.data_ptr(), x.shape[0], D, bank.shape[0], 3, _hip.stream()) == 0

    def split(x, bank, part, out, s):
        assert lib.ssad_cosine_knn_split(x.data_ptr(), bank.data_ptr(), part.data_ptr(), out.data_ptr(), x.shape[0], D, bank.shape[0], 3,
                                         s, _hip.stream()) == 0
    return fused, split


def kernels(parent):
    g = torch.Generator(device=dev).manual_seed(0)
    bank_all = ops.l2_normalize_rows(torch.randn((123000, D), device=dev, generator=g))
    x_all = torch.randn((70000, D), device=dev, generator=g)
    for r in (588, 12300, 123000):
        bank = bank_all[:r]
        for n in (841, 13456, 70000):
            x = x_all[:n]
            s = ops.knn_splits(n, r)
            fns = {"fused_ms": lambda: _one_launch(x, bank),
                   "index_ms": lambda: ops.cosine_knn_index(x, bank, 3, splits=1)}
            if s > 1:
                fns["split_rule_ms"] = lambda: ops.cosine_knn_split(x, bank, 3, s)
                fns["index_rule_ms"] = lambda: ops.cosine_knn_index(x, bank, 3, splits=s)
            if parent is not None:
                out = torch.empty(n, device=dev)
                part = torch.empty((max(s, 1), n, 3), device=dev)
                fns["parent_fused_ms"] = lambda: parent[0](x, bank, out)
                if s > 1:
                    fns["parent_split_rule_ms"] = lambda: parent[1](x, bank, part, out, s)
            row = {"N": n, "R": r, "D": D, "rule_S": s}
            row.update(alternate(fns))
            row["index_over_fused"] = row["index_ms"] / row["fused_ms"]
            if s > 1:
                row["index_rule_over_split_rule"] = row["index_rule_ms"] / row["split_rule_ms"]
            if parent is not None:
                row["index_over_parent_fused"] = row["index_ms"] / row["parent_fused_ms"]
                if s > 1:
                    row["index_rule_over_parent_split_rule"] = row["index_rule_ms"] / row["parent_split_rule_ms"]
            print(json.dumps(row), flush=True)


def _one_launch(x, bank):
    out = torch.empty(x.shape[0], device=x.device)
    _hip.check(_hip.lib().ssad_cosine_knn_fused(_hip.ptr(x), _hip.ptr(bank), _hip.ptr(out), x.shape[0], x.shape[1], bank.shape[0], 3,
                                                _hip.stream()))
    return out


def image_scores_step():
    from self_supervised.models import AnomalyDetector
    g = torch.Generator(device=dev).manual_seed(1)
    n_img, p, r = 83, 841, 123000
    det = AnomalyDetector(patch_level=True, batch=n_img, num_patches=p)
    det.fit_bank(torch.randn((r, D), device=dev, generator=g))
    x = torch.randn((n_img * p, D), device=dev, generator=g)
    s = det.predict(x).reshape(-1)
    smax, flat = ops.rows_argmax(s.reshape(n_img, p))
    xs = x.index_select(0, flat)
    _, mstar = ops.cosine_knn_index(xs, det.bank, 1)
    centre = det.bank.index_select(0, mstar.reshape(-1).long())
    sim = ops.linear_fwd(centre, det.bank)
    _, nbr = ops.rows_smallest_index(sim, 9, cosine=True)
    row = alternate({"maps_ms": lambda: det.predict(x),
                     "image_scores_max_ms": lambda: det.image_scores(x, 'max', scores=s),
                     "image_scores_reweighted_ms": lambda: det.image_scores(x, 'reweighted', 9, scores=s),
                     "rows_argmax_ms": lambda: ops.rows_argmax(s.reshape(n_img, p)),
                     "index_k1_83_rows_ms": lambda: ops.cosine_knn_index(xs, det.bank, 1),
                     "centre_similarity_gemm_ms": lambda: ops.linear_fwd(centre, det.bank),
                     "rows_smallest_b9_ms": lambda: ops.rows_smallest_index(sim, 9, cosine=True),
                     "rows_smallest_b32_ms": lambda: ops.rows_smallest_index(sim, 32, cosine=True),
                     "knn_reweight_ms": lambda: ops.knn_reweight(xs, det.bank, mstar, nbr, smax)})
    row.update({"images": n_img, "patches": p, "R": r})
    print(json.dumps({"image_scores_step": row}), flush=True)


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
        for name, kw in (("maps_only", {}), ("reweighted", {"image_scores": "reweighted"})):
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train', **kw)
            torch.cuda.synchronize()
            out[name] = time.perf_counter() - t0
    print(json.dumps({"inference_wall_s": out, "bank": "train", "train_images": 209, "test_images": 83}), flush=True)


if __name__ == "__main__":
    parent = None
    if "--parent-lib" in sys.argv:
        parent = parent_kernels(sys.argv[sys.argv.index("--parent-lib") + 1])
    kernels(parent)
    image_scores_step()
    if "--inference" in sys.argv:
        inference_wall()
