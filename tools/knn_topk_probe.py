"""Time of the flat Euclidean search for k = 4, 9, 16, 32 (csrc/knn_topk.hip, ops.l2_topk_mean / l2h_topk_mean and the index forms)
against the k = 3 kernels of the same shape (csrc/knn_l2.hip / knn_l2_half.hip -- untouched by the wider search, so this build's are
the parent commit's; --parent-lib PATH takes the fp32 ones from another build through ctypes) and against the composition
torch.cdist(x, bank).topk(k, largest=False) (queries in chunks of 8192 rows: the distance matrix of 70 000 x 123 000 is 34 GB), at
the flat-search shapes of DESIGN §4.13 / §4.19: N = 841 / 13 456 / 70 000 queries against R = 123 000 rows, D = 384, both operand
types.  The sides of a row take turns inside one loop; medians of per-call event times.  The fp16 sides include rounding the
queries.  Reported per row: t(k) / t(3), ceil(k / 3) (what re-running the k = 3 search with a floor key would cost) and the ratio to
the torch composition.
   python tools/knn_topk_probe.py [--parent-lib PATH] [--index]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd")):
    sys.path.insert(0, p)
import torch
from self_supervised import _hip, ops

dev = torch.device("cuda", 0)
KS = (4, 9, 16, 32)


def alternate(fns, reps):
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


def parent_fp32(path):
    """ssad_l2_knn_fused and ssad_l2_knn_index (k = 3) of another build of the library: fn(x, bank, sq, s)."""
    lib = ctypes.CDLL(path)
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


def torch_topk(x, bank, k, chunk=8192):
    out = []
    for i in range(0, x.shape[0], chunk):
        out.append(torch.cdist(x[i:i + chunk], bank).topk(k, dim=1, largest=False))
    return out


def one_shape(x, raw, sq, bh, bhsq, index, parent, reps):
    n, d = x.shape
    r = raw.shape[0]
    s = ops.knn_splits(n, r)
    f3, h3 = (ops.l2_knn_index, ops.l2h_knn_index) if index else (ops.l2_knn_fused, ops.l2h_knn_fused)
    fk, hk = (ops.l2_topk_index, ops.l2h_topk_index) if index else (ops.l2_topk_mean, ops.l2h_topk_mean)
    fns = {"f32_k3_ms": (lambda: parent[index](x, raw, sq, s)) if parent else (lambda: f3(x, raw, sq, 3, splits=s)),
           "f16_k3_ms": lambda: h3(x, bh, bhsq, 3, splits=s)}
    for k in KS:
        fns[f"f32_k{k}_ms"] = lambda k=k: fk(x, raw, sq, k, splits=s)
        fns[f"f16_k{k}_ms"] = lambda k=k: hk(x, bh, bhsq, k, splits=s)
        fns[f"torch_k{k}_ms"] = lambda k=k: torch_topk(x, raw, k)
    row = {"N": n, "R": r, "D": d, "rule_S": s, "form": "index" if index else "mean", "k3_side": "parent" if parent else "this build",
           "reps": reps}
    row.update(alternate(fns, reps))
    for k in KS:
        row[f"k{k}"] = {"f32_over_k3": row[f"f32_k{k}_ms"] / row["f32_k3_ms"], "f16_over_k3": row[f"f16_k{k}_ms"] / row["f16_k3_ms"],
                        "ceil_k_over_3": -(-k // 3), "f32_over_torch": row[f"f32_k{k}_ms"] / row[f"torch_k{k}_ms"],
                        "f16_over_torch": row[f"f16_k{k}_ms"] / row[f"torch_k{k}_ms"]}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    parent = parent_fp32(sys.argv[sys.argv.index("--parent-lib") + 1]) if "--parent-lib" in sys.argv else None
    g = torch.Generator(device=dev).manual_seed(0)
    raw = torch.randn((123000, 384), device=dev, generator=g)
    sq = ops.row_sqnorms(raw)
    bh, bhsq = ops.rows_to_half(raw)
    x_all = torch.randn((70000, 384), device=dev, generator=g)
    for n, reps in ((841, 15), (13456, 9), (70000, 5)):
        one_shape(x_all[:n], raw, sq, bh, bhsq, "--index" in sys.argv, parent, reps)
