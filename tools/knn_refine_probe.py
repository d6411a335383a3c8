"""Time and recall of the refined search (csrc/knn_refine.hip: ops.l2_rerank_mean on the shortlist of ops.l2h_topk_index /
l2q_topk_index) at the nine N x R shapes of DESIGN §4.22, D = 384: N = 841 / 13 456 / 70 000 queries against R = 588 / 12 300 /
123 000 bank rows, shortlists of r = 4, 8, 16, 32, mean form with k = 3, for both compressed banks.  The sides of a row take turns
inside one loop with the k = 3 kernels this change does not touch (ops.l2_knn_fused, l2h_knn_fused, l2q_knn_fused: the parent
commit's), medians of per-call event times.  Reported per shape and r: the coarse index search, the re-rank kernel alone with its
byte rate (N r D floats gathered, the queries and the lists read, N floats written) as a fraction of ops.bn_apply_fwd's on a tensor
of the bytes the r = 32 gather moves, and their sum beside the three unrefined searches.  --recall: recall@1 / recall@3 against
the fp32 flat search on the seeded Gaussian mixture of tools/knn_ivf_probe.py for each r, beside the unrefined banks'.
   python tools/knn_refine_probe.py [--small] [--recall]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch
from self_supervised import ops

from knn_l2_half_probe import alternate, dev
from knn_l2_int8_probe import code_bank

RS = (4, 8, 16, 32)
K = 3


def coarse_fns(x, bh, bhsq, bq, bqsq, quant, r, s):
    rr = min(r, int(bh.shape[0]))
    return (lambda: ops.l2h_topk_index(x, bh, bhsq, rr, splits=s)), (lambda: ops.l2q_topk_index(x, bq, bqsq, quant, rr, splits=s))


def bn_rate(nbytes, d=128):
    """Byte rate (GB/s) of ops.bn_apply_fwd reading and writing `nbytes` in all: the project's yardstick of a streaming kernel."""
    rows = max(int(nbytes // (8 * d)), 1)
    z = torch.randn((rows, d), device=dev)
    one, zero = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    ms = alternate({"bn": lambda: ops.bn_apply_fwd(z, zero, one, one, zero, None, False)}, 9)["bn"]
    return 8.0 * rows * d / ms * 1e-6


def one_shape(x, raw, sq, bh, bhsq, bq, bqsq, quant, reps):
    n, d = x.shape
    rows = raw.shape[0]
    s = ops.knn_splits(n, rows)
    fns = {"f32_mean_ms": lambda: ops.l2_knn_fused(x, raw, sq, K, splits=s), "half_mean_ms": lambda: ops.l2h_knn_fused(x, bh, bhsq, K, splits=s),
           "int8_mean_ms": lambda: ops.l2q_knn_fused(x, bq, bqsq, quant, K, splits=s)}
    lists = {}
    for r in RS:
        half, int8 = coarse_fns(x, bh, bhsq, bq, bqsq, quant, r, s)
        fns[f"half_coarse_r{r}_ms"], fns[f"int8_coarse_r{r}_ms"] = half, int8
        lists[r] = half()[1]
        fns[f"rerank_r{r}_ms"] = lambda r=r: ops.l2_rerank_mean(x, raw, lists[r], K)
    row = {"N": n, "R": rows, "D": d, "rule_S": s, "reps": reps}
    row.update(alternate(fns, reps))
    for r in RS:
        rr = lists[r].shape[1]
        nbytes = 4.0 * (n * rr * d + n * d + n * rr + n)
        row[f"r{r}"] = {"rerank_GBps": nbytes / row[f"rerank_r{r}_ms"] * 1e-6,
                        "half_refined_ms": row[f"half_coarse_r{r}_ms"] + row[f"rerank_r{r}_ms"],
                        "int8_refined_ms": row[f"int8_coarse_r{r}_ms"] + row[f"rerank_r{r}_ms"]}
        row[f"r{r}"]["int8_refined_over_f32"] = row[f"r{r}"]["int8_refined_ms"] / row["f32_mean_ms"]
        row[f"r{r}"]["half_refined_over_f32"] = row[f"r{r}"]["half_refined_ms"] / row["f32_mean_ms"]
    row["bn_apply_fwd_GBps"] = bn_rate(4.0 * n * min(32, rows) * d)
    row["rerank_r32_over_bn"] = row["r32"]["rerank_GBps"] / row["bn_apply_fwd_GBps"]
    print(json.dumps(row), flush=True)


def kernels(small):
    g = torch.Generator(device=dev).manual_seed(0)
    d = 384
    raw_all = torch.randn((123000, d), device=dev, generator=g)
    sq_all = ops.row_sqnorms(raw_all)
    bh_all, bhsq_all = ops.rows_to_half(raw_all)
    x_all = torch.randn((70000, d), device=dev, generator=g)
    for rows in (588, 12300, 123000):
        bq, bqsq, quant, _ = code_bank(raw_all[:rows])     # the code spans the rows that are kept, as the detector's fit takes it
        for n in (841, 13456, 70000):
            if small and n * rows > 13456 * 12300:
                continue
            one_shape(x_all[:n], raw_all[:rows], sq_all[:rows], bh_all[:rows], bhsq_all[:rows], bq, bqsq, quant, 9 if n * rows > 1e9 else 15)


def recall():
    """recall@1 / recall@3 of the refined searches against the fp32 flat search of this build, rows of the seeded mixture of §4.18."""
    def mixture(n, d, blobs, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        centres = torch.randn((blobs, d), generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float32) * 2.0
        which = torch.randint(0, blobs, (n,), generator=g)
        return (centres[which] + torch.randn((n, d), generator=g, dtype=torch.float32)).to(dev).contiguous()
    d = 384
    bank, x = mixture(146 * 1024, d, 64, 2), mixture(83 * 1024, d, 64, 3)
    sq = ops.row_sqnorms(bank)
    dw, want = ops.l2_knn_index(x, bank, sq, 3)
    bh, bhsq = ops.rows_to_half(bank)
    bq, bqsq, quant, _ = code_bank(bank)

    def agree(got):
        return float((got[:, 0] == want[:, 0]).float().mean()), float((got.unsqueeze(2) == want.unsqueeze(1)).any(2).float().mean())
    out = {"N": int(x.shape[0]), "R": int(bank.shape[0]), "D": d, "blobs": 64,
           "half_unrefined": agree(ops.l2h_knn_index(x, bh, bhsq, 3)[1]), "int8_unrefined": agree(ops.l2q_knn_index(x, bq, bqsq, quant, 3)[1])}
    sw = ops.l2_knn_fused(x, bank, sq, 3)
    for r in RS:
        for name, cand in (("half", ops.l2h_topk_index(x, bh, bhsq, r)[1]), ("int8", ops.l2q_topk_index(x, bq, bqsq, quant, r)[1])):
            dist, got = ops.l2_rerank_index(x, bank, cand, 3)
            so = ops.l2_rerank_mean(x, bank, cand, 3)
            out[f"{name}_r{r}"] = agree(got) + (float(((so - sw).abs() / sw).max()),)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if "--recall" in sys.argv:
        recall()
    else:
        kernels("--small" in sys.argv)
