"""Time of the flat Euclidean search on an 8-bit scalar-quantised bank (csrc/knn_l2_int8.hip, ops.l2q_knn_fused / l2q_knn_index)
against the fp16 and fp32 kernels of the same shape (ops.l2h_knn_fused, ops.l2_knn_fused; this build's -- the change that added the
int8 path does not touch them), at the 18 shapes of DESIGN §4.13: N = 841 / 13 456 / 70 000 queries, R = 588 / 12 300 / 123 000 bank
rows, D = 384 and 512, k = 3, and at the pyramid shape (340 000 x 598 000 rows, D = 448; --pyramid, fewer repetitions).  The sides of
a row take turns inside one loop (tools/knn_l2_half_probe.py's `alternate`) and the medians of the per-call event times are reported.
The int8 side INCLUDES coding the queries (ops.rows_to_int8 per call), as the fp16 side includes rounding them; coding the bank
happens once at fit time and is reported on a line of its own, as a byte rate beside ops.rows_to_half's.  Also recall@1 / recall@3,
the largest relative score change against the fp32 flat search and the largest ratio of |d_q - d_exact| to s sqrt(D) on the seeded
Gaussian mixture of tools/knn_ivf_probe.py (real features do not exist offline).
   python tools/knn_l2_int8_probe.py [--pyramid] [--small]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch
from self_supervised import ops

from knn_l2_half_probe import alternate, dev


def code_bank(raw):
    lo, hi = torch.aminmax(raw)
    lo, s, inv_s, _ = ops.int8_quantiser(lo.item(), hi.item())
    bq, bqsq, _ = ops.rows_to_int8(raw, lo, inv_s, s)
    return bq, bqsq, (lo, s), inv_s


def one_shape(x, raw, sq, bh, bhsq, bq, bqsq, quant, inv_s, reps):
    n, d = x.shape
    r = raw.shape[0]
    s = ops.knn_splits(n, r)
    fns = {"f32_mean_ms": lambda: ops.l2_knn_fused(x, raw, sq, 3, splits=s), "half_mean_ms": lambda: ops.l2h_knn_fused(x, bh, bhsq, 3, splits=s),
           "int8_mean_ms": lambda: ops.l2q_knn_fused(x, bq, bqsq, quant, 3, splits=s),
           "half_index_ms": lambda: ops.l2h_knn_index(x, bh, bhsq, 3, splits=s),
           "int8_index_ms": lambda: ops.l2q_knn_index(x, bq, bqsq, quant, 3, splits=s),
           "round_queries_ms": lambda: ops.rows_to_half(x), "code_queries_ms": lambda: ops.rows_to_int8(x, quant[0], inv_s, quant[1])}
    row = {"N": n, "R": r, "D": d, "rule_S": s, "reps": reps}
    row.update(alternate(fns, reps))
    row["half_over_int8_mean"] = row["half_mean_ms"] / row["int8_mean_ms"]
    row["f32_over_int8_mean"] = row["f32_mean_ms"] / row["int8_mean_ms"]
    row["half_over_int8_index"] = row["half_index_ms"] / row["int8_index_ms"]
    row["int8_mean_tops"] = 2.0 * n * r * d / max(row["int8_mean_ms"] - row["code_queries_ms"], 1e-6) * 1e-9
    row["half_mean_tflops"] = 2.0 * n * r * d / max(row["half_mean_ms"] - row["round_queries_ms"], 1e-6) * 1e-9
    print(json.dumps(row), flush=True)


def kernels(small):
    g = torch.Generator(device=dev).manual_seed(0)
    for d in (384, 512):
        raw_all = torch.randn((123000, d), device=dev, generator=g)
        sq_all = ops.row_sqnorms(raw_all)
        bh_all, bhsq_all = ops.rows_to_half(raw_all)
        x_all = torch.randn((70000, d), device=dev, generator=g)
        for r in (588, 12300, 123000):
            # the code spans the rows that are kept, as the detector's fit takes it
            bq, bqsq, quant, inv_s = code_bank(raw_all[:r])
            for n in (841, 13456, 70000):
                if small and n * r > 13456 * 12300:
                    continue
                one_shape(x_all[:n], raw_all[:r], sq_all[:r], bh_all[:r], bhsq_all[:r], bq, bqsq, quant, inv_s, 15)
        lo, s, inv_s, _ = ops.int8_quantiser(*[v.item() for v in torch.aminmax(raw_all)])
        row = alternate({"code_bank_123000_ms": lambda: ops.rows_to_int8(raw_all, lo, inv_s, s),
                         "round_bank_123000_ms": lambda: ops.rows_to_half(raw_all)})
        row["D"] = d
        row["rows_to_int8_GBps"] = 123000 * d * 5.0 / row["code_bank_123000_ms"] * 1e-6
        row["rows_to_half_GBps"] = 123000 * d * 6.0 / row["round_bank_123000_ms"] * 1e-6
        print(json.dumps(row), flush=True)


def pyramid():
    g = torch.Generator(device=dev).manual_seed(0)
    raw = torch.randn((598000, 448), device=dev, generator=g)
    x = torch.randn((340000, 448), device=dev, generator=g)
    bh, bhsq = ops.rows_to_half(raw)
    bq, bqsq, quant, inv_s = code_bank(raw)
    one_shape(x, raw, ops.row_sqnorms(raw), bh, bhsq, bq, bqsq, quant, inv_s, 3)


def recall():
    """recall@1 / recall@3 of the int8 search against the fp32 flat search of this build, rows of the seeded mixture of §4.18."""
    def mixture(n, d, blobs, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        centres = torch.randn((blobs, d), generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float32) * 2.0
        which = torch.randint(0, blobs, (n,), generator=g)
        return (centres[which] + torch.randn((n, d), generator=g, dtype=torch.float32)).to(dev).contiguous()
    d = 384
    bank, x = mixture(146 * 1024, d, 64, 2), mixture(83 * 1024, d, 64, 3)
    sq = ops.row_sqnorms(bank)
    dw, want = ops.l2_knn_index(x, bank, sq, 3)
    bq, bqsq, quant, _ = code_bank(bank)
    dq, got = ops.l2q_knn_index(x, bq, bqsq, quant, 3)
    r1 = float((got[:, 0] == want[:, 0]).float().mean())
    r3 = float((got.unsqueeze(2) == want.unsqueeze(1)).any(2).float().mean())
    so, sw = ops.l2q_knn_fused(x, bq, bqsq, quant, 3), ops.l2_knn_fused(x, bank, sq, 3)
    # d_q of the int8 search's own neighbours against the fp32 distance to the same bank rows, in units of s sqrt(D)
    near = bank.index_select(0, got[:, 0].long())
    exact = (x.double() - near.double()).norm(dim=1)
    bar = quant[1] * d ** 0.5
    print(json.dumps({"recall_at_1": r1, "recall_at_3": r3, "N": int(x.shape[0]), "R": int(bank.shape[0]), "D": d, "blobs": 64,
                      "max_rel_score_diff": float(((so - sw).abs() / sw).max()), "s": quant[1], "s_sqrt_D": bar,
                      "max_abs_dq_minus_dexact_over_bar": float(((dq[:, 0].double() - exact).abs() / bar).max()),
                      "share_of_queries_with_excess": float((ops.rows_to_int8(x, quant[0], 1.0 / quant[1], quant[1])[2] > 0).float().mean())}),
          flush=True)


if __name__ == "__main__":
    kernels("--small" in sys.argv)
    recall()
    if "--pyramid" in sys.argv:
        pyramid()
