"""Worker of tests/test_hip_knn_refine.py::test_two_ranks_equal_one_rank: one of two ranks that share the box's single GPU (gloo), each
running tools.inference with a refined int8 bank (bank='train', metric='euclidean', bank_dtype='int8', refine=8, coreset=0.5) on the
same tree and checkpoint.  Rank 0 fits the detector and broadcasts its state -- codes, norms, the code's (lo, s) and `bank_f32`; the
ranks exchange what they scored and what their detectors held and compare it bit for bit.
Launched by two_rank_util.launch as `dist_refine_worker.py tmp root ck`; prints `RESULT {...json...}` on rank 0 and saves rank 0's
results in tmp for the one-rank comparison the test makes."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

FILE = "refine_rank0.pt"
KWARGS = dict(bank='train', image_scores='max', metric='euclidean', bank_dtype='int8', refine=8, coreset=0.5)
EQUAL = ("scores", "maps", "bank", "bank_sq", "bank_f32", "quant", "threshold")


def inference(tools, ck, root):
    """np.random.seed(3), then the tools.inference call both the worker and the test make."""
    np.random.seed(3)
    return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, **KWARGS)


def main():
    import torch
    import torch.distributed as dist
    tmp, root, ck = sys.argv[1:4]
    os.environ.setdefault("SSAD_ALLOW_RANDOM_BACKBONE", "1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from self_supervised import tools, datasets
    from self_supervised.models import AnomalyDetector
    datasets._DataModule.num_workers = 0
    seen = {}
    orig = AnomalyDetector.predict

    def at_predict(self, x):
        seen.update(threshold=self.threshold, bank=self.bank.cpu(), bank_sq=self.bank_sq.cpu(), bank_f32=self.bank_f32.cpu(),
                    quant=tuple(self.quant), refine=self.refine, dtype=str(self.bank.dtype))
        return orig(self, x)
    AnomalyDetector.predict = at_predict
    out = inference(tools, ck, root)
    saved = dict(seen, maps=out.anomaly_maps.contiguous(), scores=out.image_scores.contiguous())
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, saved)
    same = lambda a, b: torch.equal(a, b) if torch.is_tensor(a) else a == b
    equal = all(all(same(parts[0][k], p[k]) for k in EQUAL) and p["refine"] == 8 and p["dtype"] == "torch.int8" for p in parts)
    if dist.get_rank() == 0:
        torch.save(saved, os.path.join(tmp, FILE))
        print("RESULT " + json.dumps({"equal_across_ranks": bool(equal), "world": dist.get_world_size()}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
