"""Worker of tests/test_hip_knn_index.py::test_image_scores_two_ranks_equal_one_rank: one of two ranks that share the box's single
GPU (gloo), each running tools.inference(bank='train', image_scores=...) on the same tree and checkpoint.  Each rank scores a
round-robin share of the test images against the broadcast bank; the image scores travel with their images through the one
exchange at the end, and every rank returns all of them.
Launched by `python -m torch.distributed.run`; prints `RESULT {...json...}` on rank 0 and saves rank 0's scores and maps for the
one-rank comparison."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "self-supervised-anomaly-detection_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch
import torch.distributed as dist


def main():
    tmp, root, ck = sys.argv[1], sys.argv[2], sys.argv[3]
    os.environ.setdefault("SSAD_ALLOW_RANDOM_BACKBONE", "1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from self_supervised import tools, datasets
    datasets._DataModule.num_workers = 0
    saved, equal = {}, True
    for mode in ("max", "reweighted"):
        np.random.seed(3)
        out = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                              image_scores=mode, neighbours=5)
        scores = out.image_scores.contiguous()
        parts = [torch.empty_like(scores) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, scores)
        equal = equal and all(torch.equal(parts[0], p) for p in parts)
        saved[mode] = {"scores": scores, "maps": out.anomaly_maps.contiguous()}
    res = {"equal_across_ranks": bool(equal), "n": int(saved["max"]["scores"].numel()), "world": dist.get_world_size()}
    if dist.get_rank() == 0:
        torch.save(saved, os.path.join(tmp, "scores_rank0.pt"))
        print("RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
