"""Worker of tests/test_hip_coreset.py::test_inference_with_coreset_two_ranks_equal_one_rank: one of two ranks that share the box's
single GPU (gloo), each running tools.inference(bank='train', coreset=0.25) on the same tree and checkpoint.  Each rank embeds a
round-robin share of the training images, rank 0 fits the bank -- the split and the coreset selection -- and broadcasts the smaller
bank; every rank returns the full maps.
Launched by `python -m torch.distributed.run`; prints `RESULT {...json...}` on rank 0 and saves rank 0's maps and embeddings for the
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
    np.random.seed(3)
    out = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, bank='train',
                          coreset=0.25)
    maps = out.anomaly_maps.contiguous()
    parts = [torch.empty_like(maps) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, maps)
    res = {"maps_equal_across_ranks": all(torch.equal(parts[0], p) for p in parts), "shape": list(maps.shape),
           "world": dist.get_world_size()}
    if dist.get_rank() == 0:
        torch.save({"maps": maps, "embeddings": out.embedding_vectors}, os.path.join(tmp, "maps_rank0.pt"))
        print("RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
