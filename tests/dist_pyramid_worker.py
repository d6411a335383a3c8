"""Worker of tests/test_hip_pyramid_distributed.py: one of two ranks that share the box's single GPU (gloo), each running
tools.inference(detector='padim', localization='dense', dense_features='pyramid', bank='train') on the same tree and checkpoint, the
datamodule pinned to the files' own size as in the test.  Every rank draws the same columns from the detector's seed and its model
writes only those; rank 0 fits the per-position Gaussians on the preselected rows and broadcasts (state, threshold); every rank
returns the full maps.  Launched by `python -m torch.distributed.run`; prints `RESULT {...json...}` on rank 0 and saves rank 0's maps,
image scores, embeddings and threshold for the one-rank comparison."""
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
    tmp, root, ck, channels, size = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
    os.environ.setdefault("SSAD_ALLOW_RANDOM_BACKBONE", "1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from self_supervised import tools, datasets
    datasets._DataModule.num_workers = 0
    plain = datasets.MVTecDatamodule
    tools.MVTecDatamodule = lambda r, **kw: plain(r, imsize=(size, size), **kw)
    seen = {}
    broadcast = tools.broadcast_bank

    def spy(payload):                       # (state, threshold) as every rank holds it after the broadcast
        got = broadcast(payload)
        seen["threshold"] = float(got[1])
        seen["preselected"] = bool(got[0]["preselected"])
        return got
    tools.broadcast_bank = spy
    np.random.seed(3)
    out = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, detector='padim',
                          localization='dense', dense_features='pyramid', bank='train', image_scores='max',
                          detector_options={"channels": channels})
    maps = out.anomaly_maps.contiguous()
    mine = torch.cat([maps.reshape(-1), out.image_scores.reshape(-1).float(), torch.tensor([seen["threshold"]])]).contiguous()
    parts = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, mine)
    res = {"equal_across_ranks": all(torch.equal(parts[0], p) for p in parts), "shape": list(maps.shape),
           "world": dist.get_world_size(), "preselected": seen["preselected"], "width": int(out.embedding_vectors.shape[1])}
    if dist.get_rank() == 0:
        torch.save({"maps": maps, "image_scores": out.image_scores, "embeddings": out.embedding_vectors,
                    "threshold": seen["threshold"]}, os.path.join(tmp, "pyramid_rank0.pt"))
        print("RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
