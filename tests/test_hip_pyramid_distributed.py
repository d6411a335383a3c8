"""GPU: tools.inference(dense_features='pyramid', detector='padim') under torch.distributed -- two ranks over gloo sharing the one GPU
(tests/dist_pyramid_worker.py) return the one-rank maps, bit for bit."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from fake_mvtec import make_tree

pytestmark = pytest.mark.gpu

SIZE, SIDE, N_TRAIN, CHANNELS = 128, 32, 10, 32         # 128 x 128 images: 32 x 32 maps of the pyramid, the ratios of 256 x 256


def _datamodule(root, **kw):
    from self_supervised.datasets import MVTecDatamodule
    return MVTecDatamodule(root, imsize=(SIZE, SIZE), **kw)


def test_pyramid_two_ranks_equal_one_rank(tmp_path, seeded_sd, monkeypatch):
    from self_supervised import datasets, tools
    datasets._DataModule.num_workers = 0
    monkeypatch.setattr(tools, "MVTecDatamodule", _datamodule)
    root = make_tree(str(tmp_path / "data"), categories=("bottle",), n_train=N_TRAIN, n_test_good=2, n_test_bad=2, size=SIZE)
    ck = str(tmp_path / "seeded.ckpt")
    torch.save({"state_dict": seeded_sd, "hyper_parameters": {}, "memory_bank": torch.tensor([])}, ck)
    here = os.path.dirname(os.path.abspath(__file__))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(here, "dist_pyramid_worker.py"), str(tmp_path), root, ck, str(CHANNELS), str(SIZE)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, p.stdout[-4000:]
    r = json.loads(line[-1][7:])
    assert r["equal_across_ranks"] and r["world"] == 2 and r["shape"] == [4, 1, SIDE, SIDE], r
    assert r["preselected"] and r["width"] == CHANNELS, r
    two = torch.load(str(tmp_path / "pyramid_rank0.pt"))
    np.random.seed(3)
    one = tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, detector='padim',
                          localization='dense', dense_features='pyramid', bank='train', image_scores='max',
                          detector_options={"channels": CHANNELS})
    assert torch.equal(two["embeddings"], one.embedding_vectors), "embeddings differ between the 2-rank and 1-rank runs"
    assert torch.equal(two["maps"], one.anomaly_maps) and torch.equal(two["image_scores"], one.image_scores)
