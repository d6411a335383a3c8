"""GPU: tools.inference(dense_features='pyramid', detector='padim') under torch.distributed -- two ranks over gloo sharing the one GPU
(tests/dist_inference_worker.py, case pyramid) return the one-rank maps, bit for bit."""
import pytest
import torch

import two_rank_util
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
    r = two_rank_util.launch("dist_inference_worker.py", [tmp_path, root, ck, "pyramid", CHANNELS, SIZE])
    assert r["equal_across_ranks"] and r["world"] == 2 and r["shape"] == [4, 1, SIDE, SIDE], r
    assert r["preselected"] and r["width"] == CHANNELS, r
    two = torch.load(str(tmp_path / "pyramid_rank0.pt"))
    one = two_rank_util.inference(tools, ck, root, "pyramid", channels=CHANNELS)
    assert torch.equal(two["embeddings"], one.embedding_vectors), "embeddings differ between the 2-rank and 1-rank runs"
    assert torch.equal(two["maps"], one.anomaly_maps) and torch.equal(two["image_scores"], one.image_scores)
