"""GPU test of the six ways AnomalyDetector keeps and searches its bank (self_supervised/knn_search.py): the fitted detector against
the ``ops`` layer called by hand in the documented order -- prepare the rows, ``coreset_select``, store the kept rows the path's way --
never against itself, so every comparison is torch.equal.  Shapes: 60 images of 4 patches and width 64, i.e. 240 rows (two 128-row
tiles, the second ragged) as bank rows and as queries; a coreset of half the rows everywhere but with a gallery, which takes none."""
import numpy as np
import pytest
import torch

from knn_paths_util import fp32_rows_held

pytestmark = pytest.mark.gpu

D, P, IMAGES, KEPT, CORESET_DIM, NLIST = 64, 4, 60, 120, 32, 4
PATHS = {"cosine": dict(coreset=0.5),
         "l2": dict(coreset=0.5, metric='euclidean'),
         "half": dict(coreset=0.5, metric='euclidean', bank_dtype='float16'),
         "int8": dict(coreset=0.5, metric='euclidean', bank_dtype='int8'),
         "gallery": dict(metric='euclidean', gallery=2),
         "ivf": dict(coreset=0.5, metric='euclidean', index='ivf', nlist=NLIST, nprobe=2)}


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


def make(kw):
    from self_supervised.models import AnomalyDetector
    return AnomalyDetector(patch_level=True, batch=IMAGES, num_patches=P, coreset_dim=CORESET_DIM, **kw)


def by_hand(name, rows):
    """{attribute: tensor or value} of the bank of path `name` over the fp32 device rows, from ops calls alone."""
    from self_supervised import ops
    from self_supervised.models import coreset_select
    if name == "gallery":
        return {"bank": rows, "bank_sq": ops.row_sqnorms(rows), "bank_desc": ops.group_means(rows, P)}
    prepared = ops.l2_normalize_rows(rows) if name == "cosine" else rows
    sel, _ = coreset_select(prepared, KEPT, CORESET_DIM)
    kept = prepared.index_select(0, sel).contiguous()
    if name == "cosine":
        return {"sel": sel, "bank": kept, "bank_sq": None}
    if name == "l2":
        return {"sel": sel, "bank": kept, "bank_sq": ops.row_sqnorms(kept)}
    if name == "half":
        bank, bank_sq = ops.rows_to_half(kept)
        return {"sel": sel, "bank": bank, "bank_sq": bank_sq}
    if name == "int8":
        lo, hi = torch.aminmax(kept)
        lo, s, inv_s, _ = ops.int8_quantiser(lo.item(), hi.item())
        bank, bank_sq, _ = ops.rows_to_int8(kept, lo, inv_s, s)
        return {"sel": sel, "bank": bank, "bank_sq": bank_sq, "quant": (lo, s)}
    centroids, assign = ops.kmeans_l2(kept, NLIST)
    cells, perm = torch.sort(assign, stable=True)
    bank = kept.index_select(0, perm).contiguous()
    return {"sel": sel, "bank": bank, "bank_sq": ops.row_sqnorms(bank), "offsets": ops.cell_offsets(cells, NLIST),
            "perm": perm.to(torch.int32), "centroids": centroids}


@pytest.mark.parametrize("name", list(PATHS))
def test_fitted_bank_is_the_ops_layer_called_by_hand(name):
    emb = gauss(IMAGES * P, D, seed=1) * 0.5 + gauss(1, D, seed=2)
    x = gauss(IMAGES * P, D, seed=3) * 0.5 + gauss(1, D, seed=2)
    before = np.random.get_state()
    det = make(PATHS[name])
    det.fit(emb, split=False)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), before))        # split=False draws nothing
    want = by_hand(name, emb.cuda())
    assert det.bank.dtype == want["bank"].dtype and torch.equal(det.bank, want["bank"])
    assert (det.bank_sq is None) if want["bank_sq"] is None else \
        (det.bank_sq.dtype == want["bank_sq"].dtype and torch.equal(det.bank_sq, want["bank_sq"]))
    if name == "gallery":
        assert det.coreset_rows is None and torch.equal(det.bank_desc, want["bank_desc"])
    else:
        assert torch.equal(det.coreset_rows[0], want["sel"]) and det.coreset_counts == (KEPT, IMAGES * P)
        assert det.bank.shape == (KEPT, D)
    if name == "int8":
        assert det.quant == want["quant"]
    if name == "ivf":
        assert torch.equal(det.ivf["offsets"], want["offsets"]) and torch.equal(det.ivf["perm"], want["perm"])
        assert torch.equal(det.ivf["centroids"], want["centroids"]) and (det.ivf["nlist"], det.ivf["nprobe"]) == (NLIST, 2)
    else:
        assert det.ivf is None
    if name in ("half", "int8"):
        assert fp32_rows_held(det) == []                                                   # no fp32 copy of the bank outlives fit
    assert det.threshold == det.predict(emb).max().item()
    # a fresh detector that loads the state scores and searches to the same bits
    scores, (dist, idx) = det.predict(x), det.kneighbors(x)
    assert tuple(scores.shape) == (IMAGES, 1, 2, 2) and tuple(dist.shape) == (IMAGES * P, 3) and idx.dtype == torch.int64
    other = make(PATHS[name])
    other.load_state(det.state())
    assert torch.equal(other.bank, det.bank) and torch.equal(other.predict(x), scores)
    odist, oidx = other.kneighbors(x)
    assert torch.equal(odist, dist) and torch.equal(oidx, idx)
