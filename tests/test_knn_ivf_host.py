"""Host-only tests of the inverted-file index of the Euclidean kNN detector (no GPU): the argument errors of tools.inference /
tools.sweep / AnomalyDetector / ops before anything is read or launched, the nlist rule, the keys of the state, the seeded draws of
the k-means, the work list of the search (pure tensor code: checked here on host tensors) and the float64 yardstick of
tests/ivf_ref.py against the brute force of tests/knn_l2_ref.py."""
import inspect

import numpy as np
import pytest
import torch

import ivf_ref as ref
import knn_l2_ref as l2ref

GOOD = {"index": "ivf", "metric": "euclidean"}


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


@pytest.mark.parametrize("kw,match", [
    ({**GOOD, "detector": "gde"}, "detector='knn' only"),
    ({**GOOD, "detector": "padim", "patch_localization": True, "localization": "dense", "bank": "train"}, "detector='knn' only"),
    ({**GOOD, "metric": "cosine"}, "index='ivf' needs metric='euclidean'"),
    ({"index": "ivf"}, "index='ivf' needs metric='euclidean'"),
    ({**GOOD, "gallery": 3, "patch_localization": True, "bank": "train"}, "index='ivf' needs gallery=None"),
    ({**GOOD, "index": "hnsw"}, "index must be one of"),
    ({**GOOD, "nlist": 0}, "nlist must be None or an int in 1..4096"),
    ({**GOOD, "nlist": 4097}, "nlist must be None or an int in 1..4096"),
    ({**GOOD, "nlist": 2.0}, "nlist must be None or an int in 1..4096"),
    ({**GOOD, "nprobe": 0}, "nprobe must be an int >= 1"),
    ({**GOOD, "nprobe": True}, "nprobe must be an int >= 1"),
    ({**GOOD, "index_options": {"restarts": 2}}, "index_options must be a dict with keys among"),
    ({**GOOD, "index_options": 3}, "index_options must be a dict with keys among"),
    ({"metric": "euclidean", "nlist": 8}, "apply to index='ivf' only"),
    ({"metric": "euclidean", "index_options": {"seed": 1}}, "apply to index='ivf' only"),
    ({**GOOD, "patch_localization": True, "image_scores": "reweighted"}, "does not go with index='ivf'"),
    ({**GOOD, "patch_localization": True, "image_scores": "retrieval"}, "does not go with index='ivf'")])
def test_index_argument_errors_come_before_any_file_is_read(tmp_path, kw, match):
    from self_supervised import tools
    missing = str(tmp_path / "nothing_here")
    with pytest.raises(ValueError, match=match):
        tools.inference(missing + "/model.ckpt", missing + "/", "bottle", **kw)
    with pytest.raises(ValueError, match=match):
        tools.sweep(missing + "/", missing + "/out/", ["bottle"], **{"patch_localization": False, **kw})


def test_defaults_are_the_flat_search():
    from self_supervised import tools
    from self_supervised.models import AnomalyDetector
    for fn in (tools.inference, tools.sweep, AnomalyDetector.__init__):
        par = inspect.signature(fn).parameters
        assert par["index"].default == 'flat' and par["nlist"].default is None and par["nprobe"].default == 8
        assert par["index_options"].default is None
    cls, kw = tools._check_options('knn', 'euclidean', 'patches', False, 'reference', True, None, None, 9, None)
    assert kw == {"metric": "euclidean"}                            # nothing about an index reaches a flat detector
    cls, kw = tools._check_options('knn', 'euclidean', 'patches', False, 'reference', True, 0.1, None, 9, None, index='ivf', nprobe=4)
    assert kw == {"metric": "euclidean", "coreset": 0.1, "index": "ivf", "nlist": None, "nprobe": 4, "index_options": None}


def test_detector_argument_errors_and_the_nlist_rule_without_a_gpu():
    from self_supervised.models import AnomalyDetector, check_index, ivf_nlist
    with pytest.raises(ValueError, match="index='ivf' needs metric='euclidean'"):
        AnomalyDetector(index='ivf')
    with pytest.raises(ValueError, match="index='ivf' needs gallery=None"):
        AnomalyDetector(patch_level=True, batch=1, num_patches=4, metric='euclidean', gallery=2, index='ivf')
    for bad in (0, -3, 1.5, "8", True, 5000):
        with pytest.raises(ValueError, match="nlist must be None or an int in 1..4096"):
            AnomalyDetector(metric='euclidean', index='ivf', nlist=bad)
    for bad in (0, 2.5, None, False):
        with pytest.raises(ValueError, match="nprobe must be an int >= 1"):
            AnomalyDetector(metric='euclidean', index='ivf', nprobe=bad)
    assert check_index('flat') == 'flat' and check_index('ivf', np.int64(7), np.int32(2), {"iters": 3, "seed": 1, "train_rows": 9}) == 'ivf'
    # nlist=None: ceil(sqrt(R)) clamped to 1..4096
    for rows, want in ((1, 1), (2, 2), (4, 2), (5, 3), (720, 27), (146 * 1024, 387), (146 * 4096, 774), (4096 ** 2, 4096),
                       (4096 ** 2 + 1, 4096), (10 ** 9, 4096)):
        assert ivf_nlist(None, rows) == want, rows
    assert ivf_nlist(12, 10 ** 6) == 12
    det = AnomalyDetector(metric='euclidean', index='ivf', nlist=5, nprobe=9, index_options={"iters": 2})
    assert (det.index, det.nlist, det.nprobe, det.index_options, det.ivf) == ('ivf', 5, 9, {"iters": 2}, None)
    flat = AnomalyDetector(metric='euclidean')
    assert flat.index == 'flat' and flat.ivf is None
    with pytest.raises(ValueError, match="has no index yet"):
        det.bank = gauss(4, 32, 0)
        det.state()
    with pytest.raises(ValueError, match="does not go with index='ivf'"):
        det._check_image_scores('reweighted', 9)


def test_state_keys_and_the_mismatch_errors():
    from self_supervised.models import AnomalyDetector
    det = AnomalyDetector(metric='euclidean', index='ivf', nlist=2, nprobe=1)
    det.bank = gauss(4, 32, 0)
    det.ivf = {"perm": torch.tensor([2, 0, 1, 3], dtype=torch.int32), "offsets": torch.tensor([0, 3, 4], dtype=torch.int32),
               "centroids": gauss(2, 32, 1), "cent_sq": torch.zeros(2), "nlist": 2, "nprobe": 1}
    state = det.state()
    assert sorted(state) == ["bank", "centroids", "metric", "nlist", "nprobe", "offsets", "perm"]       # bank_sq / cent_sq: recomputed
    assert state["metric"] == 'euclidean' and state["nlist"] == 2 and state["nprobe"] == 1
    assert all(not state[k].is_cuda for k in ("bank", "centroids", "offsets", "perm"))
    flat = AnomalyDetector(metric='euclidean')
    flat.bank = det.bank
    assert sorted(flat.state()) == ["bank", "metric"]


def test_ops_argument_errors_come_before_any_launch():
    """Host tensors: a launch would raise HipExtensionError, these must raise ValueError first."""
    from self_supervised import ops
    i32 = torch.int32
    x, bank = gauss(5, 64, 1), gauss(9, 64, 2)
    bsq = torch.zeros(9)
    off, perm = torch.tensor([0, 4, 9], dtype=i32), torch.arange(9, dtype=i32)
    probes = torch.zeros((5, 1), dtype=i32)
    for fn in (ops.l2_knn_ivf, ops.l2_knn_ivf_index):
        with pytest.raises(ValueError, match="multiple of 32"):
            fn(x[:, :48].contiguous(), bank[:, :48].contiguous(), bsq, off, probes, perm)
        with pytest.raises(ValueError, match="k must be 1, 2 or 3"):
            fn(x, bank, bsq, off, probes, perm, k=4)
        with pytest.raises(ValueError, match="probes must be int32"):
            fn(x, bank, bsq, off, probes.long(), perm)
        with pytest.raises(ValueError, match="probes must be int32"):
            fn(x, bank, bsq, off, probes[:4], perm)
        with pytest.raises(ValueError, match="perm must be int32"):
            fn(x, bank, bsq, off, probes, perm[:8])
        with pytest.raises(ValueError, match="offsets must be int32"):
            fn(x, bank, bsq, off.long(), probes, perm)
        with pytest.raises(ValueError, match="bank_sq must hold"):
            fn(x, bank, bsq[:8], off, probes, perm)
        with pytest.raises(ValueError, match="columns"):
            fn(x, gauss(9, 32, 3), bsq, off, probes, perm)
    with pytest.raises(ValueError, match="order must be int32"):
        ops.segment_means(x, torch.arange(5), off)
    with pytest.raises(ValueError, match="offsets must be int32"):
        ops.segment_means(x, torch.arange(5, dtype=i32), off.long())
    with pytest.raises(ValueError, match="out must be"):
        ops.segment_means(x, torch.arange(5, dtype=i32), off, out=torch.zeros(3, 64))
    with pytest.raises(ValueError, match="nlist must lie in 1..5"):
        ops.kmeans_l2(x, 6)
    with pytest.raises(ValueError, match="nlist must lie in 1..5"):
        ops.kmeans_l2(x, 0)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.kmeans_l2(x[:, :40].contiguous(), 2)
    with pytest.raises(ValueError, match="train_rows must be at least nlist"):
        ops.kmeans_l2(x, 3, train_rows=2)
    with pytest.raises(ValueError, match="nprobe must lie in 1..nlist"):
        ops.ivf_probes(x, gauss(2, 64, 4), torch.zeros(2), 3)


def test_kmeans_draws_are_seeded_distinct_and_leave_the_global_generators_alone():
    from self_supervised import ops
    torch.manual_seed(11)
    np.random.seed(11)
    want_t, want_n = torch.rand(3), np.random.rand(3)
    torch.manual_seed(11)
    np.random.seed(11)
    sample, init = ops.kmeans_init(1000, 7, seed=4)
    assert torch.equal(torch.rand(3), want_t) and np.array_equal(np.random.rand(3), want_n)
    assert sample is None and init.shape == (7,) and len(set(init.tolist())) == 7 and 0 <= int(init.min()) and int(init.max()) < 1000
    again = ops.kmeans_init(1000, 7, seed=4)
    assert again[0] is None and torch.equal(again[1], init)
    assert not torch.equal(ops.kmeans_init(1000, 7, seed=5)[1], init)
    sample, init = ops.kmeans_init(10000, 3, seed=0)                # 256 nlist = 768 rows of 10000, ascending and distinct
    assert sample.shape == (768,) and bool((sample[1:] > sample[:-1]).all()) and int(sample.max()) < 10000
    assert len(set(init.tolist())) == 3 and int(init.max()) < 768
    sample, init = ops.kmeans_init(100, 3, seed=0, train_rows=40)
    assert sample.shape == (40,) and int(init.max()) < 40
    assert ops.kmeans_init(100, 3, seed=0, train_rows=100)[0] is None


@pytest.mark.parametrize("n,nprobe,nlist", [(1, 1, 1), (5, 2, 3), (300, 3, 7), (1000, 4, 9), (257, 1, 2)])
def test_the_work_list_covers_every_valid_pair_once_within_the_grid_bound(n, nprobe, nlist):
    from self_supervised import ops
    rng = np.random.RandomState(n + nprobe)
    probes = rng.randint(-1, nlist + 1, size=(n, nprobe)).astype(np.int32)          # -1 and nlist: entries to skip
    if n == 1000:
        probes[:, 0] = 4                                                             # one crowded cell: several full tiles
    tiles, pairs = ops.ivf_schedule(torch.from_numpy(probes), nlist)
    g = -(-n * nprobe // 128) + nlist
    assert tiles.dtype == torch.int32 and tuple(tiles.shape) == (3, g) and pairs.dtype == torch.int32 and tuple(pairs.shape) == (n * nprobe,)
    assert sorted(pairs.tolist()) == list(range(n * nprobe))
    flat = probes.reshape(-1)
    seen = []
    for cell, first, count in tiles.t().tolist():
        if not 0 <= cell < nlist:
            assert cell == nlist                                                     # a surplus tile
            continue
        assert 1 <= count <= 128 and 0 <= first and first + count <= n * nprobe
        ids = pairs[first:first + count].tolist()
        assert all(flat[i] == cell for i in ids)                                     # a tile never straddles two cells
        seen += ids
    valid = [i for i in range(n * nprobe) if 0 <= flat[i] < nlist]
    assert sorted(seen) == valid                                                     # every valid pair once, no other


def test_reference_agrees_with_brute_force_when_every_cell_is_probed():
    x, bank = gauss(40, 32, 1), gauss(90, 32, 2)
    nlist = 6
    cells = np.random.RandomState(3).randint(0, nlist, size=90)
    probes = np.stack([np.random.RandomState(i).permutation(nlist) for i in range(40)])
    for k in (1, 2, 3):
        d2, rows, a = ref.restricted_knn64(x, bank, cells, probes, nlist, k)
        want_d2, want_i = l2ref.kneighbors64(x, bank, k)
        assert np.array_equal(rows, want_i) and np.array_equal(d2, want_d2)
        assert np.array_equal(a, np.take_along_axis(l2ref.scale_a(x, bank), rows, 1))
    # fewer cells: a subset of the bank, never nearer; skipped entries; cells without rows
    d2_1, rows_1, _ = ref.restricted_knn64(x, bank, cells, probes[:, :2], nlist, 3)
    assert (d2_1 >= l2ref.kneighbors64(x, bank, 3)[0]).all()
    assert all(cells[r] in probes[i, :2] for i in range(40) for r in rows_1[i] if r >= 0)
    junk = np.concatenate([probes[:, :2], np.full((40, 1), -1), np.full((40, 1), nlist)], axis=1)
    assert np.array_equal(ref.restricted_knn64(x, bank, cells, junk, nlist, 3)[1], rows_1)
    only = np.where(cells == 0, 0, 1)                                                # cell 2 has no rows
    d2_e, rows_e, a_e = ref.restricted_knn64(x, bank, only, np.full((40, 1), 2), 3, 2)
    assert np.isinf(d2_e).all() and (rows_e == -1).all() and np.isnan(a_e).all()
    # probes64: (d2, cell) order, ties to the smaller cell
    cent = gauss(5, 32, 7)
    cent[3] = cent[1]
    p = ref.probes64(x, cent, 5)
    assert all(list(row).index(1) + 1 == list(row).index(3) for row in p)
    # Lloyd on two far blobs: the objective never rises, an emptied cell keeps its centroid
    blobs = torch.cat([gauss(30, 32, 8) * 0.1, gauss(30, 32, 9) * 0.1 + 50.0])
    cent, assign, objs = ref.lloyd64(blobs, [0, 1, 45], 3, check_bar=False)
    assert (np.diff(objs) <= 0).all() and set(assign[30:]) == {2}
    same = torch.cat([gauss(1, 32, 10).repeat(6, 1), gauss(2, 32, 11) + 9.0])
    cent, assign, _ = ref.lloyd64(same, [0, 1, 7], 2, check_bar=False)
    assert np.array_equal(cent[1], same[1].double().numpy()) and 1 not in set(assign)
