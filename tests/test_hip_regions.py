"""csrc/regions.hip on the GPU against tests/regions_ref.py (scipy.ndimage / numpy): every comparison is exact equality.  The raw
C entries write into views between sentinel-filled guards, pre-filled with garbage: the guards must come back intact and every
element must have been written."""
import numpy as np
import pytest
import torch

import regions_ref as ref
from self_supervised import _hip, metrics, ops, tools

pytestmark = pytest.mark.gpu

T = ops.REGION_TILE
ZOO = ref.zoo(T)
GUARD = 64
DT = {torch.int32: (-7777777, -1234567), torch.uint8: (0xA5, 0x5A), torch.int64: (-7777777, -1234567),
      torch.float32: (-2.0 ** 100, -2.0 ** 70), torch.float64: (-2.0 ** 100, -2.0 ** 70)}


class Guarded:
    """A device array of `numel` elements between two guards of GUARD elements; the payload starts out as garbage."""

    def __init__(self, numel, dtype):
        self.sentinel, garbage = DT[dtype]
        self.whole = torch.full((numel + 2 * GUARD,), self.sentinel, dtype=dtype, device="cuda")
        self.view = self.whole[GUARD:GUARD + numel]
        self.view.fill_(garbage)
        self.garbage = garbage

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self, shape=None):
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == self.sentinel).all() and (w[len(w) - GUARD:] == self.sentinel).all(), "a guard was overwritten"
        v = w[GUARD:len(w) - GUARD]
        assert not (v == self.garbage).any(), "an output element was not written"
        return v.reshape(shape) if shape is not None else v


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_label(x, threshold=None, connectivity=8):
    """ssad_label_regions on numpy input [n][H][W] (uint8 mask, or float32 scores with a threshold) -> numpy outputs."""
    n, h, w = x.shape
    lib = _hip.lib()
    xd = dev(x)
    lab, cnt, off = Guarded(n * h * w, torch.int32), Guarded(n, torch.int32), Guarded(n + 1, torch.int32)
    nbytes = lib.ssad_label_regions_workspace(n, h, w)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    scores, mask = (xd.data_ptr(), None) if threshold is not None else (None, xd.data_ptr())
    rc = lib.ssad_label_regions(scores, 0.0 if threshold is None else threshold, mask, n, h, w, connectivity, lab.ptr(), cnt.ptr(),
                                off.ptr(), ws.data_ptr(), nbytes, _hip.stream())
    assert rc == 0, lib.ssad_last_error()
    return lab.numpy((n, h, w)), cnt.numpy(), off.numpy()


def raw_stats(labels, offsets, scores=None):
    n, h, w = labels.shape
    r = int(offsets[-1])
    ld, od = dev(labels), dev(offsets)
    sd = None if scores is None else dev(scores)
    area, bbox, csum = Guarded(r, torch.int32), Guarded(4 * r, torch.int32), Guarded(2 * r, torch.int64)
    peak, pos = (Guarded(r, torch.float32), Guarded(r, torch.int32)) if scores is not None else (None, None)
    rc = _hip.lib().ssad_region_stats(None if sd is None else sd.data_ptr(), ld.data_ptr(), od.data_ptr(), n, h, w, r, area.ptr(),
                                      bbox.ptr(), csum.ptr(), None if peak is None else peak.ptr(), None if pos is None else pos.ptr(),
                                      _hip.stream())
    assert rc == 0, _hip.lib().ssad_last_error()
    return (area.numpy(), bbox.numpy((r, 4)), csum.numpy((r, 2)), None if peak is None else peak.numpy(),
            None if pos is None else pos.numpy())


def tie_scores(shape, seed):
    """Few distinct values: every region of more than a few pixels has ties for its peak."""
    return np.random.default_rng(seed).integers(-2, 3, shape).astype(np.float32)


def test_tile_constant_is_the_kernels():
    assert _hip.lib().ssad_label_regions_tile() == T


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("name", list(ZOO))
def test_labels_equal_scipy(name, connectivity):
    m = ZOO[name]
    want, k = ref.label(m, connectivity)
    lab, cnt, off = raw_label(m[None], connectivity=connectivity)
    assert np.array_equal(lab[0], want)
    assert cnt.tolist() == [k] and off.tolist() == [0, k]
    l2, c2, o2 = ops.label_regions(dev(m[None]).bool(), connectivity=connectivity)
    assert l2.dtype == torch.int32 and np.array_equal(l2.cpu().numpy()[0], want) and c2.tolist() == [k] and o2.tolist() == [0, k]


@pytest.mark.parametrize("connectivity", [8, 4])
def test_batch_with_an_empty_image_in_the_middle(connectivity):
    batch = np.stack([ZOO["spiral"], np.zeros_like(ZOO["spiral"]), ZOO["density_0.4"]])
    want, counts, offsets = ref.label_batch(batch, connectivity)
    lab, cnt, off = raw_label(batch, connectivity=connectivity)
    assert np.array_equal(lab, want) and np.array_equal(cnt, counts) and np.array_equal(off, offsets)
    assert off[1] == off[2]                                     # the zero-length entry
    l4 = ops.label_regions(dev(batch).unsqueeze(1), connectivity=connectivity)[0]           # [n][1][H][W]
    assert np.array_equal(l4.cpu().numpy(), want)


BLOBS = ref.blobs(3, 256, seed=11)


@pytest.mark.parametrize("connectivity", [8, 4])
def test_workload_shape_thresholded_blobs(connectivity):
    thr = np.float32(0.62)
    want, counts, offsets = ref.label_batch(np.greater_equal(BLOBS, thr), connectivity)
    assert counts.min() >= 2
    lab, cnt, off = raw_label(BLOBS, threshold=float(thr), connectivity=connectivity)
    assert np.array_equal(lab, want) and np.array_equal(cnt, counts) and np.array_equal(off, offsets)
    lab_m, _, _ = raw_label(np.greater_equal(BLOBS, thr).astype(np.uint8), connectivity=connectivity)
    assert np.array_equal(lab_m, want)


@pytest.mark.parametrize("threshold", [0.5, float("inf"), float("-inf")])
def test_score_form_special_values(threshold):
    rng = np.random.default_rng(5)
    s = rng.random((2, T + 1, 2 * T + 1)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), -np.nan], np.float32)
    idx = rng.integers(0, special.size + 2, s.shape)
    s = np.where(idx < special.size, special[np.minimum(idx, special.size - 1)], s).astype(np.float32)
    fg = np.greater_equal(s, np.float32(threshold))            # NaN gives False; +inf >= +inf gives True
    assert threshold != 0.5 or (fg.any() and not fg.all())
    for c in (8, 4):
        want, counts, offsets = ref.label_batch(fg, c)
        lab, cnt, off = raw_label(s, threshold=threshold, connectivity=c)
        assert np.array_equal(lab, want) and np.array_equal(cnt, counts) and np.array_equal(off, offsets)
    assert np.array_equal(ops.label_regions(dev(s), threshold)[0].cpu().numpy(), ref.label_batch(fg, 8)[0])


def test_two_calls_give_equal_bits():
    batch = np.stack([ZOO["density_0.4"], ZOO["density_0.6"], ZOO["checkerboard"]])
    for c in (8, 4):
        a, b = raw_label(batch, connectivity=c), raw_label(batch, connectivity=c)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(ZOO))
def test_region_stats_equal_numpy(name):
    m = ZOO[name]
    scores = tie_scores(m.shape, len(name))
    for c in (8, 4):
        lab, k = ref.label(m, c)
        want = ref.stats(lab, k, scores)
        got = raw_stats(lab[None], np.array([0, k], np.int32), scores[None])
        for g, w_ in zip(got, want):
            assert g.dtype == w_.dtype and np.array_equal(g, w_)
        got = raw_stats(lab[None], np.array([0, k], np.int32))
        assert all(np.array_equal(g, w_) for g, w_ in zip(got[:3], want[:3])) and got[3] is None


def test_region_stats_of_a_batch_in_image_label_order():
    batch = np.stack([ZOO["density_0.4"], np.zeros_like(ZOO["spiral"]), ZOO["nested_u"]])
    scores = tie_scores(batch.shape, 3)
    labs, counts, offsets = ref.label_batch(batch, 8)
    want = ref.stats_batch(labs, counts, scores)
    got = raw_stats(labs, offsets, scores)
    assert all(np.array_equal(g, w_) for g, w_ in zip(got, want))
    area, bbox, csum, peak, pos = ops.region_stats(dev(labs), dev(offsets), dev(scores))
    assert all(np.array_equal(g.cpu().numpy(), w_) for g, w_ in zip((area, bbox, csum, peak, pos), want))


def test_region_stats_without_regions():
    lab = np.zeros((2, 5, 7), np.int32)
    got = raw_stats(lab, np.zeros(3, np.int32), np.ones((2, 5, 7), np.float32))
    assert all(g.size == 0 for g in got)
    assert ops.region_stats(dev(lab), dev(np.zeros(3, np.int32)))[0].numel() == 0


@pytest.mark.parametrize("min_area", [1, 4, 10 ** 6])
def test_region_filter(min_area):
    batch = np.stack([ZOO["density_0.4"], np.zeros_like(ZOO["spiral"]), ZOO["nested_u"], ZOO["density_0.1"]])
    n, h, w = batch.shape
    labs, counts, offsets = ref.label_batch(batch, 8)
    area = ref.stats_batch(labs, counts)[0]
    keep = area >= min_area
    assert {1: keep.all(), 4: keep.any() and not keep.all(), 10 ** 6: not keep.any()}[min_area]
    parts = [ref.filter_labels(labs[i], int(counts[i]), keep[offsets[i]:offsets[i + 1]]) for i in range(n)]
    want_mask, want_lab = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    want_cnt = np.array([p[2] for p in parts], np.int32)
    lib = _hip.lib()
    r = int(offsets[-1])
    ld, od, kd = dev(labs), dev(offsets), dev(keep.astype(np.uint8))
    mask, lab2, cnt2, off2 = Guarded(n * h * w, torch.uint8), Guarded(n * h * w, torch.int32), Guarded(n, torch.int32), Guarded(n + 1, torch.int32)
    nbytes = lib.ssad_region_filter_workspace(r)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.ssad_region_filter(ld.data_ptr(), od.data_ptr(), kd.data_ptr(), n, h, w, r, mask.ptr(), lab2.ptr(), cnt2.ptr(), off2.ptr(),
                                ws.data_ptr(), nbytes, _hip.stream())
    assert rc == 0, lib.ssad_last_error()
    assert np.array_equal(mask.numpy((n, h, w)), want_mask) and np.array_equal(lab2.numpy((n, h, w)), want_lab)
    assert np.array_equal(cnt2.numpy(), want_cnt) and np.array_equal(off2.numpy(), np.concatenate(([0], np.cumsum(want_cnt))))
    only = Guarded(n * h * w, torch.uint8)                       # the mask alone: no workspace, no renumbering
    rc = lib.ssad_region_filter(ld.data_ptr(), od.data_ptr(), kd.data_ptr(), n, h, w, r, only.ptr(), None, None, None, None, 0, _hip.stream())
    assert rc == 0 and np.array_equal(only.numpy((n, h, w)), want_mask)
    m, l, c, o = ops.region_filter(ld, od, kd.bool())
    assert np.array_equal(m.cpu().numpy(), want_mask) and np.array_equal(l.cpu().numpy(), want_lab) and c.tolist() == want_cnt.tolist()


def six_maps():
    """Six 64 x 64 maps and ground truths: an empty one, two regions that touch diagonally, one region on the border."""
    maps = ref.blobs(6, 64, seed=3)
    maps = (np.round(maps * 64) / 64).astype(np.float32)         # repeated scores: runs of equal thresholds in the PRO curve
    gts = np.zeros((6, 64, 64), np.uint8)
    gts[1, 10:20, 10:20] = 1
    gts[1, 20:30, 20:30] = 1                                     # one component under 8: the squares share a corner
    gts[2, 0:5, 0:64] = 1                                        # on the border
    gts[2, 40:44, 60:64] = 1
    gts[3] = ref.random_mask(64, 64, 0.08, 9)
    gts[4, 30:34, 30:34] = 1
    gts[5, 63, 63] = 1
    gts[5, 5:9, 5:9] = 1
    gts[5, 9:12, 9:12] = 1
    return maps, gts


MAPS, GTS = six_maps()


def test_pro_weights_equal_the_host_planes():
    labs, counts, offsets = ref.label_batch(GTS, 8)
    assert counts[0] == 0 and counts[1] == 1
    want_fp, want_pro = ref.pro_weights(labs, counts)
    area = ref.stats_batch(labs, counts)[0]
    ld, od, ad = dev(labs), dev(offsets), dev(area)
    fp, pro = Guarded(labs.size, torch.uint8), Guarded(labs.size, torch.float64)
    rc = _hip.lib().ssad_pro_weights(ld.data_ptr(), od.data_ptr(), ad.data_ptr(), 6, 64, 64, fp.ptr(), pro.ptr(), _hip.stream())
    assert rc == 0
    assert np.array_equal(fp.numpy(), want_fp)
    assert np.array_equal(pro.numpy().view(np.int64), want_pro.view(np.int64))          # the correctly rounded quotient, bit for bit
    f2, p2 = ops.pro_weights(ld, od, ad)
    assert np.array_equal(f2.cpu().numpy(), want_fp) and np.array_equal(p2.cpu().numpy(), want_pro)


def test_compute_pro_gpu_device_labelling_equals_host_labelling():
    md = dev(MAPS)
    f_host, p_host = metrics.compute_pro_gpu(md, torch.from_numpy(GTS))
    f_dev, p_dev = metrics.compute_pro_gpu(md, torch.from_numpy(GTS), labelling="device")
    assert f_host.dtype == f_dev.dtype and p_host.dtype == p_dev.dtype and len(f_host) > 10
    assert np.array_equal(f_host, f_dev) and np.array_equal(p_host, p_dev)
    f_dev2, p_dev2 = metrics.compute_pro_gpu(md, dev(GTS).bool().unsqueeze(1), labelling="device")      # device ground truths
    assert np.array_equal(f_host, f_dev2) and np.array_equal(p_host, p_dev2)


@pytest.mark.parametrize("min_area,connectivity", [(1, 8), (6, 8), (6, 4), (10 ** 6, 8)])
def test_defect_regions_equal_the_reference(min_area, connectivity):
    thr = 0.625
    want_mask, want_lab, want_regions = ref.defect_regions(MAPS, thr, min_area, connectivity)
    out = tools.defect_regions(dev(MAPS).unsqueeze(1), thr, min_area=min_area, connectivity=connectivity)
    assert out.pred_masks.dtype == torch.uint8 and out.pred_masks.is_cuda and tuple(out.pred_masks.shape) == (6, 1, 64, 64)
    assert out.labels.dtype == torch.int32 and out.labels.is_cuda
    assert np.array_equal(out.pred_masks.cpu().numpy()[:, 0], want_mask)
    assert np.array_equal(out.labels.cpu().numpy()[:, 0], want_lab)
    assert out.regions == want_regions
    assert min_area > 6 or sum(len(r) for r in want_regions) >= 6
    assert out.pred_boxes == [[r["box"] for r in img] for img in want_regions]
    out3 = tools.defect_regions(dev(MAPS), thr, min_area=min_area, connectivity=connectivity)           # [n][H][W]
    assert out3.regions == want_regions


def test_argument_errors_return_2_before_any_launch():
    lib = _hip.lib()
    n, h, w = 1, 8, 8
    s = torch.zeros(n, h, w, device="cuda")
    m = torch.zeros(n, h, w, dtype=torch.uint8, device="cuda")
    lab, cnt, off = Guarded(n * h * w, torch.int32), Guarded(n, torch.int32), Guarded(n + 1, torch.int32)
    nbytes = lib.ssad_label_regions_workspace(n, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def call(scores, mask, hh=h, ww=w, conn=8, wsb=nbytes):
        return lib.ssad_label_regions(scores, 0.5, mask, n, hh, ww, conn, lab.ptr(), cnt.ptr(), off.ptr(), ws.data_ptr(), wsb, _hip.stream())

    for kwargs in (dict(scores=s.data_ptr(), mask=m.data_ptr()), dict(scores=None, mask=None),
                   dict(scores=None, mask=m.data_ptr(), conn=6), dict(scores=None, mask=m.data_ptr(), hh=1 << 15, ww=1 << 15),
                   dict(scores=None, mask=m.data_ptr(), wsb=nbytes - 1)):
        assert call(**kwargs) == 2
        assert b"ssad_label_regions" in lib.ssad_last_error()
    torch.cuda.synchronize()
    for g in (lab, cnt, off):                                    # nothing ran: the garbage is still there
        assert (g.whole.cpu().numpy()[GUARD:-GUARD] == g.garbage).all()
    assert call(scores=None, mask=m.data_ptr()) == 0
    assert lab.numpy().max() == 0
    with pytest.raises(ValueError):
        ops.label_regions(m, connectivity=6)
    with pytest.raises(ValueError):
        ops.label_regions(s)                                     # float scores without a threshold
