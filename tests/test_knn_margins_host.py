"""CPU tests of the kNN margin tests' own tools (tests/knn_margins_util.py): the geometry of embedded(), and that the margins have
teeth -- for every search case of tests/test_hip_knn_margins.py, on the float64 reference of that path's ref module alone: over the
padded bank, margins included as ordinary rows, every query's nearest distance is 0 (or below the path's bar), while over the tight
bank it is at least 1.0.  A kernel that looks one row too far cannot pass the GPU file.  The last test holds that file to the
header: every kNN entry point of include/ssad.h is named in it."""
import os
import re

import numpy as np
import pytest
import torch

import ivf_ref
import knn_gallery_ref as gref
import knn_index_ref as cref
import knn_l2_half_ref as href
import knn_l2_int8_ref as qref
import knn_l2_ref as ref
import knn_margins_util as mu
import knn_topk_ref as tref
from test_hip_knn_index import DIST_TOL
from test_hip_knn_l2 import tau as tau32
from test_hip_knn_l2_half import tau as tau16

EPS = ref.EPS
FLOOR = 1.0         # the nearest real row of every query is at least this far (a condition on the inputs)
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- 1. geometry

@pytest.mark.parametrize("dtype,shape,fill", [
    (torch.float32, (3, 32), mu.NAN), (torch.float32, (130, 100), mu.NAN), (torch.float16, (129, 96), mu.NAN),
    (torch.int8, (3, 32), 0x55), (torch.float32, (300,), -1e30), (torch.int32, (129,), -2 ** 31), (torch.int32, (1, 2), 4),
    (torch.int64, (520, 3), mu.INT_FILL), (torch.float32, (1,), mu.NAN)])
def test_embedded_geometry(dtype, shape, fill):
    t = (torch.arange(int(np.prod(shape))) % 100).reshape(shape).to(dtype)
    for before, after in ((128, 128), (256, 128), (128, 384)):
        buf, view = mu.embedded(t, before, after, fill, device="cpu")
        assert buf.is_contiguous() and view.is_contiguous() and view.dtype == dtype and tuple(view.shape) == tuple(shape)
        assert view.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
        assert tuple(buf.shape) == (before + shape[0] + after,) + tuple(shape[1:])
        row = view.numel() // shape[0] * view.element_size()
        assert view.data_ptr() - buf.data_ptr() == before * row
        assert torch.equal(mu._bits(view), mu._bits(t))
        want = mu._bits(torch.full((1,), fill, dtype=dtype))[0]
        lo, hi = mu._margins(buf, view)
        assert lo.numel() == before * (row // view.element_size()) and hi.numel() == after * (row // view.element_size())
        assert bool((lo == want).all()) and bool((hi == want).all())           # bit-exact, NaN included


def test_embedded_cycles_fill_rows_and_refuses_short_margins():
    t = torch.zeros((5, 32))
    twins = torch.arange(3 * 32, dtype=torch.float32).reshape(3, 32)
    buf, view = mu.embedded(t, 256, 128, twins, device="cpu")
    assert torch.equal(buf[:256], twins[torch.arange(256) % 3]) and torch.equal(buf[261:], twins[torch.arange(128) % 3])
    assert torch.equal(view, t)
    norms = torch.arange(3, dtype=torch.float32)
    vbuf, _ = mu.embedded(torch.zeros(5), 256, 128, norms, device="cpu")
    assert torch.equal(vbuf[:256], norms[torch.arange(256) % 3])                # a vector's margin i goes with row margin i
    for before, after in ((0, 128), (128, 64), (130, 128), (127, 128)):
        with pytest.raises(ValueError, match="margins"):
            mu.embedded(t, before, after, 0.0, device="cpu")
    with pytest.raises(ValueError, match="fill rows"):
        mu.embedded(t, 128, 128, twins.half(), device="cpu")
    assert mu.margin(1) == 128 and mu.margin(128) == 128 and mu.margin(130) == 256 and mu.margin(260) == 384


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.int32, torch.int64])
def test_guards_notice_one_changed_element(dtype):
    buf, view = mu.poisoned((7, 3), dtype, device="cpu")
    assert mu.guards_intact(buf, view) and mu.untouched(view) and not mu.all_written(view)
    view.fill_(1)
    assert mu.guards_intact(buf, view) and mu.all_written(view) and not mu.untouched(view)
    view[3, 1] = mu.fill_of(dtype)
    assert not mu.all_written(view) and not mu.untouched(view)
    for at in (0, 128 * 3 - 1, (128 + 7) * 3, buf.numel() - 1):                 # the first and last element of either margin
        b2 = buf.clone()
        b2.reshape(-1)[at] = 1
        assert not mu.guards_intact(b2, b2[128:135])
    if dtype.is_floating_point:                                                 # another NaN is not the fill
        b2 = buf.clone()
        mu._bits(b2).reshape(-1)[5] += 1
        assert bool(torch.isnan(b2.reshape(-1)[5])) and not mu.guards_intact(b2, b2[128:135])


# ---------------------------------------------------------------- 2. the margins have teeth

def _teeth(padded_nearest, tight_nearest, bar, what):
    assert (padded_nearest <= bar).all(), (what, float(padded_nearest.max()))
    assert (tight_nearest >= FLOOR).all(), (what, float(tight_nearest.min()))


@pytest.mark.parametrize("d", mu.DS + (mu.D_UNFUSED,))
def test_teeth_cosine(d):
    for r in mu.RS:
        for n in mu.NS:
            x, raw = mu.flat_inputs(n, r, d, cosine=True)
            bank_n = torch.from_numpy(cref.unit_rows64(raw).astype(np.float32))
            twins = torch.from_numpy(cref.unit_rows64(x).astype(np.float32))
            padded = cref.distances64(x, mu.with_twins(bank_n, twins, mu.margin(n)))
            _teeth(padded.min(1), cref.distances64(x, bank_n).min(1), DIST_TOL, (d, r, n))


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("d", mu.DS)
def test_teeth_flat_euclidean_and_topk(d, half):
    """The k <= 3 and the list kernels meet the same banks: one assertion serves both (k <= R leaves R = 3 to the former)."""
    mod, t = (href, tau16(d)) if half else (ref, tau32(d))
    assert tref.ref is ref                                                     # the list kernels' yardstick is this d2
    for r in mu.RS:
        for n in mu.NS:
            x, bank = mu.flat_inputs(n, r, d)
            padded_bank = mu.with_twins(bank, x, mu.margin(n))
            d2 = mod.d2_64(x, padded_bank)
            near = d2.argmin(1)
            bar = t * EPS * mod.scale_a(x, padded_bank)[np.arange(n), near]
            _teeth(np.sqrt(d2.min(1)), np.sqrt(mod.d2_64(x, bank).min(1)), np.sqrt(bar), (d, r, n))
            assert (d2.min(1) <= bar).all()


@pytest.mark.parametrize("d", mu.DS)
def test_teeth_int8(d):
    for r in mu.RS:
        for n in mu.NS:
            x, bank = mu.flat_inputs(n, r, d)
            lo, s, inv_s, s2 = mu.int8_quantiser(x, bank)
            xc, bc = qref.codes(x, lo, inv_s), qref.codes(bank, lo, inv_s)
            ex = qref.excess64(x, lo, s)
            assert (ex == 0).all()                                              # the code covers the queries: a twin is at 0 exactly
            padded = np.concatenate([xc[np.arange(mu.margin(n)) % n], bc, xc[np.arange(mu.margin(n)) % n]])
            _teeth(qref.dist64(qref.d2_int(xc, padded), s2, ex).min(1), qref.dist64(qref.d2_int(xc, bc), s2, ex).min(1), 0.0, (d, r, n))


@pytest.mark.parametrize("p", mu.PATCHES)
@pytest.mark.parametrize("d", mu.DS)
def test_teeth_gallery(d, p):
    c = mu.GalleryCase(p, d)
    assert p % mu.TILE and c.TWIN not in c.gallery and (c.gallery == c.TWIN - 1).any(1).all()
    t = tau32(d)
    for bank in (c.padded_bank(), c.bank):                                      # the margins; the twin image inside the bank alone
        d2 = gref.d2_64(c.x, bank)
        if bank is c.bank:
            d2 = d2[:p]                                                         # image TWIN holds twins of the first p queries
        bar = t * EPS * gref.scale_a(c.x, bank)[np.arange(d2.shape[0]), d2.argmin(1)]
        assert (d2.min(1) <= bar).all()
    tight, rows, _ = gref.restricted_knn64(c.x, c.bank, c.gallery, p, 1, c.T)
    assert (rows >= 0).all() and (np.sqrt(tight[:, 0]) >= FLOOR).all()


@pytest.mark.parametrize("n", mu.NS)
@pytest.mark.parametrize("d", mu.DS)
def test_teeth_ivf(d, n):
    c = mu.IvfCase(n, d)
    assert all(s % mu.TILE for s in c.sizes) and not (c.probes == c.TWIN).any() and c.probes.shape == (n, mu.NPROBE)
    assert np.array_equal(np.sort(c.cell_of_row[c.twin_rows]), np.full(n, c.TWIN))
    t = ivf_ref.TAU
    for bank in (c.padded_bank(), c.bank):                                      # the margins; the unprobed cell alone
        d2 = ivf_ref.d2_64(c.x, bank)
        bar = t * EPS * ivf_ref.scale_a(c.x, bank)[np.arange(n), d2.argmin(1)]
        assert (d2.min(1) <= bar).all()
    assert (ivf_ref.d2_64(c.x, c.bank)[:, c.twin_rows].min(1) == ivf_ref.d2_64(c.x, c.bank).min(1)).all()
    tight, rows, _ = ivf_ref.restricted_knn64(c.x, c.bank, c.cell_of_row, c.probes, c.nlist, 1)
    assert (rows >= 0).all() and (np.sqrt(tight[:, 0]) >= FLOOR).all()


# ---------------------------------------------------------------- 3. no entry point is forgotten

KNN_NAMES = re.compile(r"^ssad_(\w*knn\w*|l2\w*|rows_\w+|group_means|ivf_\w+|row_sqnorms|l2_normalize_rows)$")


def test_every_knn_entry_point_of_the_header_is_called_by_the_gpu_file():
    with open(os.path.join(HERE, "..", "include", "ssad.h")) as f:
        declared = set(re.findall(r"^int (ssad_\w+)\(", f.read(), flags=re.M))
    family = sorted(name for name in declared if KNN_NAMES.match(name))
    assert len(family) >= 29 and "ssad_l2q_knn_index" in family and "ssad_rows_smallest_index" in family
    with open(os.path.join(HERE, "test_hip_knn_margins.py")) as f:
        called = set(re.findall(r"\"(ssad_\w+)\"", f.read()))
    assert not [name for name in family if name not in called]
