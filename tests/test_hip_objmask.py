"""csrc/objmask.hip against the host statement (dataset_generator._canny / obj_mask), bit for bit, where tests/test_hip_resize.py's
square 64 / 96 / 256 images do not reach: H != W, a row longer than the 1024 threads of the iterative kernels, images smaller than the
stencils, crafted images that give the three fixed-point iterations work (tests/objmask_cases.py), a batch over several chunks, repeat
calls, and a workspace of exactly ssad_obj_mask_workspace bytes between guards.

The CPU half (no mark) asserts, from the host statement's intermediates with scipy.ndimage, that every crafted image has the property
it is named for, and establishes the smallest sizes the host statement accepts; the GPU half (gpu mark) runs the kernels."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage

import objmask_cases as C
from bn_table import Arena, _bits, _lib, _p

gpu = pytest.mark.gpu


def _small_sizes():
    """Every (H, W) of SMALL_RANGE the host statement accepts (it raises on none of them: established here, asserted below)."""
    ok = []
    for h in C.SMALL_RANGE:
        for w in C.SMALL_RANGE:
            try:
                C.host_mask(C.small_image(h, w))
                ok.append((h, w))
            except Exception:
                pass
    return ok


SMALL = _small_sizes()


# ---------------------------------------------------------------- CPU half ----------------------------------------------------------------
def test_host_statement_accepts_every_small_size_and_has_no_edges_below_three():
    assert SMALL == [(h, w) for h in C.SMALL_RANGE for w in C.SMALL_RANGE] and (1, 1) in SMALL
    for h, w in SMALL:
        img = C.small_image(h, w)
        if h < 3 or w < 3:
            assert not C.host_edges(img).any() and C.host_mask(img).all()       # no interior pixel: no edges, the all-white mask
    assert any(C.host_edges(C.small_image(h, w)).any() for h, w in SMALL)        # ... and edges once there is one


def test_nonsquare_images_have_edges_and_a_proper_mask():
    for k, (h, w) in enumerate(C.NONSQUARE):
        img = C.textured(h, w, k)
        e, m = C.host_edges(img), C.host_mask(img)
        assert e.shape == (h, w) and e.any() and m.any() and not m.all(), (h, w)
    assert any(w > 1024 for _, w in C.NONSQUARE) and any(h > w for h, w in C.NONSQUARE) and any(h < w for h, w in C.NONSQUARE)


def test_serpentine_needs_many_propagation_sweeps():
    img = C.serpentine()
    th = C.host_thinned(img)
    low = th > 0
    high = low & (th >= 15 / 255.0)
    assert high.any() and high.sum() < 0.1 * low.sum()                           # one strong segment, the rest weak
    reach = C.geodesic_reach(low, high)
    assert reach > C.SIDE, reach                                                 # the weak edges hang on it through a long path
    e = C.host_edges(img)
    assert e.sum() > 0.95 * low.sum() and (e & ~high).sum() > 4 * C.SIDE         # ... and hysteresis keeps them
    first = np.zeros_like(e)
    first.flat[np.flatnonzero(e)[0]] = True
    assert C.geodesic_reach(e, first) > C.SIDE                                   # labelling spreads the first pixel's index as far


def test_two_discs_tie_goes_to_the_raster_first_component():
    img = C.two_discs()
    st = C.host_stages(img)
    lab, n = ndimage.label(st["eroded"], structure=C.S8)
    sizes = np.bincount(lab.ravel())[1:]
    assert n == 2 and sizes[0] == sizes[1] > 100
    m = C.host_mask(img)
    assert np.array_equal(m, lab == 1) and m[18, 20] and not m[44, 42]           # scipy numbers components in raster order


def test_only_the_closed_ring_fills():
    img = C.c_and_ring()
    st = C.host_stages(img)
    holes = st["filled"] & ~st["closed"]
    yy, xx = np.mgrid[0:C.SIDE, 0:C.SIDE]
    assert holes.any() and ((yy - 46) ** 2 + (xx - 44) ** 2 < 14 ** 2)[holes].all()      # every filled pixel lies inside the ring
    assert holes[46, 44]                                                         # the ring's hole
    assert not st["filled"][18, 10] and not st["filled"][10, 10]                 # the cavity, and the C's body: open to the frame
    assert not st["edges"][:, 0].any() and st["edges"][4:32, 1:4].any()          # the C's outline runs into the frame, which has no edges
    bg, _ = ndimage.label(~st["closed"], structure=C.S8)
    assert bg[18, 1] == bg[0, 63] or bg[18, 1] in set(bg[:, 0])                  # the cavity's background touches the frame


def test_cross_touches_all_four_borders():
    img = C.touches_all_borders()
    bright = img[..., 0] > 128
    assert bright[0].any() and bright[-1].any() and bright[:, 0].any() and bright[:, -1].any()
    st = C.host_stages(img)
    assert st["edges"].any() and not (st["filled"] & ~st["closed"]).any()        # four open corners: nothing encloses anything
    lab, n = ndimage.label(st["eroded"], structure=C.S8)
    assert n >= 2 and len(set(np.bincount(lab.ravel())[1:])) == 1                # several components of ONE size: the tie rule again
    assert np.array_equal(C.host_mask(img), lab == 1)


def test_flat_image_has_no_edges_and_an_all_white_mask():
    img = C.flat()
    assert not C.host_edges(img).any() and C.host_mask(img).all()


def test_batch_is_seven_different_images_over_three_chunks():
    imgs = C.batch_images()
    assert len(imgs) == 7 == len(C.BATCH_ORDER) and sorted(C.BATCH_ORDER) == list(range(7)) and list(C.BATCH_ORDER) != list(range(7))
    masks = [C.host_mask(im).tobytes() for im in imgs]
    assert len(set(masks)) >= 6                                                  # a base offset off by one image shows


# ---------------------------------------------------------------- GPU half ----------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    return torch.device("cuda:0")


def _check(imgs, dev, chunk=64, what=""):
    """ops.obj_mask_batch on a stack of images, twice: equal bits, and edges and masks equal to the host statement's."""
    from self_supervised import ops
    batch = torch.from_numpy(np.stack(imgs)).to(dev)
    mask, edges = ops.obj_mask_batch(batch, return_edges=True, chunk=chunk)
    mask2, edges2 = ops.obj_mask_batch(batch, return_edges=True, chunk=chunk)
    assert torch.equal(mask, mask2) and torch.equal(edges, edges2), f"{what}: two calls differ"
    for i, im in enumerate(imgs):
        want_e, want_m = C.host_edges(im), C.host_mask(im)
        got_e, got_m = edges[i].cpu().numpy(), mask[i].cpu().numpy()
        assert np.array_equal(got_e, want_e), f"{what}[{i}]: {int((got_e != want_e).sum())} edge pixels differ from the host statement"
        assert np.array_equal(got_m, want_m), f"{what}[{i}]: {int((got_m != want_m).sum())} mask pixels differ from the host statement"
    return mask, edges


@gpu
@pytest.mark.parametrize("hw", C.NONSQUARE, ids=lambda hw: "%dx%d" % hw)
def test_nonsquare_and_odd_sizes(dev, hw):
    h, w = hw
    _check([C.textured(h, w, k) for k in range(2)], dev, what="%dx%d" % hw)


@gpu
def test_smallest_images(dev):
    for h, w in SMALL:
        mask, edges = _check([C.small_image(h, w), C.small_image(w, h).transpose(1, 0, 2).copy()], dev, what=f"{h}x{w}")
        if h < 3 or w < 3:
            assert not bool(edges.any()) and bool(mask.all()), f"{h}x{w}: no interior pixel, yet an edge or a hole in the mask"


@gpu
@pytest.mark.parametrize("name", list(C.crafted()))
def test_crafted_images(dev, name):
    _check([C.crafted()[name]], dev, what=name)


@gpu
def test_batch_over_several_chunks(dev):
    imgs = C.batch_images()
    _check([imgs[i] for i in C.BATCH_ORDER], dev, chunk=3, what="batch of 7, chunk 3")


@gpu
def test_workspace_of_exactly_the_stated_size_between_guards(dev):
    """The C entry point with every buffer between poisoned guards and the workspace at exactly ssad_obj_mask_workspace bytes."""
    hip, lib, st = _lib()
    imgs = C.batch_images()[:3] + [C.crafted()["serpentine"]]
    b, (h, w) = len(imgs), imgs[0].shape[:2]
    sigma = 1.5
    radius = int(4.0 * sigma + 0.5)
    phi = np.exp(-0.5 / (sigma * sigma) * np.arange(-radius, radius + 1) ** 2)
    phi = (phi / phi.sum())[::-1].copy()
    wts = (ctypes.c_double * len(phi))(*phi.tolist())
    ia = Arena(dev)
    rgb = ia.inp("rgb", torch.from_numpy(np.stack(imgs)))
    nbytes = lib.ssad_obj_mask_workspace(b, h, w)
    outs = []
    for _ in range(2):
        ar = Arena(dev)
        mask, edges = ar.out("mask", (b, h, w), torch.uint8), ar.out("edges", (b, h, w), torch.uint8)
        ws = ar.out("workspace", (nbytes,), torch.uint8, all_written=False)
        assert ws.data_ptr() % 8 == 0
        hip.check(lib.ssad_obj_mask(_p(rgb), _p(mask), _p(edges), b, h, w, wts, radius, 5 / 255.0, 15 / 255.0, _p(ws), st))
        ar.check_outputs("obj_mask")
        outs.append((mask, edges))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    for i, im in enumerate(imgs):
        assert np.array_equal(outs[0][1][i].cpu().numpy().astype(bool), C.host_edges(im)), i
        assert np.array_equal(outs[0][0][i].cpu().numpy().astype(bool), C.host_mask(im)), i
    ia.check_inputs("obj_mask")
