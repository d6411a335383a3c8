"""Images for tests/test_hip_objmask.py: csrc/objmask.hip against the host statement (dataset_generator._canny / obj_mask, pinned to
scikit-image by tests/golden/skimage.npz) where the ten kernels index differently -- H != W, rows longer than a workgroup, images
smaller than the stencils -- and where the three single-workgroup fixed-point iterations have work to do: crafted images named for a
property that is asserted on the CPU from the host statement's intermediates (the CPU half of the test module)."""
import numpy as np
from PIL import Image
from scipy import ndimage

SIDE = 64
S8 = np.ones((3, 3), int)
NONSQUARE = ((48, 80), (80, 48), (37, 53), (33, 1025))          # the last: a row longer than the 1024 threads of the iterative kernels
SMALL_RANGE = range(1, 9)                                       # sides tried for the smallest images the host statement accepts
WEAK = 10                                                       # grey levels: a gradient between the thresholds 5 and 15 after smoothing
BATCH_ORDER =(3, 5, 0, 6, 2, 4, 1)                             # seven images over chunks of three


def host_edges(img):
    from self_supervised import dataset_generator as dg
    return dg._canny(np.array(Image.fromarray(img).convert("L")), sigma=1.5, low=5, high=15)


def host_mask(img):
    from self_supervised import dataset_generator as dg
    return np.asarray(dg.obj_mask(Image.fromarray(img)).convert("1"))


def host_thinned(img):
    from self_supervised import dataset_generator as dg
    return dg._canny_thinned(np.array(Image.fromarray(img).convert("L")), 1.5, 5)


def host_stages(img):
    """The planes of dataset_generator.obj_mask after each step, restated call for call."""
    e = host_edges(img)
    sq4 = np.ones((4, 4), int)
    closed = ndimage.binary_closing(ndimage.binary_dilation(e, S8), S8)
    filled = ndimage.binary_fill_holes(closed, S8)
    eroded = ndimage.binary_erosion(filled, sq4)
    return {"edges": e, "closed": closed, "filled": filled, "eroded": eroded}


def _grey(a):
    return np.repeat(np.clip(a, 0, 255).astype(np.uint8)[..., None], 3, axis=2)


def textured(h, w, seed):
    """A bright rectangle and a disc on a noisy, slowly varying background, for any H x W."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(60 + 30 * (np.sin(xx / 9.0) * np.cos(yy / 7.0))[..., None] + 6 * rng.randn(h, w, 3), 0, 255)
    if h >= 8 and w >= 8:
        img[h // 5:h // 2, w // 6:w // 2] = np.clip(190 + 8 * rng.randn(h // 2 - h // 5, w // 2 - w // 6, 3), 0, 255)
        sel = (yy - 0.7 * h) ** 2 + (xx - 0.75 * w) ** 2 < (0.2 * min(h, w)) ** 2
        img[sel] = 140
    return img.astype(np.uint8)


def small_image(h, w):
    rng = np.random.RandomState(100 * h + w)
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def serpentine():
    """A stripe of weak contrast winding over the whole image, one short segment of it strong: the weak edges hang on the strong
    ones through a path much longer than the image side."""
    a = np.full((SIDE, SIDE), 100.0)
    rows = (8, 20, 32, 44, 56)
    for i, y in enumerate(rows):                                 # one pixel wide
        a[y, 6:58] = 100 + WEAK
        if i + 1 < len(rows):
            a[y:rows[i + 1] + 1, 57 if i % 2 == 0 else 6] = 100 + WEAK
    a[8, 6:12] = 200                                             # the strong segment, at one end ...
    a[8, 12:24] = np.linspace(200, 100 + WEAK, 12)               # ... fading into the weak stripe, so that the edge line does not break
    return _grey(a)


def two_discs():
    a = np.full((SIDE, SIDE), 40.0)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    for cy, cx in ((18, 20), (44, 42)):
        a[(yy - cy) ** 2 + (xx - cx) ** 2 < 10 ** 2] = 200
    return _grey(a)


def c_and_ring():
    """A C whose cavity opens onto the left frame, and a closed ring: only the ring's hole is a hole."""
    a = np.full((SIDE, SIDE), 40.0)
    a[6:30, 0:30] = 200                                          # the C: a block on the frame ...
    a[14:22, 0:22] = 40                                          # ... with a cavity that reaches the frame
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    d = np.sqrt((yy - 46) ** 2 + (xx - 44) ** 2)
    a[(d < 14) & (d > 8)] = 200
    return _grey(a)


def touches_all_borders():
    a = np.full((SIDE, SIDE), 40.0)
    a[28:36, :] = 200
    a[:, 28:36] = 200
    return _grey(a)


def flat():
    return _grey(np.full((SIDE, SIDE), 77.0))


def crafted():
    return {"serpentine": serpentine(), "two_discs": two_discs(), "c_and_ring": c_and_ring(), "touches_all_borders": touches_all_borders(),
            "flat": flat()}


def batch_images():
    """Seven 64 x 64 images, all different: the five crafted ones, a textured one and noise."""
    c = crafted()
    rng = np.random.RandomState(7)
    return list(c.values()) + [textured(SIDE, SIDE, 3), rng.randint(0, 256, (SIDE, SIDE, 3)).astype(np.uint8)]


def geodesic_reach(mask, seeds):
    """The largest 8-connected geodesic distance inside `mask` from `seeds` to a pixel of mask reachable from them."""
    reached = seeds & mask
    steps = 0
    while True:
        grown = ndimage.binary_dilation(reached, S8) & mask
        if (grown == reached).all():
            return steps
        reached = grown
        steps += 1
