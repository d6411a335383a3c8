"""The layout helper of the kNN margin tests (tests/test_knn_margins_host.py, tests/test_hip_knn_margins.py) and the inputs the two
files share.

embedded() puts an operand into the middle of one larger contiguous buffer.  The margins are whole rows (elements for a vector),
whole multiples of TILE = 128 -- one bank tile (BB) and one query tile (BQ) of csrc/knn_tile.h -- on each side, so the whole
over-read of a ragged tile lands inside the buffer and nothing touches unallocated memory: an over-read shows by its effect on the
answer, never by a fault.  Widths are multiples of 32 elements (or the margin is 128 rows of any width), so a view starts at a
multiple of 128 elements: every 16-byte access of the kernels stays aligned.

What the margins hold:
  bank rows        "twin rows": the queries themselves, cycled, in the bank's representation -- a margin row that becomes a candidate
                   has distance 0 to a real query, while every real row is at least 1.0 away (asserted on float64 alone);
  bank norms       (a) the twins' true norms, (b) BSQ_POISON: max(qn + bn - 2 dot, 0) is then 0 whatever the row read as;
  queries          NaN (in their representation);
  integer arrays   in-range values that point at twin rows: a leaked value selects an attractive row and does not fault;
  outputs, workspaces   NaN for floats, -7 for integers."""
import numpy as np
import torch

TILE = 128
NAN = float("nan")
INT_FILL = -7
BSQ_POISON = {torch.float32: -1e30, torch.int32: -2 ** 31}

NS = (1, 130)               # one query; one full query tile and two rows
RS = (3, 129, 300)          # fewer rows than a tile; one row past a tile; two tiles and a ragged third
DS = (32, 96)
D_UNFUSED = 100             # the unfused cosine chain alone takes a width that is no multiple of 32
KS = (1, 3)                 # the three-nearest kernels
KS_TOPK = (4, 32)           # the list kernels
SPLITS = (1, 4)             # R = 300 in 4 splits: three splits of one tile, the last one ragged, and an empty one
PATCHES = (4, 130)          # gallery: rows per image
IVF_CELLS = (3, 129, 70, 98)    # rows of the four probed cells; none is a multiple of 128
NPROBE = 2
SEED = 5200                 # of the flat cases: one at which no single-query case has a near-tie among its 32 nearest rows
COSINE_SHIFT = 2.0          # cosine cases: queries N(+2, 1), bank N(-2, 1) -- every similarity is negative, every distance above 1


def gauss(n, d, seed, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((n, d), generator=g, dtype=torch.float32) + mean


def margin(n):
    """Rows of each margin beside an operand that meets n queries: whole tiles, enough of them to hold a twin of every query."""
    return TILE * max(1, -(-int(n) // TILE))


def cycled(rows, count):
    """`count` rows: rows[0], rows[1], ..., from the start again."""
    return rows[torch.arange(int(count), device=rows.device) % rows.shape[0]]


def fill_of(dtype):
    return NAN if dtype.is_floating_point else INT_FILL


def _bits(t):
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def embedded(t, before, after, fill, device="cuda"):
    """(whole buffer, view): t copied into the middle of one contiguous buffer of its dtype on `device`, `before` / `after` rows of
    margin (elements for a vector) on its sides, both whole multiples of TILE and at least TILE.  fill: a number, or a tensor of
    t's dtype and row shape whose rows are cycled through each margin (margin row i holds fill[i % len(fill)] on either side).  The
    view is contiguous and has t's shape."""
    before, after = int(before), int(after)
    if t.dim() < 1 or min(before, after) < TILE or before % TILE or after % TILE:
        raise ValueError(f"embedded: margins must be whole multiples of {TILE} rows, at least {TILE}; got {before} and {after}")
    n = t.shape[0]
    buf = torch.empty((before + n + after,) + tuple(t.shape[1:]), dtype=t.dtype, device=device)
    for lo, hi in ((0, before), (before + n, before + n + after)):
        if torch.is_tensor(fill):
            if fill.dtype != t.dtype or tuple(fill.shape[1:]) != tuple(t.shape[1:]) or fill.shape[0] < 1:
                raise ValueError(f"embedded: fill rows {fill.dtype} {tuple(fill.shape)} do not go with {t.dtype} {tuple(t.shape)}")
            buf[lo:hi] = cycled(fill.to(device), hi - lo)
        else:
            buf[lo:hi] = fill
    buf[before:before + n] = t.to(device)
    return buf, buf[before:before + n]


def poisoned(shape, dtype, device="cuda"):
    """(whole buffer, view) of an output or workspace: view and margins alike hold NaN (floats) or -7 (integers)."""
    return embedded(torch.full(tuple(shape), fill_of(dtype), dtype=dtype), TILE, TILE, fill_of(dtype), device)


def _margins(buf, view):
    item = buf.element_size()
    first = (view.data_ptr() - buf.data_ptr()) // item
    flat = _bits(buf).reshape(-1)
    return flat[:first], flat[first + view.numel():]


def guards_intact(buf, view):
    """Every margin element of an output or workspace buffer still holds its fill, bit for bit."""
    want = _bits(torch.full((1,), fill_of(buf.dtype), dtype=buf.dtype, device=buf.device))[0]
    lo, hi = _margins(buf, view)
    return lo.numel() >= TILE and hi.numel() >= TILE and bool((lo == want).all()) and bool((hi == want).all())


def untouched(view):
    """No element of an output or workspace view was written: all hold the fill, bit for bit."""
    want = _bits(torch.full((1,), fill_of(view.dtype), dtype=view.dtype, device=view.device))[0]
    return bool((_bits(view) == want).all())


def all_written(view):
    """Every element of an output or workspace view was written: none holds the fill (no kernel writes a NaN or a -7)."""
    return bool((~torch.isnan(view)).all()) if view.dtype.is_floating_point else bool((view != INT_FILL).all())


# ---------------------------------------------------------------- the inputs of the search cases, from seeds alone

def flat_inputs(n, r, d, cosine=False):
    """(x [n][d], bank [r][d]) Gaussian rows on the host.  cosine: the two sides carry opposite means, so that every cosine distance
    of the tight bank is above 1 (the Euclidean distances of N(0, 1) rows are far above 1 as they are)."""
    shift = COSINE_SHIFT if cosine else 0.0
    return gauss(n, d, seed=SEED + 3 * d + n, mean=shift), gauss(r, d, seed=SEED + 1000 + 5 * d + r, mean=-shift)


def int8_quantiser(x, bank):
    """(lo, s, inv_s, s2) of the int8 cases: the range of the bank and the queries together, widened to whole numbers, so that no
    query loses anything to the clamp and its twin is at distance 0 exactly."""
    import knn_l2_int8_ref as qref
    both = torch.cat([x, bank])
    return qref.quantiser(np.floor(float(both.min())), np.ceil(float(both.max())))


def flat_cases(ks=KS, rs=RS):
    """(n, r, d, k) of the flat searches; a bank holds at least k rows."""
    return [(n, r, d, k) for d in DS for r in rs for n in NS for k in ks if k <= r]


def with_twins(bank, twins, m):
    """The padded operand as the reference sees it: m twin rows, the bank, m twin rows -- margins included as ordinary rows."""
    return torch.cat([cycled(twins, m), bank, cycled(twins, m)])


class GalleryCase:
    """Q = 2 query images of p rows against T = 4 bank images, of which image TWIN holds twins of the queries and appears in no
    gallery; image 0 stands before it in every gallery (its ragged last tile ends where the twins begin)."""
    Q, T, K, TWIN = 2, 4, 2, 1

    def __init__(self, p, d):
        self.p, self.d = p, d
        self.x = gauss(self.Q * p, d, seed=7000 + 3 * d + p)
        self.bank = gauss(self.T * p, d, seed=7500 + 5 * d + p)
        self.bank[self.TWIN * p:(self.TWIN + 1) * p] = cycled(self.x, p)
        self.gallery = np.array([[0, 2], [3, 0]], dtype=np.int64)
        self.m = margin(self.Q * p)

    def padded_bank(self):
        return with_twins(self.bank, self.x, self.m)


class IvfCase:
    """An inverted file of NLIST = 5 cells: the four of IVF_CELLS and, stored second, cell TWIN with a twin of every query, which no
    query probes.  bank: the ORIGINAL row order (a random permutation of the sorted one)."""
    TWIN = 1

    def __init__(self, n, d):
        self.n, self.d = n, d
        sizes = list(IVF_CELLS)
        sizes.insert(self.TWIN, n)
        self.sizes, self.nlist = sizes, len(sizes)
        self.r = sum(sizes)
        self.x = gauss(n, d, seed=8000 + 3 * d + n)
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.sorted = gauss(self.r, d, seed=8500 + 5 * d + n)
        self.sorted[self.offsets[self.TWIN]:self.offsets[self.TWIN + 1]] = self.x
        rng = np.random.RandomState(9000 + d + n)
        self.perm = rng.permutation(self.r).astype(np.int32)                # the original row of every sorted row
        self.bank = torch.empty_like(self.sorted)
        self.bank[torch.from_numpy(self.perm).long()] = self.sorted
        self.cell_of_row = np.empty(self.r, dtype=np.int64)
        self.cell_of_row[self.perm] = np.repeat(np.arange(self.nlist), sizes)
        real = np.array([c for c in range(self.nlist) if c != self.TWIN])
        self.probes = np.stack([rng.permutation(real)[:NPROBE] for _ in range(n)]).astype(np.int32)
        self.twin_rows = self.perm[self.offsets[self.TWIN]:self.offsets[self.TWIN + 1]]       # original rows of the twins
        self.m = margin(n)

    def padded_bank(self):
        return with_twins(self.bank, self.x, self.m)
