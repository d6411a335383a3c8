"""The evaluation-metric table: every entry point of csrc/auroc.hip (ssad_auroc, ssad_pro_curve, ssad_best_f1_threshold,
ssad_confusion_counts) at the smallest sizes that reach each geometry of its radix sort and scans, on scores whose keys vary in every
byte, compared with exact references from numpy, torch-CPU and Python integers, over buffers between poisoned guards.

Shared by tests/test_metrics_table.py (coverage, the references themselves, the workspace formulas: no GPU) and
tests/test_hip_metrics_paths.py (the kernels).

Rows.  Row = (id, entry, n, family, L, labels, weights); entry = auroc | pro | f1 | conf.
  SIZES   n = 1, 2 (one positive, one negative), 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 5 (`equal`: one tie
          group over four tiles; AUROC exactly 0.5, one curve point), 20 463 (5 tiles; scan_u32_kernel gets 1280 counters: two per
          thread, the last 384 threads idle) and 262 144 + 4097 (65 tiles; contrib_kernel, f1_argmax_kernel and confusion_kernel
          stride a second time; a scan_u32 thread has a clipped span), each for auroc, pro (dyadic weights) and f1; the last for conf too.
  single  auroc with only positives / only negatives (n = 300); pro with fp_w all zero (n_ok passed as 1), with pro_w all zero
          (n_regions passed as 1), and the general-weights row (grid, L = 97, n = 20 463, regions of 3, 7 and 300 pixels); f1 with no
          positive, with only positives, the exact tie (80 scores: (P, R) = (0.5, 0.25) at score 77 and (0.25, 0.5) at score 65 give the
          same float32 F1, the smaller threshold 65.0 wins) and full recall reached two 4096-tiles after the arg-max (the atomicMin cut);
          conf on `bits` at n = 257.
Score families (seeded numpy generators on the CPU):
  bits       random 32-bit patterns viewed as float32, NaN patterns redrawn; the low byte of the first 256 KEYS is a permutation of
             0..255 (64 distinct digits in each wave of the first sort pass).  auroc rows keep +-inf (planted past the first 256), conf
             rows plant +-inf, +-0.0 and a pair of adjacent floats; pro / f1 rows hold none (below).
  pool37     every score one of 37 such patterns: heavy ties over the whole float range
  grid       floor(rand * L) / L            equal      one value everywhere
  zeros      a grid over [-1, 1] with +0.0 on every positive and -0.0 on every negative: one tie group (the AUROC rises if they are two)
  subnormal  +-(1 .. 0x40) * 2^-149; of two adjacent values the negative (label 0) holds the larger, the positive the smaller: a flush
             to zero in the tie comparison makes them equal and moves the result
Labels are 1 with probability 0.15 + 0.7 * (rank of the score) / n: a label that travels with the wrong key moves the result.  The pro
rows take their planes from the labels: label 0 -> fp_w = 1, pro_w = 0; label 1 -> fp_w = 0, pro_w = 2^-k, k in {0, 4, 6, 10} (dyadic:
every partial sum is exact in any order) or 1 / {3, 7, 300} (general).  n_ok and n_regions are set a little under the plane sums so that
both clips at 1 are taken.

How a row runs (run_row).  The C entry points are called directly.  Every device buffer is a view between guards of GUARD_BYTES: the
inputs between bytes 0x7f (a float of 3.4e38, a double of 1.4e306, a label 1: a read past n changes the result), outputs and workspace
between 0xff.  The workspace is EXACTLY ssad_*_workspace(n) bytes.  Each entry runs twice into fresh outputs, the workspace filled with
0xA5, then 0x5A: bit-identical outputs, every guard bit-unchanged after each launch, the part of the workspace the entry does not carve
still filled, fprs[count:] / pros[count:] still poisoned; after the row every input bit-unchanged, and the wrappers of metrics.py
(auroc_gpu, best_f1_threshold_gpu, confusion_gpu, _pro_curve_device) return the values of the direct call.

References (none from the code under test), and EVERY comparison an equality but one:
  auroc  S = sum over positives (2 #negatives below + #negatives equal), scores grouped by float equality (-0.0 == +0.0, inf == inf),
         in integers; out[0] == S / (2 P N), Python's correctly rounded quotient (the kernel forms S exactly in fp64 and divides once);
         out[1] == P; NaN when P or N is 0.  Held to sklearn.metrics.roc_auc_score within 4 ulp on the finite rows (no GPU).
  pro    metrics.compute_pro from its planes on: stable descending order, cumsum, one point per run (s[1:] != s[:-1]),
         float32(cfp / n_ok), cpro / n_regions, clip.  count, fprs, pros equal bit for bit in the dyadic rows; in the general row fprs
         and count equal and |pros - ref| <= 2 n 2^-53 ref (two summation orders of n non-negative terms, each within (n - 1) u of the
         exact sum).  Held to metrics.compute_pro on a map with labelled regions (no GPU).
  f1     metrics.best_f1_threshold restated so that it also returns the maximal F1 (float32): out[0] == threshold, out[1] == F1 bit for
         bit; with no positive the largest score and NaN.  Held to the module's function on every f1 row (no GPU).
  conf   four integers from numpy's >= on float32, at a score that occurs, at +0.0 (scores hold -0.0), -inf, +inf, the upper of two
         adjacent floats, and a double between them (the C float argument rounds it).
Left out: NaN scores (the reference stack rejects them; the kernels' behaviour on them is not specified).  Infinities in pro and f1 rows:
the host functions find runs by SUBTRACTING neighbours (inf - inf = NaN splits two equal infinities into two runs) while the kernels
compare and keep one run; both sides stay as they are.
The workspace: WS_SLICES restates what each entry carves (each slice rounded up to 256 bytes).  ssad_auroc_workspace and
ssad_pro_curve_workspace equal the sum; ssad_best_f1_workspace returns 4096 bytes more (1024 x 16 bytes for partials that take
1024 x 4 and 1024 x 8): that tail must stay untouched.

MEASURED (MI355X on 2026-10-20, `pytest -s -m gpu tests/test_hip_metrics_paths.py`; for the record, never asserted): worst
|pros - ref| / bar of the general-weights row = 0.015 (the bar is a worst case over n = 20 463 roundings of one sign; the two orders'
errors mostly cancel).  Every other comparison of every row is an equality and held.
"""
import collections
import functools

import numpy as np
import torch

from bn_table import Arena, GUARD_BYTES, twice, _lib, _p, _seed

MEASURED = {"pro_general": 0.015}
WORST = {}

TILE, ROUND, WAVE, NBLK = 4096, 256, 64, 1024
IN_GUARD, WS_FILLS = 0x7F, (0xA5, 0x5A)
INF_BITS, NEG0 = 0x7F800000, 0x80000000

Row = collections.namedtuple("Row", "id entry n family L labels weights")

SIZES = [(1, "bits", 0), (2, "bits", 0), (63, "bits", 0), (64, "bits", 0), (65, "pool37", 0), (255, "zeros", 0), (256, "bits", 0),
         (257, "subnormal", 0), (4095, "bits", 0), (4096, "pool37", 0), (4097, "grid", 13), (8192, "bits", 0), (8193, "pool37", 0), (3 * 4096 + 5, "equal", 0),
         (20463, "grid", 97), (262144 + 4097, "bits", 0)]
BIG = 262144 + 4097


def _row(entry, n, family, L=0, labels="corr", weights="dyadic", tag=None):
    rid = f"{entry}_{tag or family + (str(L) if L else '')}_{n}"
    return Row(rid, entry, n, family, L, labels, weights if entry == "pro" else None)


ROWS = [_row(e, n, f, L) for (n, f, L) in SIZES for e in ("auroc", "pro", "f1")]
ROWS += [
    _row("conf", BIG, "bits"),
    _row("auroc", 300, "grid", 13, labels="allpos", tag="allpos"),
    _row("auroc", 300, "grid", 13, labels="allneg", tag="allneg"),
    _row("pro", 300, "grid", 13, labels="allpos", tag="no_fp"),
    _row("pro", 300, "grid", 13, labels="allneg", tag="no_region"),
    _row("pro", 20463, "grid", 97, weights="general", tag="general"),
    _row("f1", 300, "grid", 13, labels="allneg", tag="no_positive"),
    _row("f1", 300, "grid", 13, labels="allpos", tag="only_positives"),
    _row("f1", 80, "f1tie", tag="exact_tie"),
    _row("f1", 3 * 4096, "f1late", tag="late_full_recall"),
    _row("conf", 257, "bits"),
]


# ---- inputs ----
def _draw_bits(rng, n):
    """n random finite float32 bit patterns (NaN and inf patterns redrawn)."""
    u = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    while True:
        bad = (u & 0x7F800000) == 0x7F800000
        if not bad.any():
            return u
        u[bad] = rng.randint(0, 1 << 32, size=int(bad.sum()), dtype=np.uint64).astype(np.uint32)


def _ranks(s):
    q = np.empty(s.size, dtype=np.float64)
    q[np.argsort(s, kind="stable")] = np.arange(s.size) / max(s.size, 1)
    return q


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(row):
    """The inputs of a row as the kernels receive them: s float32 [n], y bool [n]; pro rows: fp_w uint8, pro_w float64, n_ok, n_regions;
    conf rows: thresholds (Python floats)."""
    rng = np.random.RandomState(_seed(row.id) % (1 << 31))
    n, k = row.n, Case()
    k.row, k.n, y = row, n, None
    special = "any" if row.entry == "conf" else "tail" if row.entry == "auroc" else "none"
    if row.family == "bits":
        u = _draw_bits(rng, n)
        if special != "any":
            m = min(n, 256)
            low = rng.permutation(256)[:m].astype(np.uint32) ^ np.where(u[:m] >> 31, np.uint32(0xFF), np.uint32(0))
            u[:m] = (u[:m] & np.uint32(0xFFFFFF00)) | low                     # the low byte of the KEY is the permutation
        if special == "tail" and n >= 256 + 8:
            at = 256 + rng.permutation(n - 256)[:4]
            u[at] = np.array([INF_BITS, INF_BITS | NEG0, INF_BITS, INF_BITS | NEG0], dtype=np.uint32)
        if special == "any":
            at = rng.permutation(n)[:10]
            x = np.float32(0.3718)
            pair = np.array([x, np.nextafter(x, np.float32(1))], dtype=np.float32).view(np.uint32)
            u[at] = np.array([INF_BITS, INF_BITS | NEG0, INF_BITS, INF_BITS | NEG0, NEG0, NEG0, 0, 0, pair[0], pair[1]], dtype=np.uint32)
            k.pair_at = at[8:]
        s = u.view(np.float32)
    elif row.family == "pool37":
        pool = _draw_bits(rng, 37)
        if special == "tail":
            pool[:2] = (INF_BITS, INF_BITS | NEG0)
        s = pool[rng.randint(0, 37, size=n)].view(np.float32)
    elif row.family == "grid":
        s = (np.floor(rng.rand(n) * row.L) / row.L).astype(np.float32)
    elif row.family == "equal":
        s = np.full(n, 0.625, dtype=np.float32)
    elif row.family == "zeros":
        s = ((np.floor(rng.rand(n) * 9) - 4) / 4).astype(np.float32)
    elif row.family == "subnormal":
        j, neg = rng.randint(1, 33, size=n), rng.rand(n) < 0.5
        y = rng.rand(n) < 0.15 + 0.7 * np.where(neg, 32 - j, 32 + j) / 64
        mag = np.where(neg, 2 * j - 1 + y, 2 * j - y).astype(np.uint32)          # of an adjacent pair, label 0 holds the larger VALUE
        s = (mag | np.where(neg, np.uint32(NEG0), np.uint32(0))).view(np.float32)
    elif row.family == "f1tie":
        s = np.arange(80, 0, -1).astype(np.float32)
        y = np.array([0, 0, 1, 1] + [0] * 10 + [1, 1] + [0] * 60 + [1, 1, 1, 1], dtype=bool)
    elif row.family == "f1late":
        # descending positions 0 .. 999: nine positives in ten; one last positive at position 9000 (the third tile); shuffled
        s, y = np.arange(n, 0, -1).astype(np.float32) * np.float32(0.25), np.zeros(n, dtype=bool)
        y[:1000] = rng.rand(1000) < 0.9
        y[9000] = True
        p = rng.permutation(n)
        s, y = s[p], y[p]
    else:
        raise AssertionError(row.family)
    if y is None:
        if row.labels == "allpos":
            y = np.ones(n, dtype=bool)
        elif row.labels == "allneg":
            y = np.zeros(n, dtype=bool)
        elif n <= 2:
            y = np.array([True, False][:n])
        elif row.family == "equal":
            y = rng.rand(n) < 0.4
        else:
            y = rng.rand(n) < 0.15 + 0.7 * _ranks(s)
            y[:2] = (True, False) if y.all() or not y.any() else y[:2]
    if row.family == "zeros":
        s = s.copy()
        s[s == 0] = np.where(y[s == 0], np.float32(0.0), np.float32(-0.0))
    if row.entry == "conf" and row.family == "bits":
        y[k.pair_at] = (False, True)
        x = float(s[k.pair_at[0]])
        hi = float(s[k.pair_at[1]])
        k.thresholds = [float(s[n // 2]), 0.0, float("-inf"), float("inf"), hi, x + 0.75 * (hi - x)]
    k.s, k.y = np.ascontiguousarray(s, dtype=np.float32), np.ascontiguousarray(y, dtype=bool)
    k.s.setflags(write=False)
    k.y.setflags(write=False)
    if row.entry == "pro":
        k.fp_w = (~k.y).astype(np.uint8)
        if row.weights == "general":
            w = 1.0 / np.array([3.0, 7.0, 300.0])[rng.randint(0, 3, size=n)]
        else:
            w = np.exp2(-np.array([0.0, 4.0, 6.0, 10.0]))[rng.randint(0, 4, size=n)]
        k.pro_w = np.where(k.y, w, 0.0)
        nf = int(k.fp_w.sum())
        k.n_ok = float(max(1, nf - nf // 16))
        k.n_regions = float(max(1.0, np.floor(0.9 * k.pro_w.sum())))
    return k


# ---- references ----
def ref_auroc(s, y):
    """-> (AUROC or NaN, P): the Mann-Whitney count with ties one half, in integers, divided once."""
    _, inv = np.unique(s, return_inverse=True)                    # groups by ==: -0.0 with +0.0, inf with inf
    inv = inv.reshape(-1)
    g = int(inv.max()) + 1
    pos = np.bincount(inv[y], minlength=g).astype(np.int64)
    neg = np.bincount(inv[~y], minlength=g).astype(np.int64)
    P, N = int(pos.sum()), int(neg.sum())
    assert 2 * P * N < 1 << 62
    S = int((pos * (2 * (np.cumsum(neg) - neg) + neg)).sum())
    return (S / (2 * P * N) if P and N else float("nan")), P


def ref_pro(s, fp_w, pro_w, n_ok, n_regions):
    """metrics.compute_pro from its planes on -> (fprs float32 [count], pros float64 [count])."""
    maps = np.asarray(s, dtype=np.float64)
    order = np.argsort(maps, kind="stable")[::-1]
    ss = maps[order]
    fprs = (np.cumsum(fp_w[order].astype(np.int64)) / n_ok).astype(np.float32)
    pros = np.cumsum(np.asarray(pro_w, dtype=np.float64)[order]) / n_regions
    keep = np.append(ss[1:] != ss[:-1], True)
    return np.clip(fprs[keep], None, np.float32(1.0)), np.clip(pros[keep], None, 1.0)


F1Ref = collections.namedtuple("F1Ref", "threshold f1 curve arg last")


def ref_f1(s, y):
    """metrics.best_f1_threshold, returning as well the maximal F1 (float32), the whole F1 array (ascending thresholds, then the
    appended point), and the positions in descending order of the arg-max and of the first full-recall run end."""
    s = torch.from_numpy(np.asarray(s, dtype=np.float32).copy())
    t = torch.from_numpy(np.asarray(y).copy()).to(torch.long)
    order = torch.argsort(s, descending=True)
    s, t = s[order], t[order]
    idx = torch.cat([torch.where(s[1:] - s[:-1])[0], torch.tensor([t.numel() - 1])])
    tps = torch.cumsum(t * 1.0, dim=0)[idx]
    fps = 1 + idx - tps
    last = int(torch.where(tps == tps[-1])[0][0])
    precision = torch.cat([torch.flip((tps / (tps + fps))[:last + 1], [0]), torch.ones(1)])
    recall = torch.cat([torch.flip((tps / tps[-1])[:last + 1], [0]), torch.zeros(1)])
    thr = torch.flip(s[idx][:last + 1], [0])
    f1 = ((2 * precision * recall) / (precision + recall + 1e-10)).numpy()
    assert f1.dtype == np.float32
    a = int(np.argmax(f1))
    assert a <= last, "the arg-max is the appended (precision 1, recall 0) point: no threshold belongs to it"
    return F1Ref(float(thr[a]), f1[a], f1, int(idx[last - a]), int(idx[last]))


@functools.lru_cache(maxsize=None)
def f1_ref_of(row):
    c = make_case(row)
    return ref_f1(c.s, c.y)


def ref_confusion(s, y, thr):
    p = s >= np.float32(thr)
    return int((p & y).sum()), int((p & ~y).sum()), int((~p & y).sum()), int((~p & ~y).sum())


# ---- the workspace, restated from what each entry carves ----
def cdiv(a, b):
    return -(-a // b)


def WS_SLICES(entry, n):
    nblk = cdiv(n, TILE)
    table = 256 * nblk * 4
    return {"auroc": [4 * n, 4 * n, n, n, table, 8 * n, 8 * n, 8 * n, 8 * nblk, NBLK * 16],
            "pro": [4 * n] * 4 + [table] + [8 * n] * 3 + [8 * nblk] * 2,
            "f1": [4 * n, 4 * n, n, n, n, table, 8 * n, 8 * nblk, NBLK * 4, NBLK * 8, 8]}[entry]


WS_SLACK = {"auroc": 0, "pro": 0, "f1": 4096}
WS_FN = {"auroc": "ssad_auroc_workspace", "pro": "ssad_pro_curve_workspace", "f1": "ssad_best_f1_workspace"}


def ws_carved(entry, n):
    return sum(cdiv(b, 256) * 256 for b in WS_SLICES(entry, n))


# ---- coverage: from n and the generated inputs only ----
def keys_of(s, desc):
    u = np.ascontiguousarray(s).view(np.uint32)
    k = u ^ np.where(u >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    return ~k if desc else k


@functools.lru_cache(maxsize=None)
def digit_facts(row):
    """Per sort pass, over the keys in the order that pass's scatter meets them: (number of distinct digit values, the largest number of
    distinct digits in a full wave of 64 consecutive keys, whether some full wave holds a single digit)."""
    cur = keys_of(make_case(row).s, row.entry != "auroc")
    out = []
    for p in range(4):
        d = ((cur >> np.uint32(8 * p)) & np.uint32(255)).astype(np.int64)
        full = d[:d.size // WAVE * WAVE].reshape(-1, WAVE)
        if full.size:
            distinct = 1 + (np.diff(np.sort(full, axis=1), axis=1) != 0).sum(1)
            out.append((np.unique(d).size, int(distinct.max()), bool((distinct == 1).any())))
        else:
            out.append((np.unique(d).size, 0, False))
        cur = cur[np.argsort(d, kind="stable")]
    return out


def _sorted(c):
    return np.sort(c.s)


def _distinct(c):
    return np.unique(c.s).size


def _sorts(r):
    return r.entry != "conf"


def _tie_crosses_tile(r, c):
    s = _sorted(c)
    b = np.arange(TILE, c.n, TILE)
    return _sorts(r) and bool((s[b - 1] == s[b]).any())


def _zero_tie(r, c):
    u = c.s.view(np.uint32)
    return _sorts(r) and bool((u == NEG0).any() and (u == 0).any())


def _adjacent_subnormals(r, c):
    u = c.s.view(np.uint32).astype(np.int64)
    sub = ((u & 0x7F800000) == 0) & ((u & 0x007FFFFF) != 0)
    lab = {}
    for v, y in zip(u[sub].tolist(), c.y[sub].tolist()):
        lab.setdefault(v, set()).add(y)
    return _sorts(r) and any(v + 1 in lab and (v >> 31) == ((v + 1) >> 31) and len(lab[v] | lab[v + 1]) == 2 for v in lab)


def _scan_len(r):
    return 256 * cdiv(r.n, TILE)


CASES = {
    "n < 64": lambda r, c: _sorts(r) and r.n < WAVE,
    "n exactly a wave": lambda r, c: _sorts(r) and r.n == WAVE,
    "n exactly a round": lambda r, c: _sorts(r) and r.n == ROUND,
    "n exactly a tile": lambda r, c: _sorts(r) and r.n == TILE,
    "n exactly two tiles": lambda r, c: _sorts(r) and r.n == 2 * TILE,
    "one past a wave": lambda r, c: _sorts(r) and r.n == WAVE + 1,
    "one past a round": lambda r, c: _sorts(r) and r.n == ROUND + 1,
    "one past a tile": lambda r, c: _sorts(r) and r.n == TILE + 1,
    "one past two tiles": lambda r, c: _sorts(r) and r.n == 2 * TILE + 1,
    "ragged last round": lambda r, c: _sorts(r) and r.n > ROUND and r.n % ROUND != 0,
    "scan_u32: several counters per thread, trailing threads idle": lambda r, c: _sorts(r) and cdiv(_scan_len(r), 1024) >= 2
    and cdiv(_scan_len(r), cdiv(_scan_len(r), 1024)) < 1024,
    "scan_u32: a thread with a clipped span": lambda r, c: _sorts(r) and _scan_len(r) % cdiv(_scan_len(r), 1024) != 0,
    "more than 1024 x 256 scores, auroc": lambda r, c: r.entry == "auroc" and r.n > NBLK * 256,
    "more than 1024 x 256 scores, f1": lambda r, c: r.entry == "f1" and r.n > NBLK * 256,
    "more than 1024 x 256 scores, conf": lambda r, c: r.entry == "conf" and r.n > NBLK * 256,
    "more than 1024 x 256 scores, pro": lambda r, c: r.entry == "pro" and r.n > NBLK * 256,
    "all 256 values of each of the four digits": lambda r, c: _sorts(r) and all(f[0] == 256 for f in digit_facts(r)),
    "a wave of 64 distinct digits": lambda r, c: _sorts(r) and any(f[1] == WAVE for f in digit_facts(r)),
    "a wave of a single digit": lambda r, c: _sorts(r) and any(f[2] for f in digit_facts(r)),
    "a tie group crosses a tile boundary": _tie_crosses_tile,
    "a tie group of -0.0 and +0.0": _zero_tie,
    "adjacent subnormals with different labels": _adjacent_subnormals,
    "+inf and -inf present": lambda r, c: bool((c.s == np.inf).any() and (c.s == -np.inf).any()),
    "AUROC undefined": lambda r, c: r.entry == "auroc" and (c.y.all() or not c.y.any()),
    "F1 maximum attained twice": lambda r, c: r.entry == "f1" and c.y.any()
    and int((f1_ref_of(r).curve == f1_ref_of(r).f1).sum()) >= 2,
    "F1 arg-max in an earlier tile than the first full-recall run end": lambda r, c: r.entry == "f1" and c.y.any()
    and f1_ref_of(r).arg // TILE < f1_ref_of(r).last // TILE,
    "count = 1 with n > 1": lambda r, c: r.entry == "pro" and r.n > 1 and _distinct(c) == 1,
    "count = n with n > 1": lambda r, c: r.entry == "pro" and r.n > 1 and _distinct(c) == r.n,
    "both pro clips taken": lambda r, c: r.entry == "pro" and c.fp_w.sum() > c.n_ok and c.pro_w.sum() > c.n_regions,
}


# ---- the launches ----
class InArena(Arena):
    """Inputs: guards of 0x7f bytes -- a huge finite float or double, a label 1."""

    def _big(self, nbytes):
        return torch.full((nbytes + 2 * GUARD_BYTES,), IN_GUARD, dtype=torch.uint8, device=self.dev)


def _poisoned(t):
    return bool((t.contiguous().reshape(-1).view(torch.uint8) == 255).all())


def _workspace(ar, entry, n, lib, fill):
    nbytes = getattr(lib, WS_FN[entry])(n)
    assert nbytes == ws_carved(entry, n) + WS_SLACK[entry]
    ws = ar.out("workspace", (nbytes,), torch.uint8, all_written=False)
    ws.fill_(fill)
    return ws, nbytes


def _check_ws_tail(rid, ws, entry, n, fill):
    assert bool((ws[ws_carved(entry, n):] == fill).all()), f"{rid}: the entry wrote past what it carves from the workspace"


def _zeroed(ar, name, shape, dtype):
    t = ar.out(name, shape, dtype, all_written=False)
    t.zero_()
    return t


def _same(a, b):
    return a == b or (a != a and b != b)


def _run_auroc(rid, k, dev):
    from self_supervised import metrics
    hip, lib, st = _lib()
    ia = InArena(dev)
    sd, ld = ia.inp("scores", torch.from_numpy(k.s.copy())), ia.inp("labels", torch.from_numpy(k.y.astype(np.uint8)))
    fills = iter(WS_FILLS)

    def launch():
        ar, fill = Arena(dev), next(fills)
        ws, nbytes = _workspace(ar, "auroc", k.n, lib, fill)
        out = ar.out("out", (2,), torch.float64, all_written=False)
        hip.check(lib.ssad_auroc(_p(sd), _p(ld), k.n, _p(ws), nbytes, _p(out), st))
        ar.check_outputs(rid)
        _check_ws_tail(rid, ws, "auroc", k.n, fill)
        return {"out": out}
    out = twice(rid, launch)["out"]
    assert not _poisoned(out[:1]) and not _poisoned(out[1:]), f"{rid}: an element of `out` left unwritten"
    got, positives = out.cpu().tolist()
    want, P = ref_auroc(k.s, k.y)
    print(f"   {rid}: AUROC {got!r}, reference {want!r}; positives {positives}, reference {P}", flush=True)
    assert _same(got, want), f"{rid}: AUROC {got!r} is not the correctly rounded S / (2 P N) = {want!r}"
    assert positives == P, f"{rid}: out[1] = {positives}, {P} positives"
    assert _same(metrics.auroc_gpu(ld, sd), got), f"{rid}: metrics.auroc_gpu differs from the direct call"
    ia.check_inputs(rid)


def _run_pro(rid, k, dev):
    from self_supervised import metrics
    hip, lib, st = _lib()
    n = k.n
    ia = InArena(dev)
    sd = ia.inp("scores", torch.from_numpy(k.s.copy()))
    fd, pd = ia.inp("fp_w", torch.from_numpy(k.fp_w)), ia.inp("pro_w", torch.from_numpy(k.pro_w))
    fills = iter(WS_FILLS)

    def launch():
        ar, fill = Arena(dev), next(fills)
        ws, nbytes = _workspace(ar, "pro", n, lib, fill)
        o = {"fprs": ar.out("fprs", (n,), torch.float32, all_written=False), "pros": ar.out("pros", (n,), torch.float64, all_written=False),
             "count": _zeroed(ar, "count", (1,), torch.int64)}
        hip.check(lib.ssad_pro_curve(_p(sd), _p(fd), _p(pd), n, k.n_ok, k.n_regions, _p(ws), nbytes, _p(o["fprs"]), _p(o["pros"]),
                                     _p(o["count"]), st))
        ar.check_outputs(rid)
        _check_ws_tail(rid, ws, "pro", n, fill)
        return o
    o = twice(rid, launch)
    wf, wp = ref_pro(k.s, k.fp_w, k.pro_w, k.n_ok, k.n_regions)
    count = int(o["count"].item())
    assert count == wf.size, f"{rid}: count {count}, the reference has {wf.size} points"
    assert _poisoned(o["fprs"][count:]) and _poisoned(o["pros"][count:]), f"{rid}: fprs / pros written past `count`"
    gf, gp = o["fprs"][:count].cpu().numpy(), o["pros"][:count].cpu().numpy()
    assert np.array_equal(gf.view(np.uint32), wf.view(np.uint32)), f"{rid}: fprs differ at {int(np.argmax(gf != wf))}"
    if k.row.weights == "general":
        bar = 2 * n * 2.0 ** -53 * wp
        ratio = float(np.max(np.abs(gp - wp) / bar))
        WORST["pro_general"] = max(WORST.get("pro_general", 0.0), ratio)
        print(f"   {rid}: worst |pros - ref| / bar {ratio:.3e}", flush=True)
        assert bool(np.all(np.abs(gp - wp) <= bar)), f"{rid}: pros outside 2 n 2^-53 ref, worst ratio {ratio:.3f}"
    else:
        bad = gp.view(np.uint64) != wp.view(np.uint64)
        print(f"   {rid}: {count} points, {int(bad.sum())} pros differ", flush=True)
        assert not bad.any(), f"{rid}: pros differ at {int(np.argmax(bad))}: {gp[np.argmax(bad)]!r} != {wp[np.argmax(bad)]!r}"
    f2, p2 = metrics._pro_curve_device(sd, fd, pd, k.n_ok, k.n_regions)
    assert np.array_equal(f2[1:-1], gf.astype(np.float64)) and np.array_equal(p2[1:-1], gp), f"{rid}: _pro_curve_device differs from the direct call"
    assert (f2[0], f2[-1], p2[0], p2[-1]) == (0.0, 1.0, 0.0, 1.0)
    ia.check_inputs(rid)


def _run_f1(rid, k, dev):
    from self_supervised import metrics
    hip, lib, st = _lib()
    ia = InArena(dev)
    sd, ld = ia.inp("scores", torch.from_numpy(k.s.copy())), ia.inp("targets", torch.from_numpy(k.y.astype(np.uint8)))
    fills = iter(WS_FILLS)

    def launch():
        ar, fill = Arena(dev), next(fills)
        ws, nbytes = _workspace(ar, "f1", k.n, lib, fill)
        out = ar.out("out", (2,), torch.float32, all_written=False)
        hip.check(lib.ssad_best_f1_threshold(_p(sd), _p(ld), k.n, _p(ws), nbytes, _p(out), st))
        ar.check_outputs(rid)
        _check_ws_tail(rid, ws, "f1", k.n, fill)
        return {"out": out}
    out = twice(rid, launch)["out"]
    assert not _poisoned(out[:1]) and not _poisoned(out[1:]), f"{rid}: an element of `out` left unwritten"
    got = out.cpu().numpy()
    want = f1_ref_of(k.row)
    print(f"   {rid}: threshold {got[0]!r}, reference {want.threshold!r}; F1 {got[1]!r}, reference {want.f1!r}", flush=True)
    assert float(got[0]) == want.threshold, f"{rid}: threshold {got[0]!r}, reference {want.threshold!r}"
    if k.y.any():
        assert got[1:].view(np.uint32)[0] == np.array([want.f1]).view(np.uint32)[0], f"{rid}: F1 {got[1]!r}, reference {want.f1!r}"
    else:
        assert np.isnan(want.f1) and np.isnan(got[1]), f"{rid}: no positive, F1 {got[1]!r} is not NaN"
        assert float(got[0]) == float(k.s.max())
    assert metrics.best_f1_threshold_gpu(sd, ld) == float(got[0]), f"{rid}: metrics.best_f1_threshold_gpu differs from the direct call"
    ia.check_inputs(rid)


def _run_conf(rid, k, dev):
    from self_supervised import metrics
    hip, lib, st = _lib()
    ia = InArena(dev)
    sd, ld = ia.inp("scores", torch.from_numpy(k.s.copy())), ia.inp("targets", torch.from_numpy(k.y.astype(np.uint8)))
    for thr in k.thresholds:
        eid = f"{rid}[threshold {thr!r}]"

        def launch():
            ar = Arena(dev)
            out = _zeroed(ar, "out", (4,), torch.int64)
            hip.check(lib.ssad_confusion_counts(_p(sd), _p(ld), k.n, thr, _p(out), st))
            ar.check_outputs(eid)
            return {"out": out}
        got = tuple(twice(eid, launch)["out"].tolist())
        want = ref_confusion(k.s, k.y, thr)
        print(f"   {eid}: {got}, reference {want}", flush=True)
        assert got == want, f"{eid}: (tp, fp, fn, tn) = {got}, reference {want}"
        assert metrics.confusion_gpu(sd, ld, thr) == got, f"{eid}: metrics.confusion_gpu differs from the direct call"
    ia.check_inputs(rid)


def run_row(row, dev):
    k = make_case(row)
    {"auroc": _run_auroc, "pro": _run_pro, "f1": _run_f1, "conf": _run_conf}[row.entry](row.id, k, dev)


def run_argument_checks(dev):
    """Refusals happen before any launch: a workspace one byte short (the message names the workspace function), n = 0; the outputs stay
    poisoned."""
    hip, lib, st = _lib()
    n = 300
    ia = InArena(dev)
    sd, ld = ia.inp("scores", torch.rand(n)), ia.inp("labels", (torch.rand(n) < 0.5).to(torch.uint8))
    wd = ia.inp("pro_w", torch.rand(n, dtype=torch.float64))
    for entry in ("auroc", "pro", "f1"):
        need = getattr(lib, WS_FN[entry])(n)
        for nn, nbytes in ((n, need - 1), (0, need)):
            ar = Arena(dev)
            ws = ar.out("workspace", (need - 1,), torch.uint8, all_written=False)
            if entry == "auroc":
                outs = [ar.out("out", (2,), torch.float64, all_written=False)]
                rc = lib.ssad_auroc(_p(sd), _p(ld), nn, _p(ws), nbytes, _p(outs[0]), st)
            elif entry == "f1":
                outs = [ar.out("out", (2,), torch.float32, all_written=False)]
                rc = lib.ssad_best_f1_threshold(_p(sd), _p(ld), nn, _p(ws), nbytes, _p(outs[0]), st)
            else:
                outs = [ar.out("fprs", (n,), torch.float32, all_written=False), ar.out("pros", (n,), torch.float64, all_written=False),
                        ar.out("count", (1,), torch.int64, all_written=False)]
                rc = lib.ssad_pro_curve(_p(sd), _p(ld), _p(wd), nn, 1.0, 1.0, _p(ws), nbytes, *[_p(o) for o in outs], st)
            msg = lib.ssad_last_error().decode()
            assert rc != 0, f"{entry}: n = {nn}, workspace_bytes = {nbytes} accepted"
            if nn:
                assert WS_FN[entry] in msg, f"{entry}: the refusal does not name {WS_FN[entry]}: {msg!r}"
            ar.check_outputs(entry)
            assert all(_poisoned(o) for o in outs) and _poisoned(ws), f"{entry}: a refused call wrote to its outputs"
    out = _zeroed(Arena(dev), "out", (4,), torch.int64)
    assert lib.ssad_confusion_counts(_p(sd), _p(ld), 0, 0.5, _p(out), st) != 0
    assert out.tolist() == [0, 0, 0, 0]
    ia.check_inputs("argument checks")
