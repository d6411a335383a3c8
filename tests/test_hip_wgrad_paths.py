"""Every weight-gradient path and instantiation ops.conv_wgrad / ops.stem_wgrad can launch, against float64 (the table:
tests/wgrad_path_table.py).

Each row first asserts its (path, instantiation, splits), then runs through the ops wrapper -- twice (bit-equal), in the other layout
(to_oihw bit-equal to the permuted OHWI result) and through ops.PENDING_REDUCE + flush_reductions (bit-equal) -- and once more through
the C entry point into a NaN-filled slab reduced into a NaN-filled gradient followed by a guard region: no NaN may be left, the guard
must be untouched and the result bit-equal to the wrapper's.  Inputs sit in front of NaN guards of their own.  On the same slab the
one-float, four-float and batched reductions must agree bit for bit.  Every element is held to |err| <= 2e-5 max|want| and to
|err_e| <= tau A_e (A = the float64 gradient of |x|, |dy|).

The non-default paths are reached through switches read once per process: each switch set runs in a fresh child interpreter, one at
a time, and the first failing child stops the sequence."""
import ctypes

import numpy as np
import pytest
import torch

import wgrad_path_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    return torch.device("cuda:0")


@pytest.mark.parametrize("row", T.DEFAULT, ids=[r[0] for r in T.DEFAULT])
def test_default_path_against_fp64(dev, row):
    T.check_path(row)
    T.run_row(row, dev)


def test_switch_sets_against_fp64(dev):
    for name in T.SWITCH_SETS:
        rc, out, tiles = T.run_child(name, tiles_only=False, timeout=600)
        assert rc == 0, f"switch set {name} {T.SWITCH_SETS[name][0]}: exit status {rc}\n{out[-4000:]}"
        assert tiles is not None and len(tiles) == len(T.rows_of(name)), out[-4000:]


def _emulated_reduce(slab, cout, kpad, kreal):
    """The reducers' order of additions in float32: lane g adds splits g, g + 8, ... in order, then the eight lane sums in order."""
    s = slab.reshape(slab.shape[0], cout, kpad)[:, :, :kreal].astype(np.float32)
    lanes = []
    for g in range(8):
        v = np.zeros((cout, kreal), np.float32)
        for i in range(g, s.shape[0], 8):
            v = v + s[i]
        lanes.append(v)
    t = lanes[0]
    for q in range(1, 8):
        t = t + lanes[q]
    return t


@pytest.mark.parametrize("splits", [1, 7, 8, 25, 33, 1100])
@pytest.mark.parametrize("cout,kh,kw,cin,kpad", [(4, 1, 1, 52, 52), (24, 3, 3, 20, 184), (64, 7, 7, 3, 160), (64, 3, 3, 16, 160)])
def test_reducers_bit_identical(dev, splits, cout, kh, kw, cin, kpad):
    """wgrad_reduce (one float; forced by a dw offset by one float, or Kreal = 147) == wgrad_reduce4 == wgrad_reduce_batch, and all equal
    the float32 emulation of their documented order of additions.  Split counts reach both loops of the four-float kernel (the
    i + 24 < splits loop and the tail); Cout * Kreal is no multiple of 128 (except 64 x 144); Kpad > Kreal (the stem's 160 vs 147).
    OIHW and accumulate forms of the one- and four-float kernels too."""
    from self_supervised import _hip
    lib, st = _hip.lib(), _hip.stream()
    kreal = kh * kw * cin
    total = cout * kreal
    g = torch.Generator().manual_seed(splits * 1000 + kpad)
    slab = torch.randn(splits, cout, kpad, generator=g) * torch.exp2(torch.randint(-6, 7, (splits, 1, 1), generator=g).float())
    want = torch.from_numpy(_emulated_reduce(slab.numpy(), cout, kpad, kreal)).reshape(-1)
    sd = T._guarded(slab.to(dev))
    outs = {}
    big = torch.full((total + 1 + T.GUARD,), float("nan"), device=dev)
    _hip.check(lib.ssad_wgrad_reduce(sd.data_ptr(), big[1:].data_ptr(), splits, cout, kpad, kh, kw, cin, 0, 0, st))
    outs["reduce1"] = big[1:1 + total]
    if kreal % 4 == 0:
        four, guard = T._poisoned(total, dev)
        _hip.check(lib.ssad_wgrad_reduce(sd.data_ptr(), four.data_ptr(), splits, cout, kpad, kh, kw, cin, 0, 0, st))
        bat, bguard = T._poisoned(total, dev)
        desc = (ctypes.c_int64 * 6)(sd.data_ptr(), bat.data_ptr(), splits, cout, kpad, kreal)
        _hip.check(lib.ssad_wgrad_reduce_batch(desc, 1, st))
        outs.update(reduce4=four, batch=bat)
    torch.cuda.synchronize()
    assert torch.isnan(big[0]) and torch.isnan(big[1 + total:]).all(), "the one-float reduction wrote outside its output"
    for name, o in outs.items():
        assert torch.equal(o.cpu(), want), f"{name}: differs from the emulated order of additions"
    if kreal % 4 == 0:
        assert (guard.cpu() == T.SENTINEL).all() and (bguard.cpu() == T.SENTINEL).all()
    # OIHW and accumulate: x + t per element, permuted
    pre = torch.randn(total, generator=g)
    want_o = (pre.view(cout, cin, kh * kw) + want.view(cout, kh * kw, cin).permute(0, 2, 1)).reshape(-1)
    offs = (1, 0) if kreal % 4 == 0 else (1,)
    for off in offs:
        o = torch.full((total + 1,), float("nan"), device=dev)
        o[off:off + total] = pre.to(dev)
        _hip.check(lib.ssad_wgrad_reduce(sd.data_ptr(), o[off:].data_ptr(), splits, cout, kpad, kh, kw, cin, 1, 1, st))
        torch.cuda.synchronize()
        assert torch.equal(o[off:off + total].cpu(), want_o), f"OIHW + accumulate, dw offset {off}"


@pytest.mark.parametrize("n", [24, 25])
def test_reduce_batch_tables_of_24_and_25(dev, n):
    """One batched call over n reductions of mixed sizes and split counts (a second launch for the 25th) == one wgrad_reduce each."""
    from self_supervised import _hip
    lib, st = _hip.lib(), _hip.stream()
    g = torch.Generator().manual_seed(n)
    entries, desc = [], []
    for i in range(n):
        splits = [1, 7, 8, 25, 33, 40][i % 6]
        cout, cin, k = [(4, 8, 1), (64, 64, 3), (24, 20, 3), (128, 64, 1), (12, 36, 1)][i % 5]
        kreal = k * k * cin
        kpad = kreal + (4 if i % 3 == 0 else 0)
        slab = (torch.randn(splits, cout, kpad, generator=g)).to(dev)
        ref = torch.full((cout * kreal,), float("nan"), device=dev)
        _hip.check(lib.ssad_wgrad_reduce(slab.data_ptr(), ref.data_ptr(), splits, cout, kpad, k, k, cin, 0, 0, st))
        out, guard = T._poisoned(cout * kreal, dev)
        entries.append((slab, ref, out, guard))
        desc += [slab.data_ptr(), out.data_ptr(), splits, cout, kpad, kreal]
    _hip.check(lib.ssad_wgrad_reduce_batch((ctypes.c_int64 * len(desc))(*desc), n, st))
    torch.cuda.synchronize()
    for i, (slab, ref, out, guard) in enumerate(entries):
        assert torch.equal(out, ref), f"entry {i}"
        assert (guard.cpu() == T.SENTINEL).all(), f"entry {i}: wrote past its output"


# ---- past 2^31 elements: x holds more than 2^31 elements, zero except its first and last images ----
BIG = [
    # (id, shape, mode, expected path): halo s1 (32-bit offsets inside an image), generic fp32 (int64 pointers), g16 on half tensors
    ("big_halo_s1", (2049, 128, 128, 64, 64, 3, 1, 1), "f32", ("halo_s1", "4x16")),
    ("big_generic_f32", (4097, 128, 128, 32, 32, 3, 1, 1), "f32", ("generic_f32", "BT64")),
    ("big_g16_h", (2049, 128, 128, 64, 64, 3, 1, 1), "h16", ("g16_s1", "4x16")),
]


@pytest.mark.parametrize("row", BIG, ids=[r[0] for r in BIG])
def test_wgrad_past_2_31_elements(dev, row):
    from self_supervised import ops
    rid, shape, mode, want_path = row
    n, h, w, cin, cout, k, s, p, ho, wo = T.conv_geometry(shape)
    assert n * h * w * cin > 2 ** 31
    tdt = torch.float16 if mode == "h16" else torch.float32
    esz = 2 if mode == "h16" else 4
    need = (n * h * w * cin + n * ho * wo * cout) * esz + (1 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{rid} needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB free")
    path, inst, splits = ops.wgrad_path((n, ho, wo, cout), (n, h, w, cin), k, k, s, p, bf16=2 if mode == "h16" else False,
                                        half=mode == "h16")
    assert (path, inst) == want_path
    # the launchers' own argument limits accept the shape (checked here, on the host, before anything is launched)
    if path == "halo_s1":
        assert h * w * cin < 2 ** 28 and h * w * cout < 2 ** 28 and n * ((h + 3) // 4) * ((w + 7) // 8) < 2 ** 31
    if path == "g16_s1":
        assert n * ((ho + 3) // 4) * ((wo + 15) // 16) < 2 ** 31
    assert splits <= 65535
    g = torch.Generator().manual_seed(31)
    ends = [0, n - 1]
    xe, dye = T._scaled((2, h, w, cin), g), T._scaled((2, ho, wo, cout), g)
    x = torch.zeros((n, h, w, cin), dtype=tdt, device=dev)
    dy = torch.zeros((n, ho, wo, cout), dtype=tdt, device=dev)
    x[ends] = xe.to(dev, tdt)
    dy[ends] = dye.to(dev, tdt)
    want, a = T.reference(T._rounded(xe, mode), T._rounded(dye, mode), k, s, p)
    dw = torch.full((cout * k * k * cin,), float("nan"), device=dev)
    ops.conv_wgrad(dy, x, dw, k, k, s, p, bf16=2 if mode == "h16" else False)
    torch.cuda.synchronize()
    T.compare(rid, dw, want, a, mode)
