"""Tensor-level wrappers over the C ABI: allocate outputs with torch, launch on the current stream."""
import os

import numpy as np
import torch

from . import _hip


PROFILE = None      # bench.py sets this to a list: every launch is then bracketed by HIP events on its stream


def _new(shape, like):
    return torch.empty(shape, device=like.device, dtype=torch.float32)


def _newh(shape, like):
    """A half tensor: the activations of the precision-16 step are stored as torch.autocast stores them."""
    return torch.empty(shape, device=like.device, dtype=torch.float16)


def _is_h(t):
    return t is not None and t.dtype == torch.float16


def _p(t, allow_none=False):
    """Device pointer of a contiguous fp32 OR half tensor (the `_h` entry points take void*)."""
    return _hip.ptr(t, allow_none, torch.float16 if _is_h(t) else torch.float32)


def _run(kernel, flops, nbytes, rc_fn, exec_flops=None, tile=None):
    """Launch through the C ABI; when PROFILE is on, bracket the launch with events on the launch stream.
    flops = ALGORITHMIC FLOPs of the op; exec_flops = the FLOPs the kernel really issues to the matrix cores when that
    is fewer (position-major convs skip the taps that fall into the zero padding); tile = a callable returning the
    instantiation's tile code (ssad_conv_igemm_tile), evaluated only while profiling."""
    if PROFILE is None:
        _hip.check(rc_fn())
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _hip.check(rc_fn())
    e1.record()
    PROFILE.append((kernel, flops, nbytes, e0, e1, flops if exec_flops is None else exec_flops, tile() if tile else None))


# Launches nobody on the critical path of a training step waits for -- the slab reduction behind a weight-gradient kernel, the
# weight gradients of the head's small linear layers, global-average-pool rows that only the head reads -- may leave the main
# stream: TrainEngine sets ASIDE to an object whose launch(fn, keep) runs fn on a second HIP stream that has just been made to
# wait for the main one, and keeps `keep` (the operands) alive until the streams are joined.  Recorded into a hipGraph this is
# a fork / join: the small kernel becomes a parallel branch beside the next big kernel instead of a ~5-12 us link in the chain.
ASIDE = None


def _run_aside(kernel, flops, nbytes, rc_fn, keep=()):
    if ASIDE is None or PROFILE is not None:
        return _run(kernel, flops, nbytes, rc_fn)
    ASIDE.launch(lambda: _hip.check(rc_fn()), keep)


# Slab reductions of the weight-gradient kernels, collected while PENDING_REDUCE is a list (TrainEngine sets it for a training step)
# and run together by flush_reductions() where the gradients are first needed: one launch (ssad_wgrad_reduce_batch) instead of one
# per layer.  Entries keep their slabs alive until the flush.
PENDING_REDUCE = None


def _wgrad_reduce(slab, dw_out, splits, cout, kpad, kh, kw, cin, to_oihw, accumulate):
    kreal = kh * kw * cin
    if (PENDING_REDUCE is not None and PROFILE is None and not to_oihw and not accumulate and kreal % 4 == 0 and kpad % 4 == 0
            and slab.data_ptr() % 16 == 0 and dw_out.data_ptr() % 16 == 0):
        PENDING_REDUCE.append((slab, dw_out, int(splits), int(cout), int(kpad), int(kreal)))
        return
    _run_aside("wgrad_reduce", 0.0, 4.0 * slab.numel(),
               lambda: _hip.lib().ssad_wgrad_reduce(_hip.ptr(slab), _hip.ptr(dw_out), splits, cout, kpad, kh, kw, cin, int(to_oihw),
                                                    int(accumulate), _hip.stream()), keep=(slab,))


def flush_reductions():
    """Run the collected slab reductions (one launch per 24) and release their slabs."""
    if not PENDING_REDUCE:
        return
    import ctypes
    desc = []
    for slab, out, splits, cout, kpad, kreal in PENDING_REDUCE:
        desc += [slab.data_ptr(), out.data_ptr(), splits, cout, kpad, kreal]
    arr = (ctypes.c_int64 * len(desc))(*desc)
    _hip.check(_hip.lib().ssad_wgrad_reduce_batch(arr, len(PENDING_REDUCE), _hip.stream()))
    del PENDING_REDUCE[:]


def drain_profile():
    """-> [{kernel, flops, exec_flops, bytes, ms}] for every launch recorded since PROFILE was set."""
    global PROFILE
    recs = PROFILE or []
    torch.cuda.synchronize()
    out = [{"kernel": k, "flops": f, "bytes": b, "ms": e0.elapsed_time(e1), "exec_flops": x, "tile": t}
           for k, f, b, e0, e1, x, t in recs]
    PROFILE = [] if PROFILE is not None else None
    return out


def _inbounds_taps(h, w, kh, kw, stride, pad):
    """Sum over output positions of the filter taps that land inside the image (what a position-major conv executes)."""
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    ny = sum(sum(1 for ky in range(kh) if 0 <= oy * stride - pad + ky < h) for oy in range(ho))
    nx = sum(sum(1 for kx in range(kw) if 0 <= ox * stride - pad + kx < w) for ox in range(wo))
    return ny * nx


IGEMM_FWD, IGEMM_HWNC, IGEMM_RING, IGEMM_STATS, IGEMM_DGRAD = range(5)     # ssad_conv_igemm_tile(_id) modes (include/ssad.h)


# IgemmTile (csrc/conv_igemm.hip) in enum order: short name -> template arguments BM, BN, TM, TN, BK, DB (two LDS stages)
IGEMM_TILES = [("256x64_K16", (256, 64, 2, 2, 16, True)), ("256x64_SB", (256, 64, 2, 2, 32, False)),
               ("128x64", (128, 64, 1, 2, 32, True)), ("256x128", (256, 128, 2, 2, 32, True)),
               ("256x128_W4", (256, 128, 4, 2, 32, True)), ("128x256", (128, 256, 2, 4, 32, True)),
               ("64x64", (64, 64, 1, 1, 32, True)), ("128x128", (128, 128, 2, 2, 32, True)),
               ("256x256", (256, 256, 4, 4, 32, True)), ("128x64_SB", (128, 64, 1, 2, 32, False)),
               ("128x64_K16", (128, 64, 1, 2, 16, True)), ("128x128_K16", (128, 128, 2, 2, 16, True)),
               ("128x256_K16", (128, 256, 2, 4, 16, True))]
LINEAR_SMALL = "linear_small"


def igemm_tile(n, h, w, cin, cout, kh, kw, stride, pad, mode):
    """(short tile name, position-major) of the exact-fp32 implicit-GEMM launch of a problem (ssad_conv_igemm_tile_id).  The shape
    is the forward conv's; mode is the entry point (IGEMM_*: IGEMM_DGRAD = the input gradient of that conv).  1 x 1 layers over
    1 x 1 maps with few rows go to csrc/linear_small.hip instead: (LINEAR_SMALL, False)."""
    k = cout if mode == IGEMM_DGRAD else cin
    if (mode in (IGEMM_FWD, IGEMM_STATS, IGEMM_DGRAD) and kh == kw == h == w == 1 and stride == 1 and pad == 0 and k % 4 == 0
            and n <= _hip.lib().ssad_linear_small_max_rows()):
        return LINEAR_SMALL, False
    t = _hip.lib().ssad_conv_igemm_tile_id(n, h, w, cin, cout, kh, kw, stride, pad, int(mode))
    return IGEMM_TILES[t % 100][0], t >= 100


def igemm_tile_name(n, h, w, cin, cout, kh, kw, stride, pad, mode):
    """Template arguments of that launch (csrc/conv_igemm.hip launch<BM, BN, TM, TN, BK, TS, POS[, DB]>)."""
    name, pos = igemm_tile(n, h, w, cin, cout, kh, kw, stride, pad, mode)
    if name == LINEAR_SMALL:
        return "<linear_small: 32 x 32 tiles, csrc/linear_small.hip>"
    bm, bn, tm, tn, bk, db = dict(IGEMM_TILES)[name]
    ts = stride if mode == IGEMM_DGRAD else 1
    return f"<{bm},{bn},{tm},{tn},{bk},{ts},{'true' if pos else 'false'}{'' if db else ',false'}>"


def _kname(base, mode):
    """Profile label of an MFMA kernel by operand mode (False/0 fp32, True/1 bf16, 2 fp16, 3 / 6 split-bf16)."""
    return base + {0: "_f32", 1: "_bf16", 2: "_f16", 3: "_x3", 6: "_x6"}[int(mode)]


def repack_oihw_to_ohwi(w):
    o, i, kh, kw = w.shape
    out = _new((o, kh, kw, i), w)
    _hip.check(_hip.lib().ssad_repack_oihw_to_ohwi(_hip.ptr(w), _hip.ptr(out), o, i, kh, kw, _hip.stream()))
    return out


def repack_ohwi_to_oihw(w):
    o, kh, kw, i = w.shape
    out = _new((o, i, kh, kw), w)
    _hip.check(_hip.lib().ssad_repack_ohwi_to_oihw(_hip.ptr(w), _hip.ptr(out), o, i, kh, kw, _hip.stream()))
    return out


def pack_stem_weight(w):
    """conv1's filter in the stem kernel's K order; w OIHW [64][3][7][7], or OHWI [64][7][7][3] (the parameter arena's layout)."""
    out = _new((168, 64), w)
    if tuple(w.shape) == (64, 7, 7, 3):
        _hip.check(_hip.lib().ssad_pack_stem_weight_ohwi(_hip.ptr(w), _hip.ptr(out), _hip.stream()))
        return out
    assert tuple(w.shape) == (64, 3, 7, 7)
    _hip.check(_hip.lib().ssad_pack_stem_weight(_hip.ptr(w), _hip.ptr(out), _hip.stream()))
    return out


def stem_geometry(H, W, patch_dim, patch_stride):
    """(samples per image, Hv, Wv, Ho, Wo) -- window + nearest-resize rule of models.py:211-219."""
    if patch_dim:
        p = ((H - patch_dim) // patch_stride + 1) * ((W - patch_dim) // patch_stride + 1)
        wh = ww = patch_dim
    else:
        p, wh, ww = 1, H, W
    hv, wv = (64, 64) if (wh < 64 or ww < 64) else (wh, ww)
    return p, hv, wv, (hv - 1) // 2 + 1, (wv - 1) // 2 + 1


def stem_fwd(img, wk, scale, shift, relu=True, patch_dim=0, patch_stride=0, hwnc=False, resize_to=None):
    """-> [N][Ho][Wo][64], or the position-major [Ho][Wo][N][64] when hwnc.
    resize_to = (Hv, Wv): the whole image nearest-resized to Hv x Wv inside the loader (floor(v * H / Hv): F.interpolate's 'nearest')
    instead of the reference's to-64 rule -- the per-image dense map of the patch-scoring pass takes the 2x upsample this way."""
    b, c, h, w = img.shape
    assert c == 3
    p, hv, wv, ho, wo = stem_geometry(h, w, patch_dim, patch_stride)
    if resize_to is not None:
        assert not patch_dim
        hv, wv = resize_to
        ho, wo = (hv - 1) // 2 + 1, (wv - 1) // 2 + 1
    n = b * p
    out = _new((ho, wo, n, 64) if hwnc else (n, ho, wo, 64), img)
    _run("stem_conv7x7", 2.0 * n * ho * wo * 64 * 147, 4.0 * (b * 3 * h * w + n * ho * wo * 64),
         lambda: _hip.lib().ssad_stem_fwd(_hip.ptr(img), b, h, w, patch_dim, patch_stride, hv, wv, _hip.ptr(wk),
                                          _hip.ptr(scale, True), _hip.ptr(shift, True), int(relu), int(hwnc),
                                          _hip.ptr(out), _hip.stream()))
    return out


def stem_fwd_stats(img, wk, eps, momentum, running_mean, running_var):
    """Training stem conv: -> (z [B][Ho][Wo][64], mean, invstd) with the BatchNorm statistics taken from the accumulators."""
    b, c, h, w = img.shape
    assert c == 3
    _, hv, wv, ho, wo = stem_geometry(h, w, 0, 0)
    out = _new((b, ho, wo, 64), img)
    mean, invstd = _new((64,), img), _new((64,), img)
    ws = torch.empty(_hip.lib().ssad_stem_stats_rows() * 128, device=img.device, dtype=torch.float64)
    _run("stem_conv7x7", 2.0 * b * ho * wo * 64 * 147, 4.0 * (b * 3 * h * w + b * ho * wo * 64),
         lambda: _hip.lib().ssad_stem_fwd_stats(_hip.ptr(img), b, h, w, hv, wv, _hip.ptr(wk), _hip.ptr(out), eps, momentum,
                                                _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(running_mean, True),
                                                _hip.ptr(running_var, True), ws.data_ptr(), _hip.stream()))
    return out, mean, invstd


def stem_fwd_stats16(img, w_oihw, eps, momentum, running_mean, running_var, mode, out_half=False):
    """The training stem conv with fp16 (mode 2) or bf16 (mode 1) operands and fp32 accumulation (csrc/stem16.hip):
    -> (z [B][Ho][Wo][64] fp32, mean, invstd), statistics from the accumulators as in stem_fwd_stats.
    out_half (mode 2): z is stored as halves and the statistics are those of the stored halves."""
    b, c, h, w = img.shape
    ohwi = tuple(w_oihw.shape) == (64, 7, 7, 3)           # the parameter arena's layout: packed without an OIHW copy
    assert c == 3 and (ohwi or tuple(w_oihw.shape) == (64, 3, 7, 7)) and int(mode) in (1, 2)
    assert h >= 64 and w >= 64, "images below 64 x 64 are resized first (models.py:217-219): that is the fp32 stem's loader"
    lib = _hip.lib()
    wk = torch.empty(14 * 64 * 16, device=img.device, dtype=torch.float16 if int(mode) == 2 else torch.bfloat16)
    _hip.check((lib.ssad_pack_stem_weight16_ohwi if ohwi else lib.ssad_pack_stem_weight16)(_hip.ptr(w_oihw), wk.data_ptr(), int(int(mode) == 2),
                                                                                             _hip.stream()))
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    mean, invstd = _new((64,), img), _new((64,), img)
    ws = torch.empty(lib.ssad_stem_stats_rows() * 128, device=img.device, dtype=torch.float64)
    if out_half:
        assert int(mode) == 2
        out = _newh((b, ho, wo, 64), img)
        _run("stem_conv7x7_h16", 2.0 * b * ho * wo * 64 * 147, 4.0 * b * 3 * h * w + 2.0 * b * ho * wo * 64,
             lambda: lib.ssad_stem_fwd_stats16_h(_hip.ptr(img), b, h, w, wk.data_ptr(), out.data_ptr(), eps, momentum, _hip.ptr(mean),
                                                 _hip.ptr(invstd), _hip.ptr(running_mean, True), _hip.ptr(running_var, True),
                                                 ws.data_ptr(), _hip.stream()))
        return out, mean, invstd
    out = _new((b, ho, wo, 64), img)
    _run(_kname("stem_conv7x7", mode), 2.0 * b * ho * wo * 64 * 147, 4.0 * (b * 3 * h * w + b * ho * wo * 64),
         lambda: lib.ssad_stem_fwd_stats16(_hip.ptr(img), b, h, w, wk.data_ptr(), _hip.ptr(out), eps, momentum, _hip.ptr(mean),
                                           _hip.ptr(invstd), _hip.ptr(running_mean, True), _hip.ptr(running_var, True),
                                           ws.data_ptr(), int(int(mode) == 2), _hip.stream()))
    return out, mean, invstd


def pack_stem_weight_folded(w):
    assert tuple(w.shape) == (64, 3, 7, 7)
    out = _new((24, 2, 64), w)
    _hip.check(_hip.lib().ssad_pack_stem_weight_folded(_hip.ptr(w), _hip.ptr(out), _hip.stream()))
    return out


def stem_patch_pool_fwd(img, wf, scale, shift, patch_stride=8, hwnc=False, skip=None):
    """32x32 windows (stride patch_stride) of img [B][3][H][W] -> pooled stem output [N][16][16][64] / [16][16][N][64]:
    window + 2x nearest upsample + conv7x7/2 + affine + ReLU + max-pool in one kernel.  skip = (lo, hi): the pooled positions
    lo <= py, px <= hi of every patch are left unwritten (nobody reads them when layer1 is shared between overlapping patches)."""
    b, c, h, w = img.shape
    n = b * ((h - 32) // patch_stride + 1) * ((w - 32) // patch_stride + 1)
    out = _new((16, 16, n, 64) if hwnc else (n, 16, 16, 64), img)
    lo, hi = skip if skip is not None else (1, 0)
    _run("stem_patch_pool", 2.0 * n * 32 * 32 * 64 * 147, 4.0 * (img.numel() + out.numel()),
         lambda: _hip.lib().ssad_stem_patch_pool_fwd_ring(_hip.ptr(img), b, h, w, patch_stride, _hip.ptr(wf), _hip.ptr(scale, True),
                                                          _hip.ptr(shift, True), int(hwnc), lo, hi, _hip.ptr(out), _hip.stream()))
    return out


def stem_patch_border_fwd(img, wf, scale, shift, patch_stride=8):
    """Pooled rows / columns 0, 1 and 15 of every 32x32 window's stem map (the positions its own zero padding reaches), written into a
    position-major [16][16][N][64] buffer whose other positions stay unwritten: see patch_gather_hwnc for rows / columns 2-3, 13-14."""
    b, c, h, w = img.shape
    n = b * ((h - 32) // patch_stride + 1) * ((w - 32) // patch_stride + 1)
    out = _new((16, 16, n, 64), img)
    _run("stem_patch_pool", 2.0 * n * 13 * 32 * 64 * 147, 4.0 * (img.numel() + out.numel() * 87 // 256),
         lambda: _hip.lib().ssad_stem_patch_border_fwd(_hip.ptr(img), b, h, w, patch_stride, _hip.ptr(wf), _hip.ptr(scale, True),
                                                       _hip.ptr(shift, True), _hip.ptr(out), _hip.stream()))
    return out


def maxpool3x3s2_fwd(x, hwnc=False):
    if hwnc:
        h, w, n, c = x.shape
        out = _new(((h - 1) // 2 + 1, (w - 1) // 2 + 1, n, c), x)
    else:
        n, h, w, c = x.shape
        out = _new((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), x)
    _run("maxpool3x3s2", 0.0, 4.0 * (x.numel() + out.numel()),
         lambda: _hip.lib().ssad_maxpool3x3s2_fwd(_hip.ptr(x), _hip.ptr(out), n, h, w, c, int(hwnc), _hip.stream()))
    return out


def _split_fwd(mode):
    return _hip.lib().ssad_conv_igemm_fwd_x6 if mode == 6 else _hip.lib().ssad_conv_igemm_fwd_x3


def conv_fwd_hwnc(x, w_ohwi, scale=None, shift=None, residual=None, relu=False, stride=1, pad=0, x3=False):
    """Position-major activations: x [H][W][N][Cin] -> [Ho][Wo][N][Cout] (patch-scoring trunk layout).
    x3: split-bf16 products (SSAD_MATH=bf16x3)."""
    h, w, n, cin = x.shape
    cout, kh, kw, cin2 = w_ohwi.shape
    assert cin == cin2
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    out = _new((ho, wo, n, cout), x)
    nb = 4.0 * (x.numel() + out.numel() * (2 if residual is not None else 1) + w_ohwi.numel())
    if x3:                                       # True / 3: bf16x3, 6: bf16x6
        _run("conv_igemm_x6" if x3 == 6 else "conv_igemm_x3", 2.0 * out.numel() * kh * kw * cin, nb,
             lambda: _split_fwd(x3)(_hip.ptr(x), _hip.ptr(w_ohwi), _hip.ptr(out), _hip.ptr(scale, True),
                                    _hip.ptr(shift, True), _hip.ptr(residual, True), int(relu), n, h, w,
                                    cin, cout, kh, kw, stride, pad, 1, _hip.stream()))
        return out
    _run("conv_igemm_pos_f32", 2.0 * out.numel() * kh * kw * cin, nb,          # the position-major instantiations (POS = true)
         lambda: _hip.lib().ssad_conv_igemm_fwd_hwnc(_hip.ptr(x), _hip.ptr(w_ohwi), _hip.ptr(out), _hip.ptr(scale, True),
                                                     _hip.ptr(shift, True), _hip.ptr(residual, True), int(relu), n, h, w,
                                                     cin, cout, kh, kw, stride, pad, _hip.stream()),
         exec_flops=2.0 * n * cout * cin * _inbounds_taps(h, w, kh, kw, stride, pad) if PROFILE is not None else None,
         tile=lambda: igemm_tile_name(n, h, w, cin, cout, kh, kw, stride, pad, IGEMM_HWNC))
    return out


def conv_fwd_hwnc_ring(x, w_ohwi, scale, shift, residual, relu, skip_lo, skip_hi):
    """3x3 / stride 1 / pad 1 conv over position-major activations, ONLY the output positions outside the square
    skip_lo <= oy, ox <= skip_hi (the others are left for patch_gather_hwnc).  x [H][W][N][Cin] -> [H][W][N][Cout]."""
    h, w, n, cin = x.shape
    cout, kh, kw, cin2 = w_ohwi.shape
    assert cin == cin2 and (kh, kw) == (3, 3) and 0 <= skip_lo <= skip_hi < min(h, w)
    out = _new((h, w, n, cout), x)
    side = skip_hi - skip_lo + 1
    ring = h * w - side * side
    taps = _inbounds_taps(h, w, 3, 3, 1, 1) - 9 * side * side if PROFILE is not None else 0       # the skipped square has all nine taps
    _run("conv_igemm_pos_f32", 2.0 * n * ring * cout * 9 * cin, 4.0 * (x.numel() + n * ring * cout * (2 if residual is not None else 1) + w_ohwi.numel()),
         lambda: _hip.lib().ssad_conv_igemm_fwd_hwnc_ring(_hip.ptr(x), _hip.ptr(w_ohwi), _hip.ptr(out), _hip.ptr(scale, True),
                                                          _hip.ptr(shift, True), _hip.ptr(residual, True), int(relu), n, h, w,
                                                          cin, cout, 3, 3, 1, 1, skip_lo, skip_hi, _hip.stream()),
         exec_flops=2.0 * n * cout * cin * taps if PROFILE is not None else None,
         tile=lambda: igemm_tile_name(n, h, w, cin, cout, 3, 3, 1, 1, IGEMM_RING))
    return out


def patch_gather_hwnc(dense, out, prow, pcol, shift, lo, hi, ilo=1, ihi=0):
    """out[u][v][n][:] = dense[b][shift * pr + u][shift * pc + v][:] for lo <= u, v <= hi (n = (b * prow + pr) * pcol + pc): the
    positions of every patch's map that equal the per-image dense map.  dense NHWC [B][Hd][Wd][C], out [H][W][N][C], in place.
    ilo <= ihi: the inner square ilo <= u, v <= ihi is left untouched (nobody reads it)."""
    b, hd, wd, c = dense.shape
    h, w, n, c2 = out.shape
    assert c == c2 and n == b * prow * pcol
    side, iside = hi - lo + 1, max(ihi - ilo + 1, 0)
    _run("patch_gather", 0.0, 8.0 * n * (side * side - iside * iside) * c,
         lambda: _hip.lib().ssad_patch_gather_hwnc_band(_hip.ptr(dense), _hip.ptr(out), b, prow, pcol, shift, hd, wd, c, h, w, lo, hi,
                                                        ilo, ihi, _hip.stream()))
    return out


def conv_fwd(x, w_ohwi, scale=None, shift=None, residual=None, relu=False, stride=1, pad=0, bf16=False):
    """x NHWC [N][H][W][Cin]; w OHWI [Cout][KH][KW][Cin] -> NHWC [N][Ho][Wo][Cout].
    bf16=True: operands rounded to bf16 in the loader (fp32 storage / accumulate), the Trainer(precision=16) path;
    bf16=3: split-bf16 products (hi*hi + hi*lo + lo*hi), fp32-class accuracy from the bf16 matrix cores."""
    n, h, w, cin = x.shape
    cout, kh, kw, cin2 = w_ohwi.shape
    assert cin == cin2
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    out = _new((n, ho, wo, cout), x)
    nb = 4.0 * (x.numel() + out.numel() * (2 if residual is not None else 1) + w_ohwi.numel())
    if bf16 in (3, 6):
        _run("conv_igemm_x6" if bf16 == 6 else "conv_igemm_x3", 2.0 * out.numel() * kh * kw * cin, nb,
             lambda: _split_fwd(bf16)(_hip.ptr(x), _hip.ptr(w_ohwi), _hip.ptr(out), _hip.ptr(scale, True),
                                      _hip.ptr(shift, True), _hip.ptr(residual, True), int(relu), n, h, w,
                                      cin, cout, kh, kw, stride, pad, 0, _hip.stream()))
        return out
    fn = (_hip.lib().ssad_conv_igemm_fwd_f16 if bf16 == 2 else _hip.lib().ssad_conv_igemm_fwd_bf16 if bf16 else
          _hip.lib().ssad_conv_igemm_fwd)
    _run(_kname("conv_igemm", bf16), 2.0 * out.numel() * kh * kw * cin, nb,
         lambda: fn(_hip.ptr(x), _hip.ptr(w_ohwi), _hip.ptr(out), _hip.ptr(scale, True), _hip.ptr(shift, True),
                    _hip.ptr(residual, True), int(relu), n, h, w, cin, cout, kh, kw, stride, pad, _hip.stream()),
         tile=None if bf16 else (lambda: igemm_tile_name(n, h, w, cin, cout, kh, kw, stride, pad, 0)))
    return out


def conv_fwd_stats(x, w_ohwi, eps, momentum, running_mean, running_var, stride=1, pad=0, bf16=False):
    """Bias-free conv + the train-mode BatchNorm statistics of its output in one pass.  Returns (z, mean, invstd)."""
    n, h, w, cin = x.shape
    cout, kh, kw, cin2 = w_ohwi.shape
    assert cin == cin2
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    mean, invstd = _new((cout,), x), _new((cout,), x)
    lib = _hip.lib()
    ws = torch.empty(lib.ssad_conv_stats_workspace(n, ho, wo, cout), device=x.device, dtype=torch.float64)
    if _is_h(x):                 # precision-16 step with half tensors: x, the weights and z are halves
        assert _is_h(w_ohwi) and bf16 == 2
        out = _newh((n, ho, wo, cout), x)
        _run("conv_igemm_h16", 2.0 * out.numel() * kh * kw * cin, 2.0 * (x.numel() + out.numel() + w_ohwi.numel()),
             lambda: lib.ssad_conv_igemm_fwd_stats_h(x.data_ptr(), w_ohwi.data_ptr(), out.data_ptr(), n, h, w, cin, cout, kh, kw,
                                                     stride, pad, eps, momentum, _hip.ptr(mean), _hip.ptr(invstd),
                                                     _hip.ptr(running_mean, True), _hip.ptr(running_var, True), ws.data_ptr(),
                                                     _hip.stream()))
        return out, mean, invstd
    out = _new((n, ho, wo, cout), x)
    nb = 4.0 * (x.numel() + out.numel() + w_ohwi.numel())
    _run(_kname("conv_igemm", bf16), 2.0 * out.numel() * kh * kw * cin, nb,
         lambda: lib.ssad_conv_igemm_fwd_stats(_hip.ptr(x), _hip.ptr(w_ohwi), _hip.ptr(out), n, h, w, cin, cout, kh, kw,
                                               stride, pad, int(bf16), eps, momentum, _hip.ptr(mean), _hip.ptr(invstd),
                                               _hip.ptr(running_mean, True), _hip.ptr(running_var, True), ws.data_ptr(),
                                               _hip.stream()),
         tile=None if bf16 else (lambda: igemm_tile_name(n, h, w, cin, cout, kh, kw, stride, pad, IGEMM_STATS)))
    return out, mean, invstd


def conv3x3_c64(x, w_ohwi, residual=None, transform=None, emit=False, stats=None, res_mask=None, bf16=0):
    """Halo-tile 3x3 / stride 1 / pad 1 convolution, 64 -> 64 channels (layer1 forward and input-gradient convs).
    x NHWC [N][H][W][64], w OHWI [64][3][3][64].  transform = (mean, invstd, gamma, beta): the input is taken through
    relu(bn(x)) while it is staged (emit=True also returns that activation).  stats = (eps, momentum, running_mean,
    running_var): also the train-mode BatchNorm statistics of the output.  Returns out[, emitted][, mean, invstd]."""
    n, h, w, c = x.shape
    assert c == 64 and tuple(w_ohwi.shape) == (64, 3, 3, 64)
    lib = _hip.lib()
    half = _is_h(x)
    assert residual is None or tuple(residual.shape) == (n, h, w, 64), "residual must have the output's shape"
    out = _newh((n, h, w, 64), x) if half else _new((n, h, w, 64), x)
    em = torch.empty_like(x) if emit else None
    tr = transform if transform is not None else (None, None, None, None)
    mean = invstd = ws = None
    eps = mom = 0.0
    rm = rv = None
    if stats is not None:
        eps, mom, rm, rv = stats
        mean, invstd = _new((64,), x), _new((64,), x)
        ws = torch.empty(lib.ssad_conv3x3_c64_stats_rows(n, h, w) * 128, device=x.device, dtype=torch.float64)
    nb = 4.0 * (x.numel() + out.numel() * (2 if residual is not None else 1) + (out.numel() if emit else 0) + w_ohwi.numel())
    op = int(bf16)
    assert op in (0, 1, 2), "conv3x3_c64: exact fp32, or bf16 (1) / fp16 (2) operands"
    if half:
        assert op == 2 and res_mask is None and (residual is None or _is_h(residual))
        _run("conv_c64_h16", 2.0 * out.numel() * 9 * 64, nb / 2 + 2.0 * w_ohwi.numel(),
             lambda: lib.ssad_conv3x3_c64_h(x.data_ptr(), _hip.ptr(w_ohwi), out.data_ptr(), _p(residual, True), _hip.ptr(tr[0], True),
                                            _hip.ptr(tr[1], True), _hip.ptr(tr[2], True), _hip.ptr(tr[3], True), _p(em, True),
                                            n, h, w, ws.data_ptr() if ws is not None else None, eps, mom, _hip.ptr(mean, True),
                                            _hip.ptr(invstd, True), _hip.ptr(rm, True), _hip.ptr(rv, True), _hip.stream()))
    else:
        _run(_kname("conv_c64", op), 2.0 * out.numel() * 9 * 64, nb,
             lambda: lib.ssad_conv3x3_c64_op(_hip.ptr(x), _hip.ptr(w_ohwi), _hip.ptr(out), _hip.ptr(residual, True),
                                             res_mask.data_ptr() if res_mask is not None else None, _hip.ptr(tr[0], True),
                                             _hip.ptr(tr[1], True), _hip.ptr(tr[2], True), _hip.ptr(tr[3], True), _hip.ptr(em, True),
                                             n, h, w, ws.data_ptr() if ws is not None else None, eps, mom, _hip.ptr(mean, True),
                                             _hip.ptr(invstd, True), _hip.ptr(rm, True), _hip.ptr(rv, True), op, _hip.stream()))
    res = [out]
    if emit:
        res.append(em)
    if stats is not None:
        res += [mean, invstd]
    return res[0] if len(res) == 1 else tuple(res)


def conv3x3_h(x, w_ohwi, residual=None, transform=None, emit=False, stats=None):
    """3x3 / stride 1 / pad 1 convolution over half tensors (csrc/conv16.hip): x NHWC [N][H][W][Cin] halves, w OHWI halves
    [Cout][3][3][Cin] -> [N][H][W][Cout] halves (+ residual).  transform = (mean, invstd, gamma, beta) of the PRODUCING layer: x is
    taken through relu(bn(x)) while it is staged (emit=True also returns that activation, for the weight gradient).  stats = (eps,
    momentum, running_mean, running_var): also the train-mode BatchNorm statistics of the stored output.
    Returns out[, emitted][, mean, invstd]."""
    n, h, w, cin = x.shape
    cout = w_ohwi.shape[0]
    assert _is_h(x) and _is_h(w_ohwi) and tuple(w_ohwi.shape) == (cout, 3, 3, cin)
    assert residual is None or (_is_h(residual) and tuple(residual.shape) == (n, h, w, cout)), "residual must have the output's shape"
    lib = _hip.lib()
    out = _newh((n, h, w, cout), x)
    em = torch.empty_like(x) if emit else None
    tr = transform if transform is not None else (None, None, None, None)
    mean = invstd = ws = None
    eps = mom = 0.0
    rm = rv = None
    if stats is not None:
        eps, mom, rm, rv = stats
        mean, invstd = _new((cout,), x), _new((cout,), x)
        ws = torch.empty(lib.ssad_conv3x3_h_stats_rows(n, h, w, cout) * 2 * cout, device=x.device, dtype=torch.float64)
    nb = 2.0 * (x.numel() + out.numel() * (2 if residual is not None else 1) + (x.numel() if emit else 0) + w_ohwi.numel())
    _run("conv3x3_h16", 2.0 * out.numel() * 9 * cin, nb,
         lambda: lib.ssad_conv3x3_h(x.data_ptr(), w_ohwi.data_ptr(), out.data_ptr(), _p(residual, True), _hip.ptr(tr[0], True),
                                    _hip.ptr(tr[1], True), _hip.ptr(tr[2], True), _hip.ptr(tr[3], True), _p(em, True), n, h, w, cin, cout,
                                    ws.data_ptr() if ws is not None else None, eps, mom, _hip.ptr(mean, True), _hip.ptr(invstd, True),
                                    _hip.ptr(rm, True), _hip.ptr(rv, True), _hip.stream()))
    res = [out]
    if emit:
        res.append(em)
    if stats is not None:
        res += [mean, invstd]
    return res[0] if len(res) == 1 else tuple(res)


def conv3x3_hw_ok(n, h, w, cin, cout, f32=False):
    """Whether ssad_conv3x3_hw / _fw (csrc/conv16w.hip: register-fed filters, 128 x 64 wave tiles) takes a launch of this shape."""
    lib = _hip.lib()
    return bool((lib.ssad_conv3x3_fw_ok if f32 else lib.ssad_conv3x3_hw_ok)(n, h, w, cin, cout))


def conv3x3_hw_pack(src_f32, entries, out=None, f32=False):
    """Packs 3x3 filters for conv3x3_hw in ONE launch.  src_f32: a flat fp32 tensor holding OHWI filters; entries: iterable of
    (source offset in floats, Cout, Cin of the conv that will run on the packed filter, flip) -- flip: the source is the OHWI filter
    [Cin][3][3][Cout] of the forward conv whose input gradient this is.  f32: the pack of the exact-fp32 form (floats).
    Returns (flat tensor, [offset of each packed filter])."""
    import ctypes
    desc, offs, off = [], [], 0
    for (so, o, i, flip) in entries:
        desc += [int(so), off, int(o), int(i), int(bool(flip))]
        offs.append(off)
        off += o * 9 * i
    dt = torch.float32 if f32 else torch.float16
    if out is None:
        out = torch.empty(off, device=src_f32.device, dtype=dt)
    assert out.numel() >= off and out.dtype == dt and src_f32.dtype == torch.float32 and src_f32.is_contiguous()
    arr = (ctypes.c_int64 * len(desc))(*desc)
    lib = _hip.lib()
    _hip.check((lib.ssad_conv3x3_fw_pack_batch if f32 else lib.ssad_conv3x3_hw_pack_batch)(_hip.ptr(src_f32), out.data_ptr(), arr, len(offs),
                                                                                            _hip.stream()))
    return out, offs


def conv3x3_hw(x, w_packed, cout, residual=None, transform=None, emit=False, stats=None, res_mask=None):
    """conv3x3_h with the filter packed by conv3x3_hw_pack (a flat tensor of cout * 9 * cin values); half tensors, or -- x fp32 -- the
    exact-fp32 instantiation (res_mask: the residual is gated by the nibble mask of bn_apply_fwd_mask).  The launch must satisfy
    conv3x3_hw_ok.  Returns out[, emitted][, mean, invstd]."""
    n, h, w, cin = x.shape
    f32 = x.dtype == torch.float32
    assert (f32 or _is_h(x)) and w_packed.dtype == x.dtype and w_packed.numel() == cout * 9 * cin and w_packed.is_contiguous()
    assert x.is_contiguous() and conv3x3_hw_ok(n, h, w, cin, cout, f32), "shape outside ssad_conv3x3_hw_ok"
    assert residual is None or (residual.dtype == x.dtype and tuple(residual.shape) == (n, h, w, cout) and residual.is_contiguous()), \
        "residual must have the output's shape"
    assert res_mask is None or (residual is not None and res_mask.numel() == n * h * w * cout // 4 and res_mask.dtype == torch.uint8)
    lib = _hip.lib()
    out = torch.empty((n, h, w, cout), device=x.device, dtype=x.dtype)
    em = torch.empty_like(x) if emit else None
    tr = transform if transform is not None else (None, None, None, None)
    mean = invstd = ws = None
    eps = mom = 0.0
    rm = rv = None
    if stats is not None:
        eps, mom, rm, rv = stats
        mean, invstd = _new((cout,), x), _new((cout,), x)
        ws = torch.empty(lib.ssad_conv3x3_hw_stats_rows(n, h, w, cout) * 2 * cout, device=x.device, dtype=torch.float64)
    nb = x.element_size() * (x.numel() + out.numel() * (2 if residual is not None else 1) + (x.numel() if emit else 0) + w_packed.numel())
    wsp = ws.data_ptr() if ws is not None else None
    if f32:
        _run("conv3x3_fw32", 2.0 * out.numel() * 9 * cin, float(nb),
             lambda: lib.ssad_conv3x3_fw(x.data_ptr(), w_packed.data_ptr(), out.data_ptr(), _p(residual, True),
                                         res_mask.data_ptr() if res_mask is not None else None, _hip.ptr(tr[0], True), _hip.ptr(tr[1], True),
                                         _hip.ptr(tr[2], True), _hip.ptr(tr[3], True), _p(em, True), n, h, w, cin, cout, wsp, eps, mom,
                                         _hip.ptr(mean, True), _hip.ptr(invstd, True), _hip.ptr(rm, True), _hip.ptr(rv, True), _hip.stream()))
    else:
        _run("conv3x3_hw16", 2.0 * out.numel() * 9 * cin, float(nb),
             lambda: lib.ssad_conv3x3_hw(x.data_ptr(), w_packed.data_ptr(), out.data_ptr(), _p(residual, True),
                                         res_mask.data_ptr() if res_mask is not None else None, _hip.ptr(tr[0], True),
                                         _hip.ptr(tr[1], True), _hip.ptr(tr[2], True), _hip.ptr(tr[3], True), _p(em, True), n, h, w, cin, cout,
                                         wsp, eps, mom, _hip.ptr(mean, True), _hip.ptr(invstd, True), _hip.ptr(rm, True), _hip.ptr(rv, True),
                                         _hip.stream()))
    res = [out]
    if emit:
        res.append(em)
    if stats is not None:
        res += [mean, invstd]
    return res[0] if len(res) == 1 else tuple(res)


# Launch geometry of the 3x3 / stride 1 kernels (ssad_conv3x3_geometry, include/ssad.h): what the launchers themselves compute
CONV3X3_C64, CONV3X3_H, CONV3X3_W = 0, 1, 2
CONV3X3_GEOMETRY_FIELDS = ("inst", "ntiles", "gx", "gy", "chunks", "last", "walk", "per")


def conv3x3_geometry(path, n, h, w, cin, cout, f32=False):
    """The launch of ssad_conv3x3_c64* (CONV3X3_C64), ssad_conv3x3_h (CONV3X3_H) or ssad_conv3x3_hw / _fw / _fw_eval (CONV3X3_W, f32 for
    the float form) on n maps of h x w: a dict of the instantiation id, ntiles, gx, gy, input chunks per tile, maps present in the last
    tile, the most tiles one workgroup walks and the maps per tile -- or None where the entry point refuses the shape.  No GPU needed."""
    import ctypes
    out = (ctypes.c_int64 * 8)()
    if _hip.lib().ssad_conv3x3_geometry(int(path), n, h, w, cin, cout, int(bool(f32)), out):
        return None
    return dict(zip(CONV3X3_GEOMETRY_FIELDS, (int(v) for v in out)))


def conv3x3_fw_eval_ok(n, h, w, cin, cout):
    return bool(_hip.lib().ssad_conv3x3_fw_eval_ok(n, h, w, cin, cout))


def conv3x3_fw_pack_scaled(w_ohwi, scale):
    """The filter of an inference conv in the register-fed kernel's fragment order, the folded BatchNorm's scale multiplied in."""
    cout, kh, kw, cin = w_ohwi.shape
    assert (kh, kw) == (3, 3) and w_ohwi.is_contiguous() and (scale is None or scale.numel() == cout)
    out = torch.empty(cout * 9 * cin, device=w_ohwi.device, dtype=torch.float32)
    _hip.check(_hip.lib().ssad_conv3x3_fw_pack_scaled(_hip.ptr(w_ohwi), _hip.ptr(scale, True), _hip.ptr(out), cout, cin, _hip.stream()))
    return out


def conv3x3_fw_eval(x, w_packed, cout, shift, residual=None, relu=False, out_hwnc=False):
    """Inference 3x3 / stride 1 conv on the register-fed kernel (csrc/conv16w.hip, T = float): act(conv(x) + shift (+ residual)), x and
    residual NHWC, the output NHWC or position-major [H][W][N][C]; the filter from conv3x3_fw_pack_scaled."""
    n, h, w, cin = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and w_packed.numel() == cout * 9 * cin and shift.numel() == cout
    assert residual is None or (tuple(residual.shape) == (n, h, w, cout) and residual.is_contiguous())
    out = _new((h, w, n, cout) if out_hwnc else (n, h, w, cout), x)
    nb = 4.0 * (x.numel() + out.numel() * (2 if residual is not None else 1) + w_packed.numel())
    _run("conv3x3_fw32", 2.0 * out.numel() * 9 * cin, nb,
         lambda: _hip.lib().ssad_conv3x3_fw_eval(_hip.ptr(x), _hip.ptr(w_packed), _hip.ptr(out), _hip.ptr(shift), _hip.ptr(residual, True),
                                                 int(relu), n, h, w, cin, cout, int(out_hwnc), _hip.stream()))
    return out


def conv3x3_c64_eval(x, w_ohwi, scale=None, shift=None, residual=None, relu=False, in_hwnc=False, out_hwnc=False,
                     res_hwnc=None):
    """Halo-tile 3x3 / stride 1 / pad 1 convolution 64 -> 64 with the inference epilogue act(conv * scale + shift + residual).
    x is NHWC [N][H][W][64] or, with in_hwnc, position-major [H][W][N][64]; the output likewise under out_hwnc and the
    residual under res_hwnc (default: the output's layout)."""
    res_hwnc = out_hwnc if res_hwnc is None else res_hwnc
    if in_hwnc:
        h, w, n, c = x.shape
    else:
        n, h, w, c = x.shape
    assert c == 64 and tuple(w_ohwi.shape) == (64, 3, 3, 64)
    out = _new((h, w, n, 64) if out_hwnc else (n, h, w, 64), x)
    assert residual is None or tuple(residual.shape) == ((h, w, n, 64) if res_hwnc else (n, h, w, 64))
    nb = 4.0 * (x.numel() + out.numel() * (2 if residual is not None else 1) + w_ohwi.numel())
    _run("conv_c64_f32", 2.0 * out.numel() * 9 * 64, nb,
         lambda: _hip.lib().ssad_conv3x3_c64_eval(_hip.ptr(x), _hip.ptr(w_ohwi), _hip.ptr(out), _hip.ptr(scale, True),
                                                  _hip.ptr(shift, True), _hip.ptr(residual, True), int(relu), n, h, w,
                                                  int(in_hwnc), int(out_hwnc), int(res_hwnc), _hip.stream()))
    return out


def linear_fwd(x, w, scale=None, shift=None, relu=False, x3=False):
    """x [N][Cin], w [Cout][Cin] -> [N][Cout] (the same MFMA kernel with H=W=KH=KW=1)."""
    n, cin = x.shape
    cout = w.shape[0]
    out = _new((n, cout), x)
    if x3 and cout % 4 == 0:
        _run("conv_igemm_x6" if x3 == 6 else "conv_igemm_x3", 2.0 * n * cin * cout, 4.0 * (x.numel() + out.numel() + w.numel()),
             lambda: _split_fwd(x3)(_hip.ptr(x), _hip.ptr(w), _hip.ptr(out), _hip.ptr(scale, True),
                                    _hip.ptr(shift, True), None, int(relu), n, 1, 1, cin, cout, 1, 1, 1,
                                    0, 0, _hip.stream()))
        return out
    _run("conv_igemm_f32", 2.0 * n * cin * cout, 4.0 * (x.numel() + out.numel() + w.numel()),
         lambda: _hip.lib().ssad_conv_igemm_fwd(_hip.ptr(x), _hip.ptr(w), _hip.ptr(out), _hip.ptr(scale, True),
                                                _hip.ptr(shift, True), None, int(relu), n, 1, 1, cin, cout, 1, 1, 1, 0,
                                                _hip.stream()),
         tile=lambda: igemm_tile_name(n, 1, 1, cin, cout, 1, 1, 1, 0, 0))
    return out


def gap_fwd(x, out, offset, hwnc=False):
    if hwnc:
        h, w, n, c = x.shape
    else:
        n, h, w, c = x.shape
    if _is_h(x):
        assert not hwnc
        _run_aside("gap_h16", 0.0, 2.0 * x.numel() + 4.0 * n * c,
                   lambda: _hip.lib().ssad_gap_fwd_h(x.data_ptr(), _hip.ptr(out), n, h * w, c, out.shape[1], offset, _hip.stream()), keep=(x,))
        return out
    _run_aside("gap", 0.0, 4.0 * (x.numel() + n * c),
               lambda: _hip.lib().ssad_gap_fwd(_hip.ptr(x), _hip.ptr(out), n, h * w, c, out.shape[1], offset, int(hwnc),
                                               _hip.stream()), keep=(x,))
    return out


def l2_normalize_rows(x):
    out = torch.empty_like(x)
    _run("l2norm_rows", 0.0, 8.0 * x.numel(),
         lambda: _hip.lib().ssad_l2_normalize_rows(_hip.ptr(x), _hip.ptr(out), x.shape[0], x.shape[1], _hip.stream()))
    return out


def cosine_knn_mean(sim, k=3):
    out = _new((sim.shape[0],), sim)
    _run("knn_mean", 0.0, 4.0 * sim.numel(),
         lambda: _hip.lib().ssad_cosine_knn_mean(_hip.ptr(sim), _hip.ptr(out), sim.shape[0], sim.shape[1], k, _hip.stream()))
    return out


KNN_SPLIT_TARGET_WG = 3072  # workgroups a split launch aims at: 12 per CU of an MI355X (256 CUs), 6 rounds of the 2 resident
KNN_SPLIT_MIN_ROWS = 4096   # bank rows a split keeps at the least


def knn_splits(n, r):
    """Bank splits S of cosine_knn_fused for n queries against r bank rows: 1 -- the one-launch kernel -- when the 128-query tiles
    alone reach KNN_SPLIT_TARGET_WG workgroups or the bank has fewer than 2 x KNN_SPLIT_MIN_ROWS rows; else enough splits to reach
    that many workgroups, each split keeping at least KNN_SPLIT_MIN_ROWS rows.  Tuned with tools/knn_split_probe.py: a
    launch of few workgroups leaves CUs idle, and one of about 2 per CU leaves a half-empty last round.  The 588-row bank of the
    reference path and the million-query WideResNet-50 scales stay at 1.  SSAD_KNN_SPLIT=0 forces 1 (A/B runs)."""
    if os.environ.get("SSAD_KNN_SPLIT", "1") == "0":
        return 1
    tiles = -(-int(n) // 128)
    if tiles >= KNN_SPLIT_TARGET_WG:
        return 1
    return max(1, min(-(-KNN_SPLIT_TARGET_WG // tiles), int(r) // KNN_SPLIT_MIN_ROWS))


def cosine_knn_split(x, bank_n, k=3, splits=1):
    """cosine_knn_fused with the bank split S = `splits` ways (csrc/knn.hip ssad_cosine_knn_split): two launches, a [S][N][3]
    workspace; bit-identical to the one-launch kernel for every S."""
    n, d = x.shape
    r = bank_n.shape[0]
    out = _new((n,), x)
    part = _new((int(splits), n, 3), x)
    _run("knn_split", 2.0 * n * d * r, 4.0 * (x.numel() + bank_n.numel() + n + 6 * part.numel()),
         lambda: _hip.lib().ssad_cosine_knn_split(_hip.ptr(x), _hip.ptr(bank_n), _hip.ptr(part), _hip.ptr(out), n, d, r, k,
                                                  int(splits), _hip.stream()))
    return out


CORESET_MAX_WGS = 1024    # workgroups of a coreset step: 4 per CU of an MI355X (256 CUs), all resident in one round
CORESET_ROWS_PER_WG = 128  # rows a workgroup keeps at the least (one pass of the kernel's 128-row tile)


def coreset_workgroups(r):
    """Default workgroup count of coreset_greedy for r rows: enough workgroups of >= CORESET_ROWS_PER_WG rows, at most
    CORESET_MAX_WGS.  The selection is the same bits for every count."""
    return max(1, min(CORESET_MAX_WGS, -(-int(r) // CORESET_ROWS_PER_WG)))


def coreset_greedy(p, m, start=0, wgs=None):
    """Greedy k-center (farthest-point) selection over the rows of p [R][d] (csrc/coreset.hip ssad_coreset_greedy): sel[0] = start,
    sel[t] = the row farthest (squared Euclidean distance) from its nearest earlier centre, ties to the smallest row; rad[t] = that
    distance (rad[0] = inf).  Stops early when every row lies on a centre.  Returns (sel int64 [m'], rad float32 [m']), m' <= min(m, R),
    on p's device; one launch per step, one host sync at the end.  `wgs`: workgroup count (default coreset_workgroups(R))."""
    r, d = p.shape
    m, start = int(m), int(start)
    if m < 1:
        raise ValueError(f"coreset_greedy: m must be >= 1, got {m}")
    if not 0 <= start < r:
        raise ValueError(f"coreset_greedy: start {start} is not a row of the {r} rows")
    g = coreset_workgroups(r) if wgs is None else int(wgs)
    steps = min(m, r)
    mind = _new((r,), p)
    part = torch.empty((2, g), device=p.device, dtype=torch.int64)      # (float value, int32 row) pairs
    sel = torch.empty((steps,), device=p.device, dtype=torch.int64)
    rad = _new((steps,), p)
    m_out = torch.zeros((1,), device=p.device, dtype=torch.int32)
    _run("coreset_greedy", 3.0 * steps * r * d, 4.0 * steps * r * d,
         lambda: _hip.lib().ssad_coreset_greedy(_hip.ptr(p), r, d, m, start, g, _hip.ptr(mind), _hip.ptr(part, dtype=torch.int64),
                                                _hip.ptr(sel, dtype=torch.int64), _hip.ptr(rad), _hip.ptr(m_out, dtype=torch.int32),
                                                _hip.stream()))
    n = int(m_out.item())
    return sel[:n], rad[:n]


def cosine_knn_fused(x, bank_n, k=3):
    """x [N][D] (not normalised), bank_n [R][D] L2-normalised -> [N] mean of the k smallest cosine distances, one kernel; split over
    the bank rows (cosine_knn_split, same bits) when few queries meet a large bank (knn_splits)."""
    n, d = x.shape
    r = bank_n.shape[0]
    s = knn_splits(n, r)
    if s > 1:
        return cosine_knn_split(x, bank_n, k, s)
    out = _new((n,), x)
    _run("knn_fused", 2.0 * n * d * r, 4.0 * (x.numel() + bank_n.numel() + n),
         lambda: _hip.lib().ssad_cosine_knn_fused(_hip.ptr(x), _hip.ptr(bank_n), _hip.ptr(out), n, d, r, k, _hip.stream()))
    return out


def cosine_knn_index(x, bank_n, k=3, splits=None):
    """kneighbors of the cosine bank: x [N][D] (not normalised), bank_n [R][D] L2-normalised -> (dist [N][k] float32, idx [N][k]
    int32), the k (1..3) smallest (distance, bank row) pairs of every query, ascending, equal distances to the smaller row
    (csrc/knn.hip ssad_cosine_knn_index).  The distances are the bits cosine_knn_fused averages.  `splits`: None = the knn_splits
    rule of cosine_knn_fused; S >= 1 = that many bank splits (1: one launch); same bits for every S."""
    n, d = x.shape
    r = bank_n.shape[0]
    k = int(k)
    if not 1 <= k <= 3:
        raise ValueError(f"cosine_knn_index: k must be 1, 2 or 3, got {k}")
    if r < k:
        raise ValueError(f"cosine_knn_index: the bank has {r} rows, fewer than k = {k}")
    s = knn_splits(n, r) if splits is None else int(splits)
    if s < 1:
        raise ValueError(f"cosine_knn_index: splits must be >= 1, got {s}")
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    part = torch.empty((s, n, 3), device=x.device, dtype=torch.int64) if s > 1 else None     # (distance bits << 32 | row) keys
    _run("knn_index", 2.0 * n * d * r, 4.0 * (x.numel() + bank_n.numel() + 2 * n * k) + 16.0 * (s > 1) * s * n * 3,
         lambda: _hip.lib().ssad_cosine_knn_index(_hip.ptr(x), _hip.ptr(bank_n), _hip.ptr(part, True, torch.int64), _hip.ptr(dist),
                                                  _hip.ptr(idx, dtype=torch.int32), n, d, r, k, s, _hip.stream()))
    return dist, idx


ROWS_SMALLEST_COLS_PER_WG = 4096   # columns a workgroup of rows_smallest_index scans at the least (16 per thread and round)
ROWS_SMALLEST_MAX_KEYS = 4096      # keys the merge workgroup of a row takes: wgs * b stays below


def rows_smallest_workgroups(r, b):
    """Default workgroups per row of rows_smallest_index for r columns: one per ROWS_SMALLEST_COLS_PER_WG columns, at most
    ROWS_SMALLEST_MAX_KEYS // b.  The result is the same for every count."""
    return max(1, min(ROWS_SMALLEST_MAX_KEYS // int(b), -(-int(r) // ROWS_SMALLEST_COLS_PER_WG)))


def rows_smallest_index(m, b, cosine=False, wgs=None):
    """The min(b, R) smallest (value, column) pairs of each row of m [Q][R], ascending, lexicographic -- the first entries of a
    stable argsort (csrc/image_score.hip ssad_rows_smallest_index): (vals [Q][b'] float32, cols [Q][b'] int32).  cosine: m holds
    similarities and the values are the cosine distances clip(1 - m, 0, 2).  b in 1..32; `wgs`: workgroups per row (default
    rows_smallest_workgroups), 1 .. 4096 // b -- the same result for every count."""
    q, r = m.shape
    b = int(b)
    if not 1 <= b <= 32:
        raise ValueError(f"rows_smallest_index: b must lie in 1..32, got {b}")
    g = rows_smallest_workgroups(r, b) if wgs is None else int(wgs)
    if not 1 <= g <= ROWS_SMALLEST_MAX_KEYS // b:
        raise ValueError(f"rows_smallest_index: wgs must lie in 1..{ROWS_SMALLEST_MAX_KEYS // b} for b = {b}, got {g}")
    bp = min(b, r)
    vals = _new((q, bp), m)
    cols = torch.empty((q, bp), device=m.device, dtype=torch.int32)
    part = torch.empty((q, g, b), device=m.device, dtype=torch.int64)
    _run("rows_smallest", 0.0, 4.0 * b * m.numel() + 16.0 * part.numel(),
         lambda: _hip.lib().ssad_rows_smallest_index(_hip.ptr(m), q, r, b, int(bool(cosine)), g, _hip.ptr(part, dtype=torch.int64),
                                                     _hip.ptr(vals), _hip.ptr(cols, dtype=torch.int32), _hip.stream()))
    return vals, cols


def rows_argmax(s):
    """s [Q][P] -> (val [Q] float32: the largest entry of each row, flat [Q] int64: q P + its column, the smallest column among equal
    entries) -- csrc/image_score.hip ssad_rows_argmax."""
    q, p = s.shape
    val = _new((q,), s)
    flat = torch.empty((q,), device=s.device, dtype=torch.int64)
    _run("rows_argmax", 0.0, 4.0 * s.numel(),
         lambda: _hip.lib().ssad_rows_argmax(_hip.ptr(s), q, p, _hip.ptr(val), _hip.ptr(flat, dtype=torch.int64), _hip.stream()))
    return val, flat


def knn_reweight(xs, bank_n, mstar, nbr, smax):
    """PatchCore's image-score weight on cosine distances (csrc/image_score.hip ssad_knn_reweight): xs [Q][D] (not normalised),
    bank_n [R][D] L2-normalised, mstar [Q] / [Q][1] int32 nearest bank rows, nbr [Q][b'] int32 neighbourhood rows, smax [Q] ->
    [Q]: (1 - exp(d(x, mstar)) / sum_j exp(d(x, nbr_j))) smax."""
    q, d = xs.shape
    r = bank_n.shape[0]
    bp = nbr.shape[1]
    out = _new((q,), xs)
    i32 = torch.int32
    _run("knn_reweight", 2.0 * q * d * (bp + 1), 4.0 * q * d * (bp + 2),
         lambda: _hip.lib().ssad_knn_reweight(_hip.ptr(xs), _hip.ptr(bank_n), _hip.ptr(mstar, dtype=i32), _hip.ptr(nbr, dtype=i32),
                                              _hip.ptr(smax), _hip.ptr(out), q, d, r, bp, _hip.stream()))
    return out


def row_sqnorms(x):
    """x [N][D] -> [N] fp32 sum of squares of every row (csrc/knn_l2.hip ssad_row_sqnorms): one fixed summation order, equal rows give
    equal bits wherever they stand."""
    n, d = x.shape
    out = _new((n,), x)
    _run("row_sqnorms", 2.0 * n * d, 4.0 * (x.numel() + n),
         lambda: _hip.lib().ssad_row_sqnorms(_hip.ptr(x), _hip.ptr(out), n, d, _hip.stream()))
    return out


def _check_l2_width(name, d):
    if d % 32 or d > 65536:
        raise ValueError(f"{name}: the Euclidean kernels need a width that is a multiple of 32 (at most 65536), got {d}")


# bank dtype of a flat Euclidean search -> (dtype of bank_sq, what the two hold and the op that makes them)
_L2_BANKS = {torch.float32: (torch.float32, "float32 rows with their [R] float32 squared norms (row_sqnorms)"),
             torch.float16: (torch.float32, "float16 rows with their [R] float32 squared norms (rows_to_half)"),
             torch.int8: (torch.int32, "int8 codes with their [R] int32 squared norms (rows_to_int8)")}


def _l2_flat_args(name, x, bank, bank_sq, k, splits, bank_dtype, k_range=(1, 3)):
    """The argument checks of every flat Euclidean search (fp32, fp16 and int8 banks, k <= 3 and the list kernels), from shapes and
    dtypes alone, so before any launch: the width, the bank of `bank_dtype` with one squared norm per row, k within `k_range` and at
    most the bank's rows, `splits` None (the knn_splits rule) or >= 1.  -> (n, d, r, k, s)."""
    n, d = x.shape
    r = bank.shape[0]
    k = int(k)
    _check_l2_width(name, d)
    sq_dtype, holds = _L2_BANKS[bank_dtype]
    if bank.dtype != bank_dtype or bank.shape[1] != d or bank_sq.dtype != sq_dtype or tuple(bank_sq.shape) != (r,):
        raise ValueError(f"{name}: the bank must be [R][{d}] {holds}, got {bank.dtype} {tuple(bank.shape)} and {bank_sq.dtype} "
                         f"{tuple(bank_sq.shape)}")
    if not k_range[0] <= k <= k_range[1]:
        allowed = "be 1, 2 or 3" if k_range == (1, 3) else f"lie in {k_range[0]}..{k_range[1]} (1..3: the l2_knn / l2h_knn functions)"
        raise ValueError(f"{name}: k must {allowed}, got {k}")
    if r < k:
        raise ValueError(f"{name}: the bank has {r} rows, fewer than k = {k}")
    s = knn_splits(n, r) if splits is None else int(splits)
    if s < 1:
        raise ValueError(f"{name}: splits must be >= 1, got {s}")
    return n, d, r, k, s


def l2_knn_fused(x, bank, bank_sq, k=3, splits=None):
    """x [N][D], bank [R][D] (neither normalised), bank_sq = row_sqnorms(bank) -> [N] mean of the k smallest Euclidean distances
    sqrt(max(|x|^2 + |b|^2 - 2 <x, b>, 0)) (csrc/knn_l2.hip ssad_l2_knn_fused).  `splits`: None = the knn_splits rule; S >= 1 = that
    many bank splits (1: one launch); the same bits for every S."""
    n, d, r, k, s = _l2_flat_args("l2_knn_fused", x, bank, bank_sq, k, splits, torch.float32)
    out = _new((n,), x)
    part = _new((s, n, 3), x) if s > 1 else None
    _run("l2_knn_fused", 2.0 * n * d * r, 4.0 * (x.numel() + bank.numel() + r + n) + 24.0 * (s > 1) * s * n * 3,
         lambda: _hip.lib().ssad_l2_knn_fused(_hip.ptr(x), _hip.ptr(bank), _hip.ptr(bank_sq), _hip.ptr(part, True), _hip.ptr(out), n, d, r,
                                              k, s, _hip.stream()))
    return out


def l2_knn_index(x, bank, bank_sq, k=3, splits=None):
    """kneighbors of the Euclidean bank: (dist [N][k] float32, idx [N][k] int32), the k (1..3) smallest (squared distance, bank row)
    pairs of every query, ascending, equal ones to the smaller row; dist holds the roots -- the bits l2_knn_fused averages
    (csrc/knn_l2.hip ssad_l2_knn_index).  `splits` as in l2_knn_fused."""
    n, d, r, k, s = _l2_flat_args("l2_knn_index", x, bank, bank_sq, k, splits, torch.float32)
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    part = torch.empty((s, n, 3), device=x.device, dtype=torch.int64) if s > 1 else None     # (squared-distance bits << 32 | row) keys
    _run("l2_knn_index", 2.0 * n * d * r, 4.0 * (x.numel() + bank.numel() + r + 2 * n * k) + 16.0 * (s > 1) * s * n * 3,
         lambda: _hip.lib().ssad_l2_knn_index(_hip.ptr(x), _hip.ptr(bank), _hip.ptr(bank_sq), _hip.ptr(part, True, torch.int64),
                                              _hip.ptr(dist), _hip.ptr(idx, dtype=torch.int32), n, d, r, k, s, _hip.stream()))
    return dist, idx


def rows_to_half(x):
    """x [N][D] fp32 -> (xh [N][D] float16, sq [N] float32): every element rounded by h (round to nearest even, saturating at +-65504,
    results below 2^-14 flushed to signed zero) and the squared norms of the ROUNDED rows in row_sqnorms' order, one pass
    (csrc/knn_l2_half.hip ssad_rows_to_half)."""
    n, d = x.shape
    _check_l2_width("rows_to_half", d)
    xh = torch.empty((n, d), device=x.device, dtype=torch.float16)
    sq = _new((n,), x)
    _run("rows_to_half", 2.0 * n * d, 6.0 * x.numel() + 4.0 * n,
         lambda: _hip.lib().ssad_rows_to_half(_hip.ptr(x), _hip.hptr(xh), _hip.ptr(sq), n, d, _hip.stream()))
    return xh, sq


def l2h_knn_fused(x, bank_h, bank_sq, k=3, splits=None):
    """l2_knn_fused with half-precision operands: x [N][D] fp32 queries (rounded here, rows_to_half), (bank_h, bank_sq) =
    rows_to_half(bank) -> [N] mean of the k smallest distances BETWEEN THE ROUNDED ROWS, sqrt(max(|h(x)|^2 + |h(b)|^2 - 2 <h(x), h(b)>,
    0)), on the fp16 matrix cores (csrc/knn_l2_half.hip ssad_l2h_knn_fused).  `splits` as in l2_knn_fused; the same bits for every S."""
    n, d, r, k, s = _l2_flat_args("l2h_knn_fused", x, bank_h, bank_sq, k, splits, torch.float16)
    xh, xsq = rows_to_half(x)
    out = _new((n,), x)
    part = _new((s, n, 3), x) if s > 1 else None
    _run("l2h_knn_fused", 2.0 * n * d * r, 2.0 * (x.numel() + bank_h.numel()) + 4.0 * (r + 2 * n) + 24.0 * (s > 1) * s * n * 3,
         lambda: _hip.lib().ssad_l2h_knn_fused(_hip.hptr(xh), _hip.ptr(xsq), _hip.hptr(bank_h), _hip.ptr(bank_sq), _hip.ptr(part, True),
                                               _hip.ptr(out), n, d, r, k, s, _hip.stream()))
    return out


def l2h_knn_index(x, bank_h, bank_sq, k=3, splits=None):
    """l2_knn_index with half-precision operands (arguments as l2h_knn_fused): (dist [N][k] float32, idx [N][k] int32), the k smallest
    (squared distance, bank row) pairs between the rounded rows, equal ones to the smaller row; dist holds the bits l2h_knn_fused
    averages (csrc/knn_l2_half.hip ssad_l2h_knn_index)."""
    n, d, r, k, s = _l2_flat_args("l2h_knn_index", x, bank_h, bank_sq, k, splits, torch.float16)
    xh, xsq = rows_to_half(x)
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    part = torch.empty((s, n, 3), device=x.device, dtype=torch.int64) if s > 1 else None     # (squared-distance bits << 32 | row) keys
    _run("l2h_knn_index", 2.0 * n * d * r, 2.0 * (x.numel() + bank_h.numel()) + 4.0 * (r + n + 2 * n * k) + 16.0 * (s > 1) * s * n * 3,
         lambda: _hip.lib().ssad_l2h_knn_index(_hip.hptr(xh), _hip.ptr(xsq), _hip.hptr(bank_h), _hip.ptr(bank_sq),
                                               _hip.ptr(part, True, torch.int64), _hip.ptr(dist), _hip.ptr(idx, dtype=torch.int32), n, d, r,
                                               k, s, _hip.stream()))
    return dist, idx


INT8_MAX_D = 32768      # D 255^2 -- the largest squared code distance -- fits int32 up to here (csrc/knn_l2_int8.hip)


def _int8_from_step(s):
    """(s, inv_s, s2) from the fp32 step s: inv_s = 1 / s and s2 = s s in float64, each rounded once to fp32."""
    s = float(np.float32(s))
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(f"the int8 step must be finite and positive, got {s}")
    return s, float(np.float32(1.0 / s)), float(np.float32(s * s))


def int8_quantiser(lo, hi):
    """The uniform 8-bit code of a bank whose smallest / largest element are lo / hi (faiss' QT_8bit_uniform): (lo, s, inv_s, s2) as
    Python floats holding fp32 values -- lo as given (an fp32 value), s = (hi - lo) / 255 (1 when hi == lo) computed in float64 and
    rounded once to fp32, inv_s = 1 / s and s2 = s s likewise from that s, so (lo, s) alone reproduce all four.  ValueError unless
    both are finite."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"int8_quantiser: the bank's range must be finite, got [{lo}, {hi}]")
    return (float(np.float32(lo)),) + _int8_from_step((hi - lo) / 255.0 if hi != lo else 1.0)


def _check_int8_width(name, d):
    if d % 32 or d > INT8_MAX_D:
        raise ValueError(f"{name}: the int8 kernels need a width that is a multiple of 32 (at most {INT8_MAX_D}), got {d}")


def rows_to_int8(x, lo, inv_s, s):
    """x [N][D] fp32 -> (codes [N][D] int8, sq [N] int32, excess [N] float32) in one pass (csrc/knn_l2_int8.hip ssad_rows_to_int8):
    the code rint(min(max((x - lo) * inv_s, 0), 255)) - 128 of every element (fp32, to nearest even, NaN -> -128), the sum of the
    squared codes of every row, and excess = sum (x - clamp(x, lo, lo + 255 s))^2 in row_sqnorms' order -- what the clamp took from
    the row: 0 inside the coded range.  (lo, s, inv_s): int8_quantiser."""
    n, d = x.shape
    _check_int8_width("rows_to_int8", d)
    codes = torch.empty((n, d), device=x.device, dtype=torch.int8)
    sq = torch.empty((n,), device=x.device, dtype=torch.int32)
    excess = _new((n,), x)
    _run("rows_to_int8", 4.0 * n * d, 5.0 * x.numel() + 8.0 * n,
         lambda: _hip.lib().ssad_rows_to_int8(_hip.ptr(x), _hip.ptr(codes, dtype=torch.int8), _hip.ptr(sq, dtype=torch.int32),
                                              _hip.ptr(excess), n, d, float(lo), float(inv_s), float(s), _hip.stream()))
    return codes, sq, excess


def _l2q_args(name, x, bank_q, bank_sq, quant, k, splits):
    _check_int8_width(name, x.shape[1])
    args = _l2_flat_args(name, x, bank_q, bank_sq, k, splits, torch.int8)
    lo = float(np.float32(quant[0]))
    if not np.isfinite(lo):
        raise ValueError(f"{name}: quant = (lo, s) must be finite, got {tuple(quant)!r}")
    return args + (lo,) + _int8_from_step(quant[1])


def l2q_knn_fused(x, bank_q, bank_sq, quant, k=3, splits=None):
    """l2_knn_fused on an 8-bit scalar-quantised bank: x [N][D] fp32 queries (coded here, rows_to_int8, with the bank's code),
    (bank_q, bank_sq, _) = rows_to_int8(bank, ...), quant = (lo, s) -> [N] mean of the k smallest distances BETWEEN THE CODES,
    sqrt(s^2 D2 + excess(x)), D2 the exact int32 squared code distance on the int8 matrix cores (csrc/knn_l2_int8.hip
    ssad_l2q_knn_fused).  `splits` as in l2_knn_fused; the same bits for every S."""
    n, d, r, k, s, lo, step, inv_s, s2 = _l2q_args("l2q_knn_fused", x, bank_q, bank_sq, quant, k, splits)
    xq, xsq, xex = rows_to_int8(x, lo, inv_s, step)
    out = _new((n,), x)
    part = torch.empty((s, n, 3), device=x.device, dtype=torch.int32) if s > 1 else None     # squared code distances
    i8, i32 = torch.int8, torch.int32
    _run("l2q_knn_fused", 2.0 * n * d * r, 1.0 * (x.numel() + bank_q.numel()) + 4.0 * (r + 3 * n) + 8.0 * (s > 1) * s * n * 3,
         lambda: _hip.lib().ssad_l2q_knn_fused(_hip.ptr(xq, dtype=i8), _hip.ptr(xsq, dtype=i32), _hip.ptr(xex), _hip.ptr(bank_q, dtype=i8),
                                               _hip.ptr(bank_sq, dtype=i32), _hip.ptr(part, True, i32), _hip.ptr(out), n, d, r, k, s, s2,
                                               _hip.stream()))
    return out


def l2q_knn_index(x, bank_q, bank_sq, quant, k=3, splits=None):
    """l2_knn_index on an 8-bit scalar-quantised bank (arguments as l2q_knn_fused): (dist [N][k] float32, idx [N][k] int32), the k
    smallest (D2, bank row) pairs between the codes, equal D2 to the smaller row -- exactly the first k of a stable sort, the D2
    being integers; dist holds the bits l2q_knn_fused averages (csrc/knn_l2_int8.hip ssad_l2q_knn_index)."""
    n, d, r, k, s, lo, step, inv_s, s2 = _l2q_args("l2q_knn_index", x, bank_q, bank_sq, quant, k, splits)
    xq, xsq, xex = rows_to_int8(x, lo, inv_s, step)
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    part = torch.empty((s, n, 3), device=x.device, dtype=torch.int64) if s > 1 else None     # (D2 << 32 | row) keys
    i8, i32 = torch.int8, torch.int32
    _run("l2q_knn_index", 2.0 * n * d * r, 1.0 * (x.numel() + bank_q.numel()) + 4.0 * (r + 2 * n + 2 * n * k) + 16.0 * (s > 1) * s * n * 3,
         lambda: _hip.lib().ssad_l2q_knn_index(_hip.ptr(xq, dtype=i8), _hip.ptr(xsq, dtype=i32), _hip.ptr(xex), _hip.ptr(bank_q, dtype=i8),
                                               _hip.ptr(bank_sq, dtype=i32), _hip.ptr(part, True, torch.int64), _hip.ptr(dist),
                                               _hip.ptr(idx, dtype=i32), n, d, r, k, s, s2, _hip.stream()))
    return dist, idx


TOPK_MIN, TOPK_MAX = 4, 32     # k of the list kernels (csrc/knn_topk.hip); 1..3 stay with the kernels above


def _topk_args(name, x, bank, bank_sq, k, splits, half):
    n, d, r, k, s = _l2_flat_args(name, x, bank, bank_sq, k, splits, torch.float16 if half else torch.float32, (TOPK_MIN, TOPK_MAX))
    part = torch.empty((s, n, k), device=x.device, dtype=torch.int64) if s > 1 else None   # (squared-distance bits << 32 | row) keys
    return n, d, r, k, s, part


def l2_topk_index(x, bank, bank_sq, k, splits=None):
    """l2_knn_index for k in 4..32 (csrc/knn_topk.hip ssad_l2_knn_topk_index): (dist [N][k] float32, idx [N][k] int32), the first k
    entries of a stable ascending sort of the (squared distance, bank row) pairs of every query; a pair's squared distance has
    l2_knn_index's bits, so the first three columns are l2_knn_index(k=3).  `splits` as in l2_knn_fused; the same bits for every S
    and every batch a query sits in."""
    n, d, r, k, s, part = _topk_args("l2_topk_index", x, bank, bank_sq, k, splits, False)
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    _run("l2_topk_index", 2.0 * n * d * r, 4.0 * (x.numel() + bank.numel() + r + 2 * n * k) + 16.0 * (s > 1) * s * n * k,
         lambda: _hip.lib().ssad_l2_knn_topk_index(_hip.ptr(x), _hip.ptr(bank), _hip.ptr(bank_sq), _hip.ptr(part, True, torch.int64), _hip.ptr(dist),
                                                   _hip.ptr(idx, dtype=torch.int32), n, d, r, k, s, _hip.stream()))
    return dist, idx


def l2_topk_mean(x, bank, bank_sq, k, splits=None):
    """l2_knn_fused for k in 4..32 (csrc/knn_topk.hip ssad_l2_knn_topk) -> [N] mean of the k smallest Euclidean distances: the fp32
    sum of l2_topk_index's dist row, added smallest first one after the other, divided by k -- those bits."""
    n, d, r, k, s, part = _topk_args("l2_topk_mean", x, bank, bank_sq, k, splits, False)
    out = _new((n,), x)
    _run("l2_topk_mean", 2.0 * n * d * r, 4.0 * (x.numel() + bank.numel() + r + n) + 16.0 * (s > 1) * s * n * k,
         lambda: _hip.lib().ssad_l2_knn_topk(_hip.ptr(x), _hip.ptr(bank), _hip.ptr(bank_sq), _hip.ptr(part, True, torch.int64), _hip.ptr(out), n, d, r, k, s,
                                             _hip.stream()))
    return out


def l2h_topk_index(x, bank_h, bank_sq, k, splits=None):
    """l2h_knn_index for k in 4..32 (arguments as l2h_knn_fused; csrc/knn_topk.hip ssad_l2h_knn_topk_index): l2_topk_index between
    the rounded rows, a pair's squared distance with l2h_knn_index's bits."""
    n, d, r, k, s, part = _topk_args("l2h_topk_index", x, bank_h, bank_sq, k, splits, True)
    xh, xsq = rows_to_half(x)
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    _run("l2h_topk_index", 2.0 * n * d * r, 2.0 * (x.numel() + bank_h.numel()) + 4.0 * (r + n + 2 * n * k) + 16.0 * (s > 1) * s * n * k,
         lambda: _hip.lib().ssad_l2h_knn_topk_index(_hip.hptr(xh), _hip.ptr(xsq), _hip.hptr(bank_h), _hip.ptr(bank_sq), _hip.ptr(part, True, torch.int64),
                                                    _hip.ptr(dist), _hip.ptr(idx, dtype=torch.int32), n, d, r, k, s, _hip.stream()))
    return dist, idx


def l2h_topk_mean(x, bank_h, bank_sq, k, splits=None):
    """l2h_knn_fused for k in 4..32 (csrc/knn_topk.hip ssad_l2h_knn_topk): the sequential fp32 sum of l2h_topk_index's dist row
    divided by k."""
    n, d, r, k, s, part = _topk_args("l2h_topk_mean", x, bank_h, bank_sq, k, splits, True)
    xh, xsq = rows_to_half(x)
    out = _new((n,), x)
    _run("l2h_topk_mean", 2.0 * n * d * r, 2.0 * (x.numel() + bank_h.numel()) + 4.0 * (r + 2 * n) + 16.0 * (s > 1) * s * n * k,
         lambda: _hip.lib().ssad_l2h_knn_topk(_hip.hptr(xh), _hip.ptr(xsq), _hip.hptr(bank_h), _hip.ptr(bank_sq), _hip.ptr(part, True, torch.int64),
                                              _hip.ptr(out), n, d, r, k, s, _hip.stream()))
    return out


def l2q_topk_index(x, bank_q, bank_sq, quant, k, splits=None):
    """l2q_knn_index for k in 4..32 (arguments as l2q_knn_fused; csrc/knn_refine.hip ssad_topk_l2q_index): (dist [N][k] float32,
    idx [N][k] int32), exactly the first k entries of a stable ascending sort of the (D2, bank row) pairs between the codes; a pair's
    dist has l2q_knn_index's bits, so the first three columns are l2q_knn_index(k=3).  The same bits for every S and every batch."""
    _check_int8_width("l2q_topk_index", x.shape[1])
    n, d, r, k, s = _l2_flat_args("l2q_topk_index", x, bank_q, bank_sq, k, splits, torch.int8, (TOPK_MIN, TOPK_MAX))
    lo = float(np.float32(quant[0]))
    if not np.isfinite(lo):
        raise ValueError(f"l2q_topk_index: quant = (lo, s) must be finite, got {tuple(quant)!r}")
    step, inv_s, s2 = _int8_from_step(quant[1])
    xq, xsq, xex = rows_to_int8(x, lo, inv_s, step)
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    part = torch.empty((s, n, k), device=x.device, dtype=torch.int64) if s > 1 else None     # (D2 << 32 | row) keys
    i8, i32 = torch.int8, torch.int32
    _run("l2q_topk_index", 2.0 * n * d * r, 1.0 * (x.numel() + bank_q.numel()) + 4.0 * (r + 2 * n + 2 * n * k) + 16.0 * (s > 1) * s * n * k,
         lambda: _hip.lib().ssad_topk_l2q_index(_hip.ptr(xq, dtype=i8), _hip.ptr(xsq, dtype=i32), _hip.ptr(xex),
                                                    _hip.ptr(bank_q, dtype=i8), _hip.ptr(bank_sq, dtype=i32),
                                                    _hip.ptr(part, True, torch.int64), _hip.ptr(dist), _hip.ptr(idx, dtype=i32), n, d, r,
                                                    k, s, s2, _hip.stream()))
    return dist, idx


RERANK_MAX = 32     # the longest shortlist of csrc/knn_refine.hip (TOPK_MAX: what the coarse searches return)


def _rerank_args(name, x, bank, cand, k):
    """The argument checks of the re-rank, from shapes and dtypes alone: fp32 x [N][D] and bank [R][D], int32 cand [N][r] with r in
    1..RERANK_MAX, k in 1..r.  -> (n, d, rows, r, k)."""
    if x.dim() != 2 or bank.dim() != 2 or x.dtype != torch.float32 or bank.dtype != torch.float32 or bank.shape[1] != x.shape[1] \
            or x.shape[0] < 1 or x.shape[1] < 1 or bank.shape[0] < 1:
        raise ValueError(f"{name}: x [N][D] and bank [R][D] must be float32 of one width, got {x.dtype} {tuple(x.shape)} and "
                         f"{bank.dtype} {tuple(bank.shape)}")
    n, d = x.shape
    if cand.dim() != 2 or cand.dtype != torch.int32 or cand.shape[0] != n:
        raise ValueError(f"{name}: cand must be int32 [{n}][r], got {cand.dtype} {tuple(cand.shape)}")
    r, k = int(cand.shape[1]), int(k)
    if not 1 <= r <= RERANK_MAX:
        raise ValueError(f"{name}: a shortlist holds 1..{RERANK_MAX} rows, got r = {r}")
    if not 1 <= k <= r:
        raise ValueError(f"{name}: k must lie in 1..r = 1..{r}, got {k}")
    return n, d, int(bank.shape[0]), r, k


def l2_rerank_index(x, bank, cand, k):
    """x [N][D], bank [R][D] fp32, cand [N][r] int32 listed bank rows (r in 1..32) -> (dist [N][k] float32, idx [N][k] int32): the k
    (1..r) nearest of every query's listed rows by the direct squared distance sum (x - b)^2 -- l2_direct's bits for the pair --
    ascending by (d2, bank row, place in the list); dist holds the roots (csrc/knn_refine.hip ssad_rerank_l2_index).  An entry
    outside 0..R-1 is skipped, missing places are (+inf, -1), a row listed twice appears twice."""
    n, d, rows, r, k = _rerank_args("l2_rerank_index", x, bank, cand, k)
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    _run("l2_rerank_index", 3.0 * n * r * d, 4.0 * (x.numel() + n * r * d + n * r + 2 * n * k),
         lambda: _hip.lib().ssad_rerank_l2_index(_hip.ptr(x), _hip.ptr(bank), _hip.ptr(cand, dtype=torch.int32), _hip.ptr(dist),
                                                 _hip.ptr(idx, dtype=torch.int32), n, d, rows, r, k, _hip.stream()))
    return dist, idx


def l2_rerank_mean(x, bank, cand, k):
    """-> [N] the sequential fp32 sum of l2_rerank_index's dist row, smallest first, divided by k (csrc/knn_refine.hip
    ssad_rerank_l2): +inf for a query with fewer than k valid entries."""
    n, d, rows, r, k = _rerank_args("l2_rerank_mean", x, bank, cand, k)
    out = _new((n,), x)
    _run("l2_rerank_mean", 3.0 * n * r * d, 4.0 * (x.numel() + n * r * d + n * r + n),
         lambda: _hip.lib().ssad_rerank_l2(_hip.ptr(x), _hip.ptr(bank), _hip.ptr(cand, dtype=torch.int32), _hip.ptr(out), n, d, rows, r,
                                           k, _hip.stream()))
    return out


def l2_from_dots(sim, qsq, bsq):
    """sim [Q][R] dot products, qsq [Q], bsq [R] squared norms -> [Q][R] SQUARED Euclidean distances max(qsq + bsq - 2 sim, 0)
    (csrc/knn_l2.hip ssad_l2_from_dots; the kNN kernels' expression)."""
    q, r = sim.shape
    out = _new((q, r), sim)
    _run("l2_from_dots", 3.0 * q * r, 8.0 * q * r,
         lambda: _hip.lib().ssad_l2_from_dots(_hip.ptr(sim), _hip.ptr(qsq), _hip.ptr(bsq), _hip.ptr(out), q, r, _hip.stream()))
    return out


def knn_reweight_l2(xs, bank, mstar, nbr, smax):
    """PatchCore's image-score weight on Euclidean distances (csrc/knn_l2.hip ssad_knn_reweight_l2): xs [Q][D], bank [R][D] (neither
    normalised), mstar [Q] / [Q][1] int32 nearest bank rows, nbr [Q][b'] int32 neighbourhood rows, smax [Q] -> [Q]:
    (1 - exp(d(x, mstar) - dmax) / sum_j exp(d(x, nbr_j) - dmax)) smax, dmax = max_j d(x, nbr_j)."""
    q, d = xs.shape
    r = bank.shape[0]
    bp = nbr.shape[1]
    out = _new((q,), xs)
    i32 = torch.int32
    _run("knn_reweight_l2", 3.0 * q * d * (bp + 1), 4.0 * q * d * (bp + 2),
         lambda: _hip.lib().ssad_knn_reweight_l2(_hip.ptr(xs), _hip.ptr(bank), _hip.ptr(mstar, dtype=i32), _hip.ptr(nbr, dtype=i32),
                                                 _hip.ptr(smax), _hip.ptr(out), q, d, r, bp, _hip.stream()))
    return out


def group_means(x, p):
    """x [G p][D], p rows per image, image after image -> [G][D] per-image means (csrc/knn_gallery.hip ssad_group_means): summed in
    fp64 in row order, rounded once to fp32 -- an image's mean is the same bits in every batch.  The gallery's image descriptor."""
    n, d = x.shape
    p = int(p)
    if p < 1 or n < 1 or n % p:
        raise ValueError(f"group_means: {n} rows are not whole images of {p} rows")
    g = n // p
    out = _new((g, d), x)
    _run("group_means", 1.0 * n * d, 4.0 * (x.numel() + g * d),
         lambda: _hip.lib().ssad_group_means(_hip.ptr(x), _hip.ptr(out), g, p, d, _hip.stream()))
    return out


def l2_direct(q, b):
    """q [Q][D], b [T][D] -> [Q][T] SQUARED Euclidean distances sum (q - b)^2 by direct differences (csrc/knn_gallery.hip
    ssad_l2_direct): no cancellation, a pair's bits do not depend on Q or T."""
    nq, d = q.shape
    t = b.shape[0]
    if b.shape[1] != d or nq < 1 or t < 1:
        raise ValueError(f"l2_direct: shapes {tuple(q.shape)} and {tuple(b.shape)} do not go together")
    out = _new((nq, t), q)
    _run("l2_direct", 3.0 * nq * t * d, 4.0 * (q.numel() + nq * b.numel() + nq * t),
         lambda: _hip.lib().ssad_l2_direct(_hip.ptr(q), _hip.ptr(b), _hip.ptr(out), nq, t, d, _hip.stream()))
    return out


def gallery_splits(q, p, kk):
    """Splits S of l2_knn_gallery over the kk gallery entries of q query images of p rows: 1 when the (query tile, image) workgroups
    alone reach KNN_SPLIT_TARGET_WG, else enough splits to reach that many, at most kk.  SSAD_KNN_SPLIT=0 forces 1.  The results
    are the same bits for every S."""
    if os.environ.get("SSAD_KNN_SPLIT", "1") == "0":
        return 1
    wgs = -(-int(p) // 128) * int(q)
    if wgs >= KNN_SPLIT_TARGET_WG:
        return 1
    return max(1, min(-(-KNN_SPLIT_TARGET_WG // wgs), int(kk)))


def _gallery_args(name, x, bank, bank_sq, gallery, p, k, splits):
    n, d = x.shape
    r = bank.shape[0]
    p, k = int(p), int(k)
    _check_l2_width(name, d)
    if bank.shape[1] != d:
        raise ValueError(f"{name}: the queries have {d} columns, the bank {bank.shape[1]}")
    if p < 1 or n < 1 or n % p or r < 1 or r % p:
        raise ValueError(f"{name}: {n} query rows and {r} bank rows are not both whole images of {p} rows")
    if bank_sq.shape != (r,):
        raise ValueError(f"{name}: bank_sq must hold one squared norm per bank row ({r}), got {tuple(bank_sq.shape)}")
    q, t = n // p, r // p
    if gallery.dim() != 2 or gallery.shape[0] != q or gallery.shape[1] < 1 or gallery.dtype != torch.int32:
        raise ValueError(f"{name}: gallery must be int32 [{q}][K] with K >= 1, got {gallery.dtype} {tuple(gallery.shape)}")
    kk = int(gallery.shape[1])
    if not 1 <= k <= 3:
        raise ValueError(f"{name}: k must be 1, 2 or 3, got {k}")
    if kk * p < k:
        raise ValueError(f"{name}: a gallery of {kk} images of {p} rows has fewer than k = {k} rows")
    if q > 65535:
        raise ValueError(f"{name}: at most 65535 query images per call, got {q}")
    s = gallery_splits(q, p, kk) if splits is None else int(splits)
    if not 1 <= s <= 65535:
        raise ValueError(f"{name}: splits must lie in 1..65535, got {s}")
    return n, d, q, p, t, kk, k, s


def l2_knn_gallery(x, bank, bank_sq, gallery, p, k=3, splits=None):
    """l2_knn_fused with the bank of every query image restricted to a gallery of bank images (SPADE; csrc/knn_gallery.hip
    ssad_l2_knn_gallery): x [Q p][D] and bank [T p][D] hold p rows per image, image after image; gallery int32 [Q][K] names the K
    bank images of each query image (an entry outside 0..T-1 is skipped) -> [Q p] mean of the k smallest Euclidean distances to the
    rows of those images, +inf where fewer than k rows are left.  A (query, bank row) pair gets l2_knn_fused's bits.  `splits`: None =
    the gallery_splits rule; S >= 1 = that many splits of the K entries; the same bits for every S."""
    n, d, q, p, t, kk, k, s = _gallery_args("l2_knn_gallery", x, bank, bank_sq, gallery, p, k, splits)
    out = _new((n,), x)
    part = _new((s, n, 3), x) if s > 1 else None
    _run("l2_knn_gallery", 2.0 * n * d * kk * p, 4.0 * (x.numel() + q * kk * p * (d + 1) + n) + (24.0 * part.numel() if s > 1 else 0.0),
         lambda: _hip.lib().ssad_l2_knn_gallery(_hip.ptr(x), _hip.ptr(bank), _hip.ptr(bank_sq), _hip.ptr(gallery, dtype=torch.int32),
                                                _hip.ptr(part, allow_none=True), _hip.ptr(out), q, p, t, kk, d, k, s, _hip.stream()))
    return out


def l2_knn_gallery_index(x, bank, bank_sq, gallery, p, k=3, splits=None):
    """kneighbors over the galleries of l2_knn_gallery (csrc/knn_gallery.hip ssad_l2_knn_gallery_index): (dist [Q p][k] float32,
    idx [Q p][k] int32), the k smallest (squared distance, GLOBAL bank row) pairs of every query among its image's gallery rows,
    ascending, equal ones to the smaller global row; missing slots hold (+inf, -1).  dist holds the bits l2_knn_gallery averages."""
    n, d, q, p, t, kk, k, s = _gallery_args("l2_knn_gallery_index", x, bank, bank_sq, gallery, p, k, splits)
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    part = torch.empty((s, n, 3), device=x.device, dtype=torch.int64) if s > 1 else None      # (squared-distance bits << 32 | row) keys
    _run("l2_knn_gallery_index", 2.0 * n * d * kk * p,
         4.0 * (x.numel() + q * kk * p * (d + 1) + 2 * n * k) + (16.0 * part.numel() if s > 1 else 0.0),
         lambda: _hip.lib().ssad_l2_knn_gallery_index(_hip.ptr(x), _hip.ptr(bank), _hip.ptr(bank_sq), _hip.ptr(gallery, dtype=torch.int32),
                                                      _hip.ptr(part, allow_none=True, dtype=torch.int64), _hip.ptr(dist),
                                                      _hip.ptr(idx, dtype=torch.int32), q, p, t, kk, d, k, s, _hip.stream()))
    return dist, idx


def segment_means(x, order, offsets, out=None):
    """k-means' update step (csrc/knn_ivf.hip ssad_segment_means): x [N][D], order int32 [N] = the rows sorted by cell, offsets int32
    [nlist + 1] -> [nlist][D], row g the mean of x[order[offsets[g] : offsets[g + 1]]], summed in fp64 in order's sequence and rounded
    once to fp32: no atomics, the same bits on every call.  group_means for groups of any length.  An empty segment leaves its row of
    `out` untouched: pass the previous centroids (None: zeros)."""
    n, d = x.shape
    if order.dtype != torch.int32 or tuple(order.shape) != (n,):
        raise ValueError(f"segment_means: order must be int32 [{n}], got {order.dtype} {tuple(order.shape)}")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] < 2:
        raise ValueError(f"segment_means: offsets must be int32 [nlist + 1], got {offsets.dtype} {tuple(offsets.shape)}")
    nlist = int(offsets.shape[0]) - 1
    if n < 1 or nlist > 65535:
        raise ValueError(f"segment_means: needs at least one row and at most 65535 segments, got {n} rows and {nlist} segments")
    if out is None:
        out = torch.zeros((nlist, d), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (nlist, d):
        raise ValueError(f"segment_means: out must be [{nlist}][{d}], got {tuple(out.shape)}")
    i32 = torch.int32
    _run("segment_means", 1.0 * n * d, 4.0 * (x.numel() + n + nlist * d),
         lambda: _hip.lib().ssad_segment_means(_hip.ptr(x), _hip.ptr(order, dtype=i32), _hip.ptr(offsets, dtype=i32), _hip.ptr(out), n,
                                               nlist, d, _hip.stream()))
    return out


def cell_offsets(sorted_cells, nlist):
    """Ascending cell numbers [M] (any integer type, on the device) -> int32 [nlist + 1], the first position of every cell and M:
    cell c holds the positions offsets[c] .. offsets[c + 1] - 1.  A binary search on the device, no synchronisation."""
    edges = torch.arange(int(nlist) + 1, device=sorted_cells.device, dtype=sorted_cells.dtype)
    return torch.searchsorted(sorted_cells, edges).to(torch.int32)


def ivf_schedule(probes, nlist):
    """The work list of l2_knn_ivf for probes int32 [N][nprobe], made on the device without a synchronisation: (tiles int32 [3][G],
    pairs int32 [N nprobe]).  pairs = the pair ids n nprobe + j in a stable sort by the cell they name (entries outside 0..nlist-1
    last, in no tile); a cell's run is cut into tiles of 128 pairs; tiles[0] = the cell, tiles[1] = the first position in `pairs`,
    tiles[2] = the pairs of the tile.  G = ceil(N nprobe / 128) + nlist bounds the tiles of any probes; the surplus ones name cell
    nlist."""
    n, nprobe = probes.shape
    nlist = int(nlist)
    m = n * nprobe
    g = -(-m // 128) + nlist
    flat = probes.reshape(-1)
    cells = torch.where((flat >= 0) & (flat < nlist), flat, torch.full_like(flat, nlist))
    sorted_cells, pairs = torch.sort(cells, stable=True)
    start = cell_offsets(sorted_cells, nlist).long()                    # [nlist + 1]
    tiles_of = (start[1:] - start[:-1] + 127) // 128                    # tiles of every cell
    last = torch.cumsum(tiles_of, 0)                                    # one past the last tile of every cell
    t = torch.arange(g, device=probes.device)
    cell = torch.searchsorted(last, t, right=True)                      # nlist for a surplus tile
    safe = cell.clamp(max=nlist - 1)
    first = start[safe] + (t - (last[safe] - tiles_of[safe])) * 128
    count = (start[safe + 1] - first).clamp(min=0, max=128)
    tiles = torch.stack([cell, first, count]).to(torch.int32).contiguous()
    return tiles, pairs.to(torch.int32)


def _ivf_args(name, x, bank_sorted, bank_sq, offsets, probes, perm, k):
    n, d = x.shape
    r = bank_sorted.shape[0]
    k = int(k)
    _check_l2_width(name, d)
    i32 = torch.int32
    if bank_sorted.shape[1] != d:
        raise ValueError(f"{name}: the queries have {d} columns, the bank {bank_sorted.shape[1]}")
    if n < 1 or r < 1:
        raise ValueError(f"{name}: needs at least one query and one bank row, got {n} and {r}")
    if bank_sq.shape != (r,):
        raise ValueError(f"{name}: bank_sq must hold one squared norm per bank row ({r}), got {tuple(bank_sq.shape)}")
    if perm.dtype != i32 or tuple(perm.shape) != (r,):
        raise ValueError(f"{name}: perm must be int32 [{r}] (the original row of every sorted row), got {perm.dtype} {tuple(perm.shape)}")
    if offsets.dtype != i32 or offsets.dim() != 1 or offsets.shape[0] < 2:
        raise ValueError(f"{name}: offsets must be int32 [nlist + 1], got {offsets.dtype} {tuple(offsets.shape)}")
    nlist = int(offsets.shape[0]) - 1
    if probes.dtype != i32 or probes.dim() != 2 or probes.shape[0] != n or probes.shape[1] < 1:
        raise ValueError(f"{name}: probes must be int32 [{n}][nprobe] with nprobe >= 1, got {probes.dtype} {tuple(probes.shape)}")
    nprobe = int(probes.shape[1])
    if not 1 <= k <= 3:
        raise ValueError(f"{name}: k must be 1, 2 or 3, got {k}")
    if n * nprobe > 2 ** 31 - 1:
        raise ValueError(f"{name}: {n} queries x {nprobe} probes are too many pairs for one call")
    if x.data_ptr() % 16:
        raise ValueError(f"{name}: the queries must start at a 16-byte boundary")
    return n, d, r, nlist, nprobe, k


def _ivf_launch(name, entry, outs, x, bank_sorted, bank_sq, offsets, probes, perm, n, d, r, nlist, nprobe, k):
    i32 = torch.int32
    probes = probes.contiguous()
    tiles, pairs = ivf_schedule(probes, nlist)
    g = int(tiles.shape[1])
    part = torch.empty((n * nprobe, 3), device=x.device, dtype=torch.int64)     # (squared-distance bits << 32 | original row) keys
    # the arithmetic of the expected work (every query meets nprobe cells of R / nlist rows); the kernel issues whole 128 x 128 tiles
    flops = 2.0 * n * d * nprobe * r / nlist
    _run(name, flops, 4.0 * (x.numel() * nprobe + bank_sorted.numel() + 2 * r) + 24.0 * part.numel() * 2,
         lambda: entry(_hip.ptr(x), _hip.ptr(bank_sorted), _hip.ptr(bank_sq), _hip.ptr(offsets, dtype=i32), _hip.ptr(perm, dtype=i32),
                       _hip.ptr(probes, dtype=i32), _hip.ptr(tiles, dtype=i32), _hip.ptr(pairs, dtype=i32),
                       _hip.ptr(part, dtype=torch.int64), *outs, n, d, r, nlist, nprobe, g, k, _hip.stream()))


def l2_knn_ivf_index(x, bank_sorted, bank_sq, offsets, probes, perm, k=3):
    """kneighbors over an inverted file (csrc/knn_ivf.hip ssad_l2_knn_ivf_index): x [N][D]; bank_sorted [R][D] the bank rows stored
    cell after cell, bank_sq their squared norms, offsets int32 [nlist + 1] the cells' bounds, perm int32 [R] the original row of
    every sorted row; probes int32 [N][nprobe] the cells every query meets (an entry outside 0..nlist-1 is skipped, a cell named
    twice counts once) -> (dist [N][k] float32, idx [N][k] int32): the k (1..3) smallest (squared distance, ORIGINAL bank row) pairs
    among the rows of those cells, ascending, equal ones to the smaller original row; slots the cells cannot fill hold (+inf, -1).
    A (query, bank row) pair gets l2_knn_index's bits, however the pairs fall into tiles.  The work list (ivf_schedule) is made on the
    device: no host synchronisation."""
    n, d, r, nlist, nprobe, k = _ivf_args("l2_knn_ivf_index", x, bank_sorted, bank_sq, offsets, probes, perm, k)
    dist = _new((n, k), x)
    idx = torch.empty((n, k), device=x.device, dtype=torch.int32)
    _ivf_launch("l2_knn_ivf_index", _hip.lib().ssad_l2_knn_ivf_index, (_hip.ptr(dist), _hip.ptr(idx, dtype=torch.int32)), x, bank_sorted,
                bank_sq, offsets, probes, perm, n, d, r, nlist, nprobe, k)
    return dist, idx


def l2_knn_ivf(x, bank_sorted, bank_sq, offsets, probes, perm, k=3):
    """l2_knn_fused over an inverted file (csrc/knn_ivf.hip ssad_l2_knn_ivf; arguments as l2_knn_ivf_index) -> [N] mean of the k
    smallest Euclidean distances to the rows of the probed cells, +inf where they hold fewer than k rows: l2_knn_ivf_index's
    distances averaged, bit for bit."""
    n, d, r, nlist, nprobe, k = _ivf_args("l2_knn_ivf", x, bank_sorted, bank_sq, offsets, probes, perm, k)
    out = _new((n,), x)
    _ivf_launch("l2_knn_ivf", _hip.lib().ssad_l2_knn_ivf, (_hip.ptr(out),), x, bank_sorted, bank_sq, offsets, probes, perm, n, d, r, nlist,
                nprobe, k)
    return out


IVF_PROBE_CHUNK = 65535         # queries per pass of ivf_probes (the grid bound of l2_from_dots)


def ivf_probes(x, centroids, cent_sq, nprobe):
    """The coarse step of the inverted file: x [N][D], centroids [nlist][D], cent_sq = row_sqnorms(centroids) -> int32 [N][nprobe], the
    nprobe cells whose centroids are nearest to every query by the kernels' squared distance max(|x|^2 + |c|^2 - 2 <x, c>, 0),
    ordered by (squared distance, cell): equal distances to the smaller cell.  One GEMM (linear_fwd), l2_from_dots and a selection of
    packed (distance bits << 32 | cell) keys per pass of IVF_PROBE_CHUNK queries; no host synchronisation."""
    n = x.shape[0]
    nlist = int(centroids.shape[0])
    nprobe = int(nprobe)
    if not 1 <= nprobe <= nlist:
        raise ValueError(f"ivf_probes: nprobe must lie in 1..nlist = {nlist}, got {nprobe}")
    out = torch.empty((n, nprobe), device=x.device, dtype=torch.int32)
    cells = torch.arange(nlist, device=x.device, dtype=torch.int64)
    xsq = row_sqnorms(x)
    for i in range(0, n, IVF_PROBE_CHUNK):
        xs = x[i:i + IVF_PROBE_CHUNK]
        d2 = l2_from_dots(linear_fwd(xs, centroids), xsq[i:i + IVF_PROBE_CHUNK], cent_sq)
        keys = (d2.view(torch.int32).long() << 32) | cells                  # d2 >= 0: the keys order like (d2, cell)
        out[i:i + IVF_PROBE_CHUNK] = torch.topk(keys, nprobe, dim=1, largest=False, sorted=True).values.bitwise_and_(0xffffffff)
    return out


KMEANS_ROWS_PER_CELL = 256      # rows per cell the iterations are run on at the most (faiss' max_points_per_centroid)


def kmeans_init(n, nlist, seed=0, train_rows=None):
    """The draws of kmeans_l2 for n rows, from a dedicated CPU torch.Generator seeded with `seed` (never the global generators; the
    same on every rank): (sample, init).  sample: None when the iterations use every row, else the int64 rows they use, ascending
    -- min(n, train_rows) of them, train_rows=None meaning KMEANS_ROWS_PER_CELL * nlist; init: int64 [nlist] distinct positions in
    the rows the iterations use, the initial centroids."""
    n, nlist = int(n), int(nlist)
    if nlist < 1 or nlist > n:
        raise ValueError(f"kmeans_l2: nlist must lie in 1..{n} (the rows), got {nlist}")
    cap = KMEANS_ROWS_PER_CELL * nlist if train_rows is None else int(train_rows)
    if cap < nlist:
        raise ValueError(f"kmeans_l2: train_rows must be at least nlist = {nlist}, got {cap}")
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    sample = None
    if cap < n:
        sample = torch.randperm(n, generator=g)[:cap].sort().values
    init = torch.randperm(n if sample is None else cap, generator=g)[:nlist]
    return sample, init


def kmeans_l2(x, nlist, iters=10, seed=0, train_rows=None):
    """Lloyd's k-means in the Euclidean metric on the device: x [N][D] -> (centroids [nlist][D] float32, assign int32 [N]).  Initial
    centroids: nlist distinct rows (kmeans_init).  Every iteration: the nearest centroid of every row (l2_knn_index, k = 1: equal
    distances to the smaller cell), a stable sort of the assignments, segment_means; a cell that loses all its rows keeps its
    centroid and may stay empty.  The iterations run on at most train_rows rows (None: 256 nlist, a seeded sample as in faiss);
    the returned assignment is the nearest final centroid of EVERY row.  No host synchronisation, the same bits for the same seed."""
    n, d = x.shape
    nlist, iters = int(nlist), int(iters)
    _check_l2_width("kmeans_l2", d)
    if iters < 0:
        raise ValueError(f"kmeans_l2: iters must be >= 0, got {iters}")
    sample, init = kmeans_init(n, nlist, seed, train_rows)
    xt = x if sample is None else x.index_select(0, sample.to(x.device)).contiguous()
    cent = xt.index_select(0, init.to(x.device)).contiguous()
    for _ in range(iters):
        _, a = l2_knn_index(xt, cent, row_sqnorms(cent), 1)
        sorted_a, order = torch.sort(a.reshape(-1), stable=True)
        cent = segment_means(xt, order.to(torch.int32), cell_offsets(sorted_a, nlist), out=cent.clone())
    _, assign = l2_knn_index(x, cent, row_sqnorms(cent), 1)
    return cent, assign.reshape(-1)


def bilinear_taps(nf, nc):
    """The sample positions csrc/patch_features.hip uses to resample nc positions to nf (F.interpolate's align_corners=False rule in
    integer arithmetic): per destination index i, num = max((2 i + 1) nc - nf, 0), a = num // (2 nf), b = min(a + 1, nc - 1) and the
    weight of b as the exact fraction (num - a 2 nf, 2 nf).  Returns (a, b, weight numerators, denominator) as Python ints."""
    num = [max((2 * i + 1) * nc - nf, 0) for i in range(nf)]
    a = [v // (2 * nf) for v in num]
    return a, [min(v + 1, nc - 1) for v in a], [v - u * 2 * nf for v, u in zip(num, a)], 2 * nf


def local_patch_features(fine, coarse, out=None, rows_per_block=0):
    """Locally aware patch features (PatchCore §3.1 / anomalib; csrc/patch_features.hip): fine [N][Hf][Wf][Cf], coarse [N][Hc][Wc][Cc]
    NHWC -> [N * Hf * Wf][Cf + Cc]: the 3 x 3 average of `fine` beside the 3 x 3 average of `coarse` resampled bilinearly
    (align_corners=False) to the fine grid, rows in (n, i, j) order, not normalised.  out: a contiguous buffer of that shape to fill.
    rows_per_block: the kernel's row band (0: automatic); the result does not depend on it."""
    n, hf, wf, cf = fine.shape
    n2, hc, wc, cc = coarse.shape
    if n2 != n:
        raise _hip.HipExtensionError(f"local_patch_features: {n} fine maps but {n2} coarse maps")
    if out is None:
        out = _new((n * hf * wf, cf + cc), fine)
    elif tuple(out.shape) != (n * hf * wf, cf + cc):
        raise _hip.HipExtensionError(f"local_patch_features: out is {tuple(out.shape)}, expected {(n * hf * wf, cf + cc)}")
    _run("local_patch_features", 0.0, 4.0 * (fine.numel() + coarse.numel() + out.numel()),
         lambda: _hip.lib().ssad_local_patch_features(_hip.ptr(fine), _hip.ptr(coarse), _hip.ptr(out), n, hf, wf, cf, hc, wc, cc,
                                                      rows_per_block, _hip.stream()))
    return out


def pyramid_sel(sel, D, device=None):
    """The column selection of the stage pyramid, checked where it lives (on the host): `sel` [d] integers, strictly increasing, every
    entry in [0, D) -> an int32 tensor (on `device` when given).  HipExtensionError otherwise, before anything is launched."""
    s = torch.as_tensor(sel).detach().cpu().reshape(-1)
    if s.dtype not in (torch.int32, torch.int64) or s.numel() == 0:
        raise _hip.HipExtensionError(f"pyramid_sel: sel must be a non-empty int32 / int64 vector, got {s.dtype} x {s.numel()}")
    if int(s.min()) < 0 or int(s.max()) >= int(D):
        raise _hip.HipExtensionError(f"pyramid_sel: sel has an entry outside [0, {int(D)}) (min {int(s.min())}, max {int(s.max())})")
    if s.numel() > 1 and not bool((s[1:] > s[:-1]).all()):
        raise _hip.HipExtensionError("pyramid_sel: sel must be strictly increasing (sorted, no column twice)")
    s = s.to(torch.int32).contiguous()
    return s if device is None else s.to(device)


def stage_pyramid_rows(maps, sel=None, out=None, sel_dev=None, rows_per_block=0):
    """Stage-pyramid rows (PaDiM's and SPADE's embedding; csrc/pyramid_features.hip): maps = 2 or 3 NHWC stage maps [N][H_s][W_s][C_s] of
    one trunk pass, finest first -> [N * H_0 * W_0][d]: out[(n, i, j)][k] = m_s[n][i H_s // H_0][j W_s // W_0][c] for the stage s and
    channel c of column sel[k] of the concatenation (D = sum C_s columns); a pure copy, F.interpolate(mode='nearest') + cat where the
    ratios are integers.  sel: host integers, strictly increasing in [0, D), checked here (None: all D columns); sel_dev: its device copy
    from pyramid_sel, when the caller keeps one.  out: a contiguous buffer of that shape to fill (a row slice of a larger tensor is
    one).  Bytes: every map read once, every output row written once; columns nobody chose are never written."""
    maps = list(maps)
    if len(maps) not in (2, 3):
        raise _hip.HipExtensionError(f"stage_pyramid_rows: two or three stage maps, finest first, got {len(maps)}")
    for m in maps:
        if not (torch.is_tensor(m) and m.dim() == 4 and m.is_cuda and m.dtype == torch.float32 and m.is_contiguous()):
            raise _hip.HipExtensionError("stage_pyramid_rows: every map must be a contiguous fp32 ROCm tensor [N][H][W][C], got "
                                         + (f"device={m.device} dtype={m.dtype} shape={tuple(m.shape)}" if torch.is_tensor(m) else repr(type(m))))
    n = int(maps[0].shape[0])
    geo = [tuple(int(v) for v in m.shape[1:]) for m in maps]
    if any(int(m.shape[0]) != n for m in maps) or n < 1:
        raise _hip.HipExtensionError(f"stage_pyramid_rows: the maps hold {[int(m.shape[0]) for m in maps]} images")
    if any(c < 4 or c % 4 for _, _, c in geo):
        raise _hip.HipExtensionError(f"stage_pyramid_rows: channel counts must be positive multiples of 4, got {[g[2] for g in geo]}")
    if any(min(h, w) < 1 for h, w, _ in geo) or any(a[0] < b[0] or a[1] < b[1] for a, b in zip(geo, geo[1:])):
        raise _hip.HipExtensionError(f"stage_pyramid_rows: the maps come finest first, got sizes {[g[:2] for g in geo]}")
    D = sum(c for _, _, c in geo)
    if sel is None and sel_dev is None:
        sd, d = None, D
    else:
        sd = pyramid_sel(sel, D, maps[0].device) if sel_dev is None else sel_dev
        if not (sd.is_cuda and sd.dtype == torch.int32 and sd.dim() == 1 and 1 <= sd.numel() <= D):
            raise _hip.HipExtensionError("stage_pyramid_rows: sel_dev must be the int32 device vector of pyramid_sel")
        d = int(sd.numel())
    h0, w0 = geo[0][:2]
    if out is None:
        out = _new((n * h0 * w0, d), maps[0])
    elif tuple(out.shape) != (n * h0 * w0, d):
        raise _hip.HipExtensionError(f"stage_pyramid_rows: out is {tuple(out.shape)}, expected {(n * h0 * w0, d)}")
    g = geo + [(0, 0, 0)] * (3 - len(geo))
    m2 = maps[2] if len(maps) == 3 else None
    _run("stage_pyramid_rows", 0.0, 4.0 * (sum(m.numel() for m in maps) + out.numel() + (0 if sd is None else d)),
         lambda: _hip.lib().ssad_stage_pyramid_rows(_hip.ptr(maps[0]), _hip.ptr(maps[1]), _hip.ptr(m2, True),
                                                    _hip.ptr(sd, True, torch.int32), _hip.ptr(out), n, len(maps), *g[0], *g[1], *g[2], d,
                                                    rows_per_block, _hip.stream()))
    return out


def gaussian_fit_stats(x, normalize=True):
    """x [N][D] fp32 -> (mean [D], scatter [D][D], m4 [1]) fp64 of its rows (L2-normalised first when `normalize`): the centred
    sufficient statistics of a Ledoit-Wolf Gaussian fit (csrc/gde.hip), deterministic."""
    n, d = x.shape
    mean = torch.empty(d, device=x.device, dtype=torch.float64)
    scatter = torch.empty(d, d, device=x.device, dtype=torch.float64)
    m4 = torch.empty(1, device=x.device, dtype=torch.float64)
    f64 = torch.float64
    _run("gaussian_fit_stats", 2.0 * n * d * (d + 1) / 2 + 6.0 * n * d, 4.0 * x.numel() * (1 + (d + 63) // 64) + 8.0 * d * d,
         lambda: _hip.lib().ssad_gaussian_fit_stats(_hip.ptr(x), n, d, int(bool(normalize)), _hip.ptr(mean, dtype=f64),
                                                    _hip.ptr(scatter, dtype=f64), _hip.ptr(m4, dtype=f64), _hip.stream()))
    return mean, scatter, m4


def mahalanobis_fused(x, mu_hi, mu_lo, w, normalize=True):
    """x [N][D] fp32 -> [N] ||W (x_n - mu)||_2 with mu = mu_hi + mu_lo (fp32 pair) and W [D][D] lower triangular, one kernel
    (csrc/gde.hip); rows L2-normalised first when `normalize`.  FLOPs: the dense 2 N D^2 (the kernel skips W's zero blocks)."""
    n, d = x.shape
    out = _new((n,), x)
    _run("mahalanobis_fused", 2.0 * n * d * d, 4.0 * (x.numel() + w.numel() + 2 * d + n),
         lambda: _hip.lib().ssad_mahalanobis_fused(_hip.ptr(x), _hip.ptr(mu_hi), _hip.ptr(mu_lo), _hip.ptr(w), _hip.ptr(out), n, d,
                                                   int(bool(normalize)), _hip.stream()))
    return out


def position_sel(sel, D, device):
    """The channel selection of the per-position Gaussian, checked where it lives (on the host): `sel` [d] integers, every entry in
    [0, D) -> an int32 tensor on `device`.  HipExtensionError otherwise, before anything is launched."""
    s = torch.as_tensor(sel).detach().cpu().reshape(-1)
    if s.dtype not in (torch.int32, torch.int64) or s.numel() == 0:
        raise _hip.HipExtensionError(f"position_sel: sel must be a non-empty int32 / int64 vector, got {s.dtype} x {s.numel()}")
    if int(s.min()) < 0 or int(s.max()) >= int(D):
        raise _hip.HipExtensionError(f"position_sel: sel has an entry outside [0, {int(D)}) (min {int(s.min())}, max {int(s.max())})")
    return s.to(torch.int32).to(device).contiguous()


def _position_shape(x, n_img, P):
    rows, D = x.shape
    if n_img < 1 or P < 1 or rows != n_img * P:
        raise _hip.HipExtensionError(f"{rows} rows are not {n_img} images of {P} positions")
    return D


def position_gaussian_fit_stats(x, sel, n_img, P, sel_dev=None):
    """x [n_img * P][D] fp32 (row n P + p) -> (mean [P][d], scatter [P][d][d]) fp64 of the columns `sel` per position p over the
    images (csrc/padim.hip), deterministic.  sel: host integers, checked here; sel_dev: its device copy from position_sel, when the
    caller keeps one."""
    D = _position_shape(x, n_img, P)
    sd = position_sel(sel, D, x.device) if sel_dev is None else sel_dev
    d = int(sd.numel())
    f64 = torch.float64
    mean = torch.empty((P, d), device=x.device, dtype=f64)
    scatter = torch.empty((P, d, d), device=x.device, dtype=f64)
    t = (d + 63) // 64
    _run("position_gaussian_fit_stats", 2.0 * n_img * P * d * (d + 1) / 2 + 2.0 * n_img * P * d,
         4.0 * n_img * P * d * (1 + t) + 8.0 * P * d * (d + 1),
         lambda: _hip.lib().ssad_position_gaussian_fit_stats(_hip.ptr(x), _hip.ptr(sd, dtype=torch.int32), n_img, P, D, d,
                                                             _hip.ptr(mean, dtype=f64), _hip.ptr(scatter, dtype=f64), _hip.stream()))
    return mean, scatter


def position_gaussian_factor(mean, scatter, n, eps, want64=False):
    """The per-position Gaussians in the form position_mahalanobis takes, on the device (csrc/padim.hip): mean [P][d], scatter
    [P][d][d] fp64 device tensors of position_gaussian_fit_stats over n images -> (mu_hi [P][d], mu_lo [P][d], w [P][d][d]) fp32 with
    Sigma_p = scatter_p / (n - 1) + eps I, C_p its lower Cholesky factor and w_p = C_p^-1 rounded once, exact zeros above the
    diagonal; want64: also (c64, w64) [P][d][d] fp64, C and W before the rounding.  `scatter` is CONSUMED: it is the kernel's
    workspace and holds W in its lower triangle afterwards.  Only its lower triangle is read.  ValueError naming the first position
    and column whose pivot is not finite and positive (its rows of w are NaN).  FLOPs: 2 d^3 / 3 per position; bytes: the lower
    triangle read and written once, w and the optional fp64 copies written once."""
    f64 = torch.float64
    if mean.dim() != 2 or tuple(scatter.shape) != (mean.shape[0], mean.shape[1], mean.shape[1]):
        raise _hip.HipExtensionError(f"position_gaussian_factor: mean {tuple(mean.shape)} and scatter {tuple(scatter.shape)} are not "
                                     f"[P][d] and [P][d][d]")
    P, d = (int(v) for v in mean.shape)
    mu_hi, mu_lo, w = _new((P, d), mean), _new((P, d), mean), _new((P, d, d), mean)
    c64 = torch.empty((P, d, d), device=mean.device, dtype=f64) if want64 else None
    w64 = torch.empty((P, d, d), device=mean.device, dtype=f64) if want64 else None
    info = torch.empty((P,), device=mean.device, dtype=torch.int32)
    _run("position_gaussian_factor", 2.0 * P * d ** 3 / 3, 8.0 * P * d * (d + 1) + 4.0 * P * d * d + (16.0 * P * d * d if want64 else 0.0),
         lambda: _hip.lib().ssad_position_gaussian_factor(_hip.ptr(mean, dtype=f64), _hip.ptr(scatter, dtype=f64), P, d, int(n),
                                                          float(eps), _hip.ptr(mu_hi), _hip.ptr(mu_lo), _hip.ptr(w),
                                                          _hip.ptr(c64, True, f64), _hip.ptr(w64, True, f64),
                                                          _hip.ptr(info, dtype=torch.int32), _hip.stream()))
    bad = torch.nonzero(info)
    if bad.numel():
        p = int(bad[0])
        raise ValueError(f"the covariance of position {p} is not positive definite: pivot {int(info[p]) - 1} is not finite and "
                         f"positive ({int(bad.numel())} of {P} positions failed)")
    return (mu_hi, mu_lo, w, c64, w64) if want64 else (mu_hi, mu_lo, w)


def position_mahalanobis(x, sel, mu_hi, mu_lo, w, n_img, P, sel_dev=None, out=None):
    """x [n_img * P][D] fp32 -> [n_img * P] ||W_p (x[n P + p][sel] - mu_p)||_2 with mu = mu_hi + mu_lo ([P][d] fp32 pairs) and
    W [P][d][d] lower triangular, one kernel (csrc/padim.hip).  FLOPs: the dense 2 n P d^2 (the kernel skips W's zero blocks); bytes:
    every row of x (d random columns of D touch all its 128-byte lines) plus W and the means once."""
    D = _position_shape(x, n_img, P)
    sd = position_sel(sel, D, x.device) if sel_dev is None else sel_dev
    d = int(sd.numel())
    if tuple(mu_hi.shape) != (P, d) or tuple(mu_lo.shape) != (P, d) or tuple(w.shape) != (P, d, d):
        raise _hip.HipExtensionError(f"position_mahalanobis: mu_hi {tuple(mu_hi.shape)}, mu_lo {tuple(mu_lo.shape)}, w "
                                     f"{tuple(w.shape)} do not match P = {P}, d = {d}")
    if out is None:
        out = _new((n_img * P,), x)
    elif tuple(out.shape) != (n_img * P,):
        raise _hip.HipExtensionError(f"position_mahalanobis: out is {tuple(out.shape)}, expected {(n_img * P,)}")
    _run("position_mahalanobis", 2.0 * n_img * P * d * d, 4.0 * (x.numel() + w.numel() + 2 * P * d + n_img * P),
         lambda: _hip.lib().ssad_position_mahalanobis(_hip.ptr(x), _hip.ptr(sd, dtype=torch.int32), _hip.ptr(mu_hi), _hip.ptr(mu_lo),
                                                      _hip.ptr(w), _hip.ptr(out), n_img, P, D, d, _hip.stream()))
    return out


def blur_relu_bilinear(maps, ksize=7, target=256):
    n, c, h, w = maps.shape
    out = _new((n, c, target, target), maps)
    _run("blur_relu_bilinear", 0.0, 4.0 * (maps.numel() + out.numel()),
         lambda: _hip.lib().ssad_blur_relu_bilinear(_hip.ptr(maps), _hip.ptr(out), n * c, h, w, ksize, target, _hip.stream()))
    return out


# ---- resize, then Gaussian (csrc/resize_gaussian.hip): the anomaly map of PatchCore and PaDiM as one banded operator per axis ----
RESIZE_GAUSSIAN_BORDERS = ('symmetric', 'reflect')
_RESIZE_GAUSSIAN_TABLES = {}


def _resize_gaussian_matrix(extent, T, sigma, border):
    """A = G R in float64, [T][extent]: R the bilinear matrix of F.interpolate(align_corners=False), G the Gaussian of
    scipy.ndimage.gaussian_filter (radius int(4 sigma + 0.5)) with its border folded back into [0, T)."""
    import numpy as np
    d = np.arange(T)
    src = np.maximum((d + 0.5) * extent / T - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), extent - 1)
    i1 = np.minimum(i0 + 1, extent - 1)
    lam = src - i0
    R = np.zeros((T, extent))
    np.add.at(R, (d, i0), 1.0 - lam)
    np.add.at(R, (d, i1), lam)
    r = int(4.0 * sigma + 0.5)
    k = np.arange(-r, r + 1)
    taps = np.exp(-0.5 * (k / sigma) ** 2)
    taps /= taps.sum()
    j = d[:, None] + k[None, :]
    if border == 'symmetric':                                   # b a | a b: scipy.ndimage mode='reflect'
        j = np.where(j < 0, -j - 1, np.where(j >= T, 2 * T - 1 - j, j))
    else:                                                       # c b | a b c: torch / kornia reflect padding
        j = np.where(j < 0, -j, np.where(j >= T, 2 * T - 2 - j, j))
    G = np.zeros((T, T))
    np.add.at(G, (np.repeat(d, k.size), j.reshape(-1)), np.tile(taps, T))
    return G @ R


def resize_gaussian_operator(h, T, sigma=4.0, border='symmetric', device=None):
    """Band form of A = G R for one axis of `h` source cells and `T` output pixels: (first int32 [T], weights fp32 [T][K], K) --
    row d of A is weights[d] at source indices first[d] .. first[d] + K - 1, built in float64, rounded once, zero-padded.  Cached
    per (h, T, sigma, border, device); device None keeps the tables on the host."""
    import numpy as np
    h, T, sigma = int(h), int(T), float(sigma)
    if not sigma > 0.0:
        raise ValueError(f"resize_gaussian: sigma must be positive, got {sigma!r}")
    if border not in RESIZE_GAUSSIAN_BORDERS:
        raise ValueError(f"resize_gaussian: border is 'symmetric' (scipy.ndimage) or 'reflect' (torch / kornia), got {border!r}")
    if h < 1 or T < 1:
        raise ValueError(f"resize_gaussian: sizes must be positive, got {h} -> {T}")
    if int(4.0 * sigma + 0.5) >= T:
        raise ValueError(f"resize_gaussian: the radius int(4 sigma + 0.5) = {int(4.0 * sigma + 0.5)} must be below the target size {T}")
    key = (h, T, sigma, border, None if device is None else str(torch.device(device)))
    t = _RESIZE_GAUSSIAN_TABLES.get(key)
    if t is None:
        A = _resize_gaussian_matrix(h, T, sigma, border)
        nz = A != 0.0
        lo = nz.argmax(axis=1)
        hi = h - 1 - nz[:, ::-1].argmax(axis=1)
        K = int((hi - lo + 1).max())
        first = np.minimum(lo, h - K)
        weights = A[np.arange(T)[:, None], first[:, None] + np.arange(K)[None, :]].astype(np.float32)
        first_t, weights_t = torch.from_numpy(first.astype(np.int32)), torch.from_numpy(weights)
        if device is not None:
            first_t, weights_t = first_t.to(device), weights_t.to(device)
        t = _RESIZE_GAUSSIAN_TABLES[key] = (first_t, weights_t, K)
    return t


def resize_gaussian(maps, target, sigma=4.0, border='symmetric'):
    """maps [n][1][h][w] or [n][h][w] (float, on the device) -> [n][1][target][target] fp32: bilinear resize (align_corners=False),
    then the Gaussian of `sigma` output pixels -- scipy.ndimage.gaussian_filter with border='symmetric' (the PatchCore / PaDiM
    code), torch reflect padding with border='reflect' (anomalib) -- as out = A_y M A_x^T in one launch."""
    target = int(target)
    if not (torch.is_tensor(maps) and maps.is_floating_point() and (maps.dim() == 3 or (maps.dim() == 4 and maps.shape[1] == 1))
            and maps.numel() > 0):
        raise ValueError(f"resize_gaussian: float maps [n][1][h][w] or [n][h][w], got "
                         f"{tuple(maps.shape) if torch.is_tensor(maps) else type(maps)}")
    n, h, w = maps.shape[0], maps.shape[-2], maps.shape[-1]
    resize_gaussian_operator(h, target, sigma, border)          # the ValueErrors, before anything touches the device
    if not maps.is_cuda:
        raise RuntimeError("resize_gaussian needs GPU tensors (csrc/resize_gaussian.hip; there is no CPU fallback)")
    m = maps.detach().reshape(n, h, w).float().contiguous()
    yf, yw, ky = resize_gaussian_operator(h, target, sigma, border, m.device)
    xf, xw, kx = (yf, yw, ky) if w == h else resize_gaussian_operator(w, target, sigma, border, m.device)
    out = _new((n, 1, target, target), m)
    _run("resize_gaussian", 0.0, 4.0 * (m.numel() + out.numel()),
         lambda: _hip.lib().ssad_resize_gaussian(_hip.ptr(m), n, h, w, _hip.ptr(yf, dtype=torch.int32), _hip.ptr(yw), ky,
                                                 _hip.ptr(xf, dtype=torch.int32), _hip.ptr(xw), kx, target, 0, _hip.ptr(out),
                                                 _hip.stream()))
    return out


_RESAMPLE_TABLES = {}


def _resample_tables(n_in, n_out, device):
    """Device copies of Pillow's per-axis resampling tables, one pair per (input extent, output extent, device)."""
    key = (n_in, n_out, str(device))
    t = _RESAMPLE_TABLES.get(key)
    if t is None:
        from .pil_exact import resample_coeffs
        ks, bounds, kk = resample_coeffs(n_in, n_out)
        t = _RESAMPLE_TABLES[key] = (ks, torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device))
    return t


def resize_bicubic_u8(img, size):
    """Pillow's ``Image.resize(size)`` (BICUBIC) on a uint8 batch [B][Hin][Win][C] (C = 1: mode 'L', 3: 'RGB') that lives on the
    device; size = (width, height) as PIL takes it.  Bit-exact (csrc/resize.hip); same size = the input itself, as PIL copies."""
    b, hin, win, c = img.shape
    wout, hout = int(size[0]), int(size[1])
    if (hin, win) == (hout, wout):
        return img
    if b == 0:
        return torch.empty((0, hout, wout, c), dtype=torch.uint8, device=img.device)
    assert img.dtype == torch.uint8 and img.is_cuda and img.is_contiguous()
    out = torch.empty((b, hout, wout, c), dtype=torch.uint8, device=img.device)
    kx = ky = (0, None, None)
    if win != wout:
        kx = _resample_tables(win, wout, img.device)
    if hin != hout:
        ky = _resample_tables(hin, hout, img.device)
    tmp = torch.empty((b, hin, wout, c), dtype=torch.uint8, device=img.device) if (win != wout and hin != hout) else None
    p = lambda t: None if t is None else t.data_ptr()
    _run("resize_bicubic", 0.0, float(img.numel() + out.numel() + (2 * tmp.numel() if tmp is not None else 0)),
         lambda: _hip.lib().ssad_resize_bicubic_u8(img.data_ptr(), p(tmp), out.data_ptr(), b, hin, win, c, hout, wout,
                                                   p(kx[1]), p(kx[2]), kx[0], p(ky[1]), p(ky[2]), ky[0], _hip.stream()))
    return out


def obj_mask_batch(rgb, sigma=1.5, low=5, high=15, chunk=64, return_edges=False):
    """dataset_generator.obj_mask for a uint8 RGB batch [B][H][W][3] on the device -> bool [B][H][W] (csrc/objmask.hip; bit-exact
    against the host statement).  The Gaussian weights are scipy.ndimage's (numpy's exp on the host), everything per pixel runs on
    the device.  return_edges: also the Canny edge maps."""
    import ctypes
    import numpy as np
    assert rgb.dtype == torch.uint8 and rgb.is_cuda and rgb.is_contiguous() and rgb.shape[-1] == 3
    b, h, w, _ = rgb.shape
    radius = int(4.0 * float(sigma) + 0.5)                       # scipy.ndimage.gaussian_filter1d: truncate = 4
    xs = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * xs ** 2)
    phi = (phi / phi.sum())[::-1].copy()
    wts = (ctypes.c_double * len(phi))(*phi.tolist())
    lib = _hip.lib()
    mask = torch.empty((b, h, w), dtype=torch.uint8, device=rgb.device)
    edges = torch.empty((b, h, w), dtype=torch.uint8, device=rgb.device)
    for s in range(0, b, chunk):
        e = min(b, s + chunk)
        ws = torch.empty(lib.ssad_obj_mask_workspace(e - s, h, w), dtype=torch.uint8, device=rgb.device)
        _hip.check(lib.ssad_obj_mask(rgb[s:e].data_ptr(), mask[s:e].data_ptr(), edges[s:e].data_ptr(), e - s, h, w, wts, radius,
                                     low / 255.0, high / 255.0, ws.data_ptr(), _hip.stream()))
        torch.cuda.current_stream().synchronize()               # the weights live in this frame: the upload must have happened
    return (mask.bool(), edges.bool()) if return_edges else mask.bool()


# ---- defect regions (csrc/regions.hip): integers only, bit-equal to scipy.ndimage on the host ----
REGION_TILE = 32      # tile side of the labelling kernel (ssad_label_regions_tile()): sizes around its multiples are the ragged cases


def _regions_dev(t, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{name} needs GPU tensors (csrc/regions.hip; scipy.ndimage.label is the host statement)")
    return t


def _regions_3d(x, name):
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 3 or 0 in x.shape:
        raise ValueError(f"{name}: expected [n][H][W] or [n][1][H][W] with n, H, W >= 1, got {tuple(x.shape)}")
    return x.contiguous()


def label_regions(x, threshold=None, connectivity=8):
    """Connected components of a batch of binary images on the device.  x [n][H][W] or [n][1][H][W]: a float tensor with a
    `threshold` (foreground = x >= threshold; NaN is background) or a bool / uint8 mask (foreground = nonzero).  Returns
    (labels int32 [n][H][W], counts int32 [n], offsets int32 [n + 1]); labels equals scipy.ndimage.label's array (8: 3 x 3 ones,
    4: the cross), components numbered 1 .. counts[i] per image."""
    _regions_dev(x, "label_regions")
    if connectivity not in (4, 8):
        raise ValueError(f"label_regions: connectivity is 4 or 8, got {connectivity!r}")
    x = _regions_3d(x, "label_regions")
    scores = mask = None
    if x.is_floating_point():
        if threshold is None:
            raise ValueError("label_regions: a float tensor needs a threshold")
        scores, thr = x.float().contiguous(), float(threshold)
    elif x.dtype in (torch.bool, torch.uint8):
        if threshold is not None:
            raise ValueError("label_regions: a mask takes no threshold")
        mask, thr = x.to(torch.uint8).contiguous(), 0.0
    else:
        raise ValueError(f"label_regions: float scores or a bool / uint8 mask, got {x.dtype}")
    n, h, w = x.shape
    lib = _hip.lib()
    labels = torch.empty((n, h, w), dtype=torch.int32, device=x.device)
    counts = torch.empty(n, dtype=torch.int32, device=x.device)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=x.device)
    nbytes = lib.ssad_label_regions_workspace(n, h, w)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    _run("label_regions", 0.0, 5.0 * n * h * w,
         lambda: lib.ssad_label_regions(None if scores is None else scores.data_ptr(), thr, None if mask is None else mask.data_ptr(),
                                        n, h, w, connectivity, labels.data_ptr(), counts.data_ptr(), offsets.data_ptr(), ws.data_ptr(),
                                        nbytes, _hip.stream()))
    return labels, counts, offsets


def _regions_args(labels, offsets, name):
    _regions_dev(labels, name)
    _regions_dev(offsets, name)
    labels = _regions_3d(labels, name)
    n, h, w = labels.shape
    if labels.dtype != torch.int32 or offsets.dtype != torch.int32 or offsets.numel() != n + 1 or not offsets.is_contiguous():
        raise ValueError(f"{name}: labels int32 [n][H][W] and offsets int32 [n + 1] as label_regions returns them")
    return labels, n, h, w


def region_stats(labels, offsets, scores=None, num_regions=None):
    """Per region, in (image, label) order, as device tensors: area int32 [R], bbox int32 [R][4] (x0, y0, x1, y1, maxima
    inclusive), coord_sum int64 [R][2] (sum of x, sum of y) and, with `scores` [n][H][W], peak fp32 [R] and peak_pos int32 [R]
    (the smallest raster index within the image that attains the peak); without scores the last two are None.  R = offsets[n]
    is read back once unless `num_regions` passes it."""
    labels, n, h, w = _regions_args(labels, offsets, "region_stats")
    r = int(offsets[n].item()) if num_regions is None else int(num_regions)
    dev = labels.device
    area = torch.empty(r, dtype=torch.int32, device=dev)
    bbox = torch.empty((r, 4), dtype=torch.int32, device=dev)
    csum = torch.empty((r, 2), dtype=torch.int64, device=dev)
    peak = pos = None
    if scores is not None:
        scores = _regions_3d(_regions_dev(scores, "region_stats"), "region_stats").float().contiguous()
        if scores.shape != labels.shape:
            raise ValueError("region_stats: scores and labels differ in shape")
        peak = torch.empty(r, dtype=torch.float32, device=dev)
        pos = torch.empty(r, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    _run("region_stats", 0.0, 8.0 * labels.numel(),
         lambda: _hip.lib().ssad_region_stats(p(scores), labels.data_ptr(), offsets.data_ptr(), n, h, w, r, area.data_ptr(),
                                              bbox.data_ptr(), csum.data_ptr(), p(peak), p(pos), _hip.stream()))
    return area, bbox, csum, peak, pos


def region_filter(labels, offsets, keep, renumber=True):
    """Keeps the regions r with keep[r] != 0 (keep: bool / uint8 [R] on the device).  Returns mask uint8 [n][H][W] and, when
    `renumber`, (mask, labels_out, counts_out, offsets_out) with the kept regions numbered 1 .. per image in the same order."""
    labels, n, h, w = _regions_args(labels, offsets, "region_filter")
    keep = _regions_dev(keep, "region_filter").reshape(-1).to(torch.uint8).contiguous()
    r = keep.numel()
    dev = labels.device
    lib = _hip.lib()
    mask = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    lab2 = cnt2 = off2 = ws = None
    nbytes = 0
    if renumber:
        lab2 = torch.empty((n, h, w), dtype=torch.int32, device=dev)
        cnt2 = torch.empty(n, dtype=torch.int32, device=dev)
        off2 = torch.empty(n + 1, dtype=torch.int32, device=dev)
        nbytes = lib.ssad_region_filter_workspace(r)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    _run("region_filter", 0.0, 9.0 * labels.numel(),
         lambda: lib.ssad_region_filter(labels.data_ptr(), offsets.data_ptr(), p(keep) if r else None, n, h, w, r, mask.data_ptr(),
                                        p(lab2), p(cnt2), p(off2), p(ws), nbytes, _hip.stream()))
    return (mask, lab2, cnt2, off2) if renumber else mask


def pro_weights(labels, offsets, area):
    """The two weight planes of the PRO curve from labelled ground truths: fp_w uint8 [n * H * W] = (label == 0) and pro_w fp64 =
    1.0 / area of the pixel's region, 0 on background -- bit-equal to what metrics.compute_pro_gpu builds in numpy."""
    labels, n, h, w = _regions_args(labels, offsets, "pro_weights")
    area = _regions_dev(area, "pro_weights")
    if area.dtype != torch.int32 or not area.is_contiguous():
        raise ValueError("pro_weights: area int32 [R] as region_stats returns it")
    fp_w = torch.empty(labels.numel(), dtype=torch.uint8, device=labels.device)
    pro_w = torch.empty(labels.numel(), dtype=torch.float64, device=labels.device)
    _run("pro_weights", 0.0, 13.0 * labels.numel(),
         lambda: _hip.lib().ssad_pro_weights(labels.data_ptr(), offsets.data_ptr(), area.data_ptr(), n, h, w, fp_w.data_ptr(),
                                             pro_w.data_ptr(), _hip.stream()))
    return fp_w, pro_w


def gradcam_map(act, alpha):
    """act NHWC [B][U][V][C], alpha [B][C] (may be a column slice of a wider matrix) -> [B][1][U][V] weighted sums."""
    b, u, v, c = act.shape
    assert alpha.shape == (b, c) and alpha.stride(1) == 1 and (b == 1 or alpha.stride(0) >= c)
    assert alpha.is_cuda and alpha.dtype == torch.float32         # rows may be strided (a slice): _hip.ptr would refuse them
    out = _new((b, 1, u, v), act)
    _run("gradcam_map", 2.0 * act.numel(), 4.0 * act.numel(),
         lambda: _hip.lib().ssad_gradcam_map(_hip.ptr(act), alpha.data_ptr(), _hip.ptr(out), b, u * v, c, max(alpha.stride(0), c),
                                             _hip.stream()))
    return out


# ---------------------------------------------------------------------------------------------
# training kernels
# ---------------------------------------------------------------------------------------------
def flip_transpose_weight(w_ohwi):
    o, kh, kw, i = w_ohwi.shape
    out = _new((i, kh, kw, o), w_ohwi)
    _hip.check(_hip.lib().ssad_flip_transpose_weight(_hip.ptr(w_ohwi), _hip.ptr(out), o, i, kh, kw, _hip.stream()))
    return out


def conv_dgrad(dy, w_flipT, x_shape, stride, pad, residual=None, bf16=False, res_mask=None):
    """dy NHWC [N][Hy][Wy][Cout]; w_flipT [Cin][KH][KW][Cout] -> dx NHWC of x_shape (+ residual [under res_mask])."""
    n, hy, wy, cout = dy.shape
    cin, kh, kw, _ = w_flipT.shape
    assert residual is None or tuple(residual.shape) == tuple(x_shape), "residual must have dx's shape"
    assert tuple(x_shape) == (n, x_shape[1], x_shape[2], cin) and w_flipT.shape[-1] == cout
    if _is_h(dy):
        assert _is_h(w_flipT) and bf16 == 2 and res_mask is None and (residual is None or _is_h(residual))
        dx = _newh(tuple(x_shape), dy)
        _run("conv_igemm_h16", 2.0 * dx.numel() * kh * kw * cout / (stride * stride),
             2.0 * (dy.numel() + dx.numel() * (2 if residual is not None else 1) + w_flipT.numel()),
             lambda: _hip.lib().ssad_conv_igemm_dgrad_h(dy.data_ptr(), w_flipT.data_ptr(), dx.data_ptr(), _p(residual, True), n, hy, wy,
                                                        cout, x_shape[1], x_shape[2], cin, kh, kw, stride, pad, _hip.stream()))
        return dx
    dx = _new(tuple(x_shape), dy)
    if res_mask is not None:
        assert not bf16 and residual is not None
        _run("conv_igemm_f32", 2.0 * dx.numel() * kh * kw * cout / (stride * stride),
             4.0 * (dy.numel() + dx.numel() * 2 + w_flipT.numel()),
             lambda: _hip.lib().ssad_conv_igemm_dgrad_masked(_hip.ptr(dy), _hip.ptr(w_flipT), _hip.ptr(dx), _hip.ptr(residual),
                                                             res_mask.data_ptr(), n, hy, wy, cout, x_shape[1], x_shape[2], cin, kh,
                                                             kw, stride, pad, _hip.stream()),
             tile=lambda: igemm_tile_name(n, x_shape[1], x_shape[2], cin, cout, kh, kw, stride, pad, IGEMM_DGRAD))
        return dx
    fn = (_hip.lib().ssad_conv_igemm_dgrad_x6 if bf16 == 6 else _hip.lib().ssad_conv_igemm_dgrad_x3 if bf16 == 3 else
          _hip.lib().ssad_conv_igemm_dgrad_f16 if bf16 == 2 else
          _hip.lib().ssad_conv_igemm_dgrad_bf16 if bf16 else _hip.lib().ssad_conv_igemm_dgrad)
    _run(_kname("conv_igemm", bf16),
         2.0 * dx.numel() * kh * kw * cout / (stride * stride),
         4.0 * (dy.numel() + dx.numel() * (2 if residual is not None else 1) + w_flipT.numel()),
         lambda: fn(_hip.ptr(dy), _hip.ptr(w_flipT), _hip.ptr(dx), _hip.ptr(residual, True), n, hy, wy, cout, x_shape[1],
                    x_shape[2], cin, kh, kw, stride, pad, _hip.stream()),
         tile=None if bf16 else (lambda: igemm_tile_name(n, x_shape[1], x_shape[2], cin, cout, kh, kw, stride, pad, IGEMM_DGRAD)))
    return dx


# Weight-gradient paths (ssad_wgrad_variant_id, include/ssad.h): the instantiation a path's launcher runs
WGRAD_GENERIC, WGRAD_HALO, WGRAD_HALO16, WGRAD_G16, WGRAD_STEM = range(5)
_WGRAD_TILES = {416: "4x16", 808: "8x8", 408: "4x8", 216: "2x16"}       # TH * 100 + TW of the output-pixel tile
_WGRAD_MODES = {0: "f32", 1: "bf16", 2: "f16", 3: "x3", 6: "x6"}
STEM_WGRAD_KERNELS = ("float", "hf", "f16")     # stem_wgrad_kernel<float>, stem_wgrad_kernel<hf>, stem_wgrad16_kernel


def wgrad_path(dy_shape, x_shape, kh, kw, stride, pad, bf16=False, half=False, force_x6=False, kreal=None):
    """(path, instantiation, splits) of the launch conv_wgrad makes for dy NHWC dy_shape, x NHWC x_shape (half: both stored as
    halves) -- conv_wgrad takes its branch from here.  Paths: linear_small (instantiation = operand rounding f32 / bf16 / f16, no slab:
    splits 0); halo_s1 / halo_s2 (fp32 tensors), halo16_bf16 / halo16_f16 (fp32 tensors, 16-bit operands), halo16_h, g16_s1 / g16_s2
    (half tensors): the output-pixel tile TH x TW; generic_f32 / _bf16 / _f16 / _x3 / _x6 / _f16_h: the channel tile BT64 / BT128.
    splits = the slab count the reduction sums.  Host-only (no GPU needed)."""
    lib = _hip.lib()
    n, h, w, cin = (int(v) for v in x_shape)
    ho, wo, cout = int(dy_shape[1]), int(dy_shape[2]), int(dy_shape[-1])
    m = n * ho * wo
    mode = 0 if int(bf16) == 6 and not force_x6 else int(bf16)     # (bf16x6 training: see the generic branch of conv_wgrad)
    tile = lambda path: _WGRAD_TILES[lib.ssad_wgrad_variant_id(path, wo, cin, cout, stride, 0)]
    bt = lambda: "BT%d" % lib.ssad_wgrad_variant_id(WGRAD_GENERIC, wo, cin, cout, stride, 0)
    if half:
        assert mode == 2 and kreal is None, "half tensors go with fp16 operands"
        if lib.ssad_wgrad3x3_g16_ok(cin, cout, kh, kw, stride, pad):
            return "g16_s%d" % stride, tile(WGRAD_G16), lib.ssad_wgrad3x3_g16_splits(n, ho, wo, cin, cout, stride)
        if lib.ssad_wgrad3x3_halo16_ok(cin, cout, kh, kw, stride, pad):
            return "halo16_h", tile(WGRAD_HALO16), lib.ssad_wgrad3x3_halo16_splits(n, h, w, cin, cout)
        return "generic_f16_h", bt(), lib.ssad_wgrad_splits_bf16(m, cin, cout, kh, kw)
    if mode in (0, 1, 2) and kreal is None and kh == kw == h == w == 1 and m <= lib.ssad_linear_small_max_rows():
        return "linear_small", _WGRAD_MODES[mode], 0
    if mode == 0 and kreal is None and os.environ.get("SSAD_WGRAD_HALO", "1") != "0":
        halo = lib.ssad_wgrad3x3_halo_ok(cin, cout, kh, kw, stride, pad)
        if halo:
            return "halo_s%d" % halo, tile(WGRAD_HALO), lib.ssad_wgrad3x3_halo_splits(n, ho, wo, cin, cout)
    if mode in (1, 2) and kreal is None and lib.ssad_wgrad3x3_halo16_ok(cin, cout, kh, kw, stride, pad):
        return "halo16_" + _WGRAD_MODES[mode], tile(WGRAD_HALO16), lib.ssad_wgrad3x3_halo16_splits(n, h, w, cin, cout)
    splits = (lib.ssad_wgrad_splits_bf16 if mode else lib.ssad_wgrad_splits)(m, cin, cout, kh, kw)
    return "generic_" + _WGRAD_MODES[mode], bt(), splits


def conv_wgrad(dy, x, dw_out, kh, kw, stride, pad, kreal=None, to_oihw=False, accumulate=False, bf16=False, force_x6=False):
    """dy NHWC [N][Ho][Wo][Cout], x NHWC [N][H][W][Cin] -> dw_out (flat, Cout*KH*KW*Cin_real floats).
    kreal = (KH, KW, Cin) of the real filter when x rows are padded im2col rows (stem).  The launch is wgrad_path's."""
    n, h, w, cin = x.shape
    cout = dy.shape[-1]
    m = dy.numel() // cout
    lib = _hip.lib()
    assert tuple(dy.shape[:-1]) == (n, (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1), \
        f"dy {tuple(dy.shape)} is not the output of a {kh} x {kw} / stride {stride} / pad {pad} conv over x {tuple(x.shape)}"
    if _is_h(dy):
        assert _is_h(x) and bf16 == 2 and kreal is None
    path, _, splits = wgrad_path(dy.shape, x.shape, kh, kw, stride, pad, bf16, _is_h(dy), force_x6, kreal)
    if bf16 == 6 and not force_x6:
        # bf16x6 training keeps weight gradients on the exact fp32 kernel: the wave-specialised fp32 wgrad (110 TFLOP/s) is
        # as fast as the six-product bf16 form (measured), and exact; ssad_conv_wgrad_x6 stays available (tests)
        bf16 = False
    if path.startswith("g16_"):
        # precision-16 step with half tensors: 3 x 3 / pad 1, stride 1 or 2: tiles staged as they lie in memory, transposed by the
        # fragment reads (csrc/wgrad16.hip)
        ho, wo = dy.shape[1], dy.shape[2]
        slab = _new((splits, cout, 9 * cin), dy)
        _run("wgrad_g16", 2.0 * m * cout * 9 * cin, 2.0 * (dy.numel() + x.numel()) + 4.0 * slab.numel(),
             lambda: lib.ssad_conv_wgrad3x3_g16_h(dy.data_ptr(), x.data_ptr(), _hip.ptr(slab), splits, n, ho, wo, h, w, cin, cout,
                                                  stride, dy.numel(), _hip.stream()))
    elif path == "halo16_h":
        slab = _new((splits, cout, 9 * cin), dy)
        _run("wgrad_h16", 2.0 * m * cout * 9 * cin, 2.0 * (dy.numel() + x.numel()) + 4.0 * slab.numel(),
             lambda: lib.ssad_conv_wgrad3x3_halo16_h(dy.data_ptr(), x.data_ptr(), _hip.ptr(slab), splits, n, h, w, cin, cout,
                                                     dy.numel(), _hip.stream()))
    elif path == "generic_f16_h":
        # the same 16-bit split kernel as the fp16-operand form, its operands read as the halves they are stored as
        slab = _new((splits, cout, kh * kw * cin), dy)
        _run("wgrad_h16", 2.0 * m * cout * kh * kw * cin, 2.0 * (dy.numel() + x.numel()) * kh * kw + 4.0 * slab.numel(),
             lambda: lib.ssad_conv_wgrad_f16_h(dy.data_ptr(), x.data_ptr(), _hip.ptr(slab), splits, n, h, w, cin, cout, kh, kw,
                                               stride, pad, dy.numel(), _hip.stream()))
    elif path == "linear_small":
        # linear layer over a training batch's rows: one launch straight into the gradient (OIHW == OHWI for 1 x 1); the 16-bit modes
        # round the operands while they are loaded
        _run_aside("wgrad_f32" if not bf16 else "wgrad_small16", 2.0 * m * cout * cin, 4.0 * (dy.numel() + x.numel() + cout * cin),
                   lambda: lib.ssad_linear_wgrad_small_r(_hip.ptr(dy), _hip.ptr(x), _hip.ptr(dw_out), m, cin, cout, int(accumulate), int(bf16),
                                                         _hip.stream()), keep=(dy, x))
        return dw_out
    elif path.startswith("halo_s"):
        # 3x3 / pad 1 on the exact fp32 path: halo-tile kernel (one workgroup = a 64 x 64 block, all nine taps); stride 1 or 2
        ho, wo = dy.shape[1], dy.shape[2]
        assert (ho, wo) == ((h - 1) // stride + 1, (w - 1) // stride + 1)
        slab = _new((splits, cout, 9 * cin), dy)
        if path == "halo_s1":
            fn = lambda: lib.ssad_conv_wgrad3x3_halo(_hip.ptr(dy), _hip.ptr(x), _hip.ptr(slab), splits, n, h, w, cin, cout,
                                                     dy.numel(), _hip.stream())
        else:
            fn = lambda: lib.ssad_conv_wgrad3x3s2_halo(_hip.ptr(dy), _hip.ptr(x), _hip.ptr(slab), splits, n, ho, wo, h, w, cin,
                                                       cout, dy.numel(), _hip.stream())
        _run("wgrad_f32", 2.0 * m * cout * 9 * cin, 4.0 * (dy.numel() + x.numel() + slab.numel()), fn)
    elif path.startswith("halo16_"):
        # 16-bit operands, 3x3 / stride 1 / pad 1: halo-tile kernel (dZ and X fetched, converted and transposed once per pixel tile
        # instead of once per filter tap; csrc/wgrad_halo16.hip)
        slab = _new((splits, cout, 9 * cin), dy)
        _run(_kname("wgrad", bf16), 2.0 * m * cout * 9 * cin, 4.0 * (dy.numel() + x.numel() + slab.numel()),
             lambda: lib.ssad_conv_wgrad3x3_halo16(_hip.ptr(dy), _hip.ptr(x), _hip.ptr(slab), splits, n, h, w, cin, cout,
                                                   int(bf16 == 2), dy.numel(), _hip.stream()))
    else:
        assert path.startswith("generic_"), path
        slab = _new((splits, cout, kh * kw * cin), dy)
        fn = (lib.ssad_conv_wgrad_x6 if bf16 == 6 else lib.ssad_conv_wgrad_x3 if bf16 == 3 else
              lib.ssad_conv_wgrad_f16 if bf16 == 2 else
              lib.ssad_conv_wgrad_bf16 if bf16 else lib.ssad_conv_wgrad)
        _run(_kname("wgrad", bf16), 2.0 * m * cout * kh * kw * cin,
             4.0 * (dy.numel() * kh * kw + x.numel() * kh * kw + slab.numel()),
             lambda: fn(_hip.ptr(dy), _hip.ptr(x), _hip.ptr(slab), splits, n, h, w, cin, cout, kh, kw, stride, pad, dy.numel(),
                        _hip.stream()))
        rkh, rkw, rcin = kreal if kreal else (kh, kw, cin)
        _wgrad_reduce(slab, dw_out, splits, cout, kh * kw * cin, rkh, rkw, rcin, to_oihw, accumulate)
        return dw_out
    _wgrad_reduce(slab, dw_out, splits, cout, kh * kw * cin, kh, kw, cin, to_oihw, accumulate)
    return dw_out


def stem_wgrad_path(img_shape, half=False):
    """("stem", kernel, splits) of stem_wgrad over NCHW images of img_shape with dz stored as halves (half) or floats: kernel =
    STEM_WGRAD_KERNELS[ssad_wgrad_variant_id(WGRAD_STEM, ...)], splits = the per-workgroup slabs ssad_wgrad_reduce sums."""
    b, _, h, w = (int(v) for v in img_shape)
    lib = _hip.lib()
    return ("stem", STEM_WGRAD_KERNELS[lib.ssad_wgrad_variant_id(WGRAD_STEM, 0, 3, 64, 2, int(bool(half)))],
            lib.ssad_stem_wgrad_splits(b, h, w))


def stem_wgrad(img, dz, dw_out, to_oihw=False, accumulate=False):
    """Weight gradient of the stem conv from the NCHW image and dz [B][Ho][Wo][64] -> dw_out (64*147 floats)."""
    b, c, h, w = img.shape
    _, _, _, ho, wo = stem_geometry(h, w, 0, 0)
    assert c == 3 and tuple(dz.shape) == (b, ho, wo, 64), f"dz {tuple(dz.shape)} does not belong to images {tuple(img.shape)}"
    lib = _hip.lib()
    _, kernel, _ = stem_wgrad_path(img.shape, _is_h(dz))
    ws = torch.empty(lib.ssad_stem_wgrad_workspace(b, h, w), device=img.device, dtype=torch.float32)
    if kernel != "float":
        _run("stem_wgrad_h16", 2.0 * dz.numel() * 147, 2.0 * dz.numel() + 4.0 * img.numel() * 1.6,
             lambda: lib.ssad_stem_wgrad_h(_hip.ptr(img), dz.data_ptr(), _hip.ptr(dw_out), b, h, w, dz.numel(), int(to_oihw), int(accumulate),
                                           _hip.ptr(ws), _hip.stream()))
        return dw_out
    _run("stem_wgrad", 2.0 * dz.numel() * 147, 4.0 * (dz.numel() + img.numel() * 1.6),
         lambda: lib.ssad_stem_wgrad(_hip.ptr(img), _hip.ptr(dz), _hip.ptr(dw_out), b, h, w, dz.numel(), int(to_oihw), int(accumulate),
                                     _hip.ptr(ws), _hip.stream()))
    return dw_out


def stem_im2col(img, hv, wv):
    b, c, h, w = img.shape
    ho, wo = (hv - 1) // 2 + 1, (wv - 1) // 2 + 1
    col = _new((b, ho, wo, 160), img)
    _run("stem_im2col", 0.0, 4.0 * (img.numel() + col.numel()),
         lambda: _hip.lib().ssad_stem_im2col(_hip.ptr(img), _hip.ptr(col), b, h, w, hv, wv, _hip.stream()))
    return col


def pack_stem_weight_2d(w_oihw):
    out = _new((64, 1, 1, 160), w_oihw)
    _hip.check(_hip.lib().ssad_pack_stem_weight_2d(_hip.ptr(w_oihw), _hip.ptr(out), _hip.stream()))
    return out


def _colreduce_ws(r, c, like):
    n = _hip.lib().ssad_colreduce_workspace(r, c)
    return torch.empty(n, device=like.device, dtype=torch.float64)


def bn_stats(z, c, eps, momentum, running_mean, running_var):
    r = z.numel() // c
    mean, invstd = _new((c,), z), _new((c,), z)
    ws = _colreduce_ws(r, c, z)
    fn = _hip.lib().ssad_bn_stats_h if _is_h(z) else _hip.lib().ssad_bn_stats
    _run("bn_stats", 0.0, z.element_size() * z.numel(),
         lambda: fn(_p(z), r, c, eps, momentum, _hip.ptr(mean), _hip.ptr(invstd),
                                          _hip.ptr(running_mean, True), _hip.ptr(running_var, True), ws.data_ptr(),
                                          _hip.stream()))
    return mean, invstd


def bn_small_ok(rows, c):
    return bool(_hip.lib().ssad_bn_small_ok(rows, c))


def bn_small_fwd(z, gamma, beta, eps, momentum, running_mean, running_var, relu):
    """Train-mode BatchNorm over a few hundred rows in one launch (statistics, running statistics, apply).  -> (y, mean, invstd)"""
    c = z.shape[-1]
    r = z.numel() // c
    y, mean, invstd = torch.empty_like(z), _new((c,), z), _new((c,), z)
    _run("bn_small_fwd", 0.0, 4.0 * 3 * z.numel(),
         lambda: _hip.lib().ssad_bn_small_fwd(_hip.ptr(z), _hip.ptr(gamma), _hip.ptr(beta), _hip.ptr(y), _hip.ptr(mean),
                                              _hip.ptr(invstd), _hip.ptr(running_mean, True), _hip.ptr(running_var, True), r, c,
                                              eps, momentum, int(relu), _hip.stream()))
    return y, mean, invstd


def bn_small_bwd(dy, z, mean, invstd, gamma, zmask_beta, dbeta, dgamma, dbias=None):
    """Its backward in one launch: dbeta, dgamma (and dbias = column sums of dz) written, dz returned."""
    c = z.shape[-1]
    r = z.numel() // c
    dz = torch.empty_like(dy)
    _run("bn_small_bwd", 0.0, 4.0 * 5 * z.numel(),
         lambda: _hip.lib().ssad_bn_small_bwd(_hip.ptr(dy), _hip.ptr(z), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma),
                                              _hip.ptr(zmask_beta, True), _hip.ptr(dbeta, True), _hip.ptr(dgamma, True),
                                              _hip.ptr(dbias, True), _hip.ptr(dz), r, c, _hip.stream()))
    return dz


def bn_apply_fwd(z, mean, invstd, gamma, beta, residual, relu):
    c = mean.numel()
    y = torch.empty_like(z)
    assert residual is None or (residual.dtype == z.dtype and residual.shape == z.shape), "residual must have z's shape"
    assert z.shape[-1] == c
    fn = _hip.lib().ssad_bn_apply_fwd_h if _is_h(z) else _hip.lib().ssad_bn_apply_fwd
    _run("bn_apply_fwd_h16" if _is_h(z) else "bn_apply_fwd", 0.0, z.element_size() * z.numel() * (3 if residual is not None else 2),
         lambda: fn(_p(z), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(beta),
                    _p(residual, True), _p(y), z.numel() // c, c, int(relu), _hip.stream()))
    return y


def bn_bwd_reduce(dy, yact, z, mean, invstd, dbeta, dgamma, c):
    r = dy.numel() // c
    ws = _colreduce_ws(r, c, dy)
    assert all(t is None or (t.dtype == dy.dtype and t.shape == dy.shape) for t in (yact, z)), "dy, yact, z must share one shape"
    fn = _hip.lib().ssad_bn_bwd_reduce_h if _is_h(dy) else _hip.lib().ssad_bn_bwd_reduce
    _run("bn_bwd_reduce_h16" if _is_h(dy) else "bn_bwd_reduce", 0.0, dy.element_size() * dy.numel() * (1 + (yact is not None) + (z is not None)),
         lambda: fn(_p(dy), _p(yact, True), _p(z, True), _hip.ptr(mean, True),
                                               _hip.ptr(invstd, True), _hip.ptr(dbeta, True), _hip.ptr(dgamma, True), r, c,
                                               ws.data_ptr(), _hip.stream()))


def bn_apply_bwd(dy, yact, z, mean, invstd, gamma, dbeta, dgamma, want_dres, eval_mode=False):
    c = mean.numel()
    dz = torch.empty_like(dy)
    dres = torch.empty_like(dy) if want_dres else None
    assert all(t is None or (t.dtype == dy.dtype and t.shape == dy.shape) for t in (yact, z)), "dy, yact, z must share one shape"
    assert dy.shape[-1] == c
    fn = _hip.lib().ssad_bn_apply_bwd_h if _is_h(dy) else _hip.lib().ssad_bn_apply_bwd
    _run("bn_apply_bwd_h16" if _is_h(dy) else "bn_apply_bwd", 0.0, dy.element_size() * dy.numel() * (3 + (yact is not None) + want_dres),
         lambda: fn(_p(dy), _p(yact, True), _p(z, True), _hip.ptr(mean),
                    _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(dbeta, True), _hip.ptr(dgamma, True),
                    _p(dz), _p(dres, True), dy.numel() // c, c, int(eval_mode), _hip.stream()))
    return dz, dres


def bn_bwd_zmask(dy, z, mean, invstd, gamma, beta, dbeta, dgamma):
    """BatchNorm(train) + ReLU backward with the mask recomputed from z (no residual): returns dz."""
    c = mean.numel()
    r = dy.numel() // c
    ws = _colreduce_ws(r, c, dy)
    lib = _hip.lib()
    assert z.dtype == dy.dtype and z.shape == dy.shape, "dy and z must share one shape"
    half = _is_h(dy)
    es = dy.element_size()
    f_red = lib.ssad_bn_bwd_reduce_zmask_h if half else lib.ssad_bn_bwd_reduce_zmask
    f_app = lib.ssad_bn_apply_bwd_zmask_h if half else lib.ssad_bn_apply_bwd_zmask
    _run("bn_bwd_reduce_h16" if half else "bn_bwd_reduce", 0.0, 2.0 * es * dy.numel(),
         lambda: f_red(_p(dy), _p(z), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma),
                       _hip.ptr(beta), _hip.ptr(dbeta), _hip.ptr(dgamma), r, c, ws.data_ptr(), _hip.stream()))
    dz = torch.empty_like(dy)
    _run("bn_apply_bwd_h16" if half else "bn_apply_bwd", 0.0, 3.0 * es * dy.numel(),
         lambda: f_app(_p(dy), _p(z), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma),
                       _hip.ptr(beta), _hip.ptr(dbeta), _hip.ptr(dgamma), _p(dz), r, c, _hip.stream()))
    return dz


def bn_relu_maxpool_fwd(z, mean, invstd, gamma, beta, winners=False):
    """Training stem tail: pooled = maxpool3x3s2(relu(bn(z))) + argmax slots, without storing the activation.  winners: also the raw z of
    each window's winner ([N][Ho][Wo][C]): pool_bn_relu_bwd then takes the BatchNorm reduction over the pooled tensors."""
    n, h, w, c = z.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    idx = torch.empty((n, ho, wo, c), device=z.device, dtype=torch.uint8)
    half = _is_h(z)
    out = _newh((n, ho, wo, c), z) if half else _new((n, ho, wo, c), z)
    zw = torch.empty_like(out) if winners else None
    lib = _hip.lib()
    eb = z.element_size()
    if winners:
        fn = lib.ssad_bn_relu_maxpool_fwd_win_h if half else lib.ssad_bn_relu_maxpool_fwd_win
        _run("maxpool3x3s2_h16" if half else "maxpool3x3s2", 0.0, eb * (z.numel() + 2.0 * out.numel()) + idx.numel(),
             lambda: fn(z.data_ptr(), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(beta), out.data_ptr(), idx.data_ptr(),
                        zw.data_ptr(), n, h, w, c, _hip.stream()))
        return out, idx, zw
    fn = lib.ssad_bn_relu_maxpool_fwd_h if half else lib.ssad_bn_relu_maxpool_fwd
    _run("maxpool3x3s2_h16" if half else "maxpool3x3s2", 0.0, eb * (z.numel() + out.numel()) + idx.numel(),
         lambda: fn(z.data_ptr(), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(beta), out.data_ptr(), idx.data_ptr(), n, h, w, c,
                    _hip.stream()))
    return out, idx


def pool_bn_relu_bwd(idx, dpool, z, mean, invstd, gamma, beta, dbeta, dgamma, zwin=None):
    """Training stem head of the backward pass: (idx, dpool, z) -> dz, filling dbeta / dgamma.  zwin (bn_relu_maxpool_fwd(winners=True)):
    the BatchNorm reduction runs over (dpool, zwin) -- a quarter of the rows, no pass over z -- and only the apply pass reads z."""
    n, h, w, c = z.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert tuple(dpool.shape) == (n, ho, wo, c) and tuple(idx.shape) == (n, ho, wo, c) and dpool.dtype == z.dtype, \
        f"pooled gradient {tuple(dpool.shape)} / slots {tuple(idx.shape)} do not belong to z {tuple(z.shape)}"
    dz = torch.empty_like(z)
    half = _is_h(z)
    lib = _hip.lib()
    eb = z.element_size()
    if zwin is not None:
        assert tuple(zwin.shape) == (n, ho, wo, c) and zwin.dtype == z.dtype and dpool.is_contiguous() and zwin.is_contiguous()
        r = n * ho * wo
        ws = _colreduce_ws(r, c, z)
        red = lib.ssad_bn_bwd_reduce_zmask_h if half else lib.ssad_bn_bwd_reduce_zmask
        _run("bn_bwd_reduce_h16" if half else "bn_bwd_reduce", 0.0, eb * 2.0 * dpool.numel(),
             lambda: red(dpool.data_ptr(), zwin.data_ptr(), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(beta), _hip.ptr(dbeta),
                         _hip.ptr(dgamma), r, c, ws.data_ptr(), _hip.stream()))
        app = lib.ssad_pool_bn_relu_bwd_apply_h if half else lib.ssad_pool_bn_relu_bwd_apply
        _run("pool_bn_bwd_h16" if half else "pool_bn_bwd", 0.0, eb * (2.0 * z.numel() + dpool.numel()),
             lambda: app(idx.data_ptr(), dpool.data_ptr(), z.data_ptr(), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(beta),
                         _hip.ptr(dbeta), _hip.ptr(dgamma), dz.data_ptr(), n, h, w, c, dpool.numel(), _hip.stream()))
        return dz
    ws = _colreduce_ws(n * h * w, c, z)
    fn = lib.ssad_pool_bn_relu_bwd_h if half else lib.ssad_pool_bn_relu_bwd
    _run("pool_bn_bwd_h16" if half else "pool_bn_bwd", 0.0, eb * (3.0 * z.numel() + 2.0 * dpool.numel()),
         lambda: fn(idx.data_ptr(), dpool.data_ptr(), z.data_ptr(), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(beta),
                    _hip.ptr(dbeta), _hip.ptr(dgamma), dz.data_ptr(), n, h, w, c, dpool.numel(), ws.data_ptr(), _hip.stream()))
    return dz


def maxpool3x3s2_bwd(x, dy):
    n, h, w, c = x.shape
    dx = torch.empty_like(x)
    _run("maxpool_bwd", 0.0, 4.0 * (2 * x.numel() + dy.numel()),
         lambda: _hip.lib().ssad_maxpool3x3s2_bwd(_hip.ptr(x), _hip.ptr(dy), _hip.ptr(dx), n, h, w, c, dy.numel(), _hip.stream()))
    return dx


def maxpool3x3s2_fwd_idx(x):
    """Training forward: pooled output + uint8 argmax slots."""
    n, h, w, c = x.shape
    out = _new((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), x)
    idx = torch.empty(out.shape, dtype=torch.uint8, device=x.device)
    _run("maxpool3x3s2", 0.0, 4.0 * (x.numel() + out.numel()) + idx.numel(),
         lambda: _hip.lib().ssad_maxpool3x3s2_fwd_idx(_hip.ptr(x), _hip.ptr(out), idx.data_ptr(), n, h, w, c, _hip.stream()))
    return out, idx


def maxpool3x3s2_bwd_idx(idx, dy, x_shape):
    n, h, w, c = x_shape
    assert tuple(dy.shape) == (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c) and idx.shape == dy.shape, "dy / idx do not belong to x_shape"
    dx = _new(tuple(x_shape), dy)
    _run("maxpool_bwd", 0.0, 4.0 * (dx.numel() + dy.numel()) + idx.numel(),
         lambda: _hip.lib().ssad_maxpool3x3s2_bwd_idx(idx.data_ptr(), _hip.ptr(dy), _hip.ptr(dx), n, h, w, c, dy.numel(),
                                                      _hip.stream()))
    return dx


def gap_bwd(dpooled, dy, offset, accumulate):
    n, h, w, c = dy.shape
    if _is_h(dy):
        _run("gap_bwd_h16", 0.0, 2.0 * dy.numel() * (2 if accumulate else 1),
             lambda: _hip.lib().ssad_gap_bwd_h(_hip.ptr(dpooled), dy.data_ptr(), n, h * w, c, dpooled.shape[1], offset,
                                               int(accumulate), _hip.stream()))
        return dy
    _run("gap_bwd", 0.0, 4.0 * dy.numel() * (2 if accumulate else 1),
         lambda: _hip.lib().ssad_gap_bwd(_hip.ptr(dpooled), _hip.ptr(dy), n, h * w, c, dpooled.shape[1], offset,
                                         int(accumulate), _hip.stream()))
    return dy


def softmax_ce(logits, labels, dlogits=None, grad_scale=1.0):
    b, c = logits.shape
    out = _new((2,), logits)
    ldd = dlogits.shape[1] if dlogits is not None else 0
    _hip.check(_hip.lib().ssad_softmax_ce(_hip.ptr(logits), _hip.ptr(labels, dtype=torch.int64), b, c, _hip.ptr(out),
                                          _hip.ptr(dlogits, True), ldd, grad_scale, _hip.stream()))
    return out


def sgd_step(p, g, m, lr, momentum, weight_decay, grad_scale=1.0):
    _run("sgd", 0.0, 20.0 * p.numel(),
         lambda: _hip.lib().ssad_sgd_step(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), p.numel(), lr, momentum, weight_decay,
                                          grad_scale, _hip.stream()))


def sgd_step_dev(p, g, m, hyper, scaler=None):
    """SGD with [lr, momentum, weight_decay, grad_scale] (and the optional loss-scaler state) read from device memory."""
    _run("sgd", 0.0, 20.0 * p.numel(),
         lambda: _hip.lib().ssad_sgd_step_dev(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), p.numel(), _hip.ptr(hyper),
                                              _hip.ptr(scaler, True), _hip.stream()))


def scale_by_loss_scale(x, scaler):
    _hip.check(_hip.lib().ssad_scale_by_loss_scale(_hip.ptr(x), x.numel(), _hip.ptr(scaler), _hip.stream()))


def check_finite(g, scaler):
    _run("check_finite", 0.0, 4.0 * g.numel(),
         lambda: _hip.lib().ssad_check_finite(_hip.ptr(g), g.numel(), _hip.ptr(scaler), _hip.stream()))


def loss_scaler_update(scaler, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    _hip.check(_hip.lib().ssad_loss_scaler_update(_hip.ptr(scaler), growth_factor, backoff_factor, growth_interval,
                                                  _hip.stream()))


def bn_apply_fwd_mask(z, mean, invstd, gamma, beta, residual, relu):
    """bn_apply_fwd that also returns the final ReLU's active set as a nibble mask (uint8 [R][C/4])."""
    c = mean.numel()
    y = torch.empty_like(z)
    mask = torch.empty(z.numel() // 4, device=z.device, dtype=torch.uint8)
    if _is_h(z):                  # half tensors: two mask bytes per lane (8 channels)
        assert residual is None or _is_h(residual)
        _run("bn_apply_fwd_h16", 0.0, 2.0 * z.numel() * (3 if residual is not None else 2) + mask.numel(),
             lambda: _hip.lib().ssad_bn_apply_fwd_mask_h(z.data_ptr(), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(beta),
                                                         _p(residual, True), y.data_ptr(), mask.data_ptr(), z.numel() // c, c,
                                                         int(relu), _hip.stream()))
        return y, mask
    _run("bn_apply_fwd", 0.0, 4.0 * z.numel() * (3 if residual is not None else 2) + mask.numel(),
         lambda: _hip.lib().ssad_bn_apply_fwd_mask(_hip.ptr(z), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma), _hip.ptr(beta),
                                                   _hip.ptr(residual, True), _hip.ptr(y), mask.data_ptr(), z.numel() // c, c,
                                                   int(relu), _hip.stream()))
    return y, mask


def bn_bwd_mask(dy, mask, z, mean, invstd, gamma, dbeta, dgamma):
    """BatchNorm backward with g = dy * mask (mask None: g = dy): fills dbeta / dgamma, returns dz.  The identity-branch
    gradient (g itself) is not materialised: consumers apply `mask` to dy (conv_dgrad / conv3x3_c64 res_mask)."""
    c = mean.numel()
    r = dy.numel() // c
    ws = _colreduce_ws(r, c, dy)
    lib = _hip.lib()
    mp = mask.data_ptr() if mask is not None else None
    if _is_h(dy):
        assert _is_h(z)
        _run("bn_bwd_reduce_h16", 0.0, 4.0 * dy.numel() + (mask.numel() if mask is not None else 0),
             lambda: lib.ssad_bn_bwd_reduce_mask_h(dy.data_ptr(), mp, z.data_ptr(), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(dbeta),
                                                   _hip.ptr(dgamma), r, c, ws.data_ptr(), _hip.stream()))
        dz = torch.empty_like(dy)
        _run("bn_apply_bwd_h16", 0.0, 6.0 * dy.numel() + (mask.numel() if mask is not None else 0),
             lambda: lib.ssad_bn_apply_bwd_mask_h(dy.data_ptr(), mp, z.data_ptr(), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma),
                                                  _hip.ptr(dbeta), _hip.ptr(dgamma), dz.data_ptr(), r, c, _hip.stream()))
        return dz
    _run("bn_bwd_reduce", 0.0, 8.0 * dy.numel() + (mask.numel() if mask is not None else 0),
         lambda: lib.ssad_bn_bwd_reduce_mask(_hip.ptr(dy), mp, _hip.ptr(z), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(dbeta),
                                             _hip.ptr(dgamma), r, c, ws.data_ptr(), _hip.stream()))
    dz = torch.empty_like(dy)
    _run("bn_apply_bwd", 0.0, 12.0 * dy.numel() + (mask.numel() if mask is not None else 0),
         lambda: lib.ssad_bn_apply_bwd_mask(_hip.ptr(dy), mp, _hip.ptr(z), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(gamma),
                                            _hip.ptr(dbeta), _hip.ptr(dgamma), _hip.ptr(dz), r, c, _hip.stream()))
    return dz


def cvt_f32_f16(src, dst):
    """One rounded (half) copy of a flat fp32 arena: the weights the half-tensor kernels of the precision-16 step read."""
    assert src.dtype == torch.float32 and dst.dtype == torch.float16 and src.numel() == dst.numel()
    _run("cvt_f32_f16", 0.0, 6.0 * src.numel(),
         lambda: _hip.lib().ssad_cvt_f32_f16(_hip.ptr(src), dst.data_ptr(), src.numel(), _hip.stream()))
    return dst
