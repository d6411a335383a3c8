"""The resize-then-Gaussian operator without a GPU: tests/resize_gaussian_ref.py against scipy.ndimage.gaussian_filter and torch's
reflect-pad convolution over F.interpolate (all float64), the properties of A = G R the kernel relies on, the host half of
ops.resize_gaussian (tables, ValueErrors) and the unchanged defaults of tools.upsample / tools.sweep."""
import inspect

import numpy as np
import pytest
import scipy.ndimage
import torch
import torch.nn.functional as F

import resize_gaussian_ref as ref
from self_supervised import ops, tools

BAR = 1e-12            # float64 compositions of ~40 terms on values up to ~10: measured <= 2e-14
BORDERS = ("symmetric", "reflect")


def _resized(M, T):
    return F.interpolate(torch.from_numpy(M)[None, None], size=(T, T), mode="bilinear", align_corners=False)


def _random_map(h, w, seed):
    return 10.0 * np.random.default_rng(seed).random((h, w))


@pytest.mark.parametrize("h,T,sigma", ref.SHAPES)
def test_symmetric_is_scipy_gaussian_filter_of_the_interpolated_map(h, T, sigma):
    M = _random_map(h, h, 1)
    want = scipy.ndimage.gaussian_filter(_resized(M, T)[0, 0].numpy(), sigma)
    err = np.abs(ref.reference(M, T, sigma, "symmetric") - want).max()
    print(f"{h} -> {T} sigma {sigma}: max |ref - scipy| = {err:.3g}")
    assert err <= BAR


@pytest.mark.parametrize("h,T,sigma", ref.SHAPES)
def test_reflect_is_torch_reflect_pad_and_conv2d(h, T, sigma):
    M = _random_map(h, h, 2)
    r = int(4.0 * sigma + 0.5)
    d = torch.arange(-r, r + 1, dtype=torch.float64)
    taps = torch.exp(-0.5 * (d / sigma) ** 2)
    taps = taps / taps.sum()
    kernel = torch.outer(taps, taps)[None, None]
    want = F.conv2d(F.pad(_resized(M, T), (r, r, r, r), mode="reflect"), kernel)[0, 0].numpy()
    err = np.abs(ref.reference(M, T, sigma, "reflect") - want).max()
    print(f"{h} -> {T} sigma {sigma}: max |ref - torch| = {err:.3g}")
    assert err <= BAR


def test_non_square_map_against_scipy():
    M = _random_map(5, 9, 3)
    want = scipy.ndimage.gaussian_filter(_resized(M, 40)[0, 0].numpy(), 4.0)
    assert np.abs(ref.reference(M, 40, 4.0, "symmetric") - want).max() <= BAR


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("h,T,sigma", ref.SHAPES + [(9, 40, 4.0), (32, 250, 4.0), (24, 96, 4.0)])
def test_rows_sum_to_one_and_are_one_contiguous_run(h, T, sigma, border):
    A = ref.operator(h, T, sigma, border)
    assert np.abs(A.sum(axis=1) - 1.0).max() <= 1e-14
    assert (A >= 0.0).all()
    first, weights, K = ref.pack(A)
    for d in range(T):
        cols = np.flatnonzero(A[d])
        assert np.array_equal(cols, np.arange(cols[0], cols[-1] + 1)), f"row {d} has a gap"
        assert cols.size <= K and first[d] <= cols[0] and cols[-1] < first[d] + K <= h
    # the band form loses nothing but the one rounding to fp32
    assert np.abs(ref.unpack(first, weights, h) - A).max() <= ref.U
    assert np.all(np.diff(first) >= 0)                       # what the kernel's count of source rows per band rests on


def test_packed_run_lengths_of_the_design_note():
    got = {(h, T, s): ref.pack(ref.operator(h, T, s, "symmetric"))[2] for h, T, s in [(32, 256, 4.0), (29, 256, 4.0), (128, 512, 4.0), (32, 64, 1.5)]}
    assert got == {(32, 256, 4.0): 6, (29, 256, 4.0): 6, (128, 512, 4.0): 10, (32, 64, 1.5): 8}


@pytest.mark.parametrize("border", BORDERS)
def test_an_impulse_gives_the_outer_product_of_two_columns(border):
    h, w, T = 5, 9, 40
    Ay, Ax = ref.operator(h, T, 4.0, border), ref.operator(w, T, 4.0, border)
    for i, j in [(0, 0), (4, 8), (2, 5), (0, 8)]:
        M = np.zeros((h, w))
        M[i, j] = 1.0
        assert np.abs(ref.reference(M, T, 4.0, border) - np.outer(Ay[:, i], Ax[:, j])).max() <= 1e-16


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("h,T,sigma", ref.SHAPES + [(9, 40, 4.0), (32, 250, 4.0)])
def test_ops_operator_is_the_tests_own_packing(h, T, sigma, border):
    first, weights, K = ops.resize_gaussian_operator(h, T, sigma, border)
    want_first, want_weights, want_K = ref.pack(ref.operator(h, T, sigma, border))
    assert K == want_K and first.dtype == torch.int32 and weights.dtype == torch.float32 and not first.is_cuda
    assert np.array_equal(first.numpy(), want_first)
    assert np.array_equal(weights.numpy(), want_weights)
    assert ops.resize_gaussian_operator(h, T, sigma, border)[1] is weights              # cached


def test_value_errors():
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(border="constant"), dict(border=None)):
        with pytest.raises(ValueError):
            ops.resize_gaussian_operator(32, 256, **kw)
        with pytest.raises(ValueError):
            ops.resize_gaussian(torch.zeros(1, 1, 32, 32), 256, **kw)
    for border in BORDERS:
        with pytest.raises(ValueError):
            ops.resize_gaussian_operator(7, 16, 4.0, border)            # radius 16 >= T
        with pytest.raises(ValueError):
            ops.resize_gaussian(torch.zeros(1, 7, 7), 16, 4.0, border)
        ops.resize_gaussian_operator(7, 17, 4.0, border)                # T = radius + 1 is the limit
    with pytest.raises(ValueError):
        ops.resize_gaussian(torch.zeros(1, 2, 8, 8), 64)                # two channels
    with pytest.raises(ValueError):
        ops.resize_gaussian(torch.zeros(1, 8, 8, dtype=torch.int32), 64)
    with pytest.raises(ValueError):
        tools.upsample(torch.zeros(1, 1, 8, 8), 64, verbose=False, method="blur_resize")
    with pytest.raises(ValueError):
        tools.sweep("unused/", "unused/", [], upsample_method="blur_resize")


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError):
        ops.resize_gaussian(torch.zeros(1, 1, 8, 8), 64)                # the op takes device tensors only
    if not torch.cuda.is_available():                                   # with a GPU, tools.upsample moves the tensor there
        with pytest.raises(RuntimeError):
            tools.upsample(torch.zeros(1, 1, 8, 8), 64, verbose=False, method="resize_blur")


def test_defaults_are_the_reference_path():
    up = inspect.signature(tools.upsample).parameters
    assert up["method"].default == "reference" and up["sigma"].default == 4.0 and up["border"].default == "symmetric"
    assert [p for p in up][:3] == ["anomaly_maps", "target_size", "verbose"] and up["target_size"].default == 256
    sw = inspect.signature(tools.sweep).parameters
    assert sw["upsample_method"].default == "reference" and sw["upsample_sigma"].default == 4.0
    op = inspect.signature(ops.resize_gaussian).parameters
    assert op["sigma"].default == 4.0 and op["border"].default == "symmetric"
