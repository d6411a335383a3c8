// Anomaly maps as PatchCore and PaDiM define them: bilinear resize (align_corners=False) to T x T, THEN a Gaussian of sigma image
// pixels (scipy.ndimage.gaussian_filter / anomalib's GaussianBlur2d), as one banded operator.
//
// Both steps are separable and linear, so the whole function of a map M [h][w] is out = A_y M A_x^T with A = G R per axis: R the
// [T][h] bilinear matrix, G the [T][T] Gaussian with its border folded in.  Every row of A has one contiguous run of non-zeros,
// at most K long (6 for 32 -> 256 at sigma 4), so the host hands each axis over in band form -- first[T] int32, weights [T][K]
// fp32 zero-padded (self_supervised/ops.py resize_gaussian_operator builds them in float64 and rounds once) -- and an output pixel
// is two chains of K FMAs instead of 33 + 33 taps over a T x T intermediate in HBM.
//
// One workgroup = one map and one band of `band` output rows.  It stages the S source rows the band reads into LDS, forms
// tmp = M A_x^T for those rows in LDS (K_x FMAs per element, s = 0 .. K_x - 1), then out = A_y tmp (K_y FMAs, t = 0 .. K_y - 1)
// and stores rows of out, four pixels per lane (16-byte stores) when T % 4 == 0.  tmp[r][x] is a function of source row r and x
// alone and the second chain of y and x alone: a pixel's bits depend neither on the band height nor on the workgroup nor on n.
// HBM-bound on writing out (4 T^2 bytes per map against 4 h w read); exact fp32, no matrix cores.
//
// Every LDS and source index is clamped, so tables outside the contract (first indices that advance faster than h / T per row:
// more source rows per band than the S the launch reserved) give unspecified values, never an access out of bounds.
#include "common.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_BAND = 32;                 // default band height; halved until the band fits RG_LDS_MAX
constexpr int RG_LDS_MAX = 64 * 1024;       // dynamic LDS a launch may ask for without opting in

// source rows reserved for a band: the first indices of A = G R advance by at most ceil((band - 1) h / T) over a band, + one run
int rg_src_rows(int h, int T, int Ky, int band) {
    const int64_t s = ((int64_t)band * h + T - 1) / T + Ky + 2;
    return (int)(s < h ? s : h);
}

int64_t rg_lds_bytes(int h, int w, int T, int Ky, int band) {
    const int64_t S = rg_src_rows(h, T, Ky, band);
    return (((S * w + 3) & ~(int64_t)3) + S * (((int64_t)T + 3) & ~(int64_t)3)) * (int64_t)sizeof(float);
}

int rg_default_band(int h, int w, int T, int Ky) {
    int band = RG_BAND < T ? RG_BAND : T;
    while (band > 1 && rg_lds_bytes(h, w, T, Ky, band) > RG_LDS_MAX) band >>= 1;
    return rg_lds_bytes(h, w, T, Ky, band) <= RG_LDS_MAX ? band : 0;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool V4>
__global__ __launch_bounds__(RG_THREADS) void resize_gaussian_kernel(const float* __restrict__ maps, int h, int w,
                                                                     const int32_t* __restrict__ yf, const float* __restrict__ yw, int Ky,
                                                                     const int32_t* __restrict__ xf, const float* __restrict__ xw, int Kx,
                                                                     int T, int band, int bands, int S, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int first_row;
    const int Tp = (T + 3) & ~3;
    float* src = lds;                                  // [S][w]
    float* tmp = lds + ((S * w + 3) & ~3);             // [S][Tp]
    const int b = (int)(blockIdx.x % (unsigned)bands);
    const int64_t img = blockIdx.x / (unsigned)bands;
    const int y0 = b * band;
    const int rows = band < T - y0 ? band : T - y0;
    const int tid = threadIdx.x;

    if (tid == 0) first_row = h - 1;
    __syncthreads();
    if (tid < rows) atomicMin(&first_row, yf[y0 + tid]);
    __syncthreads();
    const int s0 = clampi(first_row, 0, h - 1);

    const float* m = maps + img * (int64_t)h * w;
    for (int i = tid; i < S * w; i += RG_THREADS) {
        const int r = i / w, c = i - r * w;
        const int gr = s0 + r < h ? s0 + r : h - 1;
        src[i] = m[(int64_t)gr * w + c];
    }
    __syncthreads();

    // tmp[r][x] = sum_s xw[x][s] * M[s0 + r][xf[x] + s], s ascending
    for (int i = tid; i < S * T; i += RG_THREADS) {
        const int r = i / T, x = i - r * T;
        const int f = xf[x];
        const float* wt = xw + (int64_t)x * Kx;
        const float* row = src + r * w;
        float acc = 0.f;
        for (int s = 0; s < Kx; ++s) acc = __builtin_fmaf(wt[s], row[clampi(f + s, 0, w - 1)], acc);
        tmp[r * Tp + x] = acc;
    }
    __syncthreads();

    // out[y][x] = sum_t yw[y][t] * tmp[yf[y] + t - s0][x], t ascending
    float* o = out + img * (int64_t)T * T;
    if (V4) {
        const int T4 = T >> 2;
        for (int i = tid; i < rows * T4; i += RG_THREADS) {
            const int yl = i / T4, x = (i - yl * T4) << 2;
            const int y = y0 + yl;
            const int f = yf[y] - s0;
            const float* wt = yw + (int64_t)y * Ky;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < Ky; ++t) {
                const f32x4 v = *(const f32x4*)(tmp + clampi(f + t, 0, S - 1) * Tp + x);
                const float wv = wt[t];
                acc[0] = __builtin_fmaf(wv, v[0], acc[0]);
                acc[1] = __builtin_fmaf(wv, v[1], acc[1]);
                acc[2] = __builtin_fmaf(wv, v[2], acc[2]);
                acc[3] = __builtin_fmaf(wv, v[3], acc[3]);
            }
            *(f32x4*)(o + (int64_t)y * T + x) = acc;
        }
    } else {
        for (int i = tid; i < rows * T; i += RG_THREADS) {
            const int yl = i / T, x = i - yl * T;
            const int y = y0 + yl;
            const int f = yf[y] - s0;
            const float* wt = yw + (int64_t)y * Ky;
            float acc = 0.f;
            for (int t = 0; t < Ky; ++t) acc = __builtin_fmaf(wt[t], tmp[clampi(f + t, 0, S - 1) * Tp + x], acc);
            o[(int64_t)y * T + x] = acc;
        }
    }
}

}  // namespace

extern "C" int ssad_resize_gaussian_band(int h, int w, int T, int Ky) {
    if (h < 1 || w < 1 || T < 1 || Ky < 1) return 0;
    return rg_default_band(h, w, T, Ky);
}

extern "C" int ssad_resize_gaussian(const float* maps, int64_t n, int h, int w, const int32_t* y_first, const float* y_weights, int Ky,
                                    const int32_t* x_first, const float* x_weights, int Kx, int T, int band, float* out, void* stream) {
    SSAD_CHECK_ARG(maps && out && y_first && y_weights && x_first && x_weights, "null pointer");
    SSAD_CHECK_ARG(n >= 1 && h >= 1 && w >= 1 && T >= 1, "sizes below 1");
    SSAD_CHECK_ARG(Ky >= 1 && Kx >= 1 && Ky <= h && Kx <= w, "a run has 1 .. extent weights");
    SSAD_CHECK_ARG(band >= 0 && band <= RG_THREADS, "band is 0 (chosen here) or 1 .. 256 output rows");
    SSAD_CHECK_ARG((int64_t)h * w < (1 << 30) && (int64_t)T * T < ((int64_t)1 << 31), "map too large");
    if (band == 0) band = rg_default_band(h, w, T, Ky);
    SSAD_CHECK_ARG(band >= 1, "no band height fits the LDS a launch may ask for");
    if (band > T) band = T;
    const int64_t lds = rg_lds_bytes(h, w, T, Ky, band);
    SSAD_CHECK_ARG(lds <= RG_LDS_MAX, "the band's source rows and intermediate exceed the LDS a launch may ask for");
    const int bands = (T + band - 1) / band;
    SSAD_CHECK_ARG(n * bands < ((int64_t)1 << 31), "grid limit");
    const int S = rg_src_rows(h, T, Ky, band);
    const dim3 grid((unsigned)(n * bands));
    if (T % 4 == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(resize_gaussian_kernel<true>, grid, dim3(RG_THREADS), (size_t)lds, (hipStream_t)stream, maps, h, w, y_first,
                           y_weights, Ky, x_first, x_weights, Kx, T, band, bands, S, out);
    else
        hipLaunchKernelGGL(resize_gaussian_kernel<false>, grid, dim3(RG_THREADS), (size_t)lds, (hipStream_t)stream, maps, h, w, y_first,
                           y_weights, Ky, x_first, x_weights, Kx, T, band, bands, S, out);
    SSAD_CHECK_LAUNCH();
    return 0;
}
