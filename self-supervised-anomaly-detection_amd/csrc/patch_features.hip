// Locally aware patch features from two stage maps of ONE trunk pass: the feature construction of PatchCore (Roth et al., CVPR 2022,
// §3.1) as anomalib implements it -- every stage map is smoothed by AvgPool2d(3, stride 1, padding 1), the coarser one is resampled to
// the finer grid with F.interpolate(mode='bilinear', align_corners=False), and the channels are concatenated, one row per position of
// the finer map.  The reference (gabry1998/Self-Supervised-Anomaly-Detection) has no counterpart: it scores 841 windows per image.
//
//   fine [N][Hf][Wf][Cf], coarse [N][Hc][Wc][Cc] NHWC fp32  ->  out [N * Hf * Wf][Cf + Cc], rows in (n, i, j) order, not normalised
//
//   out[(n, i, j)][c]        = 1/9 sum_{|di| <= 1, |dj| <= 1} fine[n][i + di][j + dj][c]                 (zeros outside the map), c < Cf
//   P[n][y][x][c]            = 1/9 sum_{|dy| <= 1, |dx| <= 1} coarse[n][y + dy][x + dx][c]               (zeros outside the map)
//   out[(n, i, j)][Cf + c]   = (1 - ly) ((1 - lx) P[y0][x0] + lx P[y0][x1]) + ly ((1 - lx) P[y1][x0] + lx P[y1][x1])
//
// with the sample position of align_corners=False, (i + 1/2) Hc / Hf - 1/2 clamped at 0, kept as an exact rational:
//
//   num = max((2 i + 1) Hc - Hf, 0),   y0 = num div (2 Hf),   y1 = min(y0 + 1, Hc - 1),   ly = (num - y0 2 Hf) / (2 Hf)
//
// (x0, x1, lx from j, Wf, Wc likewise), so ly and lx are correctly rounded quotients of two small integers and no fp32 scale factor
// enters.  P never reaches HBM.
//
// One workgroup owns a band of `rows_per_block` consecutive fine rows of one image.  Fine stage: a thread keeps the horizontal
// three-sums of rows i - 1, i, i + 1 of its (column, 4 channels) in registers and slides them down the band, so a row is read once
// per band (plus two halo rows) and its horizontal neighbours come from the cache the same workgroup has just filled.  Coarse stage:
// the two pooled rows y0, y1 a fine row needs live in LDS ([2][Wc][chunk of channels]); going down the band a row that is already
// there (y1 of one fine row is y0 of a later one) is kept and only a missing one is pooled, once per fine row and not once per
// output.  No atomics, one fixed summation order: the result does not depend on rows_per_block, and a call repeats its own bits.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int LDS_FLOATS = 16384;      // 64 KB: two pooled coarse rows of one channel chunk
constexpr int MAX_DIM = 32768;         // (2 i + 1) Hc stays below 2^31, numerators and denominators are exact in fp32

struct Tap { int a, b; float l; };

// source taps and weight of destination index i when nc source positions are resampled to nf (align_corners=False)
__device__ __forceinline__ Tap tap(int i, int nf, int nc) {
    const int num = max((2 * i + 1) * nc - nf, 0);
    Tap t;
    t.a = num / (2 * nf);
    t.b = min(t.a + 1, nc - 1);
    t.l = (float)(num - t.a * 2 * nf) / (float)(2 * nf);
    return t;
}

// grid: N * ceil(Hf / RB).  lgf / lgc: log2 of the lanes that run over the float4 channel groups of the fine map / of a coarse chunk
// (a power of two <= NT); the other NT >> lg threads run over columns.  T4: float4 groups of a coarse channel chunk.
__global__ __launch_bounds__(NT) void local_patch_features_kernel(const float* __restrict__ fine, const float* __restrict__ coarse,
                                                                  float* __restrict__ out, int Hf, int Wf, int Cf, int Hc, int Wc,
                                                                  int Cc, int RB, int T4, int lgf, int lgc) {
    extern __shared__ f32x4 pooled[];                          // [2][Wc][T4]
    const int tid = threadIdx.x;
    const int bands = (Hf + RB - 1) / RB;
    const int n = blockIdx.x / bands, i0 = (blockIdx.x % bands) * RB, i1 = min(i0 + RB, Hf);
    const int D = Cf + Cc;
    const float ninth = 1.f / 9.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    float* obase = out + (int64_t)n * Hf * Wf * D;

    {   // ---- fine stage: columns [0, Cf)
        const f32x4* f = (const f32x4*)fine + (int64_t)n * Hf * Wf * (Cf >> 2);
        const int C4 = Cf >> 2, TC = 1 << lgf, TJ = NT >> lgf, tc = tid & (TC - 1), tj = tid >> lgf;
        for (int j = tj; j < Wf; j += TJ)
            for (int c = tc; c < C4; c += TC) {
                auto hsum = [&](int r) -> f32x4 {              // fine[r][j - 1] + fine[r][j] + fine[r][j + 1], zeros outside
                    if (r < 0 || r >= Hf) return zero;
                    const f32x4* p = f + ((int64_t)r * Wf + j) * C4 + c;
                    f32x4 s = j > 0 ? p[-C4] : zero;
                    s += p[0];
                    if (j + 1 < Wf) s += p[C4];
                    return s;
                };
                f32x4 up = hsum(i0 - 1), mid = hsum(i0);
                for (int i = i0; i < i1; ++i) {
                    const f32x4 down = hsum(i + 1);
                    *(f32x4*)(obase + ((int64_t)i * Wf + j) * D + 4 * c) = ((up + mid) + down) * ninth;
                    up = mid;
                    mid = down;
                }
            }
    }

    // ---- coarse stage: columns [Cf, Cf + Cc), a chunk of T4 float4 channel groups at a time
    const f32x4* cz = (const f32x4*)coarse + (int64_t)n * Hc * Wc * (Cc >> 2);
    const int C4 = Cc >> 2, TC = 1 << lgc, TJ = NT >> lgc, tc = tid & (TC - 1), tj = tid >> lgc;
    for (int c0 = 0; c0 < C4; c0 += T4) {
        const int t4 = min(T4, C4 - c0);
        auto pool = [&](int y, int slot) {                     // P[y][.][chunk] -> pooled[slot]
            for (int x = tj; x < Wc; x += TJ)
                for (int c = tc; c < t4; c += TC) {
                    f32x4 s = zero;
                    for (int r = max(y - 1, 0); r <= min(y + 1, Hc - 1); ++r)
                        for (int xx = max(x - 1, 0); xx <= min(x + 1, Wc - 1); ++xx)
                            s += cz[((int64_t)r * Wc + xx) * C4 + c0 + c];
                    pooled[(slot * Wc + x) * T4 + c] = s * ninth;
                }
        };
        int h0 = -1, h1 = -1;                                  // the coarse rows the two LDS slots hold (uniform)
        for (int i = i0; i < i1; ++i) {
            const Tap ty = tap(i, Hf, Hc);
            // y0 stays where it is; otherwise it takes the slot that does not hold y1
            const int sa = h0 == ty.a ? 0 : h1 == ty.a ? 1 : h0 == ty.b ? 1 : 0;
            const bool pa = (sa ? h1 : h0) != ty.a;
            if (sa) h1 = ty.a; else h0 = ty.a;
            int sb = sa;
            bool pb = false;
            if (ty.b != ty.a) {
                sb = 1 - sa;
                pb = (sb ? h1 : h0) != ty.b;
                if (sb) h1 = ty.b; else h0 = ty.b;
            }
            if (pa || pb) {
                __syncthreads();                               // the previous fine row's readers are done with the slots
                if (pa) pool(ty.a, sa);
                if (pb) pool(ty.b, sb);
                __syncthreads();
            }
            const f32x4* pa0 = pooled + sa * Wc * T4;
            const f32x4* pb0 = pooled + sb * Wc * T4;
            float* orow = obase + (int64_t)i * Wf * D + Cf + 4 * c0;
            for (int j = tj; j < Wf; j += TJ) {
                const Tap tx = tap(j, Wf, Wc);
                for (int c = tc; c < t4; c += TC) {
                    const f32x4 top = (1.f - tx.l) * pa0[tx.a * T4 + c] + tx.l * pa0[tx.b * T4 + c];
                    const f32x4 bot = (1.f - tx.l) * pb0[tx.a * T4 + c] + tx.l * pb0[tx.b * T4 + c];
                    *(f32x4*)(orow + (int64_t)j * D + 4 * c) = (1.f - ty.l) * top + ty.l * bot;
                }
            }
        }
        __syncthreads();                                       // before the next chunk overwrites the slots
    }
}

int log2_lanes(int groups) {                                   // log2 of the smallest power of two >= min(groups, NT)
    int lg = 0;
    while ((1 << lg) < groups && (1 << lg) < NT) ++lg;
    return lg;
}

}  // namespace

// Locally aware patch features (see the head of this file).  fine [N][Hf][Wf][Cf], coarse [N][Hc][Wc][Cc] NHWC ->
// out [N * Hf * Wf][Cf + Cc].  Cf % 4 == 0, Cc % 4 == 0, 16-byte aligned pointers, every map side in 1 .. 32768, Wc <= 2048 (two pooled
// rows of four channels fill the LDS there), any size ratio.  rows_per_block: fine rows of one image a workgroup walks down (0: chosen
// from N * Hf); the result does not depend on it.
extern "C" int ssad_local_patch_features(const float* fine, const float* coarse, float* out, int64_t N, int Hf, int Wf, int Cf, int Hc,
                                         int Wc, int Cc, int rows_per_block, void* stream) {
    SSAD_CHECK_ARG(fine && coarse && out && N > 0, "bad argument");
    SSAD_CHECK_ARG(Hf >= 1 && Wf >= 1 && Hc >= 1 && Wc >= 1 && Hf <= MAX_DIM && Wf <= MAX_DIM && Hc <= MAX_DIM && Wc <= MAX_DIM,
                   "map sides in 1..32768");
    SSAD_CHECK_ARG(Cf >= 4 && Cc >= 4 && Cf % 4 == 0 && Cc % 4 == 0, "channel counts must be positive multiples of 4");
    SSAD_CHECK_ARG((((uintptr_t)fine | (uintptr_t)coarse | (uintptr_t)out) & 15) == 0, "pointers must be 16-byte aligned");
    SSAD_CHECK_ARG(2 * Wc * 4 <= LDS_FLOATS, "coarse maps wider than 2048 positions are not supported");
    SSAD_CHECK_ARG(rows_per_block >= 0, "rows_per_block >= 0 (0: automatic)");
    int RB = rows_per_block;
    if (RB == 0) {
        // 8-row bands read a fine row 1.25 times; shorter bands while that leaves fewer than four workgroups per CU (256 CUs)
        RB = (int)((N * Hf) / 1024);
        RB = RB < 1 ? 1 : RB > 8 ? 8 : RB;
    }
    if (RB > Hf) RB = Hf;
    const int64_t blocks = N * cdiv64(Hf, RB);
    SSAD_CHECK_ARG(blocks < (int64_t)2147483647, "too many rows for one launch");
    int T4 = LDS_FLOATS / (2 * Wc * 4);
    if (T4 > Cc / 4) T4 = Cc / 4;
    const size_t lds = (size_t)2 * Wc * T4 * sizeof(f32x4);
    hipLaunchKernelGGL(local_patch_features_kernel, dim3((unsigned)blocks), dim3(NT), lds, (hipStream_t)stream, fine, coarse, out, Hf, Wf,
                       Cf, Hc, Wc, Cc, RB, T4, log2_lanes(Cf / 4), log2_lanes(T4));
    SSAD_CHECK_LAUNCH();
    return 0;
}
