// Stage-pyramid rows from two or three stage maps of ONE trunk pass: the embedding of PaDiM (Defard et al., ICPR 2020, §III-A, and
// anomalib's PadimModel) and of SPADE's pixel stage -- the stage maps as they are, the coarser ones brought to the finest grid by
// nearest-neighbour replication, the channels concatenated, and (PaDiM) only a fixed choice of the columns kept.  The reference
// (gabry1998/Self-Supervised-Anomaly-Detection) has no counterpart: it scores 841 windows per image.
//
//   m_s [N][H_s][W_s][C_s] NHWC fp32, s = 0 (finest) .. S - 1, S = 2 or 3;  D = sum_s C_s;  sel [d] int32, strictly increasing, or null
//   out [N * H_0 * W_0][d], rows in (n, i, j) order (d = D without a selection):
//
//   out[(n, i, j)][k] = m_s[n][(i H_s) div H_0][(j W_s) div W_0][c],   s the stage that holds column sel[k],  c = sel[k] - (C_0 + .. + C_{s-1})
//
// A pure copy.  The source index is exact integer arithmetic (the convention of patch_features.hip's taps: no fp32 scale factor);
// where H_0 / H_s and W_0 / W_s are integers it is F.interpolate(mode='nearest').
//
// One workgroup owns a band of `rows_per_block` consecutive fine rows of one image.  A fine row's W_0 output rows are ONE contiguous
// run of W_0 d floats: the threads walk it front to back, a lane per 16 bytes, so every store instruction of a wave writes 1 KiB
// without a gap, and a column nobody chose is never written (nor is room left for it).  The sources are ordered for the cache instead
// of being staged: all threads of the workgroup read the same one source row per stage, the replicas of a coarse element along j are
// neighbouring lanes of the same or the next load instruction, and its replicas along i are the next rows of the same band -- the
// lines were fetched by this workgroup a few thousand cycles before.  What does go through LDS are two small tables built once per
// workgroup from the arguments: the source offset (j W_s div W_0) C_s of every fine column j and stage s, and per output column k its
// stage and channel, so the inner loop has no division and does not read `sel` again.  No atomics; a row's bits depend on nothing
// but its sources.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int LDS_INTS = 16384;        // 64 KB: the two tables, S W_0 + d entries
constexpr int MAX_DIM = 32768;         // i H_s and j W_s stay below 2^31
constexpr int MAX_STAGES = 3;
constexpr int CH_BITS = 24;            // a column-table entry is stage << CH_BITS | channel

struct Stages {
    const float* m[MAX_STAGES];
    int H[MAX_STAGES], W[MAX_STAGES], C[MAX_STAGES];
};

// grid: N * ceil(H_0 / RB).  V = 4: d % 4 == 0, a lane stores 16 bytes (without a selection it loads them as 16 bytes too: C_s % 4 == 0
// keeps four consecutive columns in one stage); V = 1: any d, 4 bytes per lane.
template <bool SEL, int V>
__global__ __launch_bounds__(NT) void stage_pyramid_rows_kernel(Stages st, const int* __restrict__ sel, float* __restrict__ out, int S,
                                                                int D, int d, int RB) {
    extern __shared__ int tab[];                               // joff [S][W_0], then kcol [d] (SEL only)
    const int tid = threadIdx.x;
    const int H0 = st.H[0], W0 = st.W[0];
    const int bands = (H0 + RB - 1) / RB;
    const int n = blockIdx.x / bands, i0 = (blockIdx.x % bands) * RB, i1 = min(i0 + RB, H0);
    int* joff = tab;
    int* kcol = tab + ((S * W0 + 3) & ~3);                     // 16-byte aligned: read four entries at a time
    for (int e = tid; e < S * W0; e += NT) {
        const int s = e / W0, j = e - s * W0;
        joff[e] = (j * st.W[s] / W0) * st.C[s];
    }
    if (SEL)
        for (int k = tid; k < d; k += NT) {
            int c = min(max(sel[k], 0), D - 1), s = 0;         // (callers check sel; a bad entry must still not read outside the maps)
            while (s + 1 < S && c >= st.C[s]) c -= st.C[s++];
            kcol[k] = s << CH_BITS | c;
        }
    __syncthreads();

    const int dv = d / V;                                      // lanes per output row
    const int step_j = NT / dv, step_k = NT - step_j * dv;
    for (int i = i0; i < i1; ++i) {
        auto row = [&](int s) -> const float* {                // the one source row of stage s this fine row replicates
            return s < S ? st.m[s] + ((int64_t)n * st.H[s] + i * st.H[s] / H0) * st.W[s] * st.C[s] : nullptr;
        };
        const float *p0 = row(0), *p1 = row(1), *p2 = row(2);
        float* orow = out + ((int64_t)n * H0 + i) * W0 * d;
        auto load = [&](int j, int code) -> float {           // one element by its column-table entry
            const int s = code >> CH_BITS, c = code & ((1 << CH_BITS) - 1);
            const float* p = s == 0 ? p0 : s == 1 ? p1 : p2;
            return p[joff[s * W0 + j] + c];
        };
        int j = tid / dv, k = tid - j * dv;
        for (; j < W0; j += step_j, k += step_k) {
            if (k >= dv) { k -= dv; ++j; if (j >= W0) break; }
            if (!SEL) {                                        // columns V k .. V k + 3 of the concatenation, one stage
                int c = V * k, s = 0;
                while (s + 1 < S && c >= st.C[s]) c -= st.C[s++];
                const float* p = s == 0 ? p0 : s == 1 ? p1 : p2;
                *(f32x4*)(orow + (int64_t)j * d + V * k) = *(const f32x4*)(p + joff[s * W0 + j] + c);
            } else if (V == 4) {
                const int4 code = *(const int4*)(kcol + 4 * k);
                const f32x4 v = {load(j, code.x), load(j, code.y), load(j, code.z), load(j, code.w)};
                *(f32x4*)(orow + (int64_t)j * d + 4 * k) = v;
            } else {
                orow[(int64_t)j * d + k] = load(j, kcol[k]);
            }
        }
    }
}

}  // namespace

// Stage-pyramid rows (see the head of this file).  m0, m1, m2 [N][H_s][W_s][C_s] NHWC, finest first (stages = 2: m2 is not read);
// sel [d] int32 on the device, strictly increasing entries in [0, D) -- the caller checks them -- or null for all D = sum C_s columns
// (then d == D) -> out [N * H0 * W0][d].  C_s % 4 == 0, H0 >= H1 >= H2 and W0 >= W1 >= W2 (any ratio), every side in 1 .. 32768,
// C_s < 2^24, stages * W0 + d <= 16384 (the workgroup's two index tables fill the LDS there); the maps are 16-byte aligned, out is
// when d % 4 == 0.  rows_per_block: fine rows of one image a workgroup walks down (0: chosen from N * H0); the result does not
// depend on it.
extern "C" int ssad_stage_pyramid_rows(const float* m0, const float* m1, const float* m2, const int* sel, float* out, int64_t N,
                                       int stages, int H0, int W0, int C0, int H1, int W1, int C1, int H2, int W2, int C2, int d,
                                       int rows_per_block, void* stream) {
    SSAD_CHECK_ARG(stages == 2 || stages == 3, "two or three stage maps");
    SSAD_CHECK_ARG(m0 && m1 && (m2 || stages == 2) && out && N > 0, "bad argument");
    Stages st = {{m0, m1, stages == 3 ? m2 : nullptr}, {H0, H1, H2}, {W0, W1, W2}, {C0, C1, C2}};
    int64_t D = 0;
    uintptr_t align = 0;
    for (int s = 0; s < stages; ++s) {
        SSAD_CHECK_ARG(st.H[s] >= 1 && st.W[s] >= 1 && st.H[s] <= MAX_DIM && st.W[s] <= MAX_DIM, "map sides in 1..32768");
        SSAD_CHECK_ARG(st.C[s] >= 4 && st.C[s] % 4 == 0 && st.C[s] < (1 << CH_BITS), "channel counts must be positive multiples of 4");
        SSAD_CHECK_ARG(s == 0 || (st.H[s] <= st.H[s - 1] && st.W[s] <= st.W[s - 1]), "the maps come finest first");
        D += st.C[s];
        align |= (uintptr_t)st.m[s];
    }
    if (stages == 2) st.H[2] = st.W[2] = st.C[2] = 0;
    SSAD_CHECK_ARG(sel ? (d >= 1 && d <= D) : d == D, "d columns: 1..D with a selection, D without");
    const int64_t koff = ((int64_t)stages * W0 + 3) & ~(int64_t)3;
    SSAD_CHECK_ARG(koff + d <= LDS_INTS, "stages * W0 + d must not exceed 16384 (the index tables live in LDS)");
    SSAD_CHECK_ARG((align & 15) == 0 && (d % 4 || ((uintptr_t)out & 15) == 0) && ((uintptr_t)sel & 3) == 0,
                   "maps (and out when d % 4 == 0) must be 16-byte aligned");
    SSAD_CHECK_ARG(rows_per_block >= 0, "rows_per_block >= 0 (0: automatic)");
    int RB = rows_per_block;
    if (RB == 0) {
        // 8-row bands keep the replicas of a coarse row along i in one workgroup; shorter bands while that leaves fewer than four
        // workgroups per CU (256 CUs)
        RB = (int)((N * H0) / 1024);
        RB = RB < 1 ? 1 : RB > 8 ? 8 : RB;
    }
    if (RB > H0) RB = H0;
    const int64_t blocks = N * cdiv64(H0, RB);
    SSAD_CHECK_ARG(blocks < (int64_t)2147483647, "too many rows for one launch");
    const size_t lds = (size_t)(koff + (sel ? d : 0)) * sizeof(int);
    const dim3 grid((unsigned)blocks), block(NT);
    hipStream_t hs = (hipStream_t)stream;
    if (!sel)
        hipLaunchKernelGGL((stage_pyramid_rows_kernel<false, 4>), grid, block, lds, hs, st, sel, out, stages, (int)D, d, RB);
    else if (d % 4 == 0)
        hipLaunchKernelGGL((stage_pyramid_rows_kernel<true, 4>), grid, block, lds, hs, st, sel, out, stages, (int)D, d, RB);
    else
        hipLaunchKernelGGL((stage_pyramid_rows_kernel<true, 1>), grid, block, lds, hs, st, sel, out, stages, (int)D, d, RB);
    SSAD_CHECK_LAUNCH();
    return 0;
}
