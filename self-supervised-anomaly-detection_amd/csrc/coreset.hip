// Greedy k-center (farthest-point) coreset of the kNN bank (PatchCore): the m bank rows that greedily minimise the covering radius.
//
// One launch per step, no atomics, no grid-wide barrier: launch t reads the G per-workgroup (max, row) partials that launch t - 1
// wrote to part[(t - 1) & 1], reduces them itself to the centre c = sel[t] (ties to the smallest row), stages row c in LDS, lowers
// mind[r] = min(mind[r], |p[r] - p[c]|^2) over its rows and writes its own (max, row) to part[t & 1].  Launch 0 takes c = start and
// sets mind[r] = |p[r] - p[start]|^2.  The last launch is one workgroup that only reduces and records.  Kernel boundaries order the
// partials between workgroups of different launches.
//
// Grid invariance: each row's distance is summed by the 16 lanes of one group in one fixed order (lane l: float4 chunks l, l + 16,
// ... of the row, each as four explicit fmaf; then a butterfly over the 16 lanes), whatever the workgroup count G and whichever
// workgroup owns the row; the partials only select (lexicographic: larger value, then smaller row), so sel and rad are the same
// bits for every G.
#include "common.h"
#include "ssad.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int CS_NT = 256;                          // threads per workgroup
constexpr int CS_LANES = 16;                        // lanes that sum one row
constexpr int CS_ROWS = 8;                          // rows per lane group and pass (loads in flight)
constexpr int CS_TILE = CS_NT / CS_LANES * CS_ROWS; // 128 rows per workgroup pass
constexpr int CS_MAX_D = 1024;

struct CsPair {
    float v;
    int i;
};

__device__ __forceinline__ bool cs_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// (v, i) <- the best of the workgroup, in every thread.  rv / ri: LDS of CS_NT / 64 entries each
__device__ __forceinline__ void cs_block_best(float& v, int& i, float* rv, int* ri) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (cs_better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        rv[threadIdx.x >> 6] = v;
        ri[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    v = rv[0];
    i = ri[0];
#pragma unroll
    for (int w = 1; w < CS_NT / 64; ++w)
        if (cs_better(rv[w], ri[w], v, i)) {
            v = rv[w];
            i = ri[w];
        }
}

// step t of the selection.  update == 0: only reduce the partials and record (the last step; one workgroup)
__global__ __launch_bounds__(CS_NT) void coreset_step_kernel(const float* __restrict__ p, int R, int d, int start, int t, int update,
                                                             float* __restrict__ mind, CsPair* __restrict__ part, int G,
                                                             int64_t* __restrict__ sel, float* __restrict__ rad, int* __restrict__ m_out) {
    __shared__ f32x4 cen[CS_MAX_D / 4];
    __shared__ float rv[CS_NT / 64];
    __shared__ int ri[CS_NT / 64];
    const CsPair* prev = part + (size_t)((t + 1) & 1) * G;
    CsPair* cur = part + (size_t)(t & 1) * G;
    int c;
    float radius;
    if (t == 0) {
        c = start;
        radius = INFINITY;
    } else {
        float v = -1.0f;
        int i = INT_MAX;
        for (int g = threadIdx.x; g < G; g += CS_NT) {
            const CsPair q = prev[g];
            if (cs_better(q.v, q.i, v, i)) {
                v = q.v;
                i = q.i;
            }
        }
        cs_block_best(v, i, rv, ri);
        c = i;
        radius = v;
        if (!(radius > 0.0f)) {
            // every row lies on a centre already: no centre is recorded, and the partials go on unchanged so that later steps stop too
            if (update && threadIdx.x == 0) cur[blockIdx.x] = prev[blockIdx.x];
            return;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sel[t] = c;
        rad[t] = radius;
        *m_out = t + 1;
    }
    if (!update) return;

    const int d4 = d >> 2;
    const f32x4* crow = (const f32x4*)(p + (int64_t)c * d);
    for (int j = threadIdx.x; j < d4; j += CS_NT) cen[j] = crow[j];
    __syncthreads();

    const int rpw = (int)(((int64_t)R + G - 1) / G);
    const int r0 = (int)min((int64_t)blockIdx.x * rpw, (int64_t)R);
    const int r1 = (int)min((int64_t)r0 + rpw, (int64_t)R);
    const int lane = threadIdx.x & (CS_LANES - 1);
    const int grp = threadIdx.x / CS_LANES;
    float bv = -1.0f;
    int bi = INT_MAX;
    for (int base = r0; base < r1; base += CS_TILE) {
        float acc[CS_ROWS];
#pragma unroll
        for (int k = 0; k < CS_ROWS; ++k) acc[k] = 0.0f;
        for (int j = lane; j < d4; j += CS_LANES) {
            const f32x4 cj = cen[j];
            f32x4 x[CS_ROWS];
#pragma unroll
            for (int k = 0; k < CS_ROWS; ++k) {
                const int r = base + grp + (CS_NT / CS_LANES) * k;
                x[k] = r < r1 ? ((const f32x4*)(p + (int64_t)r * d))[j] : cj;
            }
#pragma unroll
            for (int k = 0; k < CS_ROWS; ++k) {
                const f32x4 df = x[k] - cj;
                acc[k] = fmaf(df[0], df[0], acc[k]);
                acc[k] = fmaf(df[1], df[1], acc[k]);
                acc[k] = fmaf(df[2], df[2], acc[k]);
                acc[k] = fmaf(df[3], df[3], acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < CS_ROWS; ++k) {
#pragma unroll
            for (int o = CS_LANES / 2; o >= 1; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
            const int r = base + grp + (CS_NT / CS_LANES) * k;
            if (r < r1) {
                const float m = t == 0 ? acc[k] : fminf(mind[r], acc[k]);
                if (lane == 0) mind[r] = m;
                if (cs_better(m, r, bv, bi)) {
                    bv = m;
                    bi = r;
                }
            }
        }
    }
    __syncthreads();    // rv / ri may still be read by the partial reduction above
    cs_block_best(bv, bi, rv, ri);
    if (threadIdx.x == 0) cur[blockIdx.x] = CsPair{bv, bi};
}

}  // namespace

extern "C" int ssad_coreset_greedy(const float* p, int64_t R, int d, int m, int64_t start, int wgs, float* mind, void* part,
                                   int64_t* sel, float* rad, int* m_out, void* stream) {
    SSAD_CHECK_ARG(p && mind && part && sel && rad && m_out, "null pointer");
    SSAD_CHECK_ARG(R >= 1 && R <= (int64_t)INT_MAX - 4096, "R in 1..2^31 - 4097");
    SSAD_CHECK_ARG(d >= 4 && d % 4 == 0 && d <= CS_MAX_D, "d must be a multiple of 4, at most 1024");
    SSAD_CHECK_ARG(((uintptr_t)p & 15) == 0, "p must be 16-byte aligned");
    SSAD_CHECK_ARG(m >= 1, "m >= 1");
    SSAD_CHECK_ARG(start >= 0 && start < R, "start must be a row of p");
    SSAD_CHECK_ARG(wgs >= 1 && wgs <= 65535, "wgs in 1..65535");
    // the selection never records more than R centres: the (R + 1)-th step would find every row on a centre
    const int steps = (int)(m < R ? m : R);
    hipStream_t st = (hipStream_t)stream;
    CsPair* pp = (CsPair*)part;
    for (int t = 0; t < steps; ++t) {
        const int update = t + 1 < steps;
        hipLaunchKernelGGL(coreset_step_kernel, dim3(update ? (unsigned)wgs : 1u), dim3(CS_NT), 0, st, p, (int)R, d, (int)start, t,
                           update, mind, pp, wgs, sel, rad, m_out);
        SSAD_CHECK_LAUNCH();
    }
    return 0;
}
