// Image scores from patch scores (PatchCore, Roth et al. CVPR 2022 §3.3 eq. 6-7, with this project's cosine distance): per image the
// largest patch score and its patch, the b bank rows nearest to a given bank row, and the re-weighting of the largest score by how
// crowded the bank is around the nearest row.  Small kernels beside the index-returning kNN of knn.hip; the reference has no
// counterpart (its patch-level branch returns maps only).
//
// Every selection here is a minimum / maximum over 64-bit keys (order-preserving bits of the value << 32 | position): keys of one
// row are distinct, so the result is the lexicographic (value, position) order whatever the grid, with no atomics.
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr u64 NOKEY = ~0ull;
constexpr int NT = 256;
constexpr int MAX_B = 32;

__device__ __forceinline__ u64 umin64(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a < b ? b : a; }
__device__ __forceinline__ u64 shfl_xor64(u64 v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    return ((u64)hi << 32) | lo;
}
// unsigned integers in the order of the floats (-0 counts as +0, as a comparison sort sees it), and back
__device__ __forceinline__ unsigned ordered_bits(float v) {
    const unsigned u = __float_as_uint(v + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// The b smallest of the n distinct keys key_at(0 .. n - 1), ascending, to out[0 .. b - 1] (NOKEY where n < b): round t takes the
// smallest key above the one of round t - 1.  One workgroup of NT threads; red: 4 keys of LDS.
template <class KeyAt>
__device__ __forceinline__ void select_smallest(KeyAt key_at, int64_t n, int b, u64* out, u64* red) {
    const int tid = threadIdx.x;
    u64 last = 0;
    for (int t = 0; t < b; ++t) {
        u64 m = NOKEY;
        for (int64_t i = tid; i < n; i += NT) {
            const u64 k = key_at(i);
            if (t == 0 || k > last) m = umin64(m, k);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = umin64(m, shfl_xor64(m, o));
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        m = umin64(umin64(red[0], red[1]), umin64(red[2], red[3]));
        __syncthreads();
        if (tid == 0) out[t] = m;
        last = m;
    }
}

// part[q][g][0 .. b - 1]: the b smallest keys of the columns [g chunk, (g + 1) chunk) of row q; grid (G, Q)
__global__ __launch_bounds__(NT) void rows_smallest_part_kernel(const float* __restrict__ m, int R, int b, int cosine, int64_t chunk,
                                                                u64* __restrict__ part) {
    __shared__ u64 red[4];
    const int64_t c0 = (int64_t)blockIdx.x * chunk;
    const int64_t n = c0 >= R ? 0 : (c0 + chunk < R ? chunk : R - c0);
    const float* row = m + (int64_t)blockIdx.y * R + c0;
    u64* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * b;
    select_smallest(
        [&](int64_t i) {
            float v = row[i];
            if (cosine) v = fminf(fmaxf(1.f - v, 0.f), 2.f);     // the distance expression of knn.hip on a similarity
            return ((u64)ordered_bits(v) << 32) | (unsigned)(c0 + i);
        },
        n, b, out, red);
}

// the bp smallest of the G b keys of row q -> vals[q][0 .. bp - 1], cols[q][0 .. bp - 1]; grid (Q)
__global__ __launch_bounds__(NT) void rows_smallest_merge_kernel(const u64* __restrict__ part, int G, int b, int bp,
                                                                 float* __restrict__ vals, int* __restrict__ cols) {
    __shared__ u64 red[4];
    __shared__ u64 sel[MAX_B];
    const u64* keys = part + (int64_t)blockIdx.x * G * b;
    select_smallest([&](int64_t i) { return keys[i]; }, (int64_t)G * b, bp, sel, red);
    __syncthreads();
    if ((int)threadIdx.x < bp) {
        const u64 k = sel[threadIdx.x];
        vals[(int64_t)blockIdx.x * bp + threadIdx.x] = from_ordered_bits((unsigned)(k >> 32));
        cols[(int64_t)blockIdx.x * bp + threadIdx.x] = (int)(unsigned)k;
    }
}

// val[q] = max_p s[q][p], flat[q] = q P + the smallest p that reaches it; grid (Q)
__global__ __launch_bounds__(NT) void rows_argmax_kernel(const float* __restrict__ s, int P, float* __restrict__ val,
                                                         int64_t* __restrict__ flat) {
    __shared__ u64 red[4];
    const int tid = threadIdx.x;
    const float* row = s + (int64_t)blockIdx.x * P;
    u64 m = 0;
    for (int p = tid; p < P; p += NT) m = umax64(m, ((u64)ordered_bits(row[p]) << 32) | (0xffffffffu - (unsigned)p));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = umax64(m, shfl_xor64(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        m = umax64(umax64(red[0], red[1]), umax64(red[2], red[3]));
        val[blockIdx.x] = from_ordered_bits((unsigned)(m >> 32));
        flat[blockIdx.x] = (int64_t)blockIdx.x * P + (0xffffffffu - (unsigned)m);
    }
}

// out[q] = (1 - exp(d(x_q, m_q)) / sum_j exp(d(x_q, nbr[q][j]))) smax[q], d(x, r) = clip(1 - <x / ||x||, bank_r>, 0, 2); grid (Q).
// A wave per bank row: lane-strided products, xor butterfly; the exponentials are added in neighbour order by one thread.
__global__ __launch_bounds__(NT) void knn_reweight_kernel(const float* __restrict__ xs, const float* __restrict__ bank,
                                                          const int* __restrict__ mstar, const int* __restrict__ nbr,
                                                          const float* __restrict__ smax, float* __restrict__ out, int D, int R,
                                                          int bp) {
    __shared__ float dl[MAX_B + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = xs + (int64_t)blockIdx.x * D;
    float ss = 0.f;
    for (int k = lane; k < D; k += 64) ss += x[k] * x[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float nrm = ss == 0.f ? 1.f : sqrtf(ss);          // a zero sum divides by 1, as l2norm_rows_kernel does
    for (int j = wave; j <= bp; j += NT / 64) {             // j = bp: the nearest row itself (the numerator)
        const int row = j < bp ? nbr[(int64_t)blockIdx.x * bp + j] : mstar[blockIdx.x];
        float dot = 0.f;
        if ((unsigned)row < (unsigned)R) {
            const float* br = bank + (int64_t)row * D;
            for (int k = lane; k < D; k += 64) dot += (x[k] / nrm) * br[k];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
        if (lane == 0) dl[j] = fminf(fmaxf(1.f - dot, 0.f), 2.f);
    }
    __syncthreads();
    if (tid == 0) {
        float sum = 0.f;
        for (int j = 0; j < bp; ++j) sum += expf(dl[j]);
        out[blockIdx.x] = (1.f - expf(dl[bp]) / sum) * smax[blockIdx.x];
    }
}

}  // namespace

// The bp = min(b, R) smallest (value, column) pairs of each row of m [Q][R], ascending, lexicographic: vals [Q][bp], cols [Q][bp]
// (numpy's stable argsort, first bp entries; -0 counts as +0; no NaNs).  cosine != 0: the value of a column is
// clip(1 - m[q][c], 0, 2) -- m holds similarities, the selection runs on cosine distances.  wgs (1 .. 4096 / b) workgroups per
// row over contiguous column ranges + one merge workgroup per row; part [Q][wgs][b] 64-bit keys (caller-owned).  The result does not
// depend on wgs.
extern "C" int ssad_rows_smallest_index(const float* m, int64_t Q, int R, int b, int cosine, int wgs, void* part, float* vals, int* cols,
                                        void* stream) {
    SSAD_CHECK_ARG(m && part && vals && cols && Q > 0 && R > 0, "bad argument");
    SSAD_CHECK_ARG(b >= 1 && b <= MAX_B, "b in 1..32");
    SSAD_CHECK_ARG(wgs >= 1 && wgs * b <= 4096, "wgs in 1..4096 / b");
    SSAD_CHECK_ARG(Q <= 65535, "at most 65535 rows");
    SSAD_CHECK_ARG(((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");
    const int bp = b < R ? b : R;
    const int64_t chunk = cdiv64(R, wgs);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rows_smallest_part_kernel, dim3((unsigned)wgs, (unsigned)Q), dim3(NT), 0, st, m, R, b, cosine, chunk, (u64*)part);
    SSAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(rows_smallest_merge_kernel, dim3((unsigned)Q), dim3(NT), 0, st, (const u64*)part, wgs, b, bp, vals, cols);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// val[q] = the largest entry of row q of s [Q][P], flat[q] = q P + its column (the smallest column among equal entries; no NaNs).
extern "C" int ssad_rows_argmax(const float* s, int64_t Q, int P, float* val, int64_t* flat, void* stream) {
    SSAD_CHECK_ARG(s && val && flat && Q > 0 && P > 0, "bad argument");
    SSAD_CHECK_ARG(Q < (int64_t)2147483647, "too many rows for one launch");
    hipLaunchKernelGGL(rows_argmax_kernel, dim3((unsigned)Q), dim3(NT), 0, (hipStream_t)stream, s, P, val, flat);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// PatchCore's image-score weight on cosine distances: out[q] = (1 - exp(d(x_q, mstar[q])) / sum_{j < bp} exp(d(x_q, nbr[q][j]))) smax[q]
// for xs [Q][D] (not normalised), an L2-normalised bank [R][D], mstar [Q] and nbr [Q][bp] bank rows (a row outside 0 .. R - 1 counts
// as distance 1).  1 <= bp <= 32.  Fixed-order sums: the same bits on every call.
extern "C" int ssad_knn_reweight(const float* xs, const float* bank_normalized, const int* mstar, const int* nbr, const float* smax,
                                 float* out, int64_t Q, int D, int R, int bp, void* stream) {
    SSAD_CHECK_ARG(xs && bank_normalized && mstar && nbr && smax && out && Q > 0 && D > 0 && R > 0, "bad argument");
    SSAD_CHECK_ARG(bp >= 1 && bp <= MAX_B, "bp in 1..32");
    SSAD_CHECK_ARG(Q < (int64_t)2147483647, "too many rows for one launch");
    hipLaunchKernelGGL(knn_reweight_kernel, dim3((unsigned)Q), dim3(NT), 0, (hipStream_t)stream, xs, bank_normalized, mstar, nbr, smax,
                       out, D, R, bp);
    SSAD_CHECK_LAUNCH();
    return 0;
}
