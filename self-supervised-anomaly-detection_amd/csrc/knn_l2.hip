// Euclidean k-NN scoring (PatchCore / SPADE's metric; opt-in beside the cosine kernels of knn.hip): the distance of a query q to a bank
// row b is d = sqrt(max(|q|^2 + |b|^2 - 2 <q, b>, 0)) on the raw rows -- the expanded form torch.cdist evaluates -- formed in fp32:
//   <q, b>       the MFMA chain of knn.hip's tile (same tile, same K order, same staging) on UNNORMALISED operands,
//   |q|^2, |b|^2 one summation order (sqnorm_wave: lane-strided fma, xor butterfly) wherever they are taken, so equal rows give equal bits,
//   d2           fmaxf((qn + bn) - 2 dot, 0) in the per-tile epilogue; the K loop is knn.hip's, untouched by the metric.
// Selection runs on d2 (monotone in d); sqrtf is applied to the k winners only.  One kernel template serves the four entry points:
// mean or (distance, row) keys, one launch (S = 1) or the bank split of ssad_cosine_knn_split with a merge launch.
#include "common.h"

namespace {

constexpr int BB = 128, BQ = 128, BK = 32, LDK = BK + 4, TB = 2, TQ = 2, NT = 256;      // knn.hip's tile: bank rows x queries
constexpr int STAGE = (BB + BQ) * LDK;          // floats
constexpr int LDS_BYTES = (2 * STAGE + BQ + BB) * 4;
constexpr unsigned OOB = 0x80000000u;   // size given to the buffers: offsets from here on read zeros
constexpr int SRD3 = 0x00020000;        // raw buffer, 32-bit data format

typedef unsigned long long u64;
constexpr u64 NOKEY = ~0ull;

__device__ __forceinline__ void keep3(float v, float& a, float& b, float& c) {
    c = fminf(c, fmaxf(b, v));
    b = fminf(b, fmaxf(a, v));
    a = fminf(a, v);
}
__device__ __forceinline__ u64 umin64(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a < b ? b : a; }
__device__ __forceinline__ void keep3(u64 v, u64& a, u64& b, u64& c) {
    c = umin64(c, umax64(b, v));
    b = umin64(b, umax64(a, v));
    a = umin64(a, v);
}
__device__ __forceinline__ float shfl_xor_any(float v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ u64 shfl_xor_any(u64 v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    return ((u64)hi << 32) | lo;
}

// sum x^2 of one row by one wave -- THE summation order of every squared norm in this file: lane l takes elements l, l + 64, ... in
// an fma chain, then an xor butterfly (every lane ends with the sum).  The prologue below runs the same chain for eight rows at once.
__device__ __forceinline__ float sqnorm_wave(const float* __restrict__ row, int D, int lane) {
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s = __builtin_fmaf(row[k], row[k], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

__global__ __launch_bounds__(NT) void row_sqnorms_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t N, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= N) return;
    const float s = sqnorm_wave(x + row * D, D, lane);
    if (lane == 0) out[row] = s;
}

struct L2Params {
    const float* x;       // [N][D] queries
    const float* bank;    // [R][D] bank rows (not normalised)
    const float* bsq;     // [R] squared norms of the bank rows (ssad_row_sqnorms)
    void* part;           // [S][N][3] floats (d2) or 64-bit keys of each query over each split, ascending (S > 1 only)
    float* out;           // [N] mean form
    float* dist;          // [N][k] index form
    int* idx;             // [N][k] index form
    int64_t N;
    int D, R, rows_per, k;
};

template <bool KEYS> struct Sel;
template <> struct Sel<false> {
    typedef float T;
    static __device__ __forceinline__ float none() { return INFINITY; }
    static __device__ __forceinline__ float make(float d2, int) { return d2; }
};
template <> struct Sel<true> {
    typedef u64 T;
    static __device__ __forceinline__ u64 none() { return NOKEY; }
    // d2 >= 0: its bits order like an unsigned integer, so the key's unsigned order is the lexicographic (d2, row) order
    static __device__ __forceinline__ u64 make(float d2, int row) { return ((u64)__float_as_uint(d2) << 32) | (unsigned)row; }
};

// the k winners of query `row`: the mean of their roots, smallest first, or the (root, bank row) pairs
__device__ __forceinline__ void write_result(const L2Params& p, int64_t row, float a, float b, float c) {
    float s = sqrtf(a);
    if (p.k > 1) s += sqrtf(b);
    if (p.k > 2) s += sqrtf(c);
    p.out[row] = s / (float)p.k;
}
__device__ __forceinline__ void write_result(const L2Params& p, int64_t row, u64 a, u64 b, u64 c) {
    const u64 key[3] = {a, b, c};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < p.k) {
            p.dist[row * p.k + j] = sqrtf(__uint_as_float((unsigned)(key[j] >> 32)));
            p.idx[row * p.k + j] = (int)(unsigned)key[j];
        }
    }
}

// Grid (ceil(N / 128), S): workgroup (t, s) scores queries [128 t, 128 t + 128) against the bank rows [s rows_per, (s + 1) rows_per).
// Matrix loop, staging (buffer loads: rows past N or R read zeros) and the place of a bank row in its tile are
// cosine_knn_index_kernel's (knn.hip); the operands go to LDS as they are.
template <bool KEYS>
__global__ __launch_bounds__(NT, 2) void l2_knn_kernel(L2Params p) {
    typedef typename Sel<KEYS>::T T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* qn_s = lds + 2 * STAGE;              // [BQ] squared norms of the queries
    float* bn_s = qn_s + BQ;                    // [BB] squared norms of the current bank tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wb = wave >> 1, wq = wave & 1;    // 64-row bank block / 64-query block of this wave
    const int64_t m0 = (int64_t)blockIdx.x * BQ;
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc of rows sr + 32 i

    // ---- squared query norms: sqnorm_wave's order, eight rows in flight per wave (knn.hip's prologue); rows past N give 0 ----
    for (int base = wave; base < BQ; base += 32) {
        float s[8];
        const float* q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t row = m0 + base + 4 * u;
            q[u] = row < p.N ? p.x + row * p.D : nullptr;
            s[u] = 0.f;
        }
        for (int k = lane; k < p.D; k += 64) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = q[u] ? q[u][k] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u] = __builtin_fmaf(v[u], v[u], s[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float t = s[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == 0) qn_s[base + 4 * u] = t;
        }
    }
    unsigned qoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qoff[i] = m0 + sr + 32 * i < p.N ? (unsigned)(((sr + 32 * i) * p.D + sc * 4) * 4) : OOB;
    const float* xblk = p.x + m0 * p.D;

    // running three smallest of this lane's queries (column r of its TQ query blocks) over the bank rows it has seen
    T best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = Sel<KEYS>::none();
    const int nks = p.D / BK;
    const int64_t r_begin = (int64_t)blockIdx.y * p.rows_per;
    const int r_end = (int)(r_begin + p.rows_per < p.R ? r_begin + p.rows_per : p.R);

    for (int n0 = (int)(r_begin < p.R ? r_begin : p.R); n0 < r_end; n0 += BB) {
        unsigned boff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) boff[i] = n0 + sr + 32 * i < p.R ? (unsigned)(((sr + 32 * i) * p.D + sc * 4) * 4) : OOB;
        const float* bblk = p.bank + (int64_t)n0 * p.D;
        f32x16 acc[TB][TQ];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        f32x4 rq[4], rb[4];
        auto load = [&](int ks) {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(xblk + ks * BK), 0, (int)OOB, SRD3);
            const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(bblk + ks * BK), 0, (int)OOB, SRD3);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                rq[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, qoff[i], 0, 0));
                rb[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, boff[i], 0, 0));
            }
        };
        auto store = [&](float* st) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *(f32x4*)(st + (sr + 32 * i) * LDK + sc * 4) = rb[i];                   // bank rows: the tile's M side
                *(f32x4*)(st + BB * LDK + (sr + 32 * i) * LDK + sc * 4) = rq[i];        // queries: its N side
            }
        };
        __syncthreads();                        // every wave has left the previous bank tile's last stage and its norms
        load(0);
        if (tid < BB) bn_s[tid] = n0 + tid < p.R ? p.bsq[n0 + tid] : 0.f;
        store(lds);
        __syncthreads();
        for (int ks = 0; ks < nks; ++ks) {
            const float* cur = lds + (ks & 1) * STAGE;
            if (ks + 1 < nks) load(ks + 1);
            const float* As = cur + (wb * 32 * TB + r) * LDK + h * 4;
            const float* Bs = cur + BB * LDK + (wq * 32 * TQ + r) * LDK + h * 4;
#pragma unroll
            for (int kk = 0; kk < BK / 8; ++kk) {
                f32x4 a[TB], b[TQ];
#pragma unroll
                for (int i = 0; i < TB; ++i) a[i] = *(const f32x4*)(As + i * 32 * LDK + kk * 8);
#pragma unroll
                for (int j = 0; j < TQ; ++j) b[j] = *(const f32x4*)(Bs + j * 32 * LDK + kk * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TB; ++i)
#pragma unroll
                        for (int j = 0; j < TQ; ++j) acc[i][j] = mfma32(a[i][e], b[j][e], acc[i][j]);
            }
            if (ks + 1 < nks) store(lds + ((ks + 1) & 1) * STAGE);
            __syncthreads();
        }
        // ---- the finished tile: register e of lane (r, h) in block (i, j) is bank row row0 + (e & 3) + 8 (e >> 2) of query column r ----
        float qn[TQ];
#pragma unroll
        for (int j = 0; j < TQ; ++j) qn[j] = qn_s[(wq * TQ + j) * 32 + r];
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const int l0 = (wb * TB + i) * 32 + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bn = *(const f32x4*)(bn_s + l0 + 8 * g);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int e = 4 * g + c;
                    const int row = n0 + l0 + c + 8 * g;
                    const bool ok = row < p.R;
#pragma unroll
                    for (int j = 0; j < TQ; ++j) {
                        const float d2 = fmaxf((qn[j] + bn[c]) - 2.f * acc[i][j][e], 0.f);
                        keep3(ok ? Sel<KEYS>::make(d2, row) : Sel<KEYS>::none(), best[j][0], best[j][1], best[j][2]);
                    }
                }
            }
        }
    }
    // ---- a query's candidates sit in the two lane halves of two waves (wb = 0, 1): halves by shuffle, waves through LDS ----
    __syncthreads();                            // the stages are dead
    T* M = (T*)lds;                             // [2 wq][TQ][32][3]
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
        const T oa = shfl_xor_any(best[j][0], 32), ob = shfl_xor_any(best[j][1], 32), oc = shfl_xor_any(best[j][2], 32);
        keep3(oa, best[j][0], best[j][1], best[j][2]);
        keep3(ob, best[j][0], best[j][1], best[j][2]);
        keep3(oc, best[j][0], best[j][1], best[j][2]);
        if (wb == 1 && h == 0) {
            T* m = M + ((wq * TQ + j) * 32 + r) * 3;
            m[0] = best[j][0]; m[1] = best[j][1]; m[2] = best[j][2];
        }
    }
    __syncthreads();
    if (wb == 0 && h == 0) {
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const T* m = M + ((wq * TQ + j) * 32 + r) * 3;
            T a = best[j][0], b = best[j][1], c = best[j][2];
            keep3(m[0], a, b, c);
            keep3(m[1], a, b, c);
            keep3(m[2], a, b, c);
            const int64_t row = m0 + (wq * TQ + j) * 32 + r;
            if (row < p.N) {
                if (gridDim.y == 1) {
                    write_result(p, row, a, b, c);
                } else {
                    T* o = (T*)p.part + ((int64_t)blockIdx.y * p.N + row) * 3;
                    o[0] = a; o[1] = b; o[2] = c;
                }
            }
        }
    }
}

// the three smallest of the S triples of query n (min / max selection: any order gives the same three), then the one-launch epilogue
template <bool KEYS>
__global__ void l2_knn_merge_kernel(L2Params p, int S) {
    typedef typename Sel<KEYS>::T T;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= p.N) return;
    T a = Sel<KEYS>::none(), b = a, c = a;
    for (int s = 0; s < S; ++s) {
        const T* t = (const T*)p.part + ((int64_t)s * p.N + n) * 3;
        keep3(t[0], a, b, c);
        keep3(t[1], a, b, c);
        keep3(t[2], a, b, c);
    }
    write_result(p, n, a, b, c);
}

template <bool KEYS>
static int l2_knn_launch(L2Params p, int S, void* stream) {
    p.rows_per = (int)(cdiv64(cdiv64(p.R, BB), S) * BB);
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(l2_knn_kernel<KEYS>, LDS_BYTES);
        attr_set = true;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(l2_knn_kernel<KEYS>, dim3((unsigned)cdiv64(p.N, BQ), (unsigned)S), dim3(NT), LDS_BYTES, st, p);
    SSAD_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(l2_knn_merge_kernel<KEYS>, dim3((unsigned)cdiv64(p.N, 256)), dim3(256), 0, st, p, S);
        SSAD_CHECK_LAUNCH();
    }
    return 0;
}

// ================================================ image score (PatchCore eq. 6-7) ================================================
constexpr int MAX_B = 32;

__global__ void l2_from_dots_kernel(const float* __restrict__ sim, const float* __restrict__ qsq, const float* __restrict__ bsq,
                                    float* __restrict__ out, int R) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= R) return;
    const int64_t i = (int64_t)blockIdx.y * R + c;
    out[i] = fmaxf((qsq[blockIdx.y] + bsq[c]) - 2.f * sim[i], 0.f);
}

// image_score.hip's knn_reweight_kernel for the Euclidean distance; grid (Q).  d(x, r) = sqrt(sum (x - B_r)^2) by direct differences,
// a wave per bank row (lane-strided fma chain, xor butterfly); the weight in the shifted form -- distances are not bounded, and expf
// overflows above 88 -- 1 - exp(d(x, m) - dmax) / sum_j exp(d(x, nbr_j) - dmax), dmax the largest of the bp neighbour distances,
// the exponentials added in neighbour order by one thread.
__global__ __launch_bounds__(NT) void knn_reweight_l2_kernel(const float* __restrict__ xs, const float* __restrict__ bank,
                                                             const int* __restrict__ mstar, const int* __restrict__ nbr,
                                                             const float* __restrict__ smax, float* __restrict__ out, int D, int R,
                                                             int bp) {
    __shared__ float dl[MAX_B + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = xs + (int64_t)blockIdx.x * D;
    for (int j = wave; j <= bp; j += NT / 64) {             // j = bp: the nearest row itself (the numerator)
        const int row = j < bp ? nbr[(int64_t)blockIdx.x * bp + j] : mstar[blockIdx.x];
        float s = 0.f;
        if ((unsigned)row < (unsigned)R) {
            const float* br = bank + (int64_t)row * D;
            for (int k = lane; k < D; k += 64) {
                const float t = x[k] - br[k];
                s = __builtin_fmaf(t, t, s);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) dl[j] = sqrtf(s);
    }
    __syncthreads();
    if (tid == 0) {
        float dmax = dl[0];
        for (int j = 1; j < bp; ++j) dmax = fmaxf(dmax, dl[j]);
        float sum = 0.f;
        for (int j = 0; j < bp; ++j) sum += expf(dl[j] - dmax);
        out[blockIdx.x] = (1.f - expf(dl[bp] - dmax) / sum) * smax[blockIdx.x];
    }
}

}  // namespace

#define SSAD_L2_KNN_CHECKS()                                                                                    \
    SSAD_CHECK_ARG(D % BK == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");                     \
    SSAD_CHECK_ARG(k >= 1 && k <= 3 && k <= R, "k in 1..3 and <= bank rows");                                   \
    SSAD_CHECK_ARG(cdiv64(N, BQ) < (int64_t)2147483647, "too many rows for one launch")

// out[n] = sum x[n][:]^2 in fp32, one wave per row in one fixed order (independent of N and of the row's place): equal rows give equal bits.
extern "C" int ssad_row_sqnorms(const float* x, float* out, int64_t N, int D, void* stream) {
    SSAD_CHECK_ARG(x && out && N > 0 && D > 0, "bad argument");
    SSAD_CHECK_ARG(cdiv64(N, NT / 64) < (int64_t)2147483647, "too many rows for one launch");
    hipLaunchKernelGGL(row_sqnorms_kernel, dim3((unsigned)cdiv64(N, NT / 64)), dim3(NT), 0, (hipStream_t)stream, x, out, N, D);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// out[n] = mean of the sqrt of the k (1..3) smallest d2 = max(|x_n|^2 + |b_r|^2 - 2 <x_n, b_r>, 0) over the R bank rows, added smallest
// first; bank_sq = ssad_row_sqnorms(bank).  One launch.
extern "C" int ssad_l2_knn_fused(const float* x, const float* bank, const float* bank_sq, float* out, int64_t N, int D, int R, int k,
                                 void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2_KNN_CHECKS();
    return l2_knn_launch<false>(L2Params{x, bank, bank_sq, nullptr, out, nullptr, nullptr, N, D, R, 0, k}, 1, stream);
}

// The bank split of ssad_cosine_knn_split for ssad_l2_knn_fused: part [S][N][3] floats (caller-owned), a second launch merges them.
// out is the same bits for every S.
extern "C" int ssad_l2_knn_split(const float* x, const float* bank, const float* bank_sq, float* part, float* out, int64_t N, int D,
                                 int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && part && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2_KNN_CHECKS();
    SSAD_CHECK_ARG(S >= 1 && S <= 65535, "S in 1..65535");
    return l2_knn_launch<false>(L2Params{x, bank, bank_sq, part, out, nullptr, nullptr, N, D, R, 0, k}, S, stream);
}

// kneighbors of the Euclidean bank: the k smallest (d2, bank row) pairs of every query in lexicographic order, dist [N][k] = sqrt(d2)
// and idx [N][k] int32 -- the distances are the bits ssad_l2_knn_fused averages, equal d2 go to the smaller row.  One launch.
extern "C" int ssad_l2_knn_index(const float* x, const float* bank, const float* bank_sq, float* dist, int* idx, int64_t N, int D, int R,
                                 int k, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2_KNN_CHECKS();
    return l2_knn_launch<true>(L2Params{x, bank, bank_sq, nullptr, nullptr, dist, idx, N, D, R, 0, k}, 1, stream);
}

// The bank split of ssad_l2_knn_index: part [S][N][3] 64-bit keys (caller-owned, 8-byte aligned; not needed for S = 1).
extern "C" int ssad_l2_knn_index_split(const float* x, const float* bank, const float* bank_sq, void* part, float* dist, int* idx,
                                       int64_t N, int D, int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2_KNN_CHECKS();
    SSAD_CHECK_ARG(S >= 1 && S <= 65535 && (S == 1 || part), "S in 1..65535, with a workspace when S > 1");
    SSAD_CHECK_ARG(((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");
    return l2_knn_launch<true>(L2Params{x, bank, bank_sq, part, nullptr, dist, idx, N, D, R, 0, k}, S, stream);
}

// out[q][r] = max(qsq[q] + bsq[r] - 2 sim[q][r], 0): SQUARED Euclidean distances from a matrix of dot products (the expression of the
// kNN epilogue; the selection of ssad_rows_smallest_index, cosine = 0, runs on them as the kNN selection does).  out may be sim.
extern "C" int ssad_l2_from_dots(const float* sim, const float* qsq, const float* bsq, float* out, int64_t Q, int R, void* stream) {
    SSAD_CHECK_ARG(sim && qsq && bsq && out && Q > 0 && R > 0, "bad argument");
    SSAD_CHECK_ARG(Q <= 65535, "at most 65535 rows");
    hipLaunchKernelGGL(l2_from_dots_kernel, dim3((unsigned)cdiv64(R, 256), (unsigned)Q), dim3(256), 0, (hipStream_t)stream, sim, qsq, bsq,
                       out, R);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// PatchCore's image-score weight on Euclidean distances: out[q] = (1 - exp(d(x_q, mstar[q]) - dmax) / sum_{j < bp} exp(d(x_q, nbr[q][j])
// - dmax)) smax[q], d(x, r) = sqrt(sum (x - bank_r)^2), dmax = max_j d(x_q, nbr[q][j]) (a row outside 0 .. R - 1 counts as distance 0).
// 1 <= bp <= 32.  Fixed-order sums: the same bits on every call.
extern "C" int ssad_knn_reweight_l2(const float* xs, const float* bank, const int* mstar, const int* nbr, const float* smax, float* out,
                                    int64_t Q, int D, int R, int bp, void* stream) {
    SSAD_CHECK_ARG(xs && bank && mstar && nbr && smax && out && Q > 0 && D > 0 && R > 0, "bad argument");
    SSAD_CHECK_ARG(bp >= 1 && bp <= MAX_B, "bp in 1..32");
    SSAD_CHECK_ARG(Q < (int64_t)2147483647, "too many rows for one launch");
    hipLaunchKernelGGL(knn_reweight_l2_kernel, dim3((unsigned)cdiv64(Q, 1)), dim3(NT), 0, (hipStream_t)stream, xs, bank, mstar, nbr, smax,
                       out, D, R, bp);
    SSAD_CHECK_LAUNCH();
    return 0;
}
