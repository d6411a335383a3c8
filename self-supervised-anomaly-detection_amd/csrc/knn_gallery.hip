// SPADE's image-conditioned gallery for the Euclidean kNN detector (Cohen & Hoshen 2020; opt-in beside the whole-bank search of
// knn_l2.hip): every query image is scored against the rows of K bank images only, the ones nearest to it by an image descriptor.
//   ssad_group_means     the image descriptor: the mean of an image's P rows, summed in fp64 in row order, rounded once;
//   ssad_l2_direct       stage 1: squared distances between descriptors by direct differences (no cancellation), a wave per pair;
//   ssad_l2_knn_gallery  stage 2: knn_l2.hip's kernel on an INDIRECT bank -- the bank of query image q is the list of row blocks
//                        [g P, (g + 1) P), g = gallery[q][0 .. K - 1], instead of one contiguous range.
// The tile, the K order, the staging by buffer loads, the norms' summation order, the d2 expression and the min / max selection of
// stage 2 are copies of l2_knn_kernel (knn_l2.hip): a (query, bank row) pair gets the bits it gets there, wherever the row stands.
#include "common.h"

namespace {

constexpr int BB = 128, BQ = 128, BK = 32, LDK = BK + 4, TB = 2, TQ = 2, NT = 256;      // knn_l2.hip's tile: bank rows x queries
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

// ================================================ stage 1: descriptors and their distances ================================================

// grid (ceil(D / 64), G): thread c of workgroup (., g) sums column c of image g's P rows in fp64, rows 0, 1, ..., P - 1 in that order
// (eight loads in flight, added in row order), and rounds once: the bits depend on the image's rows alone, not on G or on g.
__global__ __launch_bounds__(64) void group_means_kernel(const float* __restrict__ x, float* __restrict__ out, int P, int D) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= D) return;
    const float* col = x + (int64_t)blockIdx.y * P * D + c;
    double s = 0.0;
    int r = 0;
    for (; r + 8 <= P; r += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = col[(int64_t)(r + u) * D];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)v[u];
    }
    for (; r < P; ++r) s += (double)col[(int64_t)r * D];
    out[(int64_t)blockIdx.y * D + c] = (float)(s / (double)P);
}

// grid (ceil(T / 4), Q): wave w of workgroup (i, q) takes the pair (q, 4 i + w) in sqnorm_wave's order (knn_l2.hip): lane l the
// elements l, l + 64, ... in an fma chain of squared differences, then the xor butterfly.  Every term is >= 0.
__global__ __launch_bounds__(NT) void l2_direct_kernel(const float* __restrict__ q, const float* __restrict__ b, float* __restrict__ out,
                                                       int T, int D) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (t >= T) return;
    const float* qr = q + (int64_t)blockIdx.y * D;
    const float* br = b + (int64_t)t * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float d = qr[k] - br[k];
        s = __builtin_fmaf(d, d, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[(int64_t)blockIdx.y * T + t] = s;
}

// ================================================ stage 2: the kNN over a gallery ================================================

struct GParams {
    const float* x;       // [Q P][D] queries, image after image
    const float* bank;    // [T P][D] bank rows, image after image (not normalised)
    const float* bsq;     // [T P] squared norms of the bank rows (ssad_row_sqnorms)
    const int* gallery;   // [Q][K] bank images of every query image; an entry outside 0 .. T - 1 is skipped
    void* part;           // [S][Q P][3] floats (d2) or 64-bit keys of each query over each split, ascending (S > 1 only)
    float* out;           // [Q P] mean form
    float* dist;          // [Q P][k] index form
    int* idx;             // [Q P][k] index form
    int Q, P, T, K, D, k, per;      // per: gallery entries of one split
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
    // d2 >= 0: its bits order like an unsigned integer, so the key's unsigned order is the lexicographic (d2, global row) order
    static __device__ __forceinline__ u64 make(float d2, int row) { return ((u64)__float_as_uint(d2) << 32) | (unsigned)row; }
};

// the k winners of query `row`: the mean of their roots, smallest first (+inf when the gallery left fewer than k rows), or the
// (root, global bank row) pairs, a missing one (+inf, -1)
__device__ __forceinline__ void write_result(const GParams& p, int64_t row, float a, float b, float c) {
    float s = sqrtf(a);
    if (p.k > 1) s += sqrtf(b);
    if (p.k > 2) s += sqrtf(c);
    p.out[row] = s / (float)p.k;
}
__device__ __forceinline__ void write_result(const GParams& p, int64_t row, u64 a, u64 b, u64 c) {
    const u64 key[3] = {a, b, c};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < p.k) {
            const bool have = key[j] != NOKEY;
            p.dist[row * p.k + j] = have ? sqrtf(__uint_as_float((unsigned)(key[j] >> 32))) : INFINITY;
            p.idx[row * p.k + j] = have ? (int)(unsigned)key[j] : -1;
        }
    }
}

// Grid (ceil(P / 128), Q, S): workgroup (t, q, s) scores the queries [128 t, 128 t + 128) of image q -- a query tile never straddles
// two images -- against the gallery entries [s per, (s + 1) per) of that image.  For an entry g it walks the 128-row tiles of the bank
// rows [g P, (g + 1) P); rows past the block's end are masked (they read zeros and make no candidate), never taken from image g + 1.
// An entry outside 0 .. T - 1 is skipped before anything is addressed with it.  Everything inside a tile is l2_knn_kernel's.
template <bool KEYS>
__global__ __launch_bounds__(NT, 2) void l2_knn_gallery_kernel(GParams p) {
    typedef typename Sel<KEYS>::T T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* qn_s = lds + 2 * STAGE;              // [BQ] squared norms of the queries
    float* bn_s = qn_s + BQ;                    // [BB] squared norms of the current bank tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wb = wave >> 1, wq = wave & 1;    // 64-row bank block / 64-query block of this wave
    const int m0 = (int)blockIdx.x * BQ;        // first query of the tile within its image
    const int64_t q0 = (int64_t)blockIdx.y * p.P + m0;     // ... among all queries
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc of rows sr + 32 i

    // ---- squared query norms: sqnorm_wave's order, eight rows in flight per wave; rows past the image's end give 0 ----
    for (int base = wave; base < BQ; base += 32) {
        float s[8];
        const float* q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = m0 + base + 4 * u;
            q[u] = row < p.P ? p.x + (q0 + base + 4 * u) * p.D : nullptr;
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
    for (int i = 0; i < 4; ++i) qoff[i] = m0 + sr + 32 * i < p.P ? (unsigned)(((sr + 32 * i) * p.D + sc * 4) * 4) : OOB;
    const float* xblk = p.x + q0 * p.D;

    // running three smallest of this lane's queries (column r of its TQ query blocks) over the bank rows it has seen
    T best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = Sel<KEYS>::none();
    const int nks = p.D / BK;
    const int e_begin = (int)blockIdx.z * p.per;
    const int e_end = e_begin + p.per < p.K ? e_begin + p.per : p.K;
    const int* gal = p.gallery + (int64_t)blockIdx.y * p.K;

    for (int en = e_begin; en < e_end; ++en) {
        const int g = __builtin_amdgcn_readfirstlane(gal[en]);      // one value for the whole workgroup
        if ((unsigned)g >= (unsigned)p.T) continue;                 // not a bank image: never dereferenced
        const int64_t g0 = (int64_t)g * p.P;                        // first global row of the block
        for (int n0 = 0; n0 < p.P; n0 += BB) {
            unsigned boff[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) boff[i] = n0 + sr + 32 * i < p.P ? (unsigned)(((sr + 32 * i) * p.D + sc * 4) * 4) : OOB;
            const float* bblk = p.bank + (g0 + n0) * p.D;
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
            if (tid < BB) bn_s[tid] = n0 + tid < p.P ? p.bsq[g0 + n0 + tid] : 0.f;
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
            // ---- the finished tile: register e of lane (r, h) in block (i, j) is row l0 + (e & 3) + 8 (e >> 2) of the tile, query column r ----
            float qn[TQ];
#pragma unroll
            for (int j = 0; j < TQ; ++j) qn[j] = qn_s[(wq * TQ + j) * 32 + r];
#pragma unroll
            for (int i = 0; i < TB; ++i) {
                const int l0 = (wb * TB + i) * 32 + 4 * h;
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    const f32x4 bn = *(const f32x4*)(bn_s + l0 + 8 * gg);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int e = 4 * gg + c;
                        const int local = n0 + l0 + c + 8 * gg;     // row within the image's block
                        const bool ok = local < p.P;
                        const int row = (int)g0 + local;            // global bank row (T P fits an int: checked by the host)
#pragma unroll
                        for (int j = 0; j < TQ; ++j) {
                            const float d2 = fmaxf((qn[j] + bn[c]) - 2.f * acc[i][j][e], 0.f);
                            keep3(ok ? Sel<KEYS>::make(d2, row) : Sel<KEYS>::none(), best[j][0], best[j][1], best[j][2]);
                        }
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
        const int64_t N = (int64_t)p.Q * p.P;
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const T* m = M + ((wq * TQ + j) * 32 + r) * 3;
            T a = best[j][0], b = best[j][1], c = best[j][2];
            keep3(m[0], a, b, c);
            keep3(m[1], a, b, c);
            keep3(m[2], a, b, c);
            const int local = m0 + (wq * TQ + j) * 32 + r;
            if (local < p.P) {
                const int64_t row = (int64_t)blockIdx.y * p.P + local;
                if (gridDim.z == 1) {
                    write_result(p, row, a, b, c);
                } else {
                    T* o = (T*)p.part + ((int64_t)blockIdx.z * N + row) * 3;
                    o[0] = a; o[1] = b; o[2] = c;
                }
            }
        }
    }
}

// the three smallest of the S triples of query n (min / max selection: any order gives the same three), then the one-launch epilogue
template <bool KEYS>
__global__ void l2_knn_gallery_merge_kernel(GParams p, int S) {
    typedef typename Sel<KEYS>::T T;
    const int64_t N = (int64_t)p.Q * p.P;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    T a = Sel<KEYS>::none(), b = a, c = a;
    for (int s = 0; s < S; ++s) {
        const T* t = (const T*)p.part + ((int64_t)s * N + n) * 3;
        keep3(t[0], a, b, c);
        keep3(t[1], a, b, c);
        keep3(t[2], a, b, c);
    }
    write_result(p, n, a, b, c);
}

template <bool KEYS>
static int l2_knn_gallery_launch(GParams p, int S, void* stream) {
    p.per = (int)cdiv64(p.K, S);
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(l2_knn_gallery_kernel<KEYS>, LDS_BYTES);
        attr_set = true;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(l2_knn_gallery_kernel<KEYS>, dim3((unsigned)cdiv64(p.P, BQ), (unsigned)p.Q, (unsigned)S), dim3(NT), LDS_BYTES, st,
                       p);
    SSAD_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(l2_knn_gallery_merge_kernel<KEYS>, dim3((unsigned)cdiv64((int64_t)p.Q * p.P, 256)), dim3(256), 0, st, p, S);
        SSAD_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

#define SSAD_L2_KNN_GALLERY_CHECKS()                                                                                        \
    SSAD_CHECK_ARG(Q > 0 && Q <= 65535 && P > 0 && T > 0 && K > 0, "Q in 1..65535, P, T and K >= 1");                       \
    SSAD_CHECK_ARG(D > 0 && D % BK == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");                        \
    SSAD_CHECK_ARG((int64_t)T * P <= (int64_t)2147483647 && (int64_t)Q * P <= (int64_t)2147483647, "too many rows");        \
    SSAD_CHECK_ARG(k >= 1 && k <= 3 && (int64_t)K * P >= k, "k in 1..3 and <= the K P rows of a gallery");                  \
    SSAD_CHECK_ARG(S >= 1 && S <= 65535 && (S == 1 || part), "S in 1..65535, with a workspace when S > 1")

// out[g][c] = the mean of x[g P + i][c], i = 0 .. P - 1: the image descriptor of the gallery (the global average of an image's
// locally aware rows).  fp64 sum in row order, one rounding to fp32: an image's descriptor is the same bits in every batch.
extern "C" int ssad_group_means(const float* x, float* out, int64_t G, int P, int D, void* stream) {
    SSAD_CHECK_ARG(x && out && G > 0 && P > 0 && D > 0, "bad argument");
    SSAD_CHECK_ARG(G <= 65535, "at most 65535 groups");
    hipLaunchKernelGGL(group_means_kernel, dim3((unsigned)cdiv64(D, 64), (unsigned)G), dim3(64), 0, (hipStream_t)stream, x, out, P, D);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// out[q][t] = sum_c (q[q][c] - b[t][c])^2 by direct differences, one wave per pair in one fixed order: the bits of a pair do not
// depend on Q or T.
extern "C" int ssad_l2_direct(const float* q, const float* b, float* out, int64_t Q, int T, int D, void* stream) {
    SSAD_CHECK_ARG(q && b && out && Q > 0 && T > 0 && D > 0, "bad argument");
    SSAD_CHECK_ARG(Q <= 65535, "at most 65535 rows");
    hipLaunchKernelGGL(l2_direct_kernel, dim3((unsigned)cdiv64(T, NT / 64), (unsigned)Q), dim3(NT), 0, (hipStream_t)stream, q, b, out, T,
                       D);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// ssad_l2_knn_fused / _split with the bank of query image q restricted to the blocks of gallery[q][0 .. K - 1]: out [Q P].
extern "C" int ssad_l2_knn_gallery(const float* x, const float* bank, const float* bank_sq, const int* gallery, float* part, float* out,
                                   int Q, int P, int T, int K, int D, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && gallery && out, "bad argument");
    SSAD_L2_KNN_GALLERY_CHECKS();
    return l2_knn_gallery_launch<false>(GParams{x, bank, bank_sq, gallery, part, out, nullptr, nullptr, Q, P, T, K, D, k, 0}, S, stream);
}

// ssad_l2_knn_index / _index_split over the same galleries: dist / idx [Q P][k], idx the GLOBAL bank row; part: 64-bit keys.
extern "C" int ssad_l2_knn_gallery_index(const float* x, const float* bank, const float* bank_sq, const int* gallery, void* part,
                                         float* dist, int* idx, int Q, int P, int T, int K, int D, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && gallery && dist && idx, "bad argument");
    SSAD_L2_KNN_GALLERY_CHECKS();
    SSAD_CHECK_ARG(((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");
    return l2_knn_gallery_launch<true>(GParams{x, bank, bank_sq, gallery, part, nullptr, dist, idx, Q, P, T, K, D, k, 0}, S, stream);
}
