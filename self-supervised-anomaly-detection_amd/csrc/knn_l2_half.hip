// Euclidean k-NN scoring with HALF-PRECISION OPERANDS (opt-in beside knn_l2.hip; faiss' GpuIndexFlat useFloat16): queries and bank rows
// are rounded once to fp16 by h (ssad_rows_to_half), the distance is that of the ROUNDED rows,
//   d = sqrt(max(|h(q)|^2 + |h(b)|^2 - 2 <h(q), h(b)>, 0)),
//   <h(q), h(b)>     v_mfma_f32_32x32x16_f16 chains: fp16 products, fp32 accumulation, K in ascending order, 16 per instruction,
//   |h(q)|^2, ...    the rounded rows' squared norms in sqnorm_wave's order (knn_l2.hip), written by the pass that rounds the rows,
//   d2               fmaxf((qn + bn) - 2 dot, 0) in the per-tile epilogue.
// h: fp32 -> fp16 round to nearest even, saturating at +-65504, results below 2^-14 in magnitude flushed to signed zero -- no half
// ever holds inf, NaN or a subnormal.  Selection, tie rule, keys, split and merge are l2_knn_kernel's.  The matrix loop holds no
// conversion and no norm prologue: both operands arrive as halves, both norm vectors as floats.
#include "common.h"

namespace {

constexpr int BB = 128, BQ = 128, BK = 64, LDK = BK + 8, TB = 2, TQ = 2, NT = 256;      // bank rows x queries x halves per K step
constexpr int STAGE = (BB + BQ) * LDK;          // halves; 144-byte rows: the 16 rows of a ds_read_b128 lane group fall on 16 distinct
                                                // 16-byte slots of the 256-byte bank row (36 r mod 64 runs over the multiples of 4)
constexpr int LDS_BYTES = 2 * STAGE * 2 + (BQ + BB) * 4;
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

// h: clamp to the largest finite half first (65504 < v < 65520 would round to it anyway, v >= 65520 to inf), round to nearest even,
// then clear the mantissa of a result whose exponent field is zero (a subnormal half or a zero): signed zero
__device__ __forceinline__ hf round_half(float v) {
    const hf r = (hf)fminf(fmaxf(v, -65504.f), 65504.f);
    unsigned short b = __builtin_bit_cast(unsigned short, r);
    if ((b & 0x7C00u) == 0) b &= 0x8000u;
    return __builtin_bit_cast(hf, b);
}

// One wave per row: element l, l + 64, ... of lane l rounded, stored (2-byte vector stores, 128 contiguous bytes per wave) and squared
// into the lane's fma chain, then the xor butterfly -- sqnorm_wave's order (knn_l2.hip) on the rounded values.
__global__ __launch_bounds__(NT) void rows_to_half_kernel(const float* __restrict__ x, hf* __restrict__ xh, float* __restrict__ sq,
                                                          int64_t N, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* src = x + row * D;
    hf* dst = xh + row * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) {
        const hf r = round_half(src[k]);
        dst[k] = r;
        const float f = (float)r;
        s = __builtin_fmaf(f, f, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) sq[row] = s;
}

struct L2hParams {
    const hf* x;          // [N][D] rounded queries
    const float* xsq;     // [N] their squared norms
    const hf* bank;       // [R][D] rounded bank rows
    const float* bsq;     // [R] their squared norms
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
__device__ __forceinline__ void write_result(const L2hParams& p, int64_t row, float a, float b, float c) {
    float s = sqrtf(a);
    if (p.k > 1) s += sqrtf(b);
    if (p.k > 2) s += sqrtf(c);
    p.out[row] = s / (float)p.k;
}
__device__ __forceinline__ void write_result(const L2hParams& p, int64_t row, u64 a, u64 b, u64 c) {
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
// Four waves, each a 64 x 64 block of the tile (2 x 2 accumulators of v_mfma_f32_32x32x16_f16).  A K step stages 64 halves (128 bytes)
// of 256 rows -- 16-byte buffer loads: rows past N or R and columns past D (the last step of D = 32 mod 64) read zeros, which add
// nothing to a chain -- in two LDS stages; per 16 columns a wave reads two bank and two query fragments (ds_read_b128: the 8 halves
// k = 8 h + j of row r for lane (r, h)) for four MFMAs.  Register e of lane (r, h) in block (i, j) is bank row (e & 3) + 8 (e >> 2) +
// 4 h of query column r, as in the fp32 instruction.
template <bool KEYS>
__global__ __launch_bounds__(NT, 2) void l2h_knn_kernel(L2hParams p) {
    typedef typename Sel<KEYS>::T T;
    extern __shared__ __attribute__((aligned(16))) hf lds[];
    float* qn_s = (float*)(lds + 2 * STAGE);    // [BQ] squared norms of the queries
    float* bn_s = qn_s + BQ;                    // [BB] squared norms of the current bank tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wb = wave >> 1, wq = wave & 1;    // 64-row bank block / 64-query block of this wave
    const int64_t m0 = (int64_t)blockIdx.x * BQ;
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc (8 halves) of rows sr + 32 i

    if (tid < BQ) qn_s[tid] = m0 + tid < p.N ? p.xsq[m0 + tid] : 0.f;
    unsigned qoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qoff[i] = m0 + sr + 32 * i < p.N ? (unsigned)(((sr + 32 * i) * p.D + sc * 8) * 2) : OOB;
    const hf* xblk = p.x + m0 * p.D;

    // running three smallest of this lane's queries (column r of its TQ query blocks) over the bank rows it has seen
    T best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = Sel<KEYS>::none();
    const int nks = (p.D + BK - 1) / BK;
    const int64_t r_begin = (int64_t)blockIdx.y * p.rows_per;
    const int r_end = (int)(r_begin + p.rows_per < p.R ? r_begin + p.rows_per : p.R);

    for (int n0 = (int)(r_begin < p.R ? r_begin : p.R); n0 < r_end; n0 += BB) {
        unsigned boff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) boff[i] = n0 + sr + 32 * i < p.R ? (unsigned)(((sr + 32 * i) * p.D + sc * 8) * 2) : OOB;
        const hf* bblk = p.bank + (int64_t)n0 * p.D;
        f32x16 acc[TB][TQ];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        f16x8 rq[4], rb[4];
        auto load = [&](int ks) {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(xblk + ks * BK), 0, (int)OOB, SRD3);
            const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(bblk + ks * BK), 0, (int)OOB, SRD3);
            const bool in = ks * BK + sc * 8 < p.D;     // this chunk's columns exist (D is a multiple of 32, a chunk is 8 wide)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                rq[i] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, in ? qoff[i] : OOB, 0, 0));
                rb[i] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, in ? boff[i] : OOB, 0, 0));
            }
        };
        auto store = [&](hf* st) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *(f16x8*)(st + (sr + 32 * i) * LDK + sc * 8) = rb[i];                   // bank rows: the tile's M side
                *(f16x8*)(st + BB * LDK + (sr + 32 * i) * LDK + sc * 8) = rq[i];        // queries: its N side
            }
        };
        __syncthreads();                        // every wave has left the previous bank tile's last stage and its norms
        load(0);
        if (tid < BB) bn_s[tid] = n0 + tid < p.R ? p.bsq[n0 + tid] : 0.f;
        store(lds);
        __syncthreads();
        for (int ks = 0; ks < nks; ++ks) {
            const hf* cur = lds + (ks & 1) * STAGE;
            if (ks + 1 < nks) load(ks + 1);
            const hf* As = cur + (wb * 32 * TB + r) * LDK + h * 8;
            const hf* Bs = cur + BB * LDK + (wq * 32 * TQ + r) * LDK + h * 8;
#pragma unroll
            for (int kk = 0; kk < BK / 16; ++kk) {
                f16x8 a[TB], b[TQ];
#pragma unroll
                for (int i = 0; i < TB; ++i) a[i] = *(const f16x8*)(As + i * 32 * LDK + kk * 16);
#pragma unroll
                for (int j = 0; j < TQ; ++j) b[j] = *(const f16x8*)(Bs + j * 32 * LDK + kk * 16);
#pragma unroll
                for (int i = 0; i < TB; ++i)
#pragma unroll
                    for (int j = 0; j < TQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
            if (ks + 1 < nks) store(lds + ((ks + 1) & 1) * STAGE);
            __syncthreads();
        }
        // ---- the finished tile ----
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
__global__ void l2h_knn_merge_kernel(L2hParams p, int S) {
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
static int l2h_knn_launch(L2hParams p, int S, void* stream) {
    p.rows_per = (int)(cdiv64(cdiv64(p.R, BB), S) * BB);
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(l2h_knn_kernel<KEYS>, LDS_BYTES);
        attr_set = true;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(l2h_knn_kernel<KEYS>, dim3((unsigned)cdiv64(p.N, BQ), (unsigned)S), dim3(NT), LDS_BYTES, st, p);
    SSAD_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(l2h_knn_merge_kernel<KEYS>, dim3((unsigned)cdiv64(p.N, 256)), dim3(256), 0, st, p, S);
        SSAD_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

#define SSAD_L2H_KNN_CHECKS()                                                                                   \
    SSAD_CHECK_ARG(D % 32 == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");                     \
    SSAD_CHECK_ARG(k >= 1 && k <= 3 && k <= R, "k in 1..3 and <= bank rows");                                   \
    SSAD_CHECK_ARG((((uintptr_t)xh | (uintptr_t)bankh) & 15) == 0, "half rows must be 16-byte aligned");        \
    SSAD_CHECK_ARG(cdiv64(N, BQ) < (int64_t)2147483647, "too many rows for one launch")

// xh[n][j] = h(x[n][j]) (fp32 -> fp16, round to nearest even, saturating at +-65504, subnormal results flushed to signed zero) and
// sq[n] = sum_j xh[n][j]^2 in fp32 in ssad_row_sqnorms' order, in one pass: equal rounded rows give equal norm bits wherever they stand.
extern "C" int ssad_rows_to_half(const float* x, void* xh, float* sq, int64_t N, int D, void* stream) {
    SSAD_CHECK_ARG(x && xh && sq && N > 0 && D > 0, "bad argument");
    SSAD_CHECK_ARG(D % 32 == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");
    SSAD_CHECK_ARG(cdiv64(N, NT / 64) < (int64_t)2147483647, "too many rows for one launch");
    hipLaunchKernelGGL(rows_to_half_kernel, dim3((unsigned)cdiv64(N, NT / 64)), dim3(NT), 0, (hipStream_t)stream, x, (hf*)xh, sq, N, D);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// ssad_l2_knn_fused on rounded rows: xh / bankh halves, x_sq / bank_sq their squared norms (ssad_rows_to_half).  One launch.
extern "C" int ssad_l2h_knn_fused(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, float* out, int64_t N,
                                  int D, int R, int k, void* stream) {
    SSAD_CHECK_ARG(xh && x_sq && bankh && bank_sq && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2H_KNN_CHECKS();
    return l2h_knn_launch<false>(L2hParams{(const hf*)xh, x_sq, (const hf*)bankh, bank_sq, nullptr, out, nullptr, nullptr, N, D, R, 0, k},
                                 1, stream);
}

// The bank split of ssad_l2_knn_split: part [S][N][3] floats (caller-owned), a second launch merges them; the same bits for every S.
extern "C" int ssad_l2h_knn_split(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, float* part, float* out,
                                  int64_t N, int D, int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(xh && x_sq && bankh && bank_sq && part && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2H_KNN_CHECKS();
    SSAD_CHECK_ARG(S >= 1 && S <= 65535, "S in 1..65535");
    return l2h_knn_launch<false>(L2hParams{(const hf*)xh, x_sq, (const hf*)bankh, bank_sq, part, out, nullptr, nullptr, N, D, R, 0, k}, S,
                                 stream);
}

// kneighbors on rounded rows: the k smallest (d2, bank row) pairs, dist = sqrt(d2) -- the bits ssad_l2h_knn_fused averages.
extern "C" int ssad_l2h_knn_index(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, float* dist, int* idx,
                                  int64_t N, int D, int R, int k, void* stream) {
    SSAD_CHECK_ARG(xh && x_sq && bankh && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2H_KNN_CHECKS();
    return l2h_knn_launch<true>(L2hParams{(const hf*)xh, x_sq, (const hf*)bankh, bank_sq, nullptr, nullptr, dist, idx, N, D, R, 0, k}, 1,
                                stream);
}

// The bank split of ssad_l2h_knn_index: part [S][N][3] 64-bit keys (caller-owned, 8-byte aligned; not needed for S = 1).
extern "C" int ssad_l2h_knn_index_split(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, void* part,
                                        float* dist, int* idx, int64_t N, int D, int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(xh && x_sq && bankh && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2H_KNN_CHECKS();
    SSAD_CHECK_ARG(S >= 1 && S <= 65535 && (S == 1 || part), "S in 1..65535, with a workspace when S > 1");
    SSAD_CHECK_ARG(((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");
    return l2h_knn_launch<true>(L2hParams{(const hf*)xh, x_sq, (const hf*)bankh, bank_sq, part, nullptr, dist, idx, N, D, R, 0, k}, S,
                                stream);
}
