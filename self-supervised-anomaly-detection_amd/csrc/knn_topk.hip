// The flat Euclidean k-NN search for k = 4 .. 32 (opt-in beside knn_l2.hip / knn_l2_half.hip, which keep k = 1 .. 3): the same tile,
// the same dot loops (knn_tile.h's dot_tile; knn_l2_half.hip's fp16 loop, restated below step for step), the same norms and the same
// d2 = fmaxf((qn + bn) - 2 dot, 0) -- a (query, bank row) pair has the bits ssad_l2_knn_index / ssad_l2h_knn_index give it.  New is
// what happens to the finished tile: a lane keeps the CAP smallest (d2 bits << 32 | row) keys of each of its two query columns as a
// sorted list in registers (knn_tile.h's tile_select_topk), CAP = 8, 16 or 32 >= k chosen on the host.  Keys are unique, so the k
// smallest of the bank do not depend on the visiting order: lane halves, waves, bank splits and batches all give the same bits.
// The mean form runs on the same keys: its sum is formed from the roots the index form writes, smallest first, one after the other.
#include "knn_tile.h"

namespace {

constexpr int LDS_BYTES = (2 * STAGE + BQ + BB) * 4;
constexpr int HK = 64, HLDK = HK + 8, HSTAGE = (BB + BQ) * HLDK;        // knn_l2_half.hip's K step and LDS rows
static_assert(2 * HSTAGE * 2 + (BQ + BB) * 4 == LDS_BYTES, "both operand types use the same LDS");

struct TopkParams {
    const void* x;        // [N][D] queries: floats, or rounded halves (ssad_rows_to_half)
    const float* xsq;     // [N] squared norms of the rounded queries (half operands only)
    const void* bank;     // [R][D] bank rows, floats or halves
    const float* bsq;     // [R] their squared norms
    u64* part;            // [S][N][k] keys of each query over each split, ascending, NOKEY where a split has fewer rows (S > 1 only)
    float* out;           // [N] mean form (else null)
    float* dist;          // [N][k] index form
    int* idx;             // [N][k] index form
    int64_t N;
    int D, R, rows_per, k;
};

// the k winners of query `row`: L[0 .. k - 1] are real keys (k <= bank rows: the entry points check)
template <int CAP>
__device__ __forceinline__ void topk_write(const TopkParams& p, int64_t row, const u64 (&L)[CAP]) {
    if (p.out) {
        float s = sqrtf(__uint_as_float((unsigned)(L[0] >> 32)));
#pragma unroll
        for (int i = 1; i < CAP; ++i)
            if (i < p.k) s += sqrtf(__uint_as_float((unsigned)(L[i] >> 32)));
        p.out[row] = s / (float)p.k;
        return;
    }
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
        if (i < p.k) {
            p.dist[row * p.k + i] = sqrtf(__uint_as_float((unsigned)(L[i] >> 32)));
            p.idx[row * p.k + i] = (int)(unsigned)L[i];
        }
    }
}

template <int CAP>
__device__ __forceinline__ void topk_emit(const TopkParams& p, int64_t row, const u64 (&L)[CAP]) {
    if (row >= p.N) return;
    if (gridDim.y == 1) {
        topk_write(p, row, L);
        return;
    }
    u64* o = p.part + ((int64_t)blockIdx.y * p.N + row) * p.k;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
        if (i < p.k) o[i] = L[i];
}

// l2_knn_kernel (knn_l2.hip) with a list in place of the three smallest.  Grid (ceil(N / 128), S).  One workgroup per CU for CAP = 32
// (its lists alone take 128 registers), two below that, as the k <= 3 kernels.
template <int CAP>
__global__ __launch_bounds__(NT, CAP <= 16 ? 2 : 1) void l2_topk_kernel(TopkParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* qn_s = lds + 2 * STAGE;              // [BQ] squared norms of the queries
    float* bn_s = qn_s + BQ;                    // [BB] squared norms of the current bank tile
    const TileThread t{};
    const int64_t m0 = (int64_t)blockIdx.x * BQ;
    const float* x = (const float*)p.x;

    tile_sqnorms<true>(qn_s, p.D, t, [&](int s) { return m0 + s < p.N ? x + (m0 + s) * p.D : nullptr; });       // rows past N give 0
    unsigned qoff[4];
    stage_offsets(qoff, m0, p.N, p.D, t);
    const float* xblk = x + m0 * p.D;

    u64 L[TQ][CAP];
#pragma unroll
    for (int j = 0; j < TQ; ++j)
#pragma unroll
        for (int i = 0; i < CAP; ++i) L[j][i] = NOKEY;
    const int64_t r_begin = (int64_t)blockIdx.y * p.rows_per;
    const int r_end = (int)(r_begin + p.rows_per < p.R ? r_begin + p.rows_per : p.R);

    for (int n0 = (int)(r_begin < p.R ? r_begin : p.R); n0 < r_end; n0 += BB) {
        unsigned boff[4];
        stage_offsets(boff, n0, p.R, p.D, t);
        f32x16 acc[TB][TQ];
        dot_tile(acc, lds, t, (const float*)p.bank + (int64_t)n0 * p.D, boff, p.D / BK,
                 [&](int ks, int i) { return buffer_load16(xblk + ks * BK, qoff[i]); },
                 [&] { if (t.tid < BB) bn_s[t.tid] = n0 + t.tid < p.R ? p.bsq[n0 + t.tid] : 0.f; });
        tile_select_topk<CAP>(acc, qn_s, bn_s, t, L, [&](int l, int c) { return RowId{n0 + l + c < p.R, n0 + l + c}; });
    }
    tile_tail_topk<CAP>(L, lds, t, [&](int slot, int j) { topk_emit(p, m0 + slot, L[j]); });
}

// l2h_knn_kernel (knn_l2_half.hip) with a list in place of the three smallest: its K loop, statement for statement.
template <int CAP>
__global__ __launch_bounds__(NT, CAP <= 16 ? 2 : 1) void l2h_topk_kernel(TopkParams p) {
    extern __shared__ __attribute__((aligned(16))) hf hlds[];
    float* qn_s = (float*)(hlds + 2 * HSTAGE);  // [BQ] squared norms of the queries
    float* bn_s = qn_s + BQ;                    // [BB] squared norms of the current bank tile
    const TileThread t{};                       // staging: 16-byte chunk sc is 8 halves
    const int64_t m0 = (int64_t)blockIdx.x * BQ;

    if (t.tid < BQ) qn_s[t.tid] = m0 + t.tid < p.N ? p.xsq[m0 + t.tid] : 0.f;
    unsigned qoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qoff[i] = m0 + t.sr + 32 * i < p.N ? (unsigned)(((t.sr + 32 * i) * p.D + t.sc * 8) * 2) : OOB;
    const hf* xblk = (const hf*)p.x + m0 * p.D;

    u64 L[TQ][CAP];
#pragma unroll
    for (int j = 0; j < TQ; ++j)
#pragma unroll
        for (int i = 0; i < CAP; ++i) L[j][i] = NOKEY;
    const int nks = (p.D + HK - 1) / HK;
    const int64_t r_begin = (int64_t)blockIdx.y * p.rows_per;
    const int r_end = (int)(r_begin + p.rows_per < p.R ? r_begin + p.rows_per : p.R);

    for (int n0 = (int)(r_begin < p.R ? r_begin : p.R); n0 < r_end; n0 += BB) {
        unsigned boff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) boff[i] = n0 + t.sr + 32 * i < p.R ? (unsigned)(((t.sr + 32 * i) * p.D + t.sc * 8) * 2) : OOB;
        const hf* bblk = (const hf*)p.bank + (int64_t)n0 * p.D;
        f32x16 acc[TB][TQ];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        f16x8 rq[4], rb[4];
        auto load = [&](int ks) {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(xblk + ks * HK), 0, (int)OOB, SRD3);
            const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(bblk + ks * HK), 0, (int)OOB, SRD3);
            const bool in = ks * HK + t.sc * 8 < p.D;   // this chunk's columns exist (D is a multiple of 32, a chunk is 8 wide)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                rq[i] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, in ? qoff[i] : OOB, 0, 0));
                rb[i] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, in ? boff[i] : OOB, 0, 0));
            }
        };
        auto store = [&](hf* st) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *(f16x8*)(st + (t.sr + 32 * i) * HLDK + t.sc * 8) = rb[i];                  // bank rows: the tile's M side
                *(f16x8*)(st + BB * HLDK + (t.sr + 32 * i) * HLDK + t.sc * 8) = rq[i];      // queries: its N side
            }
        };
        __syncthreads();                        // every wave has left the previous bank tile's last stage and its norms
        load(0);
        if (t.tid < BB) bn_s[t.tid] = n0 + t.tid < p.R ? p.bsq[n0 + t.tid] : 0.f;
        store(hlds);
        __syncthreads();
        for (int ks = 0; ks < nks; ++ks) {
            const hf* cur = hlds + (ks & 1) * HSTAGE;
            if (ks + 1 < nks) load(ks + 1);
            const hf* As = cur + (t.wb * 32 * TB + t.r) * HLDK + t.h * 8;
            const hf* Bs = cur + BB * HLDK + (t.wq * 32 * TQ + t.r) * HLDK + t.h * 8;
#pragma unroll
            for (int kk = 0; kk < HK / 16; ++kk) {
                f16x8 a[TB], b[TQ];
#pragma unroll
                for (int i = 0; i < TB; ++i) a[i] = *(const f16x8*)(As + i * 32 * HLDK + kk * 16);
#pragma unroll
                for (int j = 0; j < TQ; ++j) b[j] = *(const f16x8*)(Bs + j * 32 * HLDK + kk * 16);
#pragma unroll
                for (int i = 0; i < TB; ++i)
#pragma unroll
                    for (int j = 0; j < TQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
            if (ks + 1 < nks) store(hlds + ((ks + 1) & 1) * HSTAGE);
            __syncthreads();
        }
        tile_select_topk<CAP>(acc, qn_s, bn_s, t, L, [&](int l, int c) { return RowId{n0 + l + c < p.R, n0 + l + c}; });
    }
    tile_tail_topk<CAP>(L, hlds, t, [&](int slot, int j) { topk_emit(p, m0 + slot, L[j]); });
}

// the k smallest of the S ascending lists of query n, then the one-launch epilogue
template <int CAP>
__global__ __launch_bounds__(256) void topk_merge_kernel(TopkParams p, int S) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= p.N) return;
    u64 L[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) L[i] = NOKEY;
    for (int s = 0; s < S; ++s) topk_merge(L, p.part + ((int64_t)s * p.N + n) * p.k, 1, p.k);
    topk_write(p, n, L);
}

template <int CAP, bool HALF>
static int topk_launch_cap(TopkParams p, int S, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        if (HALF) SSAD_SET_DYN_LDS(l2h_topk_kernel<CAP>, LDS_BYTES);
        else SSAD_SET_DYN_LDS(l2_topk_kernel<CAP>, LDS_BYTES);
        attr_set = true;
    }
    const dim3 grid((unsigned)cdiv64(p.N, BQ), (unsigned)S);
    if (HALF) hipLaunchKernelGGL(l2h_topk_kernel<CAP>, grid, dim3(NT), LDS_BYTES, st, p);
    else hipLaunchKernelGGL(l2_topk_kernel<CAP>, grid, dim3(NT), LDS_BYTES, st, p);
    SSAD_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(topk_merge_kernel<CAP>, dim3((unsigned)cdiv64(p.N, 256)), dim3(256), 0, st, p, S);
        SSAD_CHECK_LAUNCH();
    }
    return 0;
}

template <bool HALF>
static int topk_launch(TopkParams p, int S, void* stream) {
    p.rows_per = (int)(cdiv64(cdiv64(p.R, BB), S) * BB);
    hipStream_t st = (hipStream_t)stream;
    if (p.k <= 8) return topk_launch_cap<8, HALF>(p, S, st);
    if (p.k <= 16) return topk_launch_cap<16, HALF>(p, S, st);
    return topk_launch_cap<32, HALF>(p, S, st);
}

}  // namespace

#define SSAD_TOPK_CHECKS()                                                                                      \
    SSAD_CHECK_ARG(D % 32 == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");                     \
    SSAD_CHECK_ARG(k >= 4 && k <= 32 && k <= R, "k in 4..32 and <= bank rows");                                 \
    SSAD_CHECK_ARG(S >= 1 && S <= 65535 && (S == 1 || part), "S in 1..65535, with a workspace when S > 1");     \
    SSAD_CHECK_ARG(((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");                                  \
    SSAD_CHECK_ARG(cdiv64(N, BQ) < (int64_t)2147483647, "too many rows for one launch")

// out[n] = mean of the sqrt of the k (4..32) smallest d2 of ssad_l2_knn_fused over the R bank rows, added smallest first one after the
// other: the sum of the row ssad_l2_knn_topk_index writes.  S bank splits (1: one launch); part [S][N][k] 64-bit keys, caller-owned,
// 8-byte aligned, not needed for S = 1.  The same bits for every S.
extern "C" int ssad_l2_knn_topk(const float* x, const float* bank, const float* bank_sq, void* part, float* out, int64_t N, int D, int R,
                                int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_TOPK_CHECKS();
    return topk_launch<false>(TopkParams{x, nullptr, bank, bank_sq, (u64*)part, out, nullptr, nullptr, N, D, R, 0, k}, S, stream);
}

// kneighbors of the Euclidean bank for k = 4..32: the first k entries of a stable ascending sort of (d2, bank row), d2 the bits of
// ssad_l2_knn_index; dist [N][k] = sqrt(d2), idx [N][k] int32.  Splits and workspace as ssad_l2_knn_topk.
extern "C" int ssad_l2_knn_topk_index(const float* x, const float* bank, const float* bank_sq, void* part, float* dist, int* idx,
                                      int64_t N, int D, int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_TOPK_CHECKS();
    return topk_launch<false>(TopkParams{x, nullptr, bank, bank_sq, (u64*)part, nullptr, dist, idx, N, D, R, 0, k}, S, stream);
}

// ssad_l2_knn_topk on rounded rows: xh / bankh halves, x_sq / bank_sq their squared norms (ssad_rows_to_half); d2 the bits of
// ssad_l2h_knn_index.
extern "C" int ssad_l2h_knn_topk(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, void* part, float* out,
                                 int64_t N, int D, int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(xh && x_sq && bankh && bank_sq && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_TOPK_CHECKS();
    SSAD_CHECK_ARG((((uintptr_t)xh | (uintptr_t)bankh) & 15) == 0, "half rows must be 16-byte aligned");
    return topk_launch<true>(TopkParams{xh, x_sq, bankh, bank_sq, (u64*)part, out, nullptr, nullptr, N, D, R, 0, k}, S, stream);
}

// ssad_l2_knn_topk_index on rounded rows.
extern "C" int ssad_l2h_knn_topk_index(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, void* part,
                                       float* dist, int* idx, int64_t N, int D, int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(xh && x_sq && bankh && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_TOPK_CHECKS();
    SSAD_CHECK_ARG((((uintptr_t)xh | (uintptr_t)bankh) & 15) == 0, "half rows must be 16-byte aligned");
    return topk_launch<true>(TopkParams{xh, x_sq, bankh, bank_sq, (u64*)part, nullptr, dist, idx, N, D, R, 0, k}, S, stream);
}
