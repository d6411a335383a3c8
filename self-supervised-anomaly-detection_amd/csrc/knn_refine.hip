// REFINING A COARSE SHORTLIST (opt-in beside knn_l2_half.hip / knn_l2_int8.hip; faiss' IndexRefineFlat): the fp16 and int8 searches
// return distances between rounded rows; a refined search takes their r nearest rows as a shortlist and ranks those again by the
// direct fp32 distance to the original rows.  Two pieces live here:
//   ssad_rerank_l2 / _index       distances of every query to ITS r listed bank rows (a gather) and the k smallest of them;
//   ssad_topk_l2q_index           the shortlist on int8 codes for r = 4 .. 32: knn_l2_int8.hip's kernel with knn_topk.hip's lists.
// The re-rank distance is l2_direct_kernel's (knn_gallery.hip): lane l takes elements l, l + 64, ... in an fma chain of squared
// differences, then the xor butterfly 32, 16, .., 1 -- a (query, row) pair has ssad_l2_direct's bits whatever N, r, the row's place
// in the list or the batch.  A row listed twice appears twice: nothing is deduplicated.
#include "knn_tile.h"

namespace {

// ================================================ the re-rank ================================================
struct RerankParams {
    const float* x;       // [N][D] queries
    const float* bank;    // [R][D] fp32 bank rows
    const int* cand;      // [N][r] listed rows of every query; an entry outside 0 .. R - 1 is skipped
    float* out;           // [N] mean form (else null)
    float* dist;          // [N][k] index form
    int* idx;             // [N][k] index form
    int64_t N;
    int D, R, r, k;
};

constexpr int RW = NT / 64;     // queries (waves) per workgroup

// The butterfly of CR sums at once.  A lane's CR partial sums are those of the CR listed rows; the butterfly's stage o leaves
// v[l] + v[l ^ o] in lane l.  Stages 32 .. 2 CR run on every sum as they stand; from stage CR down to 2 the lanes of a pair share
// the work: the lane whose bit o is clear keeps the lower half of the sums, its partner the upper half, and each receives the
// other's value OF THE SUM IT KEEPS -- that is the butterfly's own addition (fp32 addition commutes), so a sum has the butterfly's
// bits.  After stage 2 a lane holds one sum, that of listed row (lane >> 1) & (CR - 1); stage 1 finishes it.  CR + CR log2(32 /
// CR) shuffles in place of 6 CR.
template <int CR, int O>
__device__ __forceinline__ void butterfly_fold(float (&s)[CR], int lane) {
    if constexpr (O >= 2) {
        if constexpr (O > CR) {
#pragma unroll
            for (int c = 0; c < CR; ++c) s[c] += __shfl_xor(s[c], O);
        } else {
            constexpr int H = O / 2;            // sums a lane keeps after this stage
            const bool up = lane & O;
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const float keep = up ? s[i + H] : s[i], send = up ? s[i] : s[i + H];
                s[i] = keep + __shfl_xor(send, O);
            }
        }
        butterfly_fold<CR, O / 2>(s, lane);
    }
}

// A wave per query, RW queries per workgroup.  Lane c reads listed row c; the rows of four listed entries are requested together,
// NQ 256-byte wave loads each (lane l: elements l + 64 j), against the query's elements held in registers -- D <= 64 NQ: one round;
// wider rows take rounds of 64 NQ columns with the partial sums of all CR entries carried across them, which keeps every chain in
// ascending element order.  An entry that is skipped (outside the bank, or past r) reads row 0 and is dropped at the selection.
// Selection is rank counting over the at most CR keys (d2 bits << 32 | row) of a query, through LDS: rank = #smaller + #equal and
// earlier in the list, so equal keys (a row listed twice) take adjacent places.  No atomics, no data-dependent trip count.
template <int CR, int NQ>
__global__ __launch_bounds__(NT) void l2_rerank_kernel(RerankParams p) {
    __shared__ u64 keys_s[RW][CR];
    __shared__ float sorted_s[RW][CR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_raw = (int64_t)blockIdx.x * RW + wave;
    const bool live = n_raw < p.N;              // a wave past the end works on the last query and writes nothing
    const int64_t n = live ? n_raw : p.N - 1;

    const int mine = lane < p.r ? p.cand[n * p.r + lane] : -1;
    const bool ok = mine >= 0 && mine < p.R;
    const int safe = ok ? mine : 0;
    const float* xr = p.x + n * p.D;

    float s[CR];
#pragma unroll
    for (int c = 0; c < CR; ++c) s[c] = 0.f;
    for (int base = 0; base < p.D; base += 64 * NQ) {
        float q[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int e = base + lane + 64 * j;
            q[j] = e < p.D ? xr[e] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < CR / 4; ++g) {
            if (4 * g < p.r) {                  // wave-uniform
                float b[4][NQ];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float* br = p.bank + (int64_t)__builtin_amdgcn_readlane(safe, 4 * g + u) * p.D;
#pragma unroll
                    for (int j = 0; j < NQ; ++j) {
                        const int e = base + lane + 64 * j;
                        b[u][j] = e < p.D ? br[e] : 0.f;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < NQ; ++j) {      // past D: d = 0 leaves the sum as it is, bit for bit
                        const float d = q[j] - b[u][j];
                        s[4 * g + u] = __builtin_fmaf(d, d, s[4 * g + u]);
                    }
            }
        }
    }
    butterfly_fold<CR, 32>(s, lane);
    s[0] += __shfl_xor(s[0], 1);
    const int c_of = (lane >> 1) & (CR - 1);    // the listed entry whose sum this lane holds
    const int row_of = __shfl(mine, c_of);
    const bool ok_of = __shfl((int)ok, c_of);
    if (lane < 2 * CR && !(lane & 1)) keys_s[wave][c_of] = ok_of ? ((u64)__float_as_uint(s[0]) << 32) | (unsigned)row_of : NOKEY;
    if (lane < CR) sorted_s[wave][lane] = INFINITY;
    __syncthreads();

    const u64 key = lane < CR ? keys_s[wave][lane] : NOKEY;
    int rank = 0;
    for (int j = 0; j < p.r; ++j) {
        const u64 other = keys_s[wave][j];
        rank += other < key || (other == key && j < lane);
    }
    const int have = __popcll(__ballot(ok));    // valid entries: places have .. k - 1 stay (+inf, -1)
    const float root = sqrtf(__uint_as_float((unsigned)(key >> 32)));
    if (p.out) {
        if (ok) sorted_s[wave][rank] = root;
        __syncthreads();
        if (lane == 0 && live) {
            float sum = sorted_s[wave][0];
            for (int i = 1; i < p.k; ++i) sum += sorted_s[wave][i];
            p.out[n] = sum / (float)p.k;
        }
        return;
    }
    if (!live) return;
    if (ok && rank < p.k) {
        p.dist[n * p.k + rank] = root;
        p.idx[n * p.k + rank] = mine;
    }
    if (lane >= have && lane < p.k) {
        p.dist[n * p.k + lane] = INFINITY;
        p.idx[n * p.k + lane] = -1;
    }
}

template <int CR>
static void rerank_launch_cr(const RerankParams& p, hipStream_t st) {
    const dim3 grid((unsigned)cdiv64(p.N, RW));
    if (p.D <= 64) hipLaunchKernelGGL((l2_rerank_kernel<CR, 1>), grid, dim3(NT), 0, st, p);
    else if (p.D <= 128) hipLaunchKernelGGL((l2_rerank_kernel<CR, 2>), grid, dim3(NT), 0, st, p);
    else if (p.D <= 256) hipLaunchKernelGGL((l2_rerank_kernel<CR, 4>), grid, dim3(NT), 0, st, p);
    else if (p.D <= 384) hipLaunchKernelGGL((l2_rerank_kernel<CR, 6>), grid, dim3(NT), 0, st, p);
    else hipLaunchKernelGGL((l2_rerank_kernel<CR, 8>), grid, dim3(NT), 0, st, p);
}

static int rerank_launch(const RerankParams& p, void* stream) {
    if (p.r <= 8) rerank_launch_cr<8>(p, (hipStream_t)stream);
    else rerank_launch_cr<32>(p, (hipStream_t)stream);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// ================================================ the shortlist on int8 codes ================================================
// knn_l2_int8.hip's tile, restated: 128 codes per K step, 144-byte LDS rows (the reasons stand there)
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
constexpr int QK = 128, QLDK = QK + 16;
constexpr int QSTAGE = (BB + BQ) * QLDK;        // bytes
constexpr int QLDS_BYTES = 2 * QSTAGE + (BQ + BB) * 4;
constexpr int MAX_D = 32768;
static_assert(2 * QSTAGE == 2 * STAGE * 4, "tile_tail_topk's lists fit into the code stages as into the fp32 ones");

struct L2qTopkParams {
    const signed char* x;   // [N][D] query codes
    const int* xsq;         // [N] their squared norms
    const float* xex;       // [N] the queries' excess
    const signed char* bank;  // [R][D] bank codes
    const int* bsq;         // [R] their squared norms
    u64* part;              // [S][N][k] keys of each query over each split, ascending, NOKEY where a split has fewer rows (S > 1 only)
    float* dist;            // [N][k]
    int* idx;               // [N][k]
    int64_t N;
    int D, R, rows_per, k;
    float s2;               // s s
};

// the k winners of query `row`: L[0 .. k - 1] are real keys (k <= bank rows: the entry point checks); dist as knn_l2_int8.hip's root_of
template <int CAP>
__device__ __forceinline__ void l2q_topk_write(const L2qTopkParams& p, int64_t row, const u64 (&L)[CAP]) {
    const float ex = p.xex[row];
#pragma unroll
    for (int i = 0; i < CAP; ++i) {
        if (i < p.k) {
            p.dist[row * p.k + i] = sqrtf(__builtin_fmaf(p.s2, (float)(unsigned)(L[i] >> 32), ex));
            p.idx[row * p.k + i] = (int)(unsigned)L[i];
        }
    }
}

// knn_tile.h's tile_select_topk on integer accumulators: D2 = (qsq + bsq) - 2 dot, exact in unsigned arithmetic (D <= MAX_D), keys
// (D2 << 32 | row).  The same pass / insert rounds.
template <int CAP, class RowOf>
__device__ __forceinline__ void tile_select_topk_int(const i32x16 (&acc)[TB][TQ], const int* qn_s, const int* bn_s, const TileThread& t,
                                                     u64 (&L)[TQ][CAP], RowOf rowof) {
    static_assert(TB * 16 == 32, "a candidate mask is 32 bits");
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
        const unsigned qn = (unsigned)qn_s[(t.wq * TQ + j) * 32 + t.r];
        const u64 worst = L[j][CAP - 1];
        unsigned d[TB * 16];
        unsigned mask = 0;
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const int l0 = (t.wb * TB + i) * 32 + 4 * t.h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const i32x4 bn = *(const i32x4*)(bn_s + l0 + 8 * g);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const RowId row = rowof(l0 + 8 * g, c);
                    const unsigned d2 = (qn + (unsigned)bn[c]) - 2u * (unsigned)acc[i][j][4 * g + c];
                    d[i * 16 + 4 * g + c] = d2;
                    if (row.ok && (((u64)d2 << 32) | (unsigned)row.id) < worst) mask |= 1u << (i * 16 + 4 * g + c);
                }
            }
        }
        while (__any(mask != 0)) {
            const int e = mask ? __builtin_ctz(mask) : 0;       // candidate e = 16 i + 4 g + c
            unsigned d2 = d[0];
#pragma unroll
            for (int q = 1; q < TB * 16; ++q) d2 = e == q ? d[q] : d2;
            const RowId row = rowof((t.wb * TB + (e >> 4)) * 32 + 4 * t.h + 8 * ((e >> 2) & 3), e & 3);
            topk_insert(L[j], mask ? ((u64)d2 << 32) | (unsigned)row.id : NOKEY);
            mask &= mask - 1;
        }
    }
}

// l2q_knn_kernel (knn_l2_int8.hip) with a list in place of the three smallest: its K loop, statement for statement.  Two workgroups
// per CU for CAP = 8 only: with 256 registers the CAP = 16 lists, the 32 integer candidates and the accumulators spilled 32 bytes.
template <int CAP>
__global__ __launch_bounds__(NT, CAP <= 8 ? 2 : 1) void l2q_topk_kernel(L2qTopkParams p) {
    extern __shared__ __attribute__((aligned(16))) signed char lds[];
    int* qn_s = (int*)(lds + 2 * QSTAGE);       // [BQ] squared norms of the query codes
    int* bn_s = qn_s + BQ;                      // [BB] squared norms of the current bank tile
    const TileThread t{};                       // staging: 16-byte chunk sc is 16 codes
    const int64_t m0 = (int64_t)blockIdx.x * BQ;

    if (t.tid < BQ) qn_s[t.tid] = m0 + t.tid < p.N ? p.xsq[m0 + t.tid] : 0;
    unsigned qoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qoff[i] = m0 + t.sr + 32 * i < p.N ? (unsigned)((t.sr + 32 * i) * p.D + t.sc * 16) : OOB;
    const signed char* xblk = p.x + m0 * p.D;

    u64 L[TQ][CAP];
#pragma unroll
    for (int j = 0; j < TQ; ++j)
#pragma unroll
        for (int i = 0; i < CAP; ++i) L[j][i] = NOKEY;
    const int nks = (p.D + QK - 1) / QK;
    const int64_t r_begin = (int64_t)blockIdx.y * p.rows_per;
    const int r_end = (int)(r_begin + p.rows_per < p.R ? r_begin + p.rows_per : p.R);

    for (int n0 = (int)(r_begin < p.R ? r_begin : p.R); n0 < r_end; n0 += BB) {
        unsigned boff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) boff[i] = n0 + t.sr + 32 * i < p.R ? (unsigned)((t.sr + 32 * i) * p.D + t.sc * 16) : OOB;
        const signed char* bblk = p.bank + (int64_t)n0 * p.D;
        i32x16 acc[TB][TQ];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
        i32x4 rq[4], rb[4];
        auto load = [&](int ks) {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(xblk + ks * QK), 0, (int)OOB, SRD3);
            const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(bblk + ks * QK), 0, (int)OOB, SRD3);
            const bool in = ks * QK + t.sc * 16 < p.D;  // this chunk's columns exist (D is a multiple of 32, a chunk is 16 wide)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                rq[i] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, in ? qoff[i] : OOB, 0, 0));
                rb[i] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, in ? boff[i] : OOB, 0, 0));
            }
        };
        auto store = [&](signed char* st) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *(i32x4*)(st + (t.sr + 32 * i) * QLDK + t.sc * 16) = rb[i];                 // bank rows: the tile's M side
                *(i32x4*)(st + BB * QLDK + (t.sr + 32 * i) * QLDK + t.sc * 16) = rq[i];     // queries: its N side
            }
        };
        __syncthreads();                        // every wave has left the previous bank tile's last stage and its norms
        load(0);
        if (t.tid < BB) bn_s[t.tid] = n0 + t.tid < p.R ? p.bsq[n0 + t.tid] : 0;
        store(lds);
        __syncthreads();
        for (int ks = 0; ks < nks; ++ks) {
            const signed char* cur = lds + (ks & 1) * QSTAGE;
            if (ks + 1 < nks) load(ks + 1);
            const signed char* As = cur + (t.wb * 32 * TB + t.r) * QLDK + t.h * 16;
            const signed char* Bs = cur + BB * QLDK + (t.wq * 32 * TQ + t.r) * QLDK + t.h * 16;
            const int groups = (p.D - ks * QK) / 32;    // 32-column groups of this step that exist (4 or more: all)
#pragma unroll
            for (int kk = 0; kk < QK / 32; ++kk) {
                if (kk < groups) {
                    i32x4 a[TB], b[TQ];
#pragma unroll
                    for (int i = 0; i < TB; ++i) a[i] = *(const i32x4*)(As + i * 32 * QLDK + kk * 32);
#pragma unroll
                    for (int j = 0; j < TQ; ++j) b[j] = *(const i32x4*)(Bs + j * 32 * QLDK + kk * 32);
#pragma unroll
                    for (int i = 0; i < TB; ++i)
#pragma unroll
                        for (int j = 0; j < TQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
                }
            }
            if (ks + 1 < nks) store(lds + ((ks + 1) & 1) * QSTAGE);
            __syncthreads();
        }
        tile_select_topk_int<CAP>(acc, qn_s, bn_s, t, L, [&](int l, int c) { return RowId{n0 + l + c < p.R, n0 + l + c}; });
    }
    tile_tail_topk<CAP>(L, lds, t, [&](int slot, int j) {
        const int64_t row = m0 + slot;
        if (row >= p.N) return;
        if (gridDim.y == 1) {
            l2q_topk_write(p, row, L[j]);
            return;
        }
        u64* o = p.part + ((int64_t)blockIdx.y * p.N + row) * p.k;
#pragma unroll
        for (int i = 0; i < CAP; ++i)
            if (i < p.k) o[i] = L[j][i];
    });
}

// the k smallest of the S ascending lists of query n, then the one-launch epilogue
template <int CAP>
__global__ __launch_bounds__(256) void l2q_topk_merge_kernel(L2qTopkParams p, int S) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= p.N) return;
    u64 L[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) L[i] = NOKEY;
    for (int s = 0; s < S; ++s) topk_merge(L, p.part + ((int64_t)s * p.N + n) * p.k, 1, p.k);
    l2q_topk_write(p, n, L);
}

template <int CAP>
static int l2q_topk_launch_cap(const L2qTopkParams& p, int S, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(l2q_topk_kernel<CAP>, QLDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL(l2q_topk_kernel<CAP>, dim3((unsigned)cdiv64(p.N, BQ), (unsigned)S), dim3(NT), QLDS_BYTES, st, p);
    SSAD_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(l2q_topk_merge_kernel<CAP>, dim3((unsigned)cdiv64(p.N, 256)), dim3(256), 0, st, p, S);
        SSAD_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

#define SSAD_L2_RERANK_CHECKS()                                                                                 \
    SSAD_CHECK_ARG(N > 0 && D > 0 && R > 0, "N, D and R must be positive");                                     \
    SSAD_CHECK_ARG(r >= 1 && r <= 32, "r in 1..32");                                                            \
    SSAD_CHECK_ARG(k >= 1 && k <= r, "k in 1..r");                                                              \
    SSAD_CHECK_ARG(cdiv64(N, RW) < (int64_t)2147483647, "too many rows for one launch")

// kneighbors among listed rows: for query n the first k entries of an ascending sort of its r listed rows cand[n][0 .. r - 1] by
// (d2 bits, bank row, place in the list), d2 = ssad_l2_direct's bits for (x[n], bank[row]); dist [N][k] = sqrtf(d2), idx [N][k] the
// bank rows.  An entry outside 0 .. R - 1 is skipped; fewer than k valid entries leave (+inf, -1) in the missing places; a row
// listed twice appears twice.  1 <= r <= 32, 1 <= k <= r, any D >= 1.  The same bits on every call and in every batch.
extern "C" int ssad_rerank_l2_index(const float* x, const float* bank, const int* cand, float* dist, int* idx, int64_t N, int D, int R,
                                    int r, int k, void* stream) {
    SSAD_CHECK_ARG(x && bank && cand && dist && idx, "bad argument");
    SSAD_L2_RERANK_CHECKS();
    return rerank_launch(RerankParams{x, bank, cand, nullptr, dist, idx, N, D, R, r, k}, stream);
}

// out[n] = (dist[n][0] + dist[n][1] + ... + dist[n][k - 1]) / k of ssad_rerank_l2_index, added in that order in fp32: +inf for a
// query with fewer than k valid entries.
extern "C" int ssad_rerank_l2(const float* x, const float* bank, const int* cand, float* out, int64_t N, int D, int R, int r, int k,
                              void* stream) {
    SSAD_CHECK_ARG(x && bank && cand && out, "bad argument");
    SSAD_L2_RERANK_CHECKS();
    return rerank_launch(RerankParams{x, bank, cand, out, nullptr, nullptr, N, D, R, r, k}, stream);
}

// ssad_l2q_knn_index for k = 4..32: the first k entries of a stable ascending sort of (D2, bank row), D2 the exact integer squared
// code distance; dist = sqrtf(fmaf(s2, (float)D2, excess)), the k <= 3 kernel's expression, so the first three columns are
// ssad_l2q_knn_index(k = 3) bit for bit.  S bank splits; part [S][N][k] 64-bit keys when S > 1.  The same bits for every S.
extern "C" int ssad_topk_l2q_index(const void* xq, const int* x_sq, const float* x_excess, const void* bankq, const int* bank_sq,
                                       void* part, float* dist, int* idx, int64_t N, int D, int R, int k, int S, float s2,
                                       void* stream) {
    SSAD_CHECK_ARG(xq && x_sq && x_excess && bankq && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_CHECK_ARG(D % 32 == 0 && D <= MAX_D, "D must be a multiple of 32, at most 32768 (D 255^2 must fit int32)");
    SSAD_CHECK_ARG(k >= 4 && k <= 32 && k <= R, "k in 4..32 and <= bank rows");
    SSAD_CHECK_ARG((((uintptr_t)xq | (uintptr_t)bankq) & 15) == 0, "code rows must be 16-byte aligned");
    SSAD_CHECK_ARG(S >= 1 && S <= 65535 && (S == 1 || part), "S in 1..65535, with a workspace when S > 1");
    SSAD_CHECK_ARG(S == 1 || ((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");
    SSAD_CHECK_ARG(cdiv64(N, BQ) < (int64_t)2147483647, "too many rows for one launch");
    L2qTopkParams p{(const signed char*)xq, x_sq, x_excess, (const signed char*)bankq, bank_sq, (u64*)part, dist, idx, N, D, R, 0, k, s2};
    p.rows_per = (int)(cdiv64(cdiv64(p.R, BB), S) * BB);
    hipStream_t st = (hipStream_t)stream;
    if (k <= 8) return l2q_topk_launch_cap<8>(p, S, st);
    if (k <= 16) return l2q_topk_launch_cap<16>(p, S, st);
    return l2q_topk_launch_cap<32>(p, S, st);
}
