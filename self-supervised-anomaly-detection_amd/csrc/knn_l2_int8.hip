// Euclidean k-NN scoring on an 8-BIT SCALAR-QUANTISED BANK (opt-in beside knn_l2.hip and knn_l2_half.hip; faiss' IndexScalarQuantizer,
// QT_8bit_uniform): one affine code for the whole bank, (lo, s) with s = (hi - lo) / 255 (1 when hi == lo), inv_s = 1 / s, both
// computed in float64 on the host and rounded once to fp32.  THE code of an fp32 element x, in fp32 operations in this order,
//   c(x) = rint(min(max((x - lo) * inv_s, 0), 255)) - 128        (rint: to nearest even; max(NaN, 0) = 0, so NaN -> -128),
// stored as int8; it stands for the value lo + s (c + 128).  The distance is that BETWEEN THE CODES, plus what the query lost to
// the clamp:
//   D2(q, b)   = sum_j (c(q_j) - c(b_j))^2 = (qsq + bsq) - 2 <c(q), c(b)>     int32, exact, never negative (D <= 32768),
//   <., .>       v_mfma_i32_32x32x32_i8 chains: int8 products, int32 accumulation, 32 codes per instruction,
//   qsq, bsq     sum_j c_j^2, int32, written by the pass that writes the codes,
//   excess(q)  = sum_j (q_j - min(max(q_j, lo), hi_q))^2, hi_q = fmaf(255, s, lo) (the value of code 127), in fp32 in sqnorm_wave's
//                order (knn_tile.h): 0 for a row inside the coded range, NaN for a row that holds a NaN,
//   d(q, b)    = sqrtf(fmaf(s s, (float)D2, excess(q)))          on the k winners only; s s rounded once on the host.
// Every b in the coded range has |q - b|^2 >= |clamp(q) - b|^2 + excess(q) (element by element: b lies on the near side of the
// bound q left through), and excess is constant per query, so it changes no order: selection runs on the integers alone.  Keys are
// (uint32 D2 << 32 | row); the mean form selects on the 32-bit D2.  Selection, tail, split and merge are knn_tile.h's.
#include "knn_tile.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

// knn_tile.h's tile (BB x BQ, four waves of 2 x 2 accumulators) with a K step of 128 codes: the 128 bytes per row and step that
// TileThread's staging moves (8 chunks of 16 bytes).  144-byte LDS rows: the 16 rows of a ds_read_b128 lane group fall on 16 distinct
// 16-byte slots of the 256-byte bank row (36 r mod 64 runs over the multiples of 4 -- 9 r mod 16 is a bijection and the rows of a
// group are distinct mod 16); a ds_write_b128 group is 8 lanes of one row, 128 contiguous bytes.
constexpr int QK = 128, QLDK = QK + 16;         // codes per K step; bytes per LDS row
constexpr int QSTAGE = (BB + BQ) * QLDK;        // bytes
constexpr int LDS_BYTES = 2 * QSTAGE + (BQ + BB) * 4;
constexpr int MAX_D = 32768;                    // D2 <= D 255^2 < 2^31 <=> D <= 33025.03..; the multiple of 32 below it that is a power of two

__device__ __forceinline__ int code_of(float x, float lo, float inv_s) {
    return (int)__builtin_rintf(fminf(fmaxf((x - lo) * inv_s, 0.f), 255.f)) - 128;
}
__device__ __forceinline__ float over_of(float x, float lo, float hi) { return x - fminf(fmaxf(x, lo), hi); }

// One wave takes eight rows at a time; lane l the elements 8 l .. 8 l + 7 (+ 512 per round) of each: two 16-byte loads per row -- 16 in
// flight per lane -- and one 8-byte store of codes.  The squared codes are summed as integers (any order is exact).  A row with an
// element outside [lo, hi_q] (or a NaN) is read again in sqnorm_wave's order for its excess; every other row's excess is the sum of
// zeros in that order, +0.
constexpr int RQ = 8;
__global__ __launch_bounds__(NT) void rows_to_int8_kernel(const float* __restrict__ x, signed char* __restrict__ codes,
                                                          int* __restrict__ sq, float* __restrict__ excess, int64_t N, int D, float lo,
                                                          float inv_s, float s) {
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6)) * RQ;
    if (row0 >= N) return;
    const float hi = __builtin_fmaf(255.f, s, lo);
    int sum[RQ];
    bool out[RQ];
#pragma unroll
    for (int u = 0; u < RQ; ++u) {
        sum[u] = 0;
        out[u] = false;
    }
    for (int e = lane * 8; e < D; e += 512) {
        f32x4 v[RQ][2];
#pragma unroll
        for (int u = 0; u < RQ; ++u) {
            const bool have = row0 + u < N;
            const float* src = x + (row0 + u) * D + e;
            v[u][0] = have ? *(const f32x4*)src : f32x4{lo, lo, lo, lo};
            v[u][1] = have ? *(const f32x4*)(src + 4) : f32x4{lo, lo, lo, lo};
        }
#pragma unroll
        for (int u = 0; u < RQ; ++u) {
            unsigned w[2];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                w[g] = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float f = v[u][g][j];
                    const int c = code_of(f, lo, inv_s);
                    w[g] |= (unsigned)(c & 255) << (8 * j);
                    sum[u] += c * c;
                    out[u] |= !(over_of(f, lo, hi) == 0.f);
                }
            }
            if (row0 + u < N) *(i32x2*)(codes + (row0 + u) * D + e) = i32x2{(int)w[0], (int)w[1]};
        }
    }
#pragma unroll
    for (int u = 0; u < RQ; ++u) {
        if (row0 + u >= N) break;               // wave-uniform
        int t = sum[u];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        float ex = 0.f;
        if (__any(out[u])) {
            const float* src = x + (row0 + u) * D;
            for (int k = lane; k < D; k += 64) {
                const float d = over_of(src[k], lo, hi);
                ex = __builtin_fmaf(d, d, ex);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ex += __shfl_xor(ex, o);
        }
        if (lane == 0) {
            sq[row0 + u] = t;
            excess[row0 + u] = ex;
        }
    }
}

// ================================================ the integer epilogue ================================================
// what is selected: squared code distances, or (squared code distance, row) keys
template <bool KEYS> struct SelQ;
template <> struct SelQ<false> {
    typedef unsigned T;
    static __device__ __forceinline__ unsigned none() { return ~0u; }         // D2 < 2^31: never a real value
    static __device__ __forceinline__ unsigned make(unsigned d2, int) { return d2; }
};
template <> struct SelQ<true> {
    typedef u64 T;
    static __device__ __forceinline__ u64 none() { return NOKEY; }
    static __device__ __forceinline__ u64 make(unsigned d2, int row) { return ((u64)d2 << 32) | (unsigned)row; }
};

// knn_tile.h's tile_select on integer accumulators: D2 = (qsq + bsq) - 2 dot, exact (unsigned arithmetic: no step overflows, see MAX_D)
template <bool KEYS, class RowOf>
__device__ __forceinline__ void tile_select_int(const i32x16 (&acc)[TB][TQ], const int* qn_s, const int* bn_s, const TileThread& t,
                                                typename SelQ<KEYS>::T (&best)[TQ][3], RowOf rowof) {
    unsigned qn[TQ];
#pragma unroll
    for (int j = 0; j < TQ; ++j) qn[j] = (unsigned)qn_s[(t.wq * TQ + j) * 32 + t.r];
#pragma unroll
    for (int i = 0; i < TB; ++i) {
        const int l0 = (t.wb * TB + i) * 32 + 4 * t.h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const i32x4 bn = *(const i32x4*)(bn_s + l0 + 8 * g);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const RowId row = rowof(l0 + 8 * g, c);
#pragma unroll
                for (int j = 0; j < TQ; ++j) {
                    const unsigned d2 = (qn[j] + (unsigned)bn[c]) - 2u * (unsigned)acc[i][j][4 * g + c];
                    keep3(row.ok ? SelQ<KEYS>::make(d2, row.id) : SelQ<KEYS>::none(), best[j][0], best[j][1], best[j][2]);
                }
            }
        }
    }
}

struct L2qParams {
    const signed char* x;   // [N][D] query codes
    const int* xsq;         // [N] their squared norms
    const float* xex;       // [N] the queries' excess
    const signed char* bank;  // [R][D] bank codes
    const int* bsq;         // [R] their squared norms
    void* part;             // [S][N][3] 32-bit D2 or 64-bit keys of each query over each split, ascending (S > 1 only)
    float* out;             // [N] mean form
    float* dist;            // [N][k] index form
    int* idx;               // [N][k] index form
    int64_t N;
    int D, R, rows_per, k;
    float s2;               // s s
};

__device__ __forceinline__ float root_of(const L2qParams& p, int64_t row, unsigned d2) {
    return sqrtf(__builtin_fmaf(p.s2, (float)d2, p.xex[row]));
}
// the k winners of query `row`: the sequential fp32 sum of their roots over k, or the (root, row) pairs (k <= bank rows: all are real)
__device__ __forceinline__ void write_result_q(const L2qParams& p, int64_t row, unsigned a, unsigned b, unsigned c) {
    float s = root_of(p, row, a);
    if (p.k > 1) s += root_of(p, row, b);
    if (p.k > 2) s += root_of(p, row, c);
    p.out[row] = s / (float)p.k;
}
__device__ __forceinline__ void write_result_q(const L2qParams& p, int64_t row, u64 a, u64 b, u64 c) {
    const u64 key[3] = {a, b, c};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < p.k) {
            p.dist[row * p.k + j] = root_of(p, row, (unsigned)(key[j] >> 32));
            p.idx[row * p.k + j] = (int)(unsigned)key[j];
        }
    }
}

// Grid (ceil(N / 128), S): workgroup (t, s) scores queries [128 t, 128 t + 128) against the bank rows [s rows_per, (s + 1) rows_per).
// Four waves, each a 64 x 64 block of the tile (2 x 2 accumulators of v_mfma_i32_32x32x32_i8).  A K step stages 128 codes of 256 rows
// -- 16-byte buffer loads: rows past N or R and columns past D read zeros (code 0, not -128: it adds nothing to a dot; such rows are
// masked in the epilogue) -- in two LDS stages; per 32 columns a wave reads two bank and two query fragments (ds_read_b128: the 16
// codes at 32 kk + 16 h of row r for lane (r, h)) for four MFMAs.  Both operands take their k from the same (h, byte) place, so the
// instruction's own order of k inside a lane does not matter.  The 32-column groups of the last step that lie past D are skipped.
// Register e of lane (r, h) in block (i, j) is bank row (e & 3) + 8 (e >> 2) + 4 h of query column r, as in every 32 x 32 MFMA.
template <bool KEYS>
__global__ __launch_bounds__(NT, 2) void l2q_knn_kernel(L2qParams p) {
    typedef typename SelQ<KEYS>::T T;
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

    T best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = SelQ<KEYS>::none();
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
        tile_select_int<KEYS>(acc, qn_s, bn_s, t, best, [&](int l, int c) { return RowId{n0 + l + c < p.R, n0 + l + c}; });
    }
    tile_tail(best, lds, t, [&](int slot, T a, T b, T c) {
        const int64_t row = m0 + slot;
        if (row >= p.N) return;
        if (gridDim.y == 1) write_result_q(p, row, a, b, c);
        else put3((T*)p.part + ((int64_t)blockIdx.y * p.N + row) * 3, a, b, c);
    });
}

// the three smallest of the S triples of query n, then the one-launch epilogue
template <bool KEYS>
__global__ void l2q_knn_merge_kernel(L2qParams p, int S) {
    typedef typename SelQ<KEYS>::T T;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= p.N) return;
    T a = SelQ<KEYS>::none(), b = a, c = a;
    merge_splits((const T*)p.part, S, p.N, n, a, b, c);
    write_result_q(p, n, a, b, c);
}

template <bool KEYS>
static int l2q_knn_launch(L2qParams p, int S, void* stream) {
    p.rows_per = (int)(cdiv64(cdiv64(p.R, BB), S) * BB);
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(l2q_knn_kernel<KEYS>, LDS_BYTES);
        attr_set = true;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(l2q_knn_kernel<KEYS>, dim3((unsigned)cdiv64(p.N, BQ), (unsigned)S), dim3(NT), LDS_BYTES, st, p);
    SSAD_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(l2q_knn_merge_kernel<KEYS>, dim3((unsigned)cdiv64(p.N, 256)), dim3(256), 0, st, p, S);
        SSAD_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

// D 255^2 is the largest D2 (a query of codes -128 against a row of codes 127): it fits int32 for D <= 33025, and 32768 is the bound
// kept; qsq + bsq <= 2 D 128^2 = 2^30 and |dot| <= D 128^2 = 2^29 then fit as well.
#define SSAD_L2Q_KNN_CHECKS()                                                                                                    \
    SSAD_CHECK_ARG(D % 32 == 0 && D <= MAX_D, "D must be a multiple of 32, at most 32768 (D 255^2 must fit int32)");            \
    SSAD_CHECK_ARG(k >= 1 && k <= 3 && k <= R, "k in 1..3 and <= bank rows");                                                    \
    SSAD_CHECK_ARG((((uintptr_t)xq | (uintptr_t)bankq) & 15) == 0, "code rows must be 16-byte aligned");                         \
    SSAD_CHECK_ARG(S >= 1 && S <= 65535 && (S == 1 || part), "S in 1..65535, with a workspace when S > 1");                      \
    SSAD_CHECK_ARG(S == 1 || ((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");                                         \
    SSAD_CHECK_ARG(cdiv64(N, BQ) < (int64_t)2147483647, "too many rows for one launch")

// codes[n][j] = c(x[n][j]) (int8, the expression at the top of this file), sq[n] = sum_j codes[n][j]^2 (int32) and excess[n] =
// sum_j (x[n][j] - clamp(x[n][j], lo, fmaf(255, s, lo)))^2 in fp32 in ssad_row_sqnorms' order, in one pass over the rows.
extern "C" int ssad_rows_to_int8(const float* x, void* codes, int* sq, float* excess, int64_t N, int D, float lo, float inv_s, float s,
                                 void* stream) {
    SSAD_CHECK_ARG(x && codes && sq && excess && N > 0 && D > 0, "bad argument");
    SSAD_CHECK_ARG(D % 32 == 0 && D <= MAX_D, "D must be a multiple of 32, at most 32768 (D 255^2 must fit int32)");
    SSAD_CHECK_ARG((((uintptr_t)x) & 15) == 0 && (((uintptr_t)codes) & 7) == 0, "rows must be 16-byte aligned, codes 8-byte aligned");
    SSAD_CHECK_ARG(cdiv64(N, (NT / 64) * RQ) < (int64_t)2147483647, "too many rows for one launch");
    hipLaunchKernelGGL(rows_to_int8_kernel, dim3((unsigned)cdiv64(N, (NT / 64) * RQ)), dim3(NT), 0, (hipStream_t)stream, x,
                       (signed char*)codes, sq, excess, N, D, lo, inv_s, s);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// The mean of the k smallest d(q, b) of every query: xq [N][D] / bankq [R][D] codes (16-byte aligned), x_sq / bank_sq their int32
// squared norms and x_excess the queries' excess (ssad_rows_to_int8), s2 = s s.  S bank splits (1: one launch; else part [S][N][3]
// uint32, caller-owned, 8-byte aligned, and a merge launch); the same bits for every S.
extern "C" int ssad_l2q_knn_fused(const void* xq, const int* x_sq, const float* x_excess, const void* bankq, const int* bank_sq,
                                  void* part, float* out, int64_t N, int D, int R, int k, int S, float s2, void* stream) {
    SSAD_CHECK_ARG(xq && x_sq && x_excess && bankq && bank_sq && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2Q_KNN_CHECKS();
    return l2q_knn_launch<false>(L2qParams{(const signed char*)xq, x_sq, x_excess, (const signed char*)bankq, bank_sq, part, out, nullptr,
                                           nullptr, N, D, R, 0, k, s2}, S, stream);
}

// kneighbors on codes: the k smallest (D2, bank row) pairs, equal D2 to the smaller row, dist = d -- the bits ssad_l2q_knn_fused
// averages.  part [S][N][3] 64-bit keys when S > 1.
extern "C" int ssad_l2q_knn_index(const void* xq, const int* x_sq, const float* x_excess, const void* bankq, const int* bank_sq,
                                  void* part, float* dist, int* idx, int64_t N, int D, int R, int k, int S, float s2, void* stream) {
    SSAD_CHECK_ARG(xq && x_sq && x_excess && bankq && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2Q_KNN_CHECKS();
    return l2q_knn_launch<true>(L2qParams{(const signed char*)xq, x_sq, x_excess, (const signed char*)bankq, bank_sq, part, nullptr, dist,
                                          idx, N, D, R, 0, k, s2}, S, stream);
}
