// Euclidean k-NN scoring (PatchCore / SPADE's metric; opt-in beside the cosine kernels of knn.hip): the distance of a query q to a bank
// row b is d = sqrt(max(|q|^2 + |b|^2 - 2 <q, b>, 0)) on the raw rows -- the expanded form torch.cdist evaluates -- formed in fp32:
//   <q, b>       the MFMA chain of knn.hip's tile (same tile, same K order, same staging) on UNNORMALISED operands,
//   |q|^2, |b|^2 one summation order (sqnorm_wave: lane-strided fma, xor butterfly) wherever they are taken, so equal rows give equal bits,
//   d2           fmaxf((qn + bn) - 2 dot, 0) in the per-tile epilogue; the K loop is knn.hip's, untouched by the metric.
// Selection runs on d2 (monotone in d); sqrtf is applied to the k winners only.  One kernel template serves both entry points:
// mean or (distance, row) keys, each one launch (S = 1) or the bank split of ssad_cosine_knn_split with a merge launch.  The tile itself
// -- norms, K loop, epilogue, tail, result writers -- is knn_tile.h's; this file walks the bank with it.
#include "knn_tile.h"

namespace {

constexpr int LDS_BYTES = (2 * STAGE + BQ + BB) * 4;

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

// Grid (ceil(N / 128), S): workgroup (t, s) scores queries [128 t, 128 t + 128) against the bank rows [s rows_per, (s + 1) rows_per).
// Both operands are staged by buffer loads: rows past N or R read zeros.
template <bool KEYS>
__global__ __launch_bounds__(NT, 2) void l2_knn_kernel(L2Params p) {
    typedef typename Sel<KEYS>::T T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* qn_s = lds + 2 * STAGE;              // [BQ] squared norms of the queries
    float* bn_s = qn_s + BQ;                    // [BB] squared norms of the current bank tile
    const TileThread t{};
    const int64_t m0 = (int64_t)blockIdx.x * BQ;

    tile_sqnorms<true>(qn_s, p.D, t, [&](int s) { return m0 + s < p.N ? p.x + (m0 + s) * p.D : nullptr; });     // rows past N give 0
    unsigned qoff[4];
    stage_offsets(qoff, m0, p.N, p.D, t);
    const float* xblk = p.x + m0 * p.D;

    T best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = Sel<KEYS>::none();
    const int64_t r_begin = (int64_t)blockIdx.y * p.rows_per;
    const int r_end = (int)(r_begin + p.rows_per < p.R ? r_begin + p.rows_per : p.R);

    for (int n0 = (int)(r_begin < p.R ? r_begin : p.R); n0 < r_end; n0 += BB) {
        unsigned boff[4];
        stage_offsets(boff, n0, p.R, p.D, t);
        f32x16 acc[TB][TQ];
        dot_tile(acc, lds, t, p.bank + (int64_t)n0 * p.D, boff, p.D / BK,
                 [&](int ks, int i) { return buffer_load16(xblk + ks * BK, qoff[i]); },
                 [&] { if (t.tid < BB) bn_s[t.tid] = n0 + t.tid < p.R ? p.bsq[n0 + t.tid] : 0.f; });
        tile_select<KEYS>(acc, qn_s, bn_s, t, best, [&](int l, int c) { return RowId{n0 + l + c < p.R, n0 + l + c}; });
    }
    tile_tail(best, lds, t, [&](int slot, T a, T b, T c) {
        const int64_t row = m0 + slot;
        if (row >= p.N) return;
        if (gridDim.y == 1) write_result(p, row, a, b, c);
        else put3((T*)p.part + ((int64_t)blockIdx.y * p.N + row) * 3, a, b, c);
    });
}

// the three smallest of the S triples of query n, then the one-launch epilogue
template <bool KEYS>
__global__ void l2_knn_merge_kernel(L2Params p, int S) {
    typedef typename Sel<KEYS>::T T;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= p.N) return;
    T a = Sel<KEYS>::none(), b = a, c = a;
    merge_splits((const T*)p.part, S, p.N, n, a, b, c);
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

// KEYS: part holds 64-bit keys (the index form), else floats
#define SSAD_L2_KNN_CHECKS(KEYS)                                                                                \
    SSAD_CHECK_ARG(D % BK == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");                     \
    SSAD_CHECK_ARG(k >= 1 && k <= 3 && k <= R, "k in 1..3 and <= bank rows");                                   \
    SSAD_CHECK_ARG(S >= 1 && S <= 65535 && (S == 1 || part), "S in 1..65535, with a workspace when S > 1");     \
    SSAD_CHECK_ARG(!(KEYS) || ((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");                       \
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
// first; bank_sq = ssad_row_sqnorms(bank).  S = 1: one launch, part unused (may be null).  S > 1: the bank split of
// ssad_cosine_knn_split, part [S][N][3] floats (caller-owned), a second launch merges them.  out is the same bits for every S.
extern "C" int ssad_l2_knn_fused(const float* x, const float* bank, const float* bank_sq, float* part, float* out, int64_t N, int D,
                                 int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2_KNN_CHECKS(false);
    return l2_knn_launch<false>(L2Params{x, bank, bank_sq, part, out, nullptr, nullptr, N, D, R, 0, k}, S, stream);
}

// kneighbors of the Euclidean bank: the k smallest (d2, bank row) pairs of every query in lexicographic order, dist [N][k] = sqrt(d2)
// and idx [N][k] int32 -- the distances are the bits ssad_l2_knn_fused averages, equal d2 go to the smaller row.  part [S][N][3]
// 64-bit keys (caller-owned, 8-byte aligned) when S > 1; the same bits for every S.
extern "C" int ssad_l2_knn_index(const float* x, const float* bank, const float* bank_sq, void* part, float* dist, int* idx, int64_t N,
                                 int D, int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2_KNN_CHECKS(true);
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
