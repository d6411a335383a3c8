// SPADE's image-conditioned gallery for the Euclidean kNN detector (Cohen & Hoshen 2020; opt-in beside the whole-bank search of
// knn_l2.hip): every query image is scored against the rows of K bank images only, the ones nearest to it by an image descriptor.
//   ssad_group_means     the image descriptor: the mean of an image's P rows, summed in fp64 in row order, rounded once;
//   ssad_l2_direct       stage 1: squared distances between descriptors by direct differences (no cancellation), a wave per pair;
//   ssad_l2_knn_gallery  stage 2: knn_l2.hip's search on an INDIRECT bank -- the bank of query image q is the list of row blocks
//                        [g P, (g + 1) P), g = gallery[q][0 .. K - 1], instead of one contiguous range.
// Stage 2 calls the tile functions l2_knn_kernel calls (knn_tile.h): a (query, bank row) pair gets the bits it gets there, wherever
// the row stands.
#include "knn_tile.h"

namespace {

constexpr int LDS_BYTES = (2 * STAGE + BQ + BB) * 4;

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


// Grid (ceil(P / 128), Q, S): workgroup (t, q, s) scores the queries [128 t, 128 t + 128) of image q -- a query tile never straddles
// two images -- against the gallery entries [s per, (s + 1) per) of that image.  For an entry g it walks the 128-row tiles of the bank
// rows [g P, (g + 1) P); rows past the block's end are masked (they read zeros and make no candidate), never taken from image g + 1.
// An entry outside 0 .. T - 1 is skipped before anything is addressed with it.  A gallery may leave fewer than k rows: the mean is
// then +inf, a missing pair (+inf, -1).
template <bool KEYS>
__global__ __launch_bounds__(NT, 2) void l2_knn_gallery_kernel(GParams p) {
    typedef typename Sel<KEYS>::T T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* qn_s = lds + 2 * STAGE;              // [BQ] squared norms of the queries
    float* bn_s = qn_s + BQ;                    // [BB] squared norms of the current bank tile
    const TileThread t{};
    const int m0 = (int)blockIdx.x * BQ;        // first query of the tile within its image
    const int64_t q0 = (int64_t)blockIdx.y * p.P + m0;     // ... among all queries

    tile_sqnorms<true>(qn_s, p.D, t, [&](int s) { return m0 + s < p.P ? p.x + (q0 + s) * p.D : nullptr; });     // past the image's end: 0
    unsigned qoff[4];
    stage_offsets(qoff, m0, p.P, p.D, t);
    const float* xblk = p.x + q0 * p.D;

    T best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = Sel<KEYS>::none();
    const int e_begin = (int)blockIdx.z * p.per;
    const int e_end = e_begin + p.per < p.K ? e_begin + p.per : p.K;
    const int* gal = p.gallery + (int64_t)blockIdx.y * p.K;

    for (int en = e_begin; en < e_end; ++en) {
        const int g = __builtin_amdgcn_readfirstlane(gal[en]);      // one value for the whole workgroup
        if ((unsigned)g >= (unsigned)p.T) continue;                 // not a bank image: never dereferenced
        const int64_t g0 = (int64_t)g * p.P;                        // first global row of the block
        for (int n0 = 0; n0 < p.P; n0 += BB) {
            unsigned boff[4];
            stage_offsets(boff, n0, p.P, p.D, t);
            f32x16 acc[TB][TQ];
            dot_tile(acc, lds, t, p.bank + (g0 + n0) * p.D, boff, p.D / BK,
                     [&](int ks, int i) { return buffer_load16(xblk + ks * BK, qoff[i]); },
                     [&] { if (t.tid < BB) bn_s[t.tid] = n0 + t.tid < p.P ? p.bsq[g0 + n0 + t.tid] : 0.f; });
            // the global bank row (T P fits an int: checked by the host)
            tile_select<KEYS>(acc, qn_s, bn_s, t, best, [&](int l, int c) { return RowId{n0 + l + c < p.P, (int)g0 + n0 + l + c}; });
        }
    }
    tile_tail(best, lds, t, [&](int slot, T a, T b, T c) {
        if (m0 + slot >= p.P) return;
        const int64_t N = (int64_t)p.Q * p.P, row = (int64_t)blockIdx.y * p.P + m0 + slot;
        if (gridDim.z == 1) write_result<true>(p, row, a, b, c);
        else put3((T*)p.part + ((int64_t)blockIdx.z * N + row) * 3, a, b, c);
    });
}

// the three smallest of the S triples of query n, then the one-launch epilogue
template <bool KEYS>
__global__ void l2_knn_gallery_merge_kernel(GParams p, int S) {
    typedef typename Sel<KEYS>::T T;
    const int64_t N = (int64_t)p.Q * p.P;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    T a = Sel<KEYS>::none(), b = a, c = a;
    merge_splits((const T*)p.part, S, N, n, a, b, c);
    write_result<true>(p, n, a, b, c);
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

// ssad_l2_knn_fused with the bank of query image q restricted to the blocks of gallery[q][0 .. K - 1]: out [Q P].
extern "C" int ssad_l2_knn_gallery(const float* x, const float* bank, const float* bank_sq, const int* gallery, float* part, float* out,
                                   int Q, int P, int T, int K, int D, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && gallery && out, "bad argument");
    SSAD_L2_KNN_GALLERY_CHECKS();
    return l2_knn_gallery_launch<false>(GParams{x, bank, bank_sq, gallery, part, out, nullptr, nullptr, Q, P, T, K, D, k, 0}, S, stream);
}

// ssad_l2_knn_index over the same galleries: dist / idx [Q P][k], idx the GLOBAL bank row; part: 64-bit keys.
extern "C" int ssad_l2_knn_gallery_index(const float* x, const float* bank, const float* bank_sq, const int* gallery, void* part,
                                         float* dist, int* idx, int Q, int P, int T, int K, int D, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank && bank_sq && gallery && dist && idx, "bad argument");
    SSAD_L2_KNN_GALLERY_CHECKS();
    SSAD_CHECK_ARG(((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");
    return l2_knn_gallery_launch<true>(GParams{x, bank, bank_sq, gallery, part, nullptr, dist, idx, Q, P, T, K, D, k, 0}, S, stream);
}
