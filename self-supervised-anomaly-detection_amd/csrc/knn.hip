// Cosine k-NN scoring in ONE kernel: row L2-normalisation of the queries, the similarity GEMM against the (normalised) bank on the
// fp32 matrix cores and the mean of the k smallest clip(1 - sim, 0, 2) per query -- the N x R similarity matrix never exists in HBM.
//
// Replaces AnomalyDetector.predict of the reference (src/self_supervised/models.py:363-370: sklearn NearestNeighbors(metric='cosine')
// .kneighbors + torch.mean over the 3 distances) and, before this kernel, the launch chain l2norm_rows -> conv_igemm (sim) ->
// knn_mean: the chain wrote and re-read N x R floats (2.4 GB for the 1 M pixels of a WideResNet-50 layer1 scale).  Every
// intermediate value is formed by the same expression in the same order as in that chain (x / ||x|| per element; the k-order of the
// MFMA chain; the three smallest distances added smallest first), so the scores are bit-identical to it.
#include "knn_tile.h"

namespace {

// Orientation: the BANK rows are the M side of the MFMA tile and the QUERIES its N side, so that a lane's 16 accumulator registers are
// 16 bank rows of ONE query (column r) and the three smallest distances are kept straight from the accumulators, branch-free -- no
// trip of every tile through LDS and no scalar scan (round 4: the LDS epilogue was 2.4 of the 6.3 ms of the 1 M-query WideResNet-50
// layer1 call, the one-row-at-a-time norm prologue another ~2 ms; tools/knn_probe.py).
// The tile's constants and the selection (keep3) are knn_tile.h's, which the Euclidean kernels share.

struct KnnParams {
    const float* x;       // [N][D] queries (not normalised)
    const float* bank;    // [R][D] bank rows, L2-normalised (ssad_l2_normalize_rows)
    float* out;           // [N]
    int64_t N;
    int D, R, k;
};

__global__ __launch_bounds__(NT, 2) void cosine_knn_fused_kernel(KnnParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* nrm_s = lds + 2 * STAGE;             // [BQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wb = wave >> 1, wq = wave & 1;    // 64-row bank block / 64-query block of this wave
    const int64_t m0 = (int64_t)blockIdx.x * BQ;
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc of rows sr + 32 i

    // ---- query norms: one wave per row, lane-strided squares + xor butterfly (l2norm_rows_kernel's order), eight rows in flight
    // per wave (one row at a time was a chain of 32 memory latencies per workgroup) ----
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
            for (int u = 0; u < 8; ++u) s[u] += v[u] * v[u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float t = s[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == 0) nrm_s[base + 4 * u] = t == 0.f ? 1.f : sqrtf(t);     // a zero sum divides by 1 (l2norm_rows_kernel)
        }
    }
    __syncthreads();
    float nrm[4];
    const float* qptr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = m0 + sr + 32 * i;
        nrm[i] = nrm_s[sr + 32 * i];
        qptr[i] = row < p.N ? p.x + row * p.D + sc * 4 : nullptr;
    }

    // running three smallest distances of this lane's queries (column r of its TQ query blocks) over the bank rows it has seen
    float best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = INFINITY;
    const int nks = p.D / BK;

    for (int n0 = 0; n0 < p.R; n0 += BB) {
        const float* bptr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = n0 + sr + 32 * i;
            bptr[i] = row < p.R ? p.bank + (int64_t)row * p.D + sc * 4 : nullptr;
        }
        f32x16 acc[TB][TQ];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        f32x4 rq[4], rb[4];
        auto load = [&](int ks) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (qptr[i]) v = *(const f32x4*)(qptr[i] + ks * BK);
                rq[i] = v;
                f32x4 w = {0.f, 0.f, 0.f, 0.f};
                if (bptr[i]) w = *(const f32x4*)(bptr[i] + ks * BK);
                rb[i] = w;
            }
        };
        auto store = [&](float* st) {       // the loads were issued a whole K-step of MFMAs ago; normalise while staging
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (qptr[i]) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) rq[i][k] = rq[i][k] / nrm[i];  // l2norm_rows_kernel's expression
                }
                *(f32x4*)(st + (sr + 32 * i) * LDK + sc * 4) = rb[i];                   // bank rows: the tile's M side
                *(f32x4*)(st + BB * LDK + (sr + 32 * i) * LDK + sc * 4) = rq[i];        // queries: its N side
            }
        };
        __syncthreads();                        // every wave has left the previous bank tile's last stage
        load(0);
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
        // ---- register e of lane (r, h) in block (i, j): bank row n0 + (wb TB + i) 32 + (e & 3) + 8 (e >> 2) + 4 h, query column r ----
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const int row0 = n0 + (wb * TB + i) * 32 + 4 * h;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const bool ok = row0 + (e & 3) + 8 * (e >> 2) < p.R;
#pragma unroll
                for (int j = 0; j < TQ; ++j) {
                    float d = 1.f - acc[i][j][e];
                    d = fminf(fmaxf(d, 0.f), 2.f);
                    keep3(ok ? d : INFINITY, best[j][0], best[j][1], best[j][2]);
                }
            }
        }
    }
    // ---- a query's candidates sit in the two lane halves of two waves (wb = 0, 1): halves by shuffle, waves through LDS ----
    __syncthreads();                            // the stages are dead
    float* M = lds;                             // [2 wq][TQ][32][3]
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
        const float oa = __shfl_xor(best[j][0], 32), ob = __shfl_xor(best[j][1], 32), oc = __shfl_xor(best[j][2], 32);
        keep3(oa, best[j][0], best[j][1], best[j][2]);
        keep3(ob, best[j][0], best[j][1], best[j][2]);
        keep3(oc, best[j][0], best[j][1], best[j][2]);
        if (wb == 1 && h == 0) {
            float* m = M + ((wq * TQ + j) * 32 + r) * 3;
            m[0] = best[j][0]; m[1] = best[j][1]; m[2] = best[j][2];
        }
    }
    __syncthreads();
    if (wb == 0 && h == 0) {
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const float* m = M + ((wq * TQ + j) * 32 + r) * 3;
            float a = best[j][0], b = best[j][1], c = best[j][2];
            keep3(m[0], a, b, c);
            keep3(m[1], a, b, c);
            keep3(m[2], a, b, c);
            const int64_t row = m0 + (wq * TQ + j) * 32 + r;
            if (row < p.N) {
                float s = a;                    // the k smallest, smallest first
                if (p.k > 1) s += b;
                if (p.k > 2) s += c;
                p.out[row] = s / (float)p.k;
            }
        }
    }
}

// ================================================ bank-split form ================================================
// One workgroup per (128-query tile, bank split): the fused kernel's tile body over the bank rows [s rows_per, (s + 1) rows_per)
// only (rows_per a multiple of BB, so a bank tile sits in one split and every bank row at the same place of its tile as in the fused
// kernel), the three smallest distances of each query written to part[s][n][0..2] -- INFINITY where the split has fewer than three
// rows.  A second launch merges the S triples per query.  Meant for big banks and few queries: the fused kernel gives the whole bank
// to cdiv(N, 128) workgroups, 7 for one image of 841 patches on a 256-CU chip.
//
// Operands are staged with buffer loads (gde.hip's mahalanobis_fused_kernel): a scalar base per K-step, one 32-bit offset
// per staged row, rows past N or R read zeros -- no per-row pointer select in the matrix loop.

struct KnnSplitParams {
    const float* x;       // [N][D] queries (not normalised)
    const float* bank;    // [R][D] bank rows, L2-normalised
    float* part;          // [S][N][3] three smallest distances of each query over each split, ascending
    int64_t N;
    int D, R, rows_per;
};

__global__ __launch_bounds__(NT, 2) void cosine_knn_split_kernel(KnnSplitParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* nrm_s = lds + 2 * STAGE;             // [BQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wb = wave >> 1, wq = wave & 1;    // 64-row bank block / 64-query block of this wave
    const int64_t m0 = (int64_t)blockIdx.x * BQ;
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc of rows sr + 32 i

    // ---- query norms: cosine_knn_fused_kernel's prologue (l2norm_rows_kernel's order); rows past N get 1 (they read zeros) ----
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
            for (int u = 0; u < 8; ++u) s[u] += v[u] * v[u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float t = s[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == 0) nrm_s[base + 4 * u] = (m0 + base + 4 * u < p.N && t != 0.f) ? sqrtf(t) : 1.f;   // a zero sum divides by 1
        }
    }
    __syncthreads();
    float nrm[4];
    unsigned qoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        nrm[i] = nrm_s[sr + 32 * i];
        qoff[i] = m0 + sr + 32 * i < p.N ? (unsigned)(((sr + 32 * i) * p.D + sc * 4) * 4) : OOB;
    }
    const float* xblk = p.x + m0 * p.D;

    float best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = INFINITY;
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
        auto store = [&](float* st) {       // normalise while staging: the fused kernel's expression (rows past N: 0 / 1)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int k = 0; k < 4; ++k) rq[i][k] = rq[i][k] / nrm[i];
                *(f32x4*)(st + (sr + 32 * i) * LDK + sc * 4) = rb[i];
                *(f32x4*)(st + BB * LDK + (sr + 32 * i) * LDK + sc * 4) = rq[i];
            }
        };
        __syncthreads();
        load(0);
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
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const int row0 = n0 + (wb * TB + i) * 32 + 4 * h;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const bool ok = row0 + (e & 3) + 8 * (e >> 2) < p.R;
#pragma unroll
                for (int j = 0; j < TQ; ++j) {
                    float d = 1.f - acc[i][j][e];
                    d = fminf(fmaxf(d, 0.f), 2.f);
                    keep3(ok ? d : INFINITY, best[j][0], best[j][1], best[j][2]);
                }
            }
        }
    }
    // ---- the fused kernel's merge of lane halves and waves, then the triple goes out instead of the mean ----
    __syncthreads();
    float* M = lds;                             // [2 wq][TQ][32][3]
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
        const float oa = __shfl_xor(best[j][0], 32), ob = __shfl_xor(best[j][1], 32), oc = __shfl_xor(best[j][2], 32);
        keep3(oa, best[j][0], best[j][1], best[j][2]);
        keep3(ob, best[j][0], best[j][1], best[j][2]);
        keep3(oc, best[j][0], best[j][1], best[j][2]);
        if (wb == 1 && h == 0) {
            float* m = M + ((wq * TQ + j) * 32 + r) * 3;
            m[0] = best[j][0]; m[1] = best[j][1]; m[2] = best[j][2];
        }
    }
    __syncthreads();
    if (wb == 0 && h == 0) {
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const float* m = M + ((wq * TQ + j) * 32 + r) * 3;
            float a = best[j][0], b = best[j][1], c = best[j][2];
            keep3(m[0], a, b, c);
            keep3(m[1], a, b, c);
            keep3(m[2], a, b, c);
            const int64_t row = m0 + (wq * TQ + j) * 32 + r;
            if (row < p.N) {
                float* o = p.part + ((int64_t)blockIdx.y * p.N + row) * 3;
                o[0] = a; o[1] = b; o[2] = c;
            }
        }
    }
}

// out[n] = (a [+ b] [+ c]) / k of the three smallest of the S triples of query n, taken in split order
__global__ void cosine_knn_merge_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t N, int S, int k) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float a = INFINITY, b = INFINITY, c = INFINITY;
    for (int s = 0; s < S; ++s) {
        const float* t = part + ((int64_t)s * N + n) * 3;
        keep3(t[0], a, b, c);
        keep3(t[1], a, b, c);
        keep3(t[2], a, b, c);
    }
    float v = a;                                // the k smallest, smallest first: the fused kernel's epilogue
    if (k > 1) v += b;
    if (k > 2) v += c;
    out[n] = v / (float)k;
}

// ================================================ index-returning form ================================================
// The same tile once more, but the selection carries the bank row: instead of the three smallest distances, the three smallest
// (distance, row) pairs in lexicographic order.  A distance lies in [0, 2], so its bit pattern orders like an unsigned integer;
// (bits(d) << 32) | row is a 64-bit key whose unsigned order IS the lexicographic order, every key of a query is distinct (the row),
// and keep3 with 64-bit min / max keeps the three smallest keys whatever the visiting order -- lane halves, waves, splits.  Rows
// past R carry the all-ones key.  Matrix loop, K order, staging and the place of a bank row in its tile are the split kernel's, so
// the distances are the bits the mean kernels form.  Grid (ceil(N / 128), S): with S = 1 the k pairs go straight out (the one-launch
// form), else the three keys go to part [S][N][3] and cosine_knn_index_merge_kernel merges them.
struct KnnIndexParams {
    const float* x;       // [N][D] queries (not normalised)
    const float* bank;    // [R][D] bank rows, L2-normalised
    u64* part;            // [S][N][3] keys of each query over each split, ascending (S > 1 only)
    float* dist;          // [N][k]
    int* idx;             // [N][k]
    int64_t N;
    int D, R, rows_per, k;
};

__device__ __forceinline__ void write_pairs(const KnnIndexParams& p, int64_t row, u64 a, u64 b, u64 c) {
    const u64 key[3] = {a, b, c};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < p.k) {
            p.dist[row * p.k + j] = __uint_as_float((unsigned)(key[j] >> 32));
            p.idx[row * p.k + j] = (int)(unsigned)key[j];
        }
    }
}

__global__ __launch_bounds__(NT, 2) void cosine_knn_index_kernel(KnnIndexParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* nrm_s = lds + 2 * STAGE;             // [BQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wb = wave >> 1, wq = wave & 1;    // 64-row bank block / 64-query block of this wave
    const int64_t m0 = (int64_t)blockIdx.x * BQ;
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc of rows sr + 32 i

    // ---- query norms: cosine_knn_split_kernel's prologue (l2norm_rows_kernel's order); rows past N get 1 (they read zeros) ----
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
            for (int u = 0; u < 8; ++u) s[u] += v[u] * v[u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float t = s[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == 0) nrm_s[base + 4 * u] = (m0 + base + 4 * u < p.N && t != 0.f) ? sqrtf(t) : 1.f;   // a zero sum divides by 1
        }
    }
    __syncthreads();
    float nrm[4];
    unsigned qoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        nrm[i] = nrm_s[sr + 32 * i];
        qoff[i] = m0 + sr + 32 * i < p.N ? (unsigned)(((sr + 32 * i) * p.D + sc * 4) * 4) : OOB;
    }
    const float* xblk = p.x + m0 * p.D;

    // running three smallest keys of this lane's queries (column r of its TQ query blocks) over the bank rows it has seen
    u64 best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = NOKEY;
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
        auto store = [&](float* st) {       // normalise while staging: the fused kernel's expression (rows past N: 0 / 1)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int k = 0; k < 4; ++k) rq[i][k] = rq[i][k] / nrm[i];
                *(f32x4*)(st + (sr + 32 * i) * LDK + sc * 4) = rb[i];
                *(f32x4*)(st + BB * LDK + (sr + 32 * i) * LDK + sc * 4) = rq[i];
            }
        };
        __syncthreads();
        load(0);
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
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const int row0 = n0 + (wb * TB + i) * 32 + 4 * h;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = row0 + (e & 3) + 8 * (e >> 2);
                const bool ok = row < p.R;
#pragma unroll
                for (int j = 0; j < TQ; ++j) {
                    float d = 1.f - acc[i][j][e];
                    d = fminf(fmaxf(d, 0.f), 2.f);
                    const u64 key = ((u64)__float_as_uint(d) << 32) | (unsigned)row;
                    keep3(ok ? key : NOKEY, best[j][0], best[j][1], best[j][2]);
                }
            }
        }
    }
    // ---- a query's candidates sit in the two lane halves of two waves (wb = 0, 1): halves by shuffle, waves through LDS ----
    __syncthreads();                            // the stages are dead
    u64* M = (u64*)lds;                         // [2 wq][TQ][32][3]
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
        const u64 oa = shfl_xor_any(best[j][0], 32), ob = shfl_xor_any(best[j][1], 32), oc = shfl_xor_any(best[j][2], 32);
        keep3(oa, best[j][0], best[j][1], best[j][2]);
        keep3(ob, best[j][0], best[j][1], best[j][2]);
        keep3(oc, best[j][0], best[j][1], best[j][2]);
        if (wb == 1 && h == 0) {
            u64* m = M + ((wq * TQ + j) * 32 + r) * 3;
            m[0] = best[j][0]; m[1] = best[j][1]; m[2] = best[j][2];
        }
    }
    __syncthreads();
    if (wb == 0 && h == 0) {
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const u64* m = M + ((wq * TQ + j) * 32 + r) * 3;
            u64 a = best[j][0], b = best[j][1], c = best[j][2];
            keep3(m[0], a, b, c);
            keep3(m[1], a, b, c);
            keep3(m[2], a, b, c);
            const int64_t row = m0 + (wq * TQ + j) * 32 + r;
            if (row < p.N) {
                if (gridDim.y == 1) {
                    write_pairs(p, row, a, b, c);
                } else {
                    u64* o = p.part + ((int64_t)blockIdx.y * p.N + row) * 3;
                    o[0] = a; o[1] = b; o[2] = c;
                }
            }
        }
    }
}

// the k smallest of the S key triples of query n (any order gives the same three: the keys are distinct)
__global__ void cosine_knn_index_merge_kernel(KnnIndexParams p, int S) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= p.N) return;
    u64 a = NOKEY, b = NOKEY, c = NOKEY;
    for (int s = 0; s < S; ++s) {
        const u64* t = p.part + ((int64_t)s * p.N + n) * 3;
        keep3(t[0], a, b, c);
        keep3(t[1], a, b, c);
        keep3(t[2], a, b, c);
    }
    write_pairs(p, n, a, b, c);
}

static int knn_index_launch(const float* x, const float* bank, void* part, float* dist, int* idx, int64_t N, int D, int R, int k,
                            int S, void* stream) {
    const int64_t rows_per = cdiv64(cdiv64(R, BB), S) * BB;
    constexpr int lds_bytes = (2 * STAGE + BQ) * 4;
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(cosine_knn_index_kernel, lds_bytes);
        attr_set = true;
    }
    KnnIndexParams p{x, bank, (u64*)part, dist, idx, N, D, R, (int)rows_per, k};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cosine_knn_index_kernel, dim3((unsigned)cdiv64(N, BQ), (unsigned)S), dim3(NT), lds_bytes, st, p);
    SSAD_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(cosine_knn_index_merge_kernel, dim3((unsigned)cdiv64(N, 256)), dim3(256), 0, st, p, S);
        SSAD_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

// out[n] = mean of the k (1..3) smallest clip(1 - <x_n / ||x_n||, bank_r>, 0, 2) over the R bank rows; bank rows are L2-normalised
// (ssad_l2_normalize_rows).  D must be a multiple of 32.
extern "C" int ssad_cosine_knn_fused(const float* x, const float* bank_normalized, float* out, int64_t N, int D, int R, int k,
                                     void* stream) {
    SSAD_CHECK_ARG(x && bank_normalized && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_CHECK_ARG(D % BK == 0, "D must be a multiple of 32");
    SSAD_CHECK_ARG(k >= 1 && k <= 3 && k <= R, "k in 1..3 and <= bank rows");
    SSAD_CHECK_ARG(cdiv64(N, BQ) < (int64_t)2147483647, "too many rows for one launch");
    constexpr int lds_bytes = (2 * STAGE + BQ) * 4;
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(cosine_knn_fused_kernel, lds_bytes);
        attr_set = true;
    }
    KnnParams p{x, bank_normalized, out, N, D, R, k};
    hipLaunchKernelGGL(cosine_knn_fused_kernel, dim3((unsigned)cdiv64(N, BQ)), dim3(NT), lds_bytes, (hipStream_t)stream, p);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// The bank-split form of ssad_cosine_knn_fused: S workgroups per 128-query tile, split s scoring the bank rows
// [s rows_per, (s + 1) rows_per) with rows_per = BB * ceil(ceil(R / BB) / S); part [S][N][3] (caller-owned) receives each split's three
// smallest distances, a second launch merges them per query.  min / max selection and the fused kernel's distance expression and K
// order: out is bit-identical to ssad_cosine_knn_fused for every S.  No float atomics, two launches on `stream`.
extern "C" int ssad_cosine_knn_split(const float* x, const float* bank_normalized, float* part, float* out, int64_t N, int D, int R,
                                     int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank_normalized && part && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_CHECK_ARG(D % BK == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");
    SSAD_CHECK_ARG(k >= 1 && k <= 3 && k <= R, "k in 1..3 and <= bank rows");
    SSAD_CHECK_ARG(S >= 1 && S <= 65535, "S in 1..65535");
    SSAD_CHECK_ARG(cdiv64(N, BQ) < (int64_t)2147483647, "too many rows for one launch");
    const int64_t rows_per = cdiv64(cdiv64(R, BB), S) * BB;
    constexpr int lds_bytes = (2 * STAGE + BQ) * 4;
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(cosine_knn_split_kernel, lds_bytes);
        attr_set = true;
    }
    KnnSplitParams p{x, bank_normalized, part, N, D, R, (int)rows_per};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cosine_knn_split_kernel, dim3((unsigned)cdiv64(N, BQ), (unsigned)S), dim3(NT), lds_bytes, st, p);
    SSAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(cosine_knn_merge_kernel, dim3((unsigned)cdiv64(N, 256)), dim3(256), 0, st, (const float*)part, out, N, S, k);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// kneighbors of the cosine bank: for every query the k (1..3) smallest (distance, bank row) pairs in lexicographic order, ascending,
// dist [N][k] float32 and idx [N][k] int32 -- the distances are the bits ssad_cosine_knn_fused averages, equal distances go to the
// smaller row.  S = 1: one launch, part unused (may be null).  S > 1: the bank split of ssad_cosine_knn_split, part [S][N][3] 64-bit keys
// (caller-owned, 8-byte aligned), a second launch merges them.  No atomics; dist and idx are the same bits on every call and for every S.
// D a multiple of 32, at most 65536; R >= k.
extern "C" int ssad_cosine_knn_index(const float* x, const float* bank_normalized, void* part, float* dist, int* idx, int64_t N, int D,
                                     int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(x && bank_normalized && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_CHECK_ARG(D % BK == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");
    SSAD_CHECK_ARG(k >= 1 && k <= 3 && k <= R, "k in 1..3 and <= bank rows");
    SSAD_CHECK_ARG(S >= 1 && S <= 65535 && (S == 1 || part), "S in 1..65535, with a workspace when S > 1");
    SSAD_CHECK_ARG(((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");
    SSAD_CHECK_ARG(cdiv64(N, BQ) < (int64_t)2147483647, "too many rows for one launch");
    return knn_index_launch(x, bank_normalized, part, dist, idx, N, D, R, k, S, stream);
}
