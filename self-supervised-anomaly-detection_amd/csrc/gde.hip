// Gaussian density estimator (GDE) scoring of CutPaste (Li et al., CVPR 2021, §3.3): a Gaussian with Ledoit-Wolf shrinkage fitted to
// the normal embeddings, the Mahalanobis distance to it as the anomaly score.  The reference repository has no such scorer; the
// yardstick is sklearn.covariance.LedoitWolf + scipy's mahalanobis in float64 (tests/test_gde_host.py, tests/test_hip_gde.py).
//
// Two entry points:
//  * ssad_gaussian_fit_stats: mean, centred scatter matrix and sum of ||x_i - mean||^4 in fp64 (the sufficient statistics of sklearn's
//    ledoit_wolf_shrinkage); the D x D shrinkage / Cholesky / triangular inverse is a one-off on the host (self_supervised/density.py);
//  * ssad_mahalanobis_fused: out[i] = ||W (x_i - mu)||_2 with W = C^-1 (C C^T = shrunk covariance) in ONE kernel on the fp32 matrix
//    cores -- cosine_knn_fused_kernel's structure (knn.hip) with the rows of W in place of the bank and a sum of squares in place of
//    the three smallest distances.  No N x D intermediate is written.
//
// Both optionally L2-normalise a row first with l2norm_rows_kernel's expression and order (misc.hip), so that the rows they see are
// bit-identical to ssad_l2_normalize_rows.
#include "common.h"

namespace {

constexpr unsigned OOB = 0x80000000u;   // size given to the buffers: offsets from here on read zeros
constexpr int SRD3 = 0x00020000;        // raw buffer, 32-bit data format

// ================================================ fit statistics (fp64) ================================================
// Every reduction runs over row blocks whose partials are added in block order by a later launch: no float atomics, the same bits
// on every call.  Workspace (stream-ordered, freed on the stream): row norms, column-sum partials, scatter partials, m4 partials.

// one wave per row: l2norm_rows_kernel's squares, order and butterfly
__global__ void gde_row_norms_kernel(const float* __restrict__ x, float* __restrict__ nrm, int64_t N, int D) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const float* p = x + row * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s += p[k] * p[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) nrm[row] = s == 0.f ? 1.f : sqrtf(s);       // a zero sum divides by 1, as l2norm_rows_kernel does
}

// the fp32 row element the statistics are of: x itself, or l2norm_rows_kernel's x / ||x||
__device__ __forceinline__ float row_elem(const float* x, const float* nrm, int64_t row, int D, int k) {
    const float v = x[row * D + k];
    return nrm ? v / nrm[row] : v;
}

// part[s][d] = sum over the rows of split s (ascending) of row element d; grid (ceil(D / 64), S1), 64 threads
__global__ void gde_colsum_kernel(const float* __restrict__ x, const float* __restrict__ nrm, double* __restrict__ part, int64_t N,
                                  int D, int64_t rows_per) {
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (d >= D) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = r0 + rows_per < N ? r0 + rows_per : N;
    double s = 0.0;
    for (int64_t r = r0; r < r1; ++r) s += (double)row_elem(x, nrm, r, D, d);
    part[(int64_t)blockIdx.y * D + d] = s;
}

__global__ void gde_mean_kernel(const double* __restrict__ part, double* __restrict__ mean, int S1, int64_t N, int D) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (int i = 0; i < S1; ++i) s += part[(int64_t)i * D + d];
    mean[d] = s / (double)N;
}

// Scatter: 64 x 64 tiles of the lower triangle (tile row ti >= tile column tj), rows split into S ranges; a tile's partial is
// written to both triangles.  256 threads, 4 x 4 doubles each (rows ty + 16 u, columns tx + 16 v), 32 centred rows per LDS stage.
constexpr int SC_T = 64, SC_K = 32;
__global__ __launch_bounds__(256) void gde_scatter_kernel(const float* __restrict__ x, const float* __restrict__ nrm,
                                                          const double* __restrict__ mean, double* __restrict__ dst, int64_t N, int D,
                                                          int64_t rows_per) {
    __shared__ double As[SC_K][SC_T], Bs[SC_K][SC_T];
    int t = blockIdx.x, ti = 0;
    while (t > ti) { t -= ti + 1; ++ti; }      // blockIdx.x = ti (ti + 1) / 2 + tj, tj <= ti
    const int tj = t;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = r0 + rows_per < N ? r0 + rows_per : N;
    double* out = dst + (int64_t)blockIdx.y * D * D;
    double acc[4][4] = {};
    // staging: element (k = tid >> 6 + 4 q, column tid & 63) of both tiles
    const int cc = tid & 63, kr = tid >> 6;
    const int ca = ti * SC_T + cc, cb = tj * SC_T + cc;
    const double ma = ca < D ? mean[ca] : 0.0, mb = cb < D ? mean[cb] : 0.0;
    for (int64_t k0 = r0; k0 < r1; k0 += SC_K) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SC_K / 4; ++q) {
            const int k = kr + 4 * q;
            const int64_t row = k0 + k;
            const bool ok = row < r1;
            As[k][cc] = ok && ca < D ? (double)row_elem(x, nrm, row, D, ca) - ma : 0.0;
            Bs[k][cc] = ok && cb < D ? (double)row_elem(x, nrm, row, D, cb) - mb : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < SC_K; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = As[k][ty + 16 * u];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = Bs[k][tx + 16 * v];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int a = ti * SC_T + ty + 16 * u;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int b = tj * SC_T + tx + 16 * v;
            if (a < D && b < D) {
                out[(int64_t)a * D + b] = acc[u][v];
                if (ti != tj) out[(int64_t)b * D + a] = acc[u][v];    // c_a c_b == c_b c_a: the mirror is exact
            }
        }
    }
}

__global__ void gde_sum_partials_kernel(const double* __restrict__ part, double* __restrict__ out, int S, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < S; ++j) s += part[(int64_t)j * n + i];
    out[i] = s;
}

// m4 partial of a row block: sum over its rows (ascending per wave, waves in order) of (sum_d (x_d - mean_d)^2)^2
__global__ __launch_bounds__(256) void gde_m4_kernel(const float* __restrict__ x, const float* __restrict__ nrm,
                                                     const double* __restrict__ mean, double* __restrict__ part, int64_t N, int D,
                                                     int64_t rows_per) {
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < N ? r0 + rows_per : N;
    double acc = 0.0;
    for (int64_t r = r0 + wave; r < r1; r += 4) {
        double s = 0.0;
        for (int k = lane; k < D; k += 64) {
            const double c = (double)row_elem(x, nrm, r, D, k) - mean[k];
            s = fma(c, c, s);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        acc = fma(s, s, acc);
    }
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// ================================================ Mahalanobis scoring (fp32 MFMA) ================================================
// Orientation as in knn.hip: the rows of W are the M side of the MFMA tile and the QUERIES its N side, so that a lane's 16 accumulator
// registers are 16 components of W (x - mu) of ONE query (column r) and are squared and summed straight from the accumulators.
constexpr int BB = 128, BQ = 128, BK = 32, LDK = BK + 4, TB = 2, TQ = 2, NT = 256;      // W rows x queries per workgroup tile
constexpr int STAGE = (BB + BQ) * LDK;          // floats

struct MahaParams {
    const float* x;       // [N][D] queries
    const float* mu_hi;   // [D] mean, rounded to fp32
    const float* mu_lo;   // [D] mean - mu_hi, rounded to fp32
    const float* w;       // [D][D] lower-triangular inverse Cholesky factor (the upper triangle is not read)
    float* out;           // [N]
    int64_t N;
    int D;
};

template <bool NORM>
__global__ __launch_bounds__(NT, 2) void mahalanobis_fused_kernel(MahaParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* nrm_s = lds + 2 * STAGE;             // [BQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wb = wave >> 1, wq = wave & 1;    // 64-row W block / 64-query block of this wave
    const int64_t m0 = (int64_t)blockIdx.x * BQ;
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc of rows sr + 32 i

    // ---- query norms (knn.hip's prologue: l2norm_rows_kernel's order, eight rows in flight per wave) ----
    float nrm[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (NORM) {
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
#pragma unroll
        for (int i = 0; i < 4; ++i) nrm[i] = nrm_s[sr + 32 * i];
    }
    // buffer offsets: one 32-bit offset per staged row, rows outside the tensor read zeros
    unsigned qoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        qoff[i] = m0 + sr + 32 * i < p.N ? (unsigned)(((sr + 32 * i) * p.D + sc * 4) * 4) : OOB;
    const float* xblk = p.x + m0 * p.D;

    float ss[TQ] = {0.f, 0.f};                  // sum of squares of this lane's query columns over the W rows it has seen
    const int nks = p.D / BK;

    for (int n0 = 0; n0 < p.D; n0 += BB) {
        unsigned woff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) woff[i] = n0 + sr + 32 * i < p.D ? (unsigned)(((sr + 32 * i) * p.D + sc * 4) * 4) : OOB;
        const float* wblk = p.w + (int64_t)n0 * p.D;
        // W is lower triangular: rows n0 .. n0 + BB - 1 are zero from column n0 + BB on
        const int nk = nks < (n0 + BB) / BK ? nks : (n0 + BB) / BK;
        f32x16 acc[TB][TQ];
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int j = 0; j < TQ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        f32x4 rq[4], rb[4], mh, ml;
        int kc = 0;                             // first column of the chunk the registers hold
        auto load = [&](int ks) {
            kc = ks * BK + sc * 4;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(xblk + ks * BK), 0, (int)OOB, SRD3);
            const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(wblk + ks * BK), 0, (int)OOB, SRD3);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                rq[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, qoff[i], 0, 0));
                rb[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, woff[i], 0, 0));
            }
            mh = *(const f32x4*)(p.mu_hi + ks * BK + sc * 4);
            ml = *(const f32x4*)(p.mu_lo + ks * BK + sc * 4);
        };
        auto store = [&](float* st) {       // the loads were issued a whole K-step of MFMAs ago; normalise and centre while staging
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float v = rq[i][k];
                    if constexpr (NORM) v = v / nrm[i];                   // l2norm_rows_kernel's expression
                    c[k] = (v - mh[k]) - ml[k];                           // exact first difference near the mean (Sterbenz)
                }
                // W rows, the tile's M side: whatever sits above the diagonal is replaced by the zero it stands for
                f32x4 wv;
#pragma unroll
                for (int k = 0; k < 4; ++k) wv[k] = kc + k <= n0 + sr + 32 * i ? rb[i][k] : 0.f;
                *(f32x4*)(st + (sr + 32 * i) * LDK + sc * 4) = wv;
                *(f32x4*)(st + BB * LDK + (sr + 32 * i) * LDK + sc * 4) = c;            // centred queries: its N side
            }
        };
        __syncthreads();                        // every wave has left the previous W tile's last stage
        load(0);
        store(lds);
        __syncthreads();
        for (int ks = 0; ks < nk; ++ks) {
            const float* cur = lds + (ks & 1) * STAGE;
            if (ks + 1 < nk) load(ks + 1);
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
            if (ks + 1 < nk) store(lds + ((ks + 1) & 1) * STAGE);
            __syncthreads();
        }
        // register e of lane (r, h) in block (i, j): component n0 + (wb TB + i) 32 + (e & 3) + 8 (e >> 2) + 4 h of query column r;
        // components past D are rows of zeros (out-of-range buffer reads) and add nothing
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e)
#pragma unroll
                for (int j = 0; j < TQ; ++j) ss[j] = fmaf(acc[i][j][e], acc[i][j][e], ss[j]);
    }
    // ---- a query's partial sums sit in the two lane halves of two waves (wb = 0, 1): halves by shuffle, waves through LDS,
    // always in the same order -- a row's score does not depend on where it sits in the launch ----
    __syncthreads();                            // the stages are dead
    float* M = lds;                             // [2 wq][TQ][32]
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
        ss[j] += __shfl_xor(ss[j], 32);
        if (wb == 1 && h == 0) M[(wq * TQ + j) * 32 + r] = ss[j];
    }
    __syncthreads();
    if (wb == 0 && h == 0) {
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const int64_t row = m0 + (wq * TQ + j) * 32 + r;
            if (row < p.N) p.out[row] = sqrtf(ss[j] + M[(wq * TQ + j) * 32 + r]);
        }
    }
}

}  // namespace

// mean[D], scatter[D][D] = sum_i (x_i - mean)(x_i - mean)^T and m4[0] = sum_i ||x_i - mean||^4, all fp64, of the N rows of x (each
// first L2-normalised as ssad_l2_normalize_rows does when `normalize`).  Deterministic: fixed-order reductions, no float atomics.
extern "C" int ssad_gaussian_fit_stats(const float* x, int64_t N, int D, int normalize, double* mean, double* scatter, double* m4,
                                       void* stream) {
    SSAD_CHECK_ARG(x && mean && scatter && m4 && N >= 1 && D > 0, "bad argument");
    SSAD_CHECK_ARG(D % 32 == 0 && D <= 4096, "D must be a multiple of 32, at most 4096");
    SSAD_CHECK_ARG(N < (int64_t)1 << 40, "too many rows");
    hipStream_t st = (hipStream_t)stream;
    const int T = (D + SC_T - 1) / SC_T, tiles = T * (T + 1) / 2;
    // row splits: enough workgroups for the chip, at least 256 rows each
    int64_t S = cdiv64(N, 256);
    const int64_t smax = 1024 / tiles > 1 ? 1024 / tiles : 1;
    if (S > smax) S = smax;
    const int64_t sc_rows = cdiv64(N, S);
    S = cdiv64(N, sc_rows);
    int64_t S1 = cdiv64(N, 128);
    if (S1 > 2048) S1 = 2048;
    const int64_t cs_rows = cdiv64(N, S1);
    S1 = cdiv64(N, cs_rows);
    int64_t S3 = cdiv64(N, 64);
    if (S3 > 2048) S3 = 2048;
    const int64_t m4_rows = cdiv64(N, S3);
    S3 = cdiv64(N, m4_rows);

    const size_t nrm_bytes = normalize ? (size_t)((N * 4 + 255) / 256 * 256) : 0;
    const size_t cs_bytes = (size_t)S1 * D * 8, sc_bytes = S > 1 ? (size_t)S * D * D * 8 : 0, m4_bytes = (size_t)S3 * 8;
    char* ws = nullptr;
    hipError_t e = hipMallocAsync((void**)&ws, nrm_bytes + cs_bytes + sc_bytes + m4_bytes, st);
    if (e != hipSuccess) {
        ssad_set_error("%s: workspace allocation failed: %s", __func__, hipGetErrorString(e));
        return 1;
    }
    float* nrm = normalize ? (float*)ws : nullptr;
    double* cs_part = (double*)(ws + nrm_bytes);
    double* sc_part = S > 1 ? (double*)(ws + nrm_bytes + cs_bytes) : scatter;
    double* m4_part = (double*)(ws + nrm_bytes + cs_bytes + sc_bytes);
    int rc = 0;
    do {
        if (normalize) hipLaunchKernelGGL(gde_row_norms_kernel, dim3((unsigned)cdiv64(N, 4)), dim3(256), 0, st, x, nrm, N, D);
        hipLaunchKernelGGL(gde_colsum_kernel, dim3((unsigned)cdiv64(D, 64), (unsigned)S1), dim3(64), 0, st, x, nrm, cs_part, N, D,
                           cs_rows);
        hipLaunchKernelGGL(gde_mean_kernel, dim3((unsigned)cdiv64(D, 256)), dim3(256), 0, st, cs_part, mean, (int)S1, N, D);
        hipLaunchKernelGGL(gde_scatter_kernel, dim3((unsigned)tiles, (unsigned)S), dim3(256), 0, st, x, nrm, mean, sc_part, N, D,
                           sc_rows);
        if (S > 1)
            hipLaunchKernelGGL(gde_sum_partials_kernel, dim3((unsigned)cdiv64((int64_t)D * D, 256)), dim3(256), 0, st, sc_part, scatter,
                               (int)S, (int64_t)D * D);
        hipLaunchKernelGGL(gde_m4_kernel, dim3((unsigned)S3), dim3(256), 0, st, x, nrm, mean, m4_part, N, D, m4_rows);
        hipLaunchKernelGGL(gde_sum_partials_kernel, dim3(1), dim3(1), 0, st, m4_part, m4, (int)S3, (int64_t)1);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) {
            ssad_set_error("%s: launch failed: %s", __func__, hipGetErrorString(le));
            rc = 1;
        }
    } while (0);
    e = hipFreeAsync(ws, st);
    if (e != hipSuccess && rc == 0) {
        ssad_set_error("%s: workspace release failed: %s", __func__, hipGetErrorString(e));
        rc = 1;
    }
    return rc;
}

// out[i] = ||W (x_i - mu)||_2, mu = mu_hi + mu_lo, W [D][D] lower triangular (its upper triangle is not read: what the tile loads of
// it is replaced by zeros while staging, so it may hold anything, NaN included); x_i first
// L2-normalised as ssad_l2_normalize_rows does when `normalize`.  32 <= D <= 1024, D % 32 == 0.  One workgroup scores 128 rows over
// all of W: no split over K or W rows across workgroups, so a row's score is the same bits whatever N and wherever it sits.
extern "C" int ssad_mahalanobis_fused(const float* x, const float* mu_hi, const float* mu_lo, const float* w, float* out, int64_t N,
                                      int D, int normalize, void* stream) {
    SSAD_CHECK_ARG(x && mu_hi && mu_lo && w && out && N > 0, "bad argument");
    SSAD_CHECK_ARG(D % BK == 0 && D >= 32 && D <= 1024, "D must be a multiple of 32 in 32..1024");
    SSAD_CHECK_ARG(cdiv64(N, BQ) < (int64_t)2147483647, "too many rows for one launch");
    constexpr int lds_bytes = (2 * STAGE + BQ) * 4;
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(mahalanobis_fused_kernel<true>, lds_bytes);
        SSAD_SET_DYN_LDS(mahalanobis_fused_kernel<false>, lds_bytes);
        attr_set = true;
    }
    MahaParams p{x, mu_hi, mu_lo, w, out, N, D};
    if (normalize)
        hipLaunchKernelGGL(mahalanobis_fused_kernel<true>, dim3((unsigned)cdiv64(N, BQ)), dim3(NT), lds_bytes, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(mahalanobis_fused_kernel<false>, dim3((unsigned)cdiv64(N, BQ)), dim3(NT), lds_bytes, (hipStream_t)stream, p);
    SSAD_CHECK_LAUNCH();
    return 0;
}
