// Per-position Gaussian detector (PaDiM: Defard et al., ICPR 2020, as anomalib implements it) on the dense rows of
// PeraNet.enable_dense_mode: x [n_img * P][D], row n P + p = position p of image n.  `sel` picks d of the D columns; every position p
// has its own Gaussian over the n_img fit images and the Mahalanobis distance to it is the pixel score.  The reference repository has
// no such scorer: the yardstick is numpy.cov + scipy's mahalanobis in float64 (tests/padim_ref.py).
//
// Three entry points, the first and the last the batched forms of gde.hip's:
//  * ssad_position_gaussian_fit_stats: per position the mean and the centred scatter matrix of the selected columns in fp64; the
//    regulariser, the P Cholesky factors and their triangular inverses are a one-off on the host (self_supervised/density.py), or
//  * ssad_position_gaussian_factor (factor='device'): the same step in fp64 on the device, in place in the scatter buffer;
//  * ssad_position_mahalanobis: out[n P + p] = ||W_p (x_sel - mu_p)||_2 in ONE kernel on the fp32 matrix cores --
//    mahalanobis_fused_kernel's tile (gde.hip) with a workgroup that owns one position and 128 images: W and the mean are that
//    position's, the query rows are gathered through `sel` at a stride of P D floats between images.
#include "common.h"

namespace {

constexpr unsigned OOB = 0x80000000u;   // size given to the buffers: offsets from here on read zeros
constexpr int SRD3 = 0x00020000;        // raw buffer, 32-bit data format

// ================================================ fit statistics (fp64) ================================================
// Images are summed in ascending order by one thread per output element: no split, no float atomics, the same bits on every call.

// mean[p][k] = (sum over the images, ascending, of x[n][p][sel[k]]) / n_img; grid (ceil(d / 64) * P), 64 threads
__global__ void padim_mean_kernel(const float* __restrict__ x, const int* __restrict__ sel, double* __restrict__ mean, int n_img,
                                  int64_t P, int D, int d) {
    const int cb = (d + 63) / 64;
    const int64_t p = blockIdx.x / cb;
    const int k = (int)(blockIdx.x % cb) * 64 + threadIdx.x;
    if (k >= d) return;
    const float* q = x + p * D + sel[k];
    const int64_t stride = P * D;
    double s = 0.0;
    for (int n = 0; n < n_img; ++n) s += (double)q[(int64_t)n * stride];
    mean[p * d + k] = s / (double)n_img;
}

// Scatter of one position: 64 x 64 tiles of the lower triangle (tile row ti >= tile column tj), written to both triangles --
// gde_scatter_kernel with the images of one position as its rows.  256 threads, 4 x 4 doubles each (rows ty + 16 u, columns
// tx + 16 v), 32 centred rows per LDS stage.  blockIdx.x = p * tiles + ti (ti + 1) / 2 + tj.
constexpr int SC_T = 64, SC_K = 32;
__global__ __launch_bounds__(256) void padim_scatter_kernel(const float* __restrict__ x, const int* __restrict__ sel,
                                                            const double* __restrict__ mean, double* __restrict__ dst, int n_img,
                                                            int64_t P, int D, int d, int tiles) {
    __shared__ double As[SC_K][SC_T], Bs[SC_K][SC_T];
    const int64_t p = blockIdx.x / tiles;
    int t = (int)(blockIdx.x % tiles), ti = 0;
    while (t > ti) { t -= ti + 1; ++ti; }
    const int tj = t;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double* out = dst + p * d * d;
    const double* mu = mean + p * d;
    const int64_t stride = P * D;
    double acc[4][4] = {};
    // staging: element (k = tid >> 6 + 4 q, column tid & 63) of both tiles
    const int cc = tid & 63, kr = tid >> 6;
    const int ca = ti * SC_T + cc, cb = tj * SC_T + cc;
    const double ma = ca < d ? mu[ca] : 0.0, mb = cb < d ? mu[cb] : 0.0;
    const float* xa = ca < d ? x + p * D + sel[ca] : nullptr;
    const float* xb = cb < d ? x + p * D + sel[cb] : nullptr;
    for (int k0 = 0; k0 < n_img; k0 += SC_K) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SC_K / 4; ++q) {
            const int k = kr + 4 * q;
            const int n = k0 + k;
            const bool ok = n < n_img;
            As[k][cc] = ok && xa ? (double)xa[(int64_t)n * stride] - ma : 0.0;
            Bs[k][cc] = ok && xb ? (double)xb[(int64_t)n * stride] - mb : 0.0;
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
            if (a < d && b < d) {
                out[(int64_t)a * d + b] = acc[u][v];
                if (ti != tj) out[(int64_t)b * d + a] = acc[u][v];    // c_a c_b == c_b c_a: the mirror is exact
            }
        }
    }
}

// ================================================ Mahalanobis scoring (fp32 MFMA) ================================================
// gde.hip's orientation: the rows of W_p are the M side of the MFMA tile and the QUERIES (the images at position p) its N side, so
// that a lane's 16 accumulator registers are 16 components of W_p (x - mu_p) of ONE image and are squared and summed straight from
// the accumulators.
constexpr int BB = 128, BQ = 128, BK = 32, LDK = BK + 4, TB = 2, TQ = 2, NT = 256;      // W rows x images per workgroup tile
constexpr int STAGE = (BB + BQ) * LDK;          // floats

struct PadimParams {
    const float* x;       // [n_img * P][D]
    const int* sel;       // [d] columns of x, each in [0, D)
    const float* mu_hi;   // [P][d] means, rounded to fp32
    const float* mu_lo;   // [P][d] mean - mu_hi, rounded to fp32
    const float* w;       // [P][d][d] lower-triangular inverse Cholesky factors (the upper triangles are never used)
    float* out;           // [n_img * P]
    int n_img;
    int64_t P;
    int D, d;
    int img_tiles;        // ceil(n_img / BQ)
};

__global__ __launch_bounds__(NT, 2) void position_mahalanobis_kernel(PadimParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wb = wave >> 1, wq = wave & 1;    // 64-row W block / 64-image block of this wave
    const int64_t pos = blockIdx.x / p.img_tiles;
    const int m0 = (int)(blockIdx.x % p.img_tiles) * BQ;      // first image of this tile
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc of rows sr + 32 i
    const int d = p.d;
    const int64_t img_stride = p.P * p.D;       // floats between two images at one position

    // buffer offsets: one 32-bit byte offset per staged image row (the launcher keeps BQ * P * D * 4 below 2^31), images past
    // n_img read zeros without touching memory
    unsigned qoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qoff[i] = m0 + sr + 32 * i < p.n_img ? (unsigned)((int64_t)(sr + 32 * i) * img_stride * 4) : OOB;
    const float* xblk = p.x + ((int64_t)m0 * p.P + pos) * p.D;
    const float* wpos = p.w + pos * d * d;
    const float* mh_p = p.mu_hi + pos * d;
    const float* ml_p = p.mu_lo + pos * d;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)xblk, 0, (int)OOB, SRD3);

    float ss[TQ] = {0.f, 0.f};                  // sum of squares of this lane's image columns over the W rows it has seen
    const int nks = d / BK;

    for (int n0 = 0; n0 < d; n0 += BB) {
        unsigned woff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) woff[i] = n0 + sr + 32 * i < d ? (unsigned)(((sr + 32 * i) * d + sc * 4) * 4) : OOB;
        const float* wblk = wpos + (int64_t)n0 * d;
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
            const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(wblk + ks * BK), 0, (int)OOB, SRD3);
            // the four selected columns of this lane's chunk: a gather inside the image's row
            const int4 c4 = *(const int4*)(p.sel + ks * BK + sc * 4);
            const unsigned co[4] = {(unsigned)c4.x * 4u, (unsigned)c4.y * 4u, (unsigned)c4.z * 4u, (unsigned)c4.w * 4u};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    rq[i][k] = __builtin_bit_cast(
                        float, __builtin_amdgcn_raw_buffer_load_b32(rs, qoff[i] == OOB ? OOB : qoff[i] + co[k], 0, 0));
                rb[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, woff[i], 0, 0));
            }
            mh = *(const f32x4*)(mh_p + ks * BK + sc * 4);
            ml = *(const f32x4*)(ml_p + ks * BK + sc * 4);
        };
        auto store = [&](float* st) {       // the loads were issued a whole K-step of MFMAs ago; centre while staging
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 c;
#pragma unroll
                for (int k = 0; k < 4; ++k) c[k] = (rq[i][k] - mh[k]) - ml[k];     // exact first difference near the mean (Sterbenz)
                // W rows, the tile's M side: whatever sits above the diagonal is replaced by the zero it stands for
                f32x4 wv;
#pragma unroll
                for (int k = 0; k < 4; ++k) wv[k] = kc + k <= n0 + sr + 32 * i ? rb[i][k] : 0.f;
                *(f32x4*)(st + (sr + 32 * i) * LDK + sc * 4) = wv;
                *(f32x4*)(st + BB * LDK + (sr + 32 * i) * LDK + sc * 4) = c;            // centred images: its N side
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
        // register e of lane (r, h) in block (i, j): component n0 + (wb TB + i) 32 + (e & 3) + 8 (e >> 2) + 4 h of image column r;
        // components past d are rows of zeros (out-of-range buffer reads) and add nothing
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e)
#pragma unroll
                for (int j = 0; j < TQ; ++j) ss[j] = fmaf(acc[i][j][e], acc[i][j][e], ss[j]);
    }
    // ---- an image's partial sums sit in the two lane halves of two waves (wb = 0, 1): halves by shuffle, waves through LDS,
    // always in the same order -- a score does not depend on where its image sits in the launch ----
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
            const int img = m0 + (wq * TQ + j) * 32 + r;
            if (img < p.n_img) p.out[(int64_t)img * p.P + pos] = sqrtf(ss[j] + M[(wq * TQ + j) * 32 + r]);
        }
    }
}

bool padim_shape_ok(int n_img, int64_t P, int D, int d) {
    return n_img >= 1 && P >= 1 && D > 0 && D % 4 == 0 && d % 32 == 0 && d >= 32 && d <= D;
}

// ================================================ covariance factor (fp64) ================================================
// Per position: Sigma = scatter / (n - 1) + eps I -> C = chol(Sigma) -> W = C^-1, in place in the lower triangle of the scatter
// buffer (the upper triangle is neither read nor written).  One workgroup of d threads owns one matrix and thread i owns ROW i for
// the whole kernel: what a thread reads from global memory is its own row, written by itself, except the 32 x 32 blocks staged
// through LDS.  Both phases walk 32-column blocks; the O(d^3) part of each is one routine, rank32: a row's 32 accumulators take
// 32 columns of that row times a 32 x 32 block that every thread reads from LDS at the same address (a broadcast).
//  * Cholesky, left-looking: block column J starts from Sigma (formed here, where each element of the lower triangle is read
//    exactly once), takes the block columns K < J (rank32 with L[J][K] staged), the 32 x 32 diagonal block is factored in LDS, the
//    rows below solve against it.
//  * Inverse, by forward substitution down block column J = 0, 1, ..: W[K][J] = C[K][K]^-1 (delta_KJ I - sum_{J <= K' < K} C[K][K']
//    W[K'][J]).  Block column J of W replaces block column J of C, which the later columns no longer need; the sums are carried in
//    the rows' accumulators (rank32 with W[K][J] staged), the 32 x 32 solve has one thread per column.
// Every element is (a - sum_k l_k b_k) / pivot as ONE fma chain with k ascending and a true division: Higham's Lemma 8.4, hence
// the componentwise bounds of his Theorems 10.3 (Cholesky) and 8.5 (substitution) with their textbook constants.  No atomics, no
// split of a sum: the same bits on every call and for every P.
constexpr int FB = 32, FLD = 34, FDG = 33, FACTOR_MAX_D = 512;

struct FactorParams {
    const double* mean;   // [P][d]
    double* a;            // [P][d][d] scatter in, workspace
    float* mu_hi;         // [P][d]
    float* mu_lo;         // [P][d]
    float* w;             // [P][d][d]
    double* c_out;        // [P][d][d] or null
    double* w64_out;      // [P][d][d] or null
    int* info;            // [P]
    int d;
    double nm1, eps;
};

// acc[c] -= sum_k l[k] B[c][k], k ascending
__device__ __forceinline__ void rank32(double (&acc)[FB], const double (&l)[FB], const double (*B)[FLD]) {
#pragma unroll
    for (int k = 0; k < FB; k += 2)
#pragma unroll
        for (int c = 0; c < FB; ++c) {
            const double2 b = *(const double2*)&B[c][k];
            acc[c] = fma(-l[k], b.x, acc[c]);
            acc[c] = fma(-l[k + 1], b.y, acc[c]);
        }
}

__global__ __launch_bounds__(FACTOR_MAX_D) void position_factor_kernel(FactorParams q) {
    __shared__ __attribute__((aligned(16))) double B[FB][FLD];     // the staged block, B[c][k]
    __shared__ double Dg[FB][FDG];                                  // a diagonal block
    __shared__ double Sb[FB][FDG];                                  // right-hand sides of the 32 x 32 solve
    __shared__ int fail;
    const int d = q.d, nb = d / FB, i = threadIdx.x, nt = blockDim.x;      // nt == d
    const int ib = i / FB, r = i % FB;
    const int64_t p = blockIdx.x, dd = (int64_t)d * d;
    double* A = q.a + p * dd;
    double* row = A + (int64_t)i * d;
    {
        const double m = q.mean[p * d + i];
        const float hi = (float)m;
        q.mu_hi[p * d + i] = hi;
        q.mu_lo[p * d + i] = (float)(m - (double)hi);
    }
    if (i == 0) fail = 0;
    __syncthreads();
    double acc[FB], l[FB];

    // ---- Cholesky ----
    for (int J = 0; J < nb; ++J) {
        const int J0 = J * FB;
        if (ib > J) {
#pragma unroll
            for (int c = 0; c < FB; ++c) acc[c] = row[J0 + c] / q.nm1;
        } else if (ib == J) {
#pragma unroll
            for (int c = 0; c < FB; ++c) {
                double v = c <= r ? row[J0 + c] / q.nm1 : 0.0;
                if (c == r) v += q.eps;
                acc[c] = v;
            }
        }
        for (int K = 0; K < J; ++K) {
            for (int e = i; e < FB * FB; e += nt) B[e >> 5][e & 31] = A[(int64_t)(J0 + (e >> 5)) * d + K * FB + (e & 31)];
            __syncthreads();
            if (ib >= J) {
#pragma unroll
                for (int k = 0; k < FB; ++k) l[k] = row[K * FB + k];
                rank32(acc, l, B);
            }
            __syncthreads();
        }
        if (ib == J) {
#pragma unroll
            for (int c = 0; c < FB; ++c)
                if (c <= r) Dg[r][c] = acc[c];
        }
        __syncthreads();
        // the diagonal block, right-looking inside LDS: pivot, column, trailing update
        for (int j = 0; j < FB; ++j) {
            if (i == 0) {
                const double piv = Dg[j][j];
                if (piv > 0.0 && piv < __builtin_huge_val()) Dg[j][j] = sqrt(piv);
                else fail = J0 + j + 1;          // LAPACK's info: a status, the workgroup leaves the loop below
            }
            __syncthreads();
            if (fail) break;
            if (i > j && i < FB) Dg[i][j] /= Dg[j][j];
            __syncthreads();
            for (int e = i; e < FB * FB; e += nt) {
                const int rr = e >> 5, cc = e & 31;
                if (cc > j && rr >= cc) Dg[rr][cc] = fma(-Dg[rr][j], Dg[cc][j], Dg[rr][cc]);
            }
            __syncthreads();
        }
        if (fail) break;
        if (ib == J) {
#pragma unroll
            for (int c = 0; c < FB; ++c)
                if (c <= r) row[J0 + c] = Dg[r][c];
        } else if (ib > J) {
#pragma unroll
            for (int c = 0; c < FB; ++c) {
                double s = acc[c];
#pragma unroll
                for (int k = 0; k < c; ++k) s = fma(-acc[k], Dg[c][k], s);
                acc[c] = s / Dg[c][c];
                row[J0 + c] = acc[c];
            }
        }
        __syncthreads();
    }
    if (fail) {         // nothing a caller could take for a factor
        if (i == 0) q.info[p] = fail;
        const float nanf_ = __builtin_nanf("");
        const double nan_ = __builtin_nan("");
        for (int64_t e = i; e < dd; e += d) {
            q.w[p * dd + e] = nanf_;
            if (q.c_out) q.c_out[p * dd + e] = nan_;
            if (q.w64_out) q.w64_out[p * dd + e] = nan_;
        }
        return;
    }
    if (q.c_out) {
        for (int rr = 0; rr < d; ++rr) q.c_out[p * dd + (int64_t)rr * d + i] = i <= rr ? A[(int64_t)rr * d + i] : 0.0;
        __syncthreads();
    }

    // ---- W = C^-1 ----
    for (int J = 0; J < nb; ++J) {
        const int J0 = J * FB;
#pragma unroll
        for (int c = 0; c < FB; ++c) acc[c] = 0.0;
        for (int K = J; K < nb; ++K) {
            const int K0 = K * FB;
            if (ib == K) {
#pragma unroll
                for (int c = 0; c < FB; ++c) {
                    if (c <= r) Dg[r][c] = row[K0 + c];
                    Sb[r][c] = K == J ? (c == r ? 1.0 : 0.0) : acc[c];
                }
            }
            __syncthreads();
            if (i < FB) {       // column i of C[K][K]^-1 Sb
                double x[FB];
#pragma unroll
                for (int rr = 0; rr < FB; ++rr) {
                    double s = Sb[rr][i];
#pragma unroll
                    for (int qq = 0; qq < rr; ++qq) s = fma(-Dg[rr][qq], x[qq], s);
                    x[rr] = s / Dg[rr][rr];
                    B[i][rr] = x[rr];
                }
            }
            __syncthreads();
            if (ib == K) {
#pragma unroll
                for (int c = 0; c < FB; ++c)
                    if (K > J || c <= r) row[J0 + c] = B[c][r];
            } else if (ib > K) {
#pragma unroll
                for (int k = 0; k < FB; ++k) l[k] = row[K0 + k];
                rank32(acc, l, B);
            }
            __syncthreads();
        }
    }
    for (int rr = 0; rr < d; ++rr) {         // element (rr, i): coalesced, and only the lower triangle is read
        const int64_t e = (int64_t)rr * d + i;
        const bool low = i <= rr;
        const double v = low ? A[e] : 0.0;
        q.w[p * dd + e] = low ? (float)v : 0.f;
        if (q.w64_out) q.w64_out[p * dd + e] = v;
    }
    if (i == 0) q.info[p] = 0;
}

}  // namespace

// Per position p of the n_img images of x [n_img * P][D] (row n P + p), over the d columns sel[0..d): mean[p][k] and
// scatter[p][a][b] = sum_n (x[n][p][sel[a]] - mean[p][a]) (x[n][p][sel[b]] - mean[p][b]) in fp64.  Images are summed in ascending
// order, every scatter tile of the lower triangle is mirrored exactly: the same bits on every call.  sel lives on the device and
// every entry lies in [0, D) (the caller checks it).
extern "C" int ssad_position_gaussian_fit_stats(const float* x, const int* sel, int n_img, int64_t P, int D, int d, double* mean,
                                                double* scatter, void* stream) {
    SSAD_CHECK_ARG(x && sel && mean && scatter, "null pointer");
    SSAD_CHECK_ARG(padim_shape_ok(n_img, P, D, d), "need P >= 1, D % 4 == 0, d a multiple of 32 in 32..D");
    SSAD_CHECK_ARG(n_img >= 2, "a covariance needs at least 2 images");
    const int T = (d + SC_T - 1) / SC_T, tiles = T * (T + 1) / 2, cb = (d + 63) / 64;
    SSAD_CHECK_ARG(P * tiles < (int64_t)2147483647 && P * cb < (int64_t)2147483647, "too many positions for one launch");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(padim_mean_kernel, dim3((unsigned)(P * cb)), dim3(64), 0, st, x, sel, mean, n_img, P, D, d);
    hipLaunchKernelGGL(padim_scatter_kernel, dim3((unsigned)(P * tiles)), dim3(256), 0, st, x, sel, (const double*)mean, scatter,
                       n_img, P, D, d, tiles);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// Per position p: Sigma = scatter[p] / (n - 1) + eps I, C = its lower Cholesky factor, W = C^-1, all fp64 in place in the lower
// triangle of scatter[p] (consumed; the upper triangle is neither read nor written); w = fp32(W) with +0 above the diagonal, mu_hi /
// mu_lo the float pair of the mean, info[p] = 0 or 1 + the column of the first pivot that is not finite and positive (then w[p] is
// all NaN).  One workgroup of d threads per position, fixed summation order: the same bits on every call and for every P.
extern "C" int ssad_position_gaussian_factor(const double* mean, double* scatter, int64_t P, int d, int64_t n, double eps,
                                             float* mu_hi, float* mu_lo, float* w, double* c_out, double* w64_out, int* info,
                                             void* stream) {
    SSAD_CHECK_ARG(mean && scatter && mu_hi && mu_lo && w && info, "null pointer");
    SSAD_CHECK_ARG(d >= 32 && d % 32 == 0 && d <= FACTOR_MAX_D, "d must be a multiple of 32 in 32..512");
    SSAD_CHECK_ARG(P >= 1 && P < (int64_t)2147483647, "need 1 <= P < 2^31");
    SSAD_CHECK_ARG(n >= 2, "a covariance needs at least 2 images");
    SSAD_CHECK_ARG(eps > 0.0, "eps must be positive");
    SSAD_CHECK_ARG(((uintptr_t)mean | (uintptr_t)scatter | (uintptr_t)(c_out ? c_out : scatter) | (uintptr_t)(w64_out ? w64_out : scatter)) % 8 == 0, "fp64 buffers must be 8-byte aligned");
    FactorParams q{mean, scatter, mu_hi, mu_lo, w, c_out, w64_out, info, d, (double)(n - 1), eps};
    hipLaunchKernelGGL(position_factor_kernel, dim3((unsigned)P), dim3(d), 0, (hipStream_t)stream, q);
    SSAD_CHECK_LAUNCH();
    return 0;
}

// out[n P + p] = ||W_p (x[n][p][sel] - mu_p)||_2, mu_p = mu_hi[p] + mu_lo[p] (a float pair: (x - mu_hi) - mu_lo), W_p = w[p] [d][d]
// lower triangular (its upper triangle is never used: the kernel puts zeros in its place).  One workgroup scores 128 images of one position over all of W_p: no split
// over K or W rows across workgroups, so a score is the same bits whatever n_img and wherever its image sits in the launch.
extern "C" int ssad_position_mahalanobis(const float* x, const int* sel, const float* mu_hi, const float* mu_lo, const float* w,
                                         float* out, int n_img, int64_t P, int D, int d, void* stream) {
    SSAD_CHECK_ARG(x && sel && mu_hi && mu_lo && w && out, "null pointer");
    SSAD_CHECK_ARG(padim_shape_ok(n_img, P, D, d), "need n_img >= 1, P >= 1, D % 4 == 0, d a multiple of 32 in 32..D");
    SSAD_CHECK_ARG(d <= 1024, "d must be at most 1024");
    SSAD_CHECK_ARG(((uintptr_t)sel | (uintptr_t)mu_hi | (uintptr_t)mu_lo | (uintptr_t)w) % 16 == 0, "sel, mu_hi, mu_lo and w must be 16-byte aligned");
    // the kernel addresses the images of a tile through 32-bit byte offsets from the tile's first row
    SSAD_CHECK_ARG(P * D <= ((int64_t)1 << 31) / (4 * BQ) - D, "P * D too large for one launch");
    const int64_t img_tiles = cdiv64(n_img, BQ);
    SSAD_CHECK_ARG(P * img_tiles < (int64_t)2147483647, "too many positions for one launch");
    constexpr int lds_bytes = 2 * STAGE * 4;
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(position_mahalanobis_kernel, lds_bytes);
        attr_set = true;
    }
    PadimParams p{x, sel, mu_hi, mu_lo, w, out, n_img, P, D, d, (int)img_tiles};
    hipLaunchKernelGGL(position_mahalanobis_kernel, dim3((unsigned)(P * img_tiles)), dim3(NT), lds_bytes, (hipStream_t)stream, p);
    SSAD_CHECK_LAUNCH();
    return 0;
}
