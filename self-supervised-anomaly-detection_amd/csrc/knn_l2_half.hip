// Euclidean k-NN scoring with HALF-PRECISION OPERANDS (opt-in beside knn_l2.hip; faiss' GpuIndexFlat useFloat16): queries and bank rows
// are rounded once to fp16 by h (ssad_rows_to_half), the distance is that of the ROUNDED rows,
//   d = sqrt(max(|h(q)|^2 + |h(b)|^2 - 2 <h(q), h(b)>, 0)),
//   <h(q), h(b)>     v_mfma_f32_32x32x16_f16 chains: fp16 products, fp32 accumulation, K in ascending order, 16 per instruction,
//   |h(q)|^2, ...    the rounded rows' squared norms in sqnorm_wave's order (knn_l2.hip), written by the pass that rounds the rows,
//   d2               fmaxf((qn + bn) - 2 dot, 0) in the per-tile epilogue.
// h: fp32 -> fp16 round to nearest even, saturating at +-65504, results below 2^-14 in magnitude flushed to signed zero -- no half
// ever holds inf, NaN or a subnormal.  Selection, tie rule, keys, split and merge are l2_knn_kernel's.  The matrix loop holds no
// conversion and no norm prologue: both operands arrive as halves, both norm vectors as floats.
#include "knn_tile.h"

namespace {

// knn_tile.h's tile (BB x BQ, four waves of 2 x 2 accumulators) with a K step of its own
constexpr int HK = 64, HLDK = HK + 8;           // halves per K step; 144-byte rows: the 16 rows of a ds_read_b128 lane group fall on 16
constexpr int HSTAGE = (BB + BQ) * HLDK;        // distinct 16-byte slots of the 256-byte bank row (36 r mod 64 runs over the multiples of 4)
constexpr int LDS_BYTES = 2 * HSTAGE * 2 + (BQ + BB) * 4;

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
    float* qn_s = (float*)(lds + 2 * HSTAGE);   // [BQ] squared norms of the queries
    float* bn_s = qn_s + BQ;                    // [BB] squared norms of the current bank tile
    const TileThread t{};                       // staging: 16-byte chunk sc is 8 halves
    const int64_t m0 = (int64_t)blockIdx.x * BQ;

    if (t.tid < BQ) qn_s[t.tid] = m0 + t.tid < p.N ? p.xsq[m0 + t.tid] : 0.f;
    unsigned qoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qoff[i] = m0 + t.sr + 32 * i < p.N ? (unsigned)(((t.sr + 32 * i) * p.D + t.sc * 8) * 2) : OOB;
    const hf* xblk = p.x + m0 * p.D;

    T best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = Sel<KEYS>::none();
    const int nks = (p.D + HK - 1) / HK;
    const int64_t r_begin = (int64_t)blockIdx.y * p.rows_per;
    const int r_end = (int)(r_begin + p.rows_per < p.R ? r_begin + p.rows_per : p.R);

    for (int n0 = (int)(r_begin < p.R ? r_begin : p.R); n0 < r_end; n0 += BB) {
        unsigned boff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) boff[i] = n0 + t.sr + 32 * i < p.R ? (unsigned)(((t.sr + 32 * i) * p.D + t.sc * 8) * 2) : OOB;
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
        store(lds);
        __syncthreads();
        for (int ks = 0; ks < nks; ++ks) {
            const hf* cur = lds + (ks & 1) * HSTAGE;
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
            if (ks + 1 < nks) store(lds + ((ks + 1) & 1) * HSTAGE);
            __syncthreads();
        }
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
__global__ void l2h_knn_merge_kernel(L2hParams p, int S) {
    typedef typename Sel<KEYS>::T T;
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= p.N) return;
    T a = Sel<KEYS>::none(), b = a, c = a;
    merge_splits((const T*)p.part, S, p.N, n, a, b, c);
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

// KEYS: part holds 64-bit keys (the index form), else floats
#define SSAD_L2H_KNN_CHECKS(KEYS)                                                                               \
    SSAD_CHECK_ARG(D % 32 == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");                     \
    SSAD_CHECK_ARG(k >= 1 && k <= 3 && k <= R, "k in 1..3 and <= bank rows");                                   \
    SSAD_CHECK_ARG((((uintptr_t)xh | (uintptr_t)bankh) & 15) == 0, "half rows must be 16-byte aligned");        \
    SSAD_CHECK_ARG(S >= 1 && S <= 65535 && (S == 1 || part), "S in 1..65535, with a workspace when S > 1");     \
    SSAD_CHECK_ARG(!(KEYS) || ((uintptr_t)part & 7) == 0, "part must be 8-byte aligned");                       \
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

// ssad_l2_knn_fused on rounded rows: xh / bankh halves, x_sq / bank_sq their squared norms (ssad_rows_to_half).  part [S][N][3] floats
// (caller-owned) when S > 1, merged by a second launch; the same bits for every S.
extern "C" int ssad_l2h_knn_fused(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, float* part, float* out,
                                  int64_t N, int D, int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(xh && x_sq && bankh && bank_sq && out && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2H_KNN_CHECKS(false);
    return l2h_knn_launch<false>(L2hParams{(const hf*)xh, x_sq, (const hf*)bankh, bank_sq, part, out, nullptr, nullptr, N, D, R, 0, k}, S,
                                 stream);
}

// kneighbors on rounded rows: the k smallest (d2, bank row) pairs, dist = sqrt(d2) -- the bits ssad_l2h_knn_fused averages.  part
// [S][N][3] 64-bit keys (caller-owned, 8-byte aligned) when S > 1; the same bits for every S.
extern "C" int ssad_l2h_knn_index(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, void* part, float* dist,
                                  int* idx, int64_t N, int D, int R, int k, int S, void* stream) {
    SSAD_CHECK_ARG(xh && x_sq && bankh && bank_sq && dist && idx && N > 0 && D > 0 && R > 0, "bad argument");
    SSAD_L2H_KNN_CHECKS(true);
    return l2h_knn_launch<true>(L2hParams{(const hf*)xh, x_sq, (const hf*)bankh, bank_sq, part, nullptr, dist, idx, N, D, R, 0, k}, S,
                                stream);
}
