// An inverted-file (IVF-Flat) index for the Euclidean kNN detector (PatchCore's approximate search, faiss' IndexIVFFlat; opt-in
// beside the whole-bank search of knn_l2.hip): the bank rows are clustered into nlist cells, stored cell after cell, and a query
// meets the rows of its nprobe nearest cells only.
//   ssad_segment_means    k-means' update step: the mean of the rows of every cell, ssad_group_means for groups of any length;
//   ssad_l2_knn_ivf       the search: knn_l2.hip's search with an INDIRECT query side -- a workgroup takes one cell and up to 128 of
//   / _index              the (query, probe slot) pairs that name it, gathers those queries by row while staging, walks the cell's
//                         rows and leaves every pair's three best (squared-distance bits << 32 | original bank row) keys; a second
//                         kernel merges the nprobe triples of a query, takes the roots and writes the mean or (dist, idx).
// The search kernel keeps the tile's norm prologue, K loop, epilogue and tail written out in place -- built on the shared functions
// (dot_tile, tile_select, tile_tail) it measured 1.3-1.9 % slower than this form, beyond the run-to-run spread -- on knn_tile.h's
// constants and selection.  The text follows the header's functions line for line: the same tile, K order, norm order and d2
// expression, so a (query, bank row) pair gets the bits l2_knn_kernel gives it, whichever tile it falls into.
#include "knn_tile.h"

namespace {

constexpr int LDS_BYTES = (2 * STAGE + BQ + BB + BB + 2 * BQ) * 4;      // stages, norms, the tile's original rows, pair ids and query rows
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ================================================ k-means' update step ================================================

// grid (ceil(D / 64), nlist): thread c of workgroup (., g) sums column c of the rows order[offsets[g] .. offsets[g + 1] - 1] in fp64,
// in that sequence (eight loads in flight, added in order), and rounds once.  An empty segment writes nothing: its output row keeps
// what the caller put there.  Segment bounds are clamped to 0 .. N and an entry of `order` outside 0 .. N - 1 is left out, so nothing
// is addressed with a value that was not checked.
__global__ __launch_bounds__(64) void segment_means_kernel(const float* __restrict__ x, const int* __restrict__ order,
                                                           const int* __restrict__ offsets, float* __restrict__ out, int64_t N, int D) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= D) return;
    const int64_t lo = offsets[blockIdx.y], hi = offsets[blockIdx.y + 1];
    const int64_t s0 = lo < 0 ? 0 : (lo > N ? N : lo);
    const int64_t s1 = hi < s0 ? s0 : (hi > N ? N : hi);
    const float* col = x + c;
    double s = 0.0;
    int64_t cnt = 0;
    int64_t i = s0;
    for (; i + 8 <= s1; i += 8) {
        float v[8];
        int r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = order[i + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (unsigned)r[u] < (uint64_t)N ? col[(int64_t)r[u] * D] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            s += (double)v[u];
            cnt += (unsigned)r[u] < (uint64_t)N;
        }
    }
    for (; i < s1; ++i) {
        const int r = order[i];
        if ((unsigned)r < (uint64_t)N) {
            s += (double)col[(int64_t)r * D];
            ++cnt;
        }
    }
    if (cnt > 0) out[(int64_t)blockIdx.y * D + c] = (float)(s / (double)cnt);
}

// ================================================ the search ================================================

struct IvfParams {
    const float* x;       // [N][D] queries
    const float* bank;    // [R][D] bank rows sorted by cell (not normalised)
    const float* bsq;     // [R] squared norms of those rows (ssad_row_sqnorms)
    const int* offsets;   // [nlist + 1] cell c holds the sorted rows offsets[c] .. offsets[c + 1] - 1
    const int* perm;      // [R] original bank row of every sorted row
    const int* probes;    // [N][nprobe] cells of every query; an entry outside 0 .. nlist - 1 is skipped
    const int* tiles;     // [3][G] cell, first pair and pairs (1 .. 128) of every tile; a cell outside 0 .. nlist - 1: a surplus tile
    const int* pairs;     // [N nprobe] pair ids n nprobe + j, sorted by cell
    u64* part;            // [N nprobe][3] keys of every pair, ascending
    float* out;           // [N] mean form
    float* dist;          // [N][k] index form
    int* idx;             // [N][k] index form
    int64_t N;
    int D, R, nlist, nprobe, G, k;
};

// Grid (G): workgroup t takes tile t of the work list -- cell tiles[0][t] and the pairs pairs[first .. first + cnt), all of which name
// that cell -- and scores their queries against the cell's rows [offsets[cell], offsets[cell + 1]) in 128-row tiles; rows past the
// cell's end are masked (they read zeros and make no candidate), never taken from the next cell.  Slots past cnt stage query row 0 and
// are never written.  Everything a value read from device memory addresses is checked first: the cell, the pair range, the pair ids
// and the cell's bounds.  The tile is knn_tile.h's, written out in place (see the head of this file); the queries are staged with
// plain 16-byte loads (a row of x is anywhere in a buffer that may exceed the 2 GB an offset of a buffer load reaches).
__global__ __launch_bounds__(NT, 2) void l2_knn_ivf_kernel(IvfParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* qn_s = lds + 2 * STAGE;              // [BQ] squared norms of the queries
    float* bn_s = qn_s + BQ;                    // [BB] squared norms of the current bank tile
    int* pm_s = (int*)(bn_s + BB);              // [BB] original rows of the current bank tile
    int* pid_s = pm_s + BB;                     // [BQ] pair id of every query slot, -1: none
    int* row_s = pid_s + BQ;                    // [BQ] query row of every slot (0 for an empty one)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wb = wave >> 1, wq = wave & 1;    // 64-row bank block / 64-query block of this wave
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc of rows sr + 32 i

    const int cell = p.tiles[blockIdx.x];
    if ((unsigned)cell >= (unsigned)p.nlist) return;            // a surplus tile of the upper-bound grid (the whole workgroup)
    const int first = p.tiles[p.G + blockIdx.x], cnt = p.tiles[2 * p.G + blockIdx.x];
    const int64_t NP = p.N * p.nprobe;
    if (tid < BQ) {
        int pid = -1;
        if (tid < cnt && first >= 0 && (int64_t)first + tid < NP) {
            pid = p.pairs[first + tid];
            if ((uint64_t)(int64_t)pid >= (uint64_t)NP) pid = -1;
        }
        pid_s[tid] = pid;
        row_s[tid] = pid < 0 ? 0 : pid / p.nprobe;
    }
    __syncthreads();
    const int c0 = p.offsets[cell], c1 = p.offsets[cell + 1];
    const int b_begin = c0 < 0 ? 0 : (c0 > p.R ? p.R : c0);
    const int b_end = c1 < b_begin ? b_begin : (c1 > p.R ? p.R : c1);

    // ---- squared query norms: sqnorm_wave's order (knn_l2.hip), eight rows in flight per wave ----
    for (int base = wave; base < BQ; base += 32) {
        float s[8];
        const float* q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            q[u] = p.x + (int64_t)row_s[base + 4 * u] * p.D;
            s[u] = 0.f;
        }
        for (int k = lane; k < p.D; k += 64) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = q[u][k];
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u] = __builtin_fmaf(v[u], v[u], s[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float t = s[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == 0) qn_s[base + 4 * u] = t;
        }
    }
    const float* qptr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qptr[i] = p.x + (int64_t)row_s[sr + 32 * i] * p.D + sc * 4;

    // running three smallest of this lane's queries (column r of its TQ query blocks) over the bank rows it has seen
    u64 best[TQ][3];
#pragma unroll
    for (int j = 0; j < TQ; ++j) best[j][0] = best[j][1] = best[j][2] = NOKEY;
    const int nks = p.D / BK;

    for (int n0 = b_begin; n0 < b_end; n0 += BB) {
        unsigned boff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) boff[i] = n0 + sr + 32 * i < b_end ? (unsigned)(((sr + 32 * i) * p.D + sc * 4) * 4) : OOB;
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
            const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(bblk + ks * BK), 0, (int)OOB, SRD3);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                rq[i] = *(const f32x4*)(qptr[i] + ks * BK);
                rb[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, boff[i], 0, 0));
            }
        };
        auto store = [&](float* st) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *(f32x4*)(st + (sr + 32 * i) * LDK + sc * 4) = rb[i];                   // bank rows: the tile's M side
                *(f32x4*)(st + BB * LDK + (sr + 32 * i) * LDK + sc * 4) = rq[i];        // queries: its N side
            }
        };
        __syncthreads();                        // every wave has left the previous bank tile's last stage, its norms and its rows
        load(0);
        if (tid < BB) {
            const bool in = n0 + tid < b_end;
            bn_s[tid] = in ? p.bsq[n0 + tid] : 0.f;
            pm_s[tid] = in ? p.perm[n0 + tid] : -1;
        }
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
        // ---- the finished tile: register e of lane (r, h) in block (i, j) is row l0 + (e & 3) + 8 (e >> 2) of the tile, query column r ----
        float qn[TQ];
#pragma unroll
        for (int j = 0; j < TQ; ++j) qn[j] = qn_s[(wq * TQ + j) * 32 + r];
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const int l0 = (wb * TB + i) * 32 + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bn = *(const f32x4*)(bn_s + l0 + 8 * g);
                const i32x4 pm = *(const i32x4*)(pm_s + l0 + 8 * g);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int e = 4 * g + c;
                    const bool ok = n0 + l0 + c + 8 * g < b_end;
                    const int row = pm[c];                      // the caller's row number
#pragma unroll
                    for (int j = 0; j < TQ; ++j) {
                        const float d2 = fmaxf((qn[j] + bn[c]) - 2.f * acc[i][j][e], 0.f);
                        keep3(ok ? Sel<true>::make(d2, row) : NOKEY, best[j][0], best[j][1], best[j][2]);
                    }
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
            const int slot = (wq * TQ + j) * 32 + r;
            const u64* m = M + slot * 3;
            u64 a = best[j][0], b = best[j][1], c = best[j][2];
            keep3(m[0], a, b, c);
            keep3(m[1], a, b, c);
            keep3(m[2], a, b, c);
            const int pid = pid_s[slot];
            if (pid >= 0) {
                u64* o = p.part + (int64_t)pid * 3;
                o[0] = a; o[1] = b; o[2] = c;
            }
        }
    }
}

// The three smallest keys of the nprobe triples of query n (min / max selection: any order of the slots gives the same three; a key
// met twice -- a cell named twice -- counts once), then the roots: the mean, added smallest first (+inf when fewer than k rows were
// met), or the (root, original row) pairs, a missing one (+inf, -1).  A slot whose probe entry is no cell was never written and is
// never read.
__global__ void l2_knn_ivf_merge_kernel(IvfParams p) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= p.N) return;
    u64 key[3] = {NOKEY, NOKEY, NOKEY};
    for (int j = 0; j < p.nprobe; ++j) {
        const int64_t pid = n * p.nprobe + j;
        if ((unsigned)p.probes[pid] >= (unsigned)p.nlist) continue;
        const u64* t = p.part + pid * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const u64 v = t[e];
            if (v != key[0] && v != key[1] && v != key[2]) keep3(v, key[0], key[1], key[2]);
        }
    }
    float d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) d[j] = key[j] != NOKEY ? sqrtf(__uint_as_float((unsigned)(key[j] >> 32))) : INFINITY;
    if (p.out) {
        float s = d[0];
        if (p.k > 1) s += d[1];
        if (p.k > 2) s += d[2];
        p.out[n] = s / (float)p.k;
        return;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < p.k) {
            p.dist[n * p.k + j] = d[j];
            p.idx[n * p.k + j] = key[j] != NOKEY ? (int)(unsigned)key[j] : -1;
        }
    }
}

static int l2_knn_ivf_launch(IvfParams p, void* stream) {
    static bool attr_set = false;
    if (!attr_set) {
        SSAD_SET_DYN_LDS(l2_knn_ivf_kernel, LDS_BYTES);
        attr_set = true;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(l2_knn_ivf_kernel, dim3((unsigned)p.G), dim3(NT), LDS_BYTES, st, p);
    SSAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(l2_knn_ivf_merge_kernel, dim3((unsigned)cdiv64(p.N, 256)), dim3(256), 0, st, p);
    SSAD_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// out[g][c] = the mean of x[order[i]][c], i = offsets[g] .. offsets[g + 1] - 1: k-means' update step over rows sorted by cell.
// fp64 sum in `order`'s sequence, one rounding to fp32, no atomics: the same bits on every call.  An empty segment leaves out[g]
// as it is (the caller passes the previous centroids).
extern "C" int ssad_segment_means(const float* x, const int* order, const int* offsets, float* out, int64_t N, int nlist, int D,
                                  void* stream) {
    SSAD_CHECK_ARG(x && order && offsets && out && N > 0 && nlist > 0 && D > 0, "bad argument");
    SSAD_CHECK_ARG(N <= (int64_t)2147483647 && nlist <= 65535, "at most 2^31 - 1 rows and 65535 segments");
    hipLaunchKernelGGL(segment_means_kernel, dim3((unsigned)cdiv64(D, 64), (unsigned)nlist), dim3(64), 0, (hipStream_t)stream, x, order,
                       offsets, out, N, D);
    SSAD_CHECK_LAUNCH();
    return 0;
}

#define SSAD_L2_KNN_IVF_CHECKS()                                                                                            \
    SSAD_CHECK_ARG(x && bank && bank_sq && offsets && perm && probes && tiles && pairs && part, "bad argument");            \
    SSAD_CHECK_ARG(N > 0 && R > 0 && nlist > 0 && nprobe > 0 && G > 0, "N, R, nlist, nprobe and G >= 1");                   \
    SSAD_CHECK_ARG(D > 0 && D % BK == 0 && D <= 65536, "D must be a multiple of 32, at most 65536");                        \
    SSAD_CHECK_ARG(N <= (int64_t)2147483647 && N * nprobe <= (int64_t)2147483647, "too many (query, probe) pairs for one launch");                  \
    SSAD_CHECK_ARG(k >= 1 && k <= 3, "k in 1..3");                                                                          \
    SSAD_CHECK_ARG(((uintptr_t)x & 15) == 0, "x must be 16-byte aligned");                                                  \
    SSAD_CHECK_ARG(((uintptr_t)part & 7) == 0, "part must be 8-byte aligned")

// ssad_l2_knn_fused over an inverted file: out[n] = the mean of the roots of the k smallest d2 among the rows of the cells
// probes[n][0 .. nprobe - 1], +inf where those cells hold fewer than k rows.
extern "C" int ssad_l2_knn_ivf(const float* x, const float* bank, const float* bank_sq, const int* offsets, const int* perm,
                               const int* probes, const int* tiles, const int* pairs, void* part, float* out, int64_t N, int D, int R,
                               int nlist, int nprobe, int G, int k, void* stream) {
    SSAD_L2_KNN_IVF_CHECKS();
    SSAD_CHECK_ARG(out, "bad argument");
    return l2_knn_ivf_launch(IvfParams{x, bank, bank_sq, offsets, perm, probes, tiles, pairs, (u64*)part, out, nullptr, nullptr, N, D, R,
                                       nlist, nprobe, G, k}, stream);
}

// ssad_l2_knn_index over the same cells: dist / idx [N][k], idx the ORIGINAL bank row (perm), equal d2 to the smaller original row;
// slots the probed cells cannot fill hold (+inf, -1).  dist holds the bits ssad_l2_knn_ivf averages.
extern "C" int ssad_l2_knn_ivf_index(const float* x, const float* bank, const float* bank_sq, const int* offsets, const int* perm,
                                     const int* probes, const int* tiles, const int* pairs, void* part, float* dist, int* idx, int64_t N,
                                     int D, int R, int nlist, int nprobe, int G, int k, void* stream) {
    SSAD_L2_KNN_IVF_CHECKS();
    SSAD_CHECK_ARG(dist && idx, "bad argument");
    return l2_knn_ivf_launch(IvfParams{x, bank, bank_sq, offsets, perm, probes, tiles, pairs, (u64*)part, nullptr, dist, idx, N, D, R,
                                       nlist, nprobe, G, k}, stream);
}
