// The 128 x 128 tile of the Euclidean k-NN kernels (knn_l2.hip, knn_gallery.hip, knn_ivf.hip; its selection, tail and result
// writers also serve knn_l2_half.hip and the index kernel of knn.hip).  Every piece stands here once, and the contract with it:
// the same tile, the same K order (the fp32 MFMA chain, 32 columns per step, ascending), the same summation order of the squared
// norms (sqnorm_wave) and the same expression d2 = fmaxf((qn + bn) - 2 dot, 0) -- hence the same bits for a (query, bank row)
// pair wherever the row stands in the bank, whichever tile it falls into and whoever shares that tile.  Selection is min / max
// only, so the three smallest do not depend on the visiting order either (lane halves, waves, splits).
#pragma once
#include "common.h"

namespace {

constexpr int BB = 128, BQ = 128, BK = 32, LDK = BK + 4, TB = 2, TQ = 2, NT = 256;      // bank rows x queries per workgroup tile
constexpr int STAGE = (BB + BQ) * LDK;  // floats
constexpr unsigned OOB = 0x80000000u;   // size given to the buffers: offsets from here on read zeros
constexpr int SRD3 = 0x00020000;        // raw buffer, 32-bit data format

typedef unsigned long long u64;
constexpr u64 NOKEY = ~0ull;

// ================================================ selection ================================================
// a <= b <= c are the three smallest so far; v joins them (no branches: min / max only)
__device__ __forceinline__ void keep3(float v, float& a, float& b, float& c) {
    c = fminf(c, fmaxf(b, v));
    b = fminf(b, fmaxf(a, v));
    a = fminf(a, v);
}
__device__ __forceinline__ u64 umin64(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a < b ? b : a; }
__device__ __forceinline__ void keep3(u64 v, u64& a, u64& b, u64& c) {
    c = umin64(c, umax64(b, v));
    b = umin64(b, umax64(a, v));
    a = umin64(a, v);
}
// 32-bit integer squared distances (knn_l2_int8.hip)
__device__ __forceinline__ void keep3(unsigned v, unsigned& a, unsigned& b, unsigned& c) {
    c = min(c, max(b, v));
    b = min(b, max(a, v));
    a = min(a, v);
}
__device__ __forceinline__ unsigned shfl_xor_any(unsigned v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ float shfl_xor_any(float v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ u64 shfl_xor_any(u64 v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    return ((u64)hi << 32) | lo;
}

// what is selected: squared distances, or (squared distance, row) keys
template <bool KEYS> struct Sel;
template <> struct Sel<false> {
    typedef float T;
    static __device__ __forceinline__ float none() { return INFINITY; }
    static __device__ __forceinline__ float make(float d2, int) { return d2; }
};
template <> struct Sel<true> {
    typedef u64 T;
    static __device__ __forceinline__ u64 none() { return NOKEY; }
    // d2 >= 0: its bits order like an unsigned integer, so the key's unsigned order is the lexicographic (d2, row) order
    static __device__ __forceinline__ u64 make(float d2, int row) { return ((u64)__float_as_uint(d2) << 32) | (unsigned)row; }
};

template <class T> __device__ __forceinline__ void put3(T* o, T a, T b, T c) { o[0] = a; o[1] = b; o[2] = c; }

// a thread's places in the tile
struct TileThread {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;     // lane (r, h) of the MFMA
    const int wb = wave >> 1, wq = wave & 1;    // 64-row bank block / 64-query block of this wave
    const int sc = tid & 7, sr = tid >> 3;      // staging: 16-byte chunk sc of rows sr + 32 i
};

// ================================================ norms ================================================
// sum x^2 of one row by one wave -- THE summation order of every squared norm: lane l takes elements l, l + 64, ... in an fma chain,
// then an xor butterfly (every lane ends with the sum).  tile_sqnorms runs the same chain for eight rows at once.
__device__ __forceinline__ float sqnorm_wave(const float* __restrict__ row, int D, int lane) {
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s = __builtin_fmaf(row[k], row[k], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// qn_s[s] = the squared norm of the row of query slot s, s = 0 .. BQ - 1, eight rows in flight per wave (one row at a time was a chain
// of 32 memory latencies per workgroup).  rowptr(s): that row; with MAY_BE_NULL it may be null (a slot past the end), which gives 0.
template <bool MAY_BE_NULL, class RowPtr>
__device__ __forceinline__ void tile_sqnorms(float* qn_s, int D, const TileThread& t, RowPtr rowptr) {
    for (int base = t.wave; base < BQ; base += 32) {
        float s[8];
        const float* q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            q[u] = rowptr(base + 4 * u);
            s[u] = 0.f;
        }
        for (int k = t.lane; k < D; k += 64) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = !MAY_BE_NULL || q[u] ? q[u][k] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u] = __builtin_fmaf(v[u], v[u], s[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float v = s[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (t.lane == 0) qn_s[base + 4 * u] = v;
        }
    }
}

// ================================================ the fp32 dot tile ================================================
// byte offsets of this thread's four staged chunks (rows sr + 32 i of a 128-row block that starts at row `first`); rows from `limit`
// on read zeros
template <class I>
__device__ __forceinline__ void stage_offsets(unsigned (&off)[4], I first, I limit, int D, const TileThread& t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) off[i] = first + t.sr + 32 * i < limit ? (unsigned)(((t.sr + 32 * i) * D + t.sc * 4) * 4) : OOB;
}
__device__ __forceinline__ f32x4 buffer_load16(const float* base, unsigned off) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)OOB, SRD3);
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}

// acc = the dots of the 128 bank rows at bblk (chunk offsets boff) with the tile's 128 queries over nks steps of 32 columns: stage 0
// is primed, then every step loads the next one ahead, reads LDS, runs the MFMA chain, stores and meets one barrier.  loadq(ks, i):
// chunk i of this thread's four query chunks of step ks.  side(): the caller's per-tile LDS side data (the bank rows' norms), written
// between the first barrier -- every wave has left the previous tile's last stage and side data -- and the first store.
template <class LoadQ, class Side>
__device__ __forceinline__ void dot_tile(f32x16 (&acc)[TB][TQ], float* lds, const TileThread& t, const float* bblk,
                                         const unsigned (&boff)[4], int nks, LoadQ loadq, Side side) {
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
            rq[i] = loadq(ks, i);
            rb[i] = buffer_load16(bblk + ks * BK, boff[i]);
        }
    };
    auto store = [&](float* st) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *(f32x4*)(st + (t.sr + 32 * i) * LDK + t.sc * 4) = rb[i];                   // bank rows: the tile's M side
            *(f32x4*)(st + BB * LDK + (t.sr + 32 * i) * LDK + t.sc * 4) = rq[i];        // queries: its N side
        }
    };
    __syncthreads();
    load(0);
    side();
    store(lds);
    __syncthreads();
    for (int ks = 0; ks < nks; ++ks) {
        const float* cur = lds + (ks & 1) * STAGE;
        if (ks + 1 < nks) load(ks + 1);
        const float* As = cur + (t.wb * 32 * TB + t.r) * LDK + t.h * 4;
        const float* Bs = cur + BB * LDK + (t.wq * 32 * TQ + t.r) * LDK + t.h * 4;
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
}

// ================================================ the tile epilogue ================================================
struct RowId {
    bool ok;    // the row exists (a row past its block's end read zeros and makes no candidate)
    int id;     // the number it goes by in the result
};

// The finished tile joins the running three smallest of this lane's queries (column r of its TQ query blocks): register e = 4 g + c
// of lane (r, h) in block (i, j) is tile row l + c, l = (wb TB + i) 32 + 4 h + 8 g, of query column r.  rowof(l, c): that row's
// RowId (l is a multiple of 4: side data of rows l .. l + 3 can be read as one vector).
template <bool KEYS, class RowOf>
__device__ __forceinline__ void tile_select(const f32x16 (&acc)[TB][TQ], const float* qn_s, const float* bn_s, const TileThread& t,
                                            typename Sel<KEYS>::T (&best)[TQ][3], RowOf rowof) {
    float qn[TQ];
#pragma unroll
    for (int j = 0; j < TQ; ++j) qn[j] = qn_s[(t.wq * TQ + j) * 32 + t.r];
#pragma unroll
    for (int i = 0; i < TB; ++i) {
        const int l0 = (t.wb * TB + i) * 32 + 4 * t.h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 bn = *(const f32x4*)(bn_s + l0 + 8 * g);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const RowId row = rowof(l0 + 8 * g, c);
#pragma unroll
                for (int j = 0; j < TQ; ++j) {
                    const float d2 = fmaxf((qn[j] + bn[c]) - 2.f * acc[i][j][4 * g + c], 0.f);
                    keep3(row.ok ? Sel<KEYS>::make(d2, row.id) : Sel<KEYS>::none(), best[j][0], best[j][1], best[j][2]);
                }
            }
        }
    }
}

// ================================================ the tail ================================================
// A query's candidates sit in the two lane halves of two waves (wb = 0, 1): halves by shuffle, waves through LDS (the stages are
// dead after the first barrier).  emit(slot, a, b, c): the three smallest of query slot `slot` of the tile, once per slot.
template <class T, class Emit>
__device__ __forceinline__ void tile_tail(T (&best)[TQ][3], void* lds, const TileThread& t, Emit emit) {
    __syncthreads();
    T* M = (T*)lds;                             // [2 wq][TQ][32][3]
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
        const T oa = shfl_xor_any(best[j][0], 32), ob = shfl_xor_any(best[j][1], 32), oc = shfl_xor_any(best[j][2], 32);
        keep3(oa, best[j][0], best[j][1], best[j][2]);
        keep3(ob, best[j][0], best[j][1], best[j][2]);
        keep3(oc, best[j][0], best[j][1], best[j][2]);
        if (t.wb == 1 && t.h == 0) put3(M + ((t.wq * TQ + j) * 32 + t.r) * 3, best[j][0], best[j][1], best[j][2]);
    }
    __syncthreads();
    if (t.wb == 0 && t.h == 0) {
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const int slot = (t.wq * TQ + j) * 32 + t.r;
            const T* m = M + slot * 3;
            T a = best[j][0], b = best[j][1], c = best[j][2];
            keep3(m[0], a, b, c);
            keep3(m[1], a, b, c);
            keep3(m[2], a, b, c);
            emit(slot, a, b, c);
        }
    }
}

// ================================================ results and the merge of splits ================================================
// The k winners of query `row` (p: a kernel's parameters, with k and out or dist / idx): the mean of their roots, smallest first, or
// the (root, row) pairs.  MAY_MISS: fewer than k rows may have been met -- the mean is then +inf by itself, a missing pair is
// (+inf, -1); without it every key is a real one (k <= bank rows: the host checks).
template <bool MAY_MISS = false, class P>
__device__ __forceinline__ void write_result(const P& p, int64_t row, float a, float b, float c) {
    float s = sqrtf(a);
    if (p.k > 1) s += sqrtf(b);
    if (p.k > 2) s += sqrtf(c);
    p.out[row] = s / (float)p.k;
}
template <bool MAY_MISS = false, class P>
__device__ __forceinline__ void write_result(const P& p, int64_t row, u64 a, u64 b, u64 c) {
    const u64 key[3] = {a, b, c};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < p.k) {
            const bool have = !MAY_MISS || key[j] != NOKEY;
            p.dist[row * p.k + j] = have ? sqrtf(__uint_as_float((unsigned)(key[j] >> 32))) : INFINITY;
            p.idx[row * p.k + j] = have ? (int)(unsigned)key[j] : -1;
        }
    }
}

// the three smallest of the S triples part[s][n][0 .. 2] of query n among N (min / max selection: any order gives the same three)
template <class T>
__device__ __forceinline__ void merge_splits(const T* part, int S, int64_t N, int64_t n, T& a, T& b, T& c) {
    for (int s = 0; s < S; ++s) {
        const T* t = part + ((int64_t)s * N + n) * 3;
        keep3(t[0], a, b, c);
        keep3(t[1], a, b, c);
        keep3(t[2], a, b, c);
    }
}

// ================================================ the k smallest keys, k = 4 .. 32 (knn_topk.hip) ================================================
// L[0] < L[1] < ... < L[CAP - 1] are the CAP smallest keys so far (NOKEY where fewer were met); v joins them.  Keys are unique (one
// per bank row), so the CAP smallest of a set do not depend on the order in which its members arrive.  Branch-free, indices known at
// compile time (the list stays in registers): slot i takes its lower neighbour when v goes below that, else the smaller of itself and
// v.  A v that is not below L[CAP - 1] -- NOKEY never is -- changes nothing.
template <int CAP>
__device__ __forceinline__ void topk_insert(u64 (&L)[CAP], u64 v) {
#pragma unroll
    for (int i = CAP - 1; i > 0; --i) L[i] = v < L[i - 1] ? L[i - 1] : umin64(L[i], v);
    L[0] = umin64(L[0], v);
}

// the ascending keys src[0], src[stride], ... (count of them) join L; a wave stops at the first key that no lane can use
template <int CAP>
__device__ __forceinline__ void topk_merge(u64 (&L)[CAP], const u64* src, int stride, int count) {
#pragma unroll 1
    for (int i = 0; i < count; ++i) {
        const u64 v = src[(int64_t)i * stride];
        if (!__any(v < L[CAP - 1])) break;
        topk_insert(L, v);
    }
}

// tile_select for a list: the finished tile joins the CAP smallest keys of this lane's queries.  d2 is tile_select's expression on the
// same accumulators, so a (query, bank row) pair has the bits the k <= 3 kernels give it.  A candidate passes when its key is below
// the list's last entry as the tile begins (a bit of `mask`); after the first tiles almost none does, and a wave runs the insertion
// network once per round for the lowest passing candidate of every lane -- as many rounds as its busiest lane has candidates.
template <int CAP, class RowOf>
__device__ __forceinline__ void tile_select_topk(const f32x16 (&acc)[TB][TQ], const float* qn_s, const float* bn_s, const TileThread& t,
                                                 u64 (&L)[TQ][CAP], RowOf rowof) {
    static_assert(TB * 16 == 32, "a candidate mask is 32 bits");
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
        const float qn = qn_s[(t.wq * TQ + j) * 32 + t.r];
        const u64 worst = L[j][CAP - 1];
        float d[TB * 16];
        unsigned mask = 0;
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const int l0 = (t.wb * TB + i) * 32 + 4 * t.h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bn = *(const f32x4*)(bn_s + l0 + 8 * g);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const RowId row = rowof(l0 + 8 * g, c);
                    const float d2 = fmaxf((qn + bn[c]) - 2.f * acc[i][j][4 * g + c], 0.f);
                    d[i * 16 + 4 * g + c] = d2;
                    if (row.ok && Sel<true>::make(d2, row.id) < worst) mask |= 1u << (i * 16 + 4 * g + c);
                }
            }
        }
        while (__any(mask != 0)) {
            const int e = mask ? __builtin_ctz(mask) : 0;       // candidate e = 16 i + 4 g + c
            float d2 = d[0];
#pragma unroll
            for (int q = 1; q < TB * 16; ++q) d2 = e == q ? d[q] : d2;
            const RowId row = rowof((t.wb * TB + (e >> 4)) * 32 + 4 * t.h + 8 * ((e >> 2) & 3), e & 3);
            topk_insert(L[j], mask ? Sel<true>::make(d2, row.id) : NOKEY);
            mask &= mask - 1;
        }
    }
}

// tile_tail for lists: lane halves, then waves, through LDS (the stages are dead; 2 x 128 x CAP keys, key i of slot s at [i][s]).
// emit(slot, j): L[j] holds the CAP smallest keys of query slot `slot` of the tile, once per slot.
template <int CAP, class Emit>
__device__ __forceinline__ void tile_tail_topk(u64 (&L)[TQ][CAP], void* lds, const TileThread& t, Emit emit) {
    static_assert(2 * CAP * BQ * 8 <= 2 * STAGE * 4, "the lists of two waves fit into the stages");
    u64* M = (u64*)lds;                         // [2 wb][CAP][BQ]
    __syncthreads();
    if (t.h == 1) {
#pragma unroll
        for (int j = 0; j < TQ; ++j)
#pragma unroll
            for (int i = 0; i < CAP; ++i) M[(t.wb * CAP + i) * BQ + (t.wq * TQ + j) * 32 + t.r] = L[j][i];
    }
    __syncthreads();
    if (t.h == 0) {
#pragma unroll
        for (int j = 0; j < TQ; ++j) topk_merge(L[j], M + t.wb * CAP * BQ + (t.wq * TQ + j) * 32 + t.r, BQ, CAP);
    }
    __syncthreads();
    if (t.wb == 1 && t.h == 0) {
#pragma unroll
        for (int j = 0; j < TQ; ++j)
#pragma unroll
            for (int i = 0; i < CAP; ++i) M[i * BQ + (t.wq * TQ + j) * 32 + t.r] = L[j][i];
    }
    __syncthreads();
    if (t.wb == 0 && t.h == 0) {
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const int slot = (t.wq * TQ + j) * 32 + t.r;
            topk_merge(L[j], M + slot, BQ, CAP);
            emit(slot, j);
        }
    }
}

}  // namespace
