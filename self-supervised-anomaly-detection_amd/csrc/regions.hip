// Defect regions on the device: connected-component labelling of a batch of binary images, per-region statistics, a region filter
// and the two weight planes of the PRO curve.  Everything here is integers and min / max: every output is decided by the mask
// (and the scores) alone, bit for bit the same on every call, whatever order the atomics land in.
//
// Labelling is a union-find over pixel indices, not a sweep to a fixed point: the work does not grow with the length of a
// component's path (csrc/objmask.hip's om_largest_kernel needs O(path) sweeps; it serves its once-per-category job and is not
// used here).  While the kernels work, a label is the raster index (y * W + x, within its image) of a pixel of the same component,
// -1 on background.  Seven launches (the scan runs twice), each a grid-wide ordering point:
//   1. rg_local_kernel    one workgroup per RG_T x RG_T tile: row runs from a wave ballot, then unions with the row above inside
//                         the tile, in LDS; every pixel is written with the smallest raster index of its piece of the tile
//   2. rg_merge_kernel    pixels on the first row / column of a tile union with their neighbours in the tile above / to the left
//                         (atomic minimum on the global label plane)
//   3. rg_flatten_kernel  every pixel follows its chain to the root; roots (label == own index) are counted per 1024-pixel chunk
//   4. rg_scan_kernel     exclusive scan of the chunk counts per image (-> counts), then of counts over the batch (-> offsets)
//   5. rg_rank_kernel     a root's rank = roots before it in raster order + 1: scipy.ndimage.label's numbering
//   6. rg_final_kernel    label = rank of the root, 0 on background
//
// TERMINATION (these loops must end on their own: nothing else would end them).
//   Invariant: every value ever stored at index i of a label plane is the index of a pixel of i's component and is <= i.  It holds
//   after initialisation (a run's first pixel), and the only later writes are atomic minima with the index of a pixel that is
//   connected to i and smaller, and stores of a root found by following the plane from i.
//   * rg_find follows a = label[a] while label[a] != a.  By the invariant each step strictly decreases a, whatever other threads
//     write in the meantime (a stale or a fresh value are both < a), so it ends within H * W steps.
//   * rg_union retries with (old, b) after an atomic minimum at a returned old != a.  Both are smaller than a = max(a, b), so the
//     larger index of the pair strictly decreases: at most H * W retries.
//   * No loop waits for another thread's or workgroup's progress: no flag is polled, there is no grid barrier; where a grid-wide
//     order is needed, a new kernel is launched.  The scan loops run over a count fixed at launch.
#include "common.h"

#include <limits.h>

namespace {

constexpr int RG_T = 32;                    // tile side of rg_local_kernel: a row of a tile is half a wave
constexpr int RG_TT = RG_T * RG_T;          // threads of a tile's workgroup, one per pixel
constexpr int RG_CHUNK = 1024;              // consecutive pixels of one image that a workgroup of the scan-side kernels takes

// SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP for a plane in LDS, __HIP_MEMORY_SCOPE_AGENT for the global plane
template <int SCOPE> __device__ __forceinline__ int rg_load(const int* L, int a) { return __hip_atomic_load(L + a, __ATOMIC_RELAXED, SCOPE); }

template <int SCOPE> __device__ __forceinline__ int rg_find(const int* L, int a) {
    for (;;) {
        const int v = rg_load<SCOPE>(L, a);
        if (v >= a) return a;               // v == a: a root (v > a cannot happen; written so that the loop can only descend)
        a = v;
    }
}

template <int SCOPE> __device__ __forceinline__ void rg_union(int* L, int a, int b) {
    a = rg_find<SCOPE>(L, a);
    b = rg_find<SCOPE>(L, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }                                   // a > b: hang a below b
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old >= a) break;                // a was a root and now points to b
        a = old;                            // a had a parent old < a: (old, b) still have to be joined
    }
}

__device__ __forceinline__ bool rg_fg(const float* scores, float thr, const uint8_t* mask, int64_t p) {
    return scores ? scores[p] >= thr : mask[p] != 0;         // NaN >= thr is false: background, as ssad_confusion_counts counts it
}

__global__ __launch_bounds__(RG_TT) void rg_local_kernel(const float* __restrict__ scores, float thr, const uint8_t* __restrict__ mask,
                                                        int* __restrict__ labels, int H, int W, int tiles_x, int tiles, int conn8) {
    __shared__ int L[RG_TT];
    __shared__ unsigned rows[RG_T];
    const int t = threadIdx.x, lx = t & (RG_T - 1), ly = t / RG_T;
    const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
    const int ty0 = (tile / tiles_x) * RG_T, tx0 = (tile % tiles_x) * RG_T;
    const int x = tx0 + lx, y = ty0 + ly;
    const bool in = x < W && y < H;
    const int64_t p = (int64_t)img * H * W + (int64_t)y * W + x;
    const bool fg = in && rg_fg(scores, thr, mask, p);
    const unsigned long long b = __ballot(fg);
    const unsigned row = (unsigned)(t & 32 ? b >> 32 : b);                              // this tile row's foreground bits
    const unsigned gaps = ~row & ((1u << lx) - 1u);                                     // background to the left of this pixel
    const int start = gaps ? 32 - __clz(gaps) : 0;                                      // first pixel of this pixel's run
    L[t] = fg ? ly * RG_T + start : -1;
    if (lx == 0) rows[ly] = row;
    __syncthreads();
    if (fg && ly > 0) {
        const unsigned above = rows[ly - 1];
        const bool up = above >> lx & 1u;
        const bool left = lx > 0 && (row >> (lx - 1) & 1u), upleft = lx > 0 && (above >> (lx - 1) & 1u);
        const bool upright = lx < RG_T - 1 && (above >> (lx + 1) & 1u);
        // a union is left out where the pixels are already joined through runs and the left neighbour's own union
        if (up && !(left && upleft)) rg_union<__HIP_MEMORY_SCOPE_WORKGROUP>(L, t, t - RG_T);
        if (conn8) {
            if (upleft && !up && !left) rg_union<__HIP_MEMORY_SCOPE_WORKGROUP>(L, t, t - RG_T - 1);
            if (upright && !up) rg_union<__HIP_MEMORY_SCOPE_WORKGROUP>(L, t, t - RG_T + 1);
        }
    }
    __syncthreads();
    if (!in) return;
    int out = -1;
    if (fg) {
        const int r = rg_find<__HIP_MEMORY_SCOPE_WORKGROUP>(L, t);                       // local raster order = raster order in the image
        out = (ty0 + r / RG_T) * W + tx0 + (r & (RG_T - 1));
    }
    labels[p] = out;
}

// one thread per pixel of the batch; only the first row and column of a tile have work
__global__ void rg_merge_kernel(int* __restrict__ labels, int H, int W, int64_t total, int conn8) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int hw = H * W;
    const int q = (int)(i % hw), y = q / W, x = q - y * W;
    const bool col0 = x > 0 && (x & (RG_T - 1)) == 0, row0 = y > 0 && (y & (RG_T - 1)) == 0;
    if (!col0 && !row0) return;
    int* L = labels + (i - q);
    if (L[q] < 0) return;                                                               // background never changes
    auto join = [&](int xx, int yy) {
        if ((unsigned)xx >= (unsigned)W || (unsigned)yy >= (unsigned)H) return;
        const int o = yy * W + xx;
        if (rg_load<__HIP_MEMORY_SCOPE_AGENT>(L, o) >= 0) rg_union<__HIP_MEMORY_SCOPE_AGENT>(L, q, o);
    };
    if (col0) {
        join(x - 1, y);
        if (conn8) { join(x - 1, y - 1); join(x - 1, y + 1); }
    }
    if (row0) {
        join(x, y - 1);
        if (conn8) { join(x - 1, y - 1); join(x + 1, y - 1); }
    }
}

// one workgroup per RG_CHUNK consecutive pixels of an image
__global__ __launch_bounds__(RG_CHUNK) void rg_flatten_kernel(int* __restrict__ labels, int* __restrict__ chunk_count, int hw, int chunks) {
    const int img = blockIdx.x / chunks, q = (blockIdx.x - img * chunks) * RG_CHUNK + threadIdx.x;
    int* L = labels + (int64_t)img * hw;
    int root = 0;
    if (q < hw && rg_load<__HIP_MEMORY_SCOPE_AGENT>(L, q) >= 0) {
        const int r = rg_find<__HIP_MEMORY_SCOPE_AGENT>(L, q);
        __hip_atomic_store(L + q, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // roots keep their value: r == q there
        root = r == q;
    }
    const int c = __syncthreads_count(root);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = c;
}

// exclusive scan over the 1024 threads of a workgroup; *total = the sum
__device__ __forceinline__ int rg_block_scan(int v, int* total) {
    __shared__ int wave_sum[RG_CHUNK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < RG_CHUNK / 64; ++k) {
        const int s = wave_sum[k];
        base += k < w ? s : 0;
        tot += s;
    }
    __syncthreads();                        // wave_sum is free for the next call
    *total = tot;
    return base + inc - v;
}

// out[r][0 .. len) = exclusive scan of in[r][0 .. len), totals[r] = the sum; one workgroup per row, in == out allowed
__global__ __launch_bounds__(RG_CHUNK) void rg_scan_kernel(const int* in, int* out, int* totals, int64_t len) {
    const int64_t row = (int64_t)blockIdx.x * len;
    int carry = 0;
    for (int64_t base = 0; base < len; base += RG_CHUNK) {
        const int64_t k = base + threadIdx.x;
        const int v = k < len ? in[row + k] : 0;
        int tot;
        const int e = rg_block_scan(v, &tot);
        if (k < len) out[row + k] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(RG_CHUNK) void rg_rank_kernel(const int* __restrict__ labels, const int* __restrict__ chunk_off,
                                                          int* __restrict__ rank, int hw, int chunks) {
    const int img = blockIdx.x / chunks, q = (blockIdx.x - img * chunks) * RG_CHUNK + threadIdx.x;
    const int64_t base = (int64_t)img * hw;
    const int root = q < hw && labels[base + q] == q;
    int tot;
    const int e = rg_block_scan(root, &tot);
    if (root) rank[base + q] = chunk_off[blockIdx.x] + e + 1;
}

__global__ void rg_final_kernel(int* __restrict__ labels, const int* __restrict__ rank, int hw, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int v = labels[i];
    labels[i] = v < 0 ? 0 : rank[i - i % hw + v];
}

// ---- per-region statistics ----
// fp32 -> uint32 whose unsigned order is the numbers' order; NaN -> 0 (below -inf), -0 -> the key of +0
__device__ __forceinline__ unsigned rg_key(float f) {
    if (f != f) return 0u;
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return u & 0x80000000u ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float rg_unkey(unsigned k) {
    if (k == 0u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float(k & 0x80000000u ? k ^ 0x80000000u : ~k);
}

__global__ void rg_stats_init_kernel(int* area, int* bbox, long long* coord_sum, unsigned* peak, int* peak_pos, int R, int W, int H) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    area[r] = 0;
    bbox[4 * r] = W; bbox[4 * r + 1] = H; bbox[4 * r + 2] = -1; bbox[4 * r + 3] = -1;
    coord_sum[2 * r] = 0; coord_sum[2 * r + 1] = 0;
    if (peak) { peak[r] = 0u; peak_pos[r] = INT_MAX; }
}

constexpr int RG_SPT = 16;                  // pixels a thread of rg_stats_kernel takes, 256 apart

struct RgAcc {
    int r, cnt, x0, y0, x1, y1;
    long long sx, sy;
    unsigned key;
    __device__ __forceinline__ void reset(int region) { r = region; cnt = 0; x0 = y0 = INT_MAX; x1 = y1 = -1; sx = sy = 0; key = 0u; }
    __device__ __forceinline__ void merge(const RgAcc& o) {
        cnt += o.cnt; x0 = min(x0, o.x0); y0 = min(y0, o.y0); x1 = max(x1, o.x1); y1 = max(y1, o.y1); sx += o.sx; sy += o.sy;
        key = max(key, o.key);
    }
    __device__ __forceinline__ void flush(int* area, int* bbox, unsigned long long* coord_sum, unsigned* peak) const {
        atomicAdd(&area[r], cnt);
        atomicMin(&bbox[4 * r], x0); atomicMin(&bbox[4 * r + 1], y0);
        atomicMax(&bbox[4 * r + 2], x1); atomicMax(&bbox[4 * r + 3], y1);
        atomicAdd(&coord_sum[2 * r], (unsigned long long)sx); atomicAdd(&coord_sum[2 * r + 1], (unsigned long long)sy);
        if (peak) atomicMax(&peak[r], key);
    }
};

// One workgroup of 256 per 256 * RG_SPT consecutive pixels of an image.  A thread accumulates while the region stays the same
// (its pixels are 256 apart: a vertical strip of a 256-wide map) and sends atomics when it changes; at the end a wave whose
// threads all hold one region reduces in registers, and waves that agree are merged through LDS: one set of atomics per
// workgroup inside a large region instead of one per pixel -- the atomics of a region all go to the same eight addresses.
__global__ __launch_bounds__(256) void rg_stats_kernel(const float* __restrict__ scores, const int* __restrict__ labels,
                                                      const int* __restrict__ offsets, int* area, int* bbox,
                                                      unsigned long long* coord_sum, unsigned* peak, int hw, int W, int chunks, int R) {
    __shared__ RgAcc wave_acc[4];
    const int img = blockIdx.x / chunks, base = (blockIdx.x - img * chunks) * (256 * RG_SPT);
    const int64_t ibase = (int64_t)img * hw;
    const int off = offsets[img];
    RgAcc acc;
    acc.reset(-1);
    for (int j = 0; j < RG_SPT; ++j) {
        const int q = base + j * 256 + threadIdx.x;
        if (q >= hw) break;
        const int lab = labels[ibase + q];
        int r = lab > 0 ? off + lab - 1 : -1;
        if (r >= R) r = -1;                                                              // never past the caller's arrays
        if (r < 0) continue;
        if (r != acc.r) {
            if (acc.r >= 0) acc.flush(area, bbox, coord_sum, peak);
            acc.reset(r);
        }
        const int y = q / W, x = q - y * W;
        ++acc.cnt;
        acc.x0 = min(acc.x0, x); acc.y0 = min(acc.y0, y); acc.x1 = max(acc.x1, x); acc.y1 = max(acc.y1, y);
        acc.sx += x; acc.sy += y;
        if (scores) acc.key = max(acc.key, rg_key(scores[ibase + q]));
    }
    const bool have = acc.r >= 0;
    const unsigned long long b = __ballot(have);
    int wave_r = -1;                                                                     // >= 0: lane 0 holds the wave's sums
    if (b != 0) {
        const int first = __shfl(acc.r, __ffsll((long long)b) - 1);
        if (__all(!have || acc.r == first)) {                                            // lanes without a region hold the neutral values
            for (int o = 32; o > 0; o >>= 1) {
                acc.cnt += __shfl_xor(acc.cnt, o);
                acc.x0 = min(acc.x0, __shfl_xor(acc.x0, o)); acc.y0 = min(acc.y0, __shfl_xor(acc.y0, o));
                acc.x1 = max(acc.x1, __shfl_xor(acc.x1, o)); acc.y1 = max(acc.y1, __shfl_xor(acc.y1, o));
                acc.sx += __shfl_xor(acc.sx, o); acc.sy += __shfl_xor(acc.sy, o);
                acc.key = max(acc.key, (unsigned)__shfl_xor((int)acc.key, o));
            }
            wave_r = first;
        } else if (have) {
            acc.flush(area, bbox, coord_sum, peak);
        }
    }
    if ((threadIdx.x & 63) == 0) {
        acc.r = wave_r;
        wave_acc[threadIdx.x >> 6] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < 4; ++w) {
            if (wave_acc[w].r < 0) continue;
            RgAcc sum = wave_acc[w];
            for (int v = w + 1; v < 4; ++v)
                if (wave_acc[v].r == sum.r) { sum.merge(wave_acc[v]); wave_acc[v].r = -1; }
            sum.flush(area, bbox, coord_sum, peak);
        }
    }
}

// the peaks are final (a launch later): the smallest raster index that attains a region's peak.  A saturated map ties at every
// pixel of a region: of a wave's pixels that attain the peak of one region only the first asks, and nobody asks who reads a
// smaller position already (a stale read only costs an atomic that changes nothing).
__global__ void rg_peak_pos_kernel(const float* __restrict__ scores, const int* __restrict__ labels, const int* __restrict__ offsets,
                                   const unsigned* __restrict__ peak, int* peak_pos, int hw, int64_t total, int R) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lab = i < total ? labels[i] : 0;
    int r = lab > 0 ? offsets[i / hw] + lab - 1 : -1;
    if (r >= R) r = -1;
    const bool hit = r >= 0 && rg_key(scores[i]) == peak[r];
    const unsigned long long b = __ballot(hit);
    if (b == 0) return;
    const int lead = __ffsll((long long)b) - 1, q = (int)(i % hw);
    const int r0 = __shfl(r, lead);
    const bool ask = __all(!hit || r == r0) ? (int)(threadIdx.x & 63) == lead : hit;    // one region: its first pixel of the wave
    if (ask && q < peak_pos[r]) atomicMin(&peak_pos[r], q);
}

__global__ void rg_peak_decode_kernel(unsigned* peak, int R) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) ((float*)peak)[r] = rg_unkey(peak[r]);
}

// ---- filter ----
// new_label[r] = kept regions of r's image up to and including r, 0 when r is dropped; one workgroup per image
__global__ __launch_bounds__(RG_CHUNK) void rg_renumber_kernel(const int* __restrict__ offsets, const uint8_t* __restrict__ keep,
                                                              int* __restrict__ new_label, int* counts_out, int R) {
    const int lo = offsets[blockIdx.x], hi = min(offsets[blockIdx.x + 1], R);
    int carry = 0;
    for (int base = lo; base < hi; base += RG_CHUNK) {
        const int r = base + threadIdx.x;
        const int k = r < hi && keep[r] != 0;
        int tot;
        const int e = rg_block_scan(k, &tot);
        if (r < hi) new_label[r] = k ? carry + e + 1 : 0;
        carry += tot;
    }
    if (threadIdx.x == 0 && counts_out) counts_out[blockIdx.x] = carry;
}

__global__ void rg_filter_kernel(const int* labels, const int* __restrict__ offsets, const uint8_t* __restrict__ keep,
                                 const int* __restrict__ new_label, uint8_t* __restrict__ mask_out, int* labels_out, int hw,
                                 int64_t total, int R) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int lab = labels[i];
    int r = lab > 0 ? offsets[i / hw] + lab - 1 : -1;
    if (r >= R) r = -1;
    const int kept = r >= 0 && keep[r] != 0;
    mask_out[i] = (uint8_t)kept;
    if (labels_out) labels_out[i] = kept ? new_label[r] : 0;
}

__global__ void rg_pro_weights_kernel(const int* __restrict__ labels, const int* __restrict__ offsets, const int* __restrict__ area,
                                      uint8_t* __restrict__ fp_w, double* __restrict__ pro_w, int hw, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int lab = labels[i];
    fp_w[i] = lab == 0;
    pro_w[i] = lab > 0 ? 1.0 / (double)area[offsets[i / hw] + lab - 1] : 0.0;           // IEEE division: numpy's 1.0 / sizes
}

inline unsigned rg_grid(int64_t n, int block) { return (unsigned)cdiv64(n, block); }
inline int64_t rg_align(int64_t b) { return (b + 255) & ~(int64_t)255; }
inline bool rg_shape_ok(int64_t n, int H, int W) {
    return n >= 1 && H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 30) && n * H * W < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int ssad_label_regions_tile(void) { return RG_T; }

extern "C" int64_t ssad_label_regions_workspace(int64_t n, int H, int W) {
    if (!rg_shape_ok(n, H, W)) return 0;
    const int64_t hw = (int64_t)H * W;
    return rg_align(n * hw * 4) + rg_align(n * cdiv64(hw, RG_CHUNK) * 4);               // root ranks, chunk counts
}

extern "C" int ssad_label_regions(const float* scores, float threshold, const uint8_t* mask, int64_t n, int H, int W, int connectivity,
                                  int32_t* labels, int32_t* counts, int32_t* offsets, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    SSAD_CHECK_ARG((scores != nullptr) != (mask != nullptr), "exactly one of scores / mask");
    SSAD_CHECK_ARG(connectivity == 4 || connectivity == 8, "connectivity is 4 or 8");
    SSAD_CHECK_ARG(n >= 1 && H >= 1 && W >= 1, "empty batch or image");
    SSAD_CHECK_ARG((int64_t)H * W < ((int64_t)1 << 30), "image too large (labels are pixel indices)");
    SSAD_CHECK_ARG(n * H * W < ((int64_t)1 << 31), "batch too large (offsets are int32)");
    SSAD_CHECK_ARG(labels && counts && offsets && workspace, "null output or workspace");
    SSAD_CHECK_ARG(workspace_bytes >= ssad_label_regions_workspace(n, H, W), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int hw = H * W, chunks = (int)cdiv64(hw, RG_CHUNK);
    const int64_t total = n * hw;
    const int tiles_x = (W + RG_T - 1) / RG_T, tiles = tiles_x * ((H + RG_T - 1) / RG_T);
    int* rank = (int*)workspace;
    int* chunk = (int*)((char*)workspace + rg_align(total * 4));
    const int conn8 = connectivity == 8;
    hipLaunchKernelGGL(rg_local_kernel, dim3((unsigned)(n * tiles)), dim3(RG_TT), 0, st, scores, threshold, mask, labels, H, W, tiles_x,
                       tiles, conn8);
    hipLaunchKernelGGL(rg_merge_kernel, dim3(rg_grid(total, 256)), dim3(256), 0, st, labels, H, W, total, conn8);
    hipLaunchKernelGGL(rg_flatten_kernel, dim3((unsigned)(n * chunks)), dim3(RG_CHUNK), 0, st, labels, chunk, hw, chunks);
    hipLaunchKernelGGL(rg_scan_kernel, dim3((unsigned)n), dim3(RG_CHUNK), 0, st, (const int*)chunk, chunk, counts, (int64_t)chunks);
    hipLaunchKernelGGL(rg_scan_kernel, dim3(1), dim3(RG_CHUNK), 0, st, (const int*)counts, offsets, offsets + n, n);
    hipLaunchKernelGGL(rg_rank_kernel, dim3((unsigned)(n * chunks)), dim3(RG_CHUNK), 0, st, (const int*)labels, (const int*)chunk, rank,
                       hw, chunks);
    hipLaunchKernelGGL(rg_final_kernel, dim3(rg_grid(total, 256)), dim3(256), 0, st, labels, (const int*)rank, hw, total);
    SSAD_CHECK_LAUNCH();
    return 0;
}

extern "C" int ssad_region_stats(const float* scores, const int32_t* labels, const int32_t* offsets, int64_t n, int H, int W, int64_t R,
                                 int32_t* area, int32_t* bbox, int64_t* coord_sum, float* peak, int32_t* peak_pos, void* stream) {
    SSAD_CHECK_ARG(labels && offsets && rg_shape_ok(n, H, W), "bad argument");
    SSAD_CHECK_ARG(R >= 0 && R < ((int64_t)1 << 31), "R is offsets[n]");
    if (R == 0) return 0;
    SSAD_CHECK_ARG(area && bbox && coord_sum, "null output");
    SSAD_CHECK_ARG(scores ? (peak && peak_pos) : (!peak && !peak_pos), "peak / peak_pos go with scores");
    hipStream_t st = (hipStream_t)stream;
    const int hw = H * W, chunks = (int)cdiv64(hw, 256 * RG_SPT);
    const int64_t total = n * hw;
    hipLaunchKernelGGL(rg_stats_init_kernel, dim3(rg_grid(R, 256)), dim3(256), 0, st, area, bbox, (long long*)coord_sum, (unsigned*)peak,
                       peak_pos, (int)R, W, H);
    hipLaunchKernelGGL(rg_stats_kernel, dim3((unsigned)(n * chunks)), dim3(256), 0, st, scores, labels, offsets, area, bbox,
                       (unsigned long long*)coord_sum, (unsigned*)peak, hw, W, chunks, (int)R);
    if (scores) {
        hipLaunchKernelGGL(rg_peak_pos_kernel, dim3(rg_grid(total, 256)), dim3(256), 0, st, scores, labels, offsets,
                           (const unsigned*)peak, peak_pos, hw, total, (int)R);
        hipLaunchKernelGGL(rg_peak_decode_kernel, dim3(rg_grid(R, 256)), dim3(256), 0, st, (unsigned*)peak, (int)R);
    }
    SSAD_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t ssad_region_filter_workspace(int64_t R) { return R > 0 ? rg_align(R * 4) : 256; }

extern "C" int ssad_region_filter(const int32_t* labels, const int32_t* offsets, const uint8_t* keep, int64_t n, int H, int W, int64_t R,
                                  uint8_t* mask_out, int32_t* labels_out, int32_t* counts_out, int32_t* offsets_out, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    SSAD_CHECK_ARG(labels && offsets && mask_out && rg_shape_ok(n, H, W), "bad argument");
    SSAD_CHECK_ARG(R >= 0 && R < ((int64_t)1 << 31) && (R == 0 || keep), "R is offsets[n]; keep holds R flags");
    SSAD_CHECK_ARG(labels_out ? (counts_out && offsets_out) : (!counts_out && !offsets_out), "counts_out / offsets_out go with labels_out");
    SSAD_CHECK_ARG(!labels_out || (workspace && workspace_bytes >= ssad_region_filter_workspace(R)), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int hw = H * W;
    const int64_t total = n * hw;
    int* new_label = (int*)workspace;
    if (labels_out) {
        hipLaunchKernelGGL(rg_renumber_kernel, dim3((unsigned)n), dim3(RG_CHUNK), 0, st, offsets, keep, new_label, counts_out, (int)R);
        hipLaunchKernelGGL(rg_scan_kernel, dim3(1), dim3(RG_CHUNK), 0, st, (const int*)counts_out, offsets_out, offsets_out + n, n);
    }
    hipLaunchKernelGGL(rg_filter_kernel, dim3(rg_grid(total, 256)), dim3(256), 0, st, labels, offsets, keep, (const int*)new_label,
                       mask_out, labels_out, hw, total, (int)R);
    SSAD_CHECK_LAUNCH();
    return 0;
}

extern "C" int ssad_pro_weights(const int32_t* labels, const int32_t* offsets, const int32_t* area, int64_t n, int H, int W,
                                uint8_t* fp_w, double* pro_w, void* stream) {
    SSAD_CHECK_ARG(labels && offsets && fp_w && pro_w && rg_shape_ok(n, H, W), "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = n * H * W;
    hipLaunchKernelGGL(rg_pro_weights_kernel, dim3(rg_grid(total, 256)), dim3(256), 0, st, labels, offsets, area, fp_w, pro_w, H * W, total);
    SSAD_CHECK_LAUNCH();
    return 0;
}
