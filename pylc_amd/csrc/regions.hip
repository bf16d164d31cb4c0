// Connected regions of a class mask and the small-region sieve (not in the reference).
//
// A label is the minimum linear index of its region, so the whole computation is a union-find in which a union always hangs the LARGER
// root under the SMALLER one: parent[i] <= i everywhere and at all times, a root is its set's minimum, and the result does not depend on
// the order of the unions.
//
//   tile pass     one block per 128 x 16 tile, entirely in LDS: horizontal runs from a wave ballot (no atomics), vertical and diagonal links
//                 as unions by atomicMin on LDS indices, flatten, labels = GLOBAL index of the tile-local root (raster order inside a tile
//                 agrees with the global one: the minimum stays the minimum).
//   border pass   one thread per pixel of a tile's top row or left column: the links that cross a tile border, as unions in `labels`
//                 (which is the parent array of a forest of depth <= 1 at that point).
//   flatten pass  labels[i] = root(i).
//
// A link is left out where others already imply it: the vertical link of p when the pixel to its left and the two above them all have
// p's value (the pair to the left makes the same union; by induction along the run its leftmost pair is never left out), a diagonal link
// when one of the two pixels completing the 2 x 2 square has p's value (a vertical link and a horizontal one go the same way).
// Horizontal links are never left out.  The rules only read mask values, so every block decides the same.
//
// No kernel waits for another block: a kernel boundary is the only inter-block synchronisation.  Every loop is a parent chase
// (parent[i] < i at a non-root: strictly decreasing, ends at a root) or an atomicMin retry whose larger index strictly decreases.
//
// Sizes are counted from the labels alone (pylc_region_sizes): a wave first adds up its pixels per label in registers (ballot rounds as
// in score.hip -- a sky of ten million pixels is ONE label), a block then merges its waves' partial counts in LDS, so that the constant
// mask costs one global atomic per 8192 pixels instead of one per pixel on a single word.
//
// The sieve is two launches: small regions' border pixels bid for their region with a 64-bit atomicMax of
// key = size << 32 | (0xFFFFFFFF - root) of each large 4-neighbour; the second writes the output and counts changes per block.
#include "common.h"

namespace pylc {

constexpr int RG_TW = 128, RG_TH = 16;                 // tile: 2048 pixels, 8 per thread
constexpr int RG_TILE = RG_TW * RG_TH;
constexpr int RG_INVALID = 0x100;                      // LDS value of a pixel that is ignored or outside the image: equal to nothing
constexpr int RG_SZ_ITERS = 8;                         // pylc_region_sizes: rounds of 1024 labels per block
constexpr int RG_SZ_ROUNDS = 4;                        // wave-level rounds per 256 labels before the per-pixel atomics
constexpr int RG_SZ_ENTRIES = 4 * RG_SZ_ITERS * RG_SZ_ROUNDS;

// ---- union-find, shared by the LDS and the global form ---------------------------------------------------------------------------------
struct LdsParents {
    int* p;
    // (an atomic load: other waves of the block change parents while this one chases, the value must come from LDS every time)
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int amin(int i, int v) const { return atomicMin(&p[i], v); }
};
// the border pass reads parents that other blocks (on other XCDs) are changing: agent-scope loads, so that every read is served past the
// per-CU L1 and per-XCD caches.  (A stale parent would still be an ancestor -- parents only ever move up the same tree -- and cost
// iterations, never correctness.)
struct GlobalParents {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int amin(int i, int v) const { return atomicMin(&p[i], v); }
};

template <typename P>
__device__ __forceinline__ int rg_find(const P& par, int a) {
    // parent chase: par[a] < a at every non-root, so a strictly decreases and the loop ends at a root (par[a] == a), after at most a steps
    for (;;) {
        const int n = par.load(a);
        if (n == a) return a;
        a = n;
    }
}

template <typename P>
__device__ __forceinline__ void rg_union(const P& par, int a, int b) {
    // atomicMin retry: each pass either ends or replaces the pair (a, b) by one whose LARGER index is strictly smaller (hi's old parent is
    // below hi, and so is lo), so the loop is bounded by the indices themselves
    for (;;) {
        a = rg_find(par, a);
        b = rg_find(par, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = par.amin(hi, lo);
        if (old == hi) return;                         // hi was a root and now hangs under lo
        // hi had stopped being a root: its parent is now min(old, lo), which keeps it joined to one of the two; join the other
        a = old;
        b = lo;
    }
}

// ---- tile pass -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_tile_kernel(const unsigned char* __restrict__ mask, int H, int W, int tiles_x, int conn8, int ign,
                                                      int* __restrict__ labels) {
    __shared__ unsigned short val[RG_TILE];
    __shared__ int parent[RG_TILE];
    const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * RG_TH, tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * RG_TW;
    const int tid = threadIdx.x, lane = tid & 63;
    const LdsParents par{parent};
    // a wave holds 64 consecutive pixels of one tile row
#pragma unroll
    for (int s = 0; s < RG_TILE / 256; ++s) {
        const int p = s * 256 + tid, y = ty0 + (p >> 7), x = tx0 + (p & (RG_TW - 1));
        int v = RG_INVALID;
        if (y < H && x < W) {
            v = mask[(long long)y * W + x];
            if (v == ign) v = RG_INVALID;
        }
        val[p] = (unsigned short)v;
        // horizontal runs: a lane continues its left neighbour's run when both hold the same valid value; the run's first lane is the
        // highest head at or below the lane (lane 0 is always one: the seam between the two waves of a row is a union below)
        const int left = __shfl_up(v, 1, 64);
        const bool cont = lane > 0 && v != RG_INVALID && left == v;
        const unsigned long long heads = ~__ballot(cont);
        const int first = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
        parent[p] = p - lane + first;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < RG_TILE / 256; ++s) {
        const int p = s * 256 + tid, ly = p >> 7, lx = p & (RG_TW - 1);
        const int v = val[p];
        if (v == RG_INVALID) continue;
        const bool lf = lx > 0 && val[p - 1] == v;
        if (lx == 64 && lf) rg_union(par, p, p - 1);
        if (ly == 0) continue;
        const int up = p - RG_TW;
        const bool u = val[up] == v;
        if (u && !(lf && val[up - 1] == v)) rg_union(par, p, up);
        if (conn8 && !u) {
            if (lx > 0 && !lf && val[up - 1] == v) rg_union(par, p, up - 1);
            if (lx < RG_TW - 1 && val[up + 1] == v && val[p + 1] != v) rg_union(par, p, up + 1);
        }
    }
    __syncthreads();
    int root[RG_TILE / 256];
#pragma unroll
    for (int s = 0; s < RG_TILE / 256; ++s) root[s] = rg_find(par, s * 256 + tid);
#pragma unroll
    for (int s = 0; s < RG_TILE / 256; ++s) {
        const int p = s * 256 + tid, y = ty0 + (p >> 7), x = tx0 + (p & (RG_TW - 1));
        if (y < H && x < W) {
            const int r = root[s];
            labels[(long long)y * W + x] = val[p] == RG_INVALID ? -1 : (ty0 + (r >> 7)) * W + tx0 + (r & (RG_TW - 1));
        }
    }
}

// ---- border pass -----------------------------------------------------------------------------------------------------------------------
// threads 0 .. n_row-1: the pixels of the rows y = k * RG_TH (k >= 1), links upwards; then n_col threads: the pixels of the columns
// x = k * RG_TW (k >= 1), links to the left, and the diagonals that cross only the column border
__global__ __launch_bounds__(256) void rg_border_kernel(const unsigned char* __restrict__ mask, int H, int W, long long n_row, long long n_col,
                                                        int conn8, int ign, int* labels) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_row + n_col) return;
    const GlobalParents par{labels};
    if (t < n_row) {
        const int y = (int)(t / W + 1) * RG_TH, x = (int)(t % W);
        const long long pl = (long long)y * W + x;          // < 2^31
        const int p = (int)pl, up = p - W;
        const int v = mask[p];
        if (v == ign) return;
        const bool lf = x > 0 && mask[p - 1] == v;
        const bool u = mask[up] == v;
        if (u && !(lf && mask[up - 1] == v)) rg_union(par, p, up);
        if (conn8 && !u) {
            if (x > 0 && !lf && mask[up - 1] == v) rg_union(par, p, up - 1);
            if (x + 1 < W && mask[up + 1] == v && mask[p + 1] != v) rg_union(par, p, up + 1);
        }
    } else {
        const long long c = t - n_row;
        const int x = (int)(c / H + 1) * RG_TW, y = (int)(c % H);
        const int p = (int)((long long)y * W + x), q = p - 1;
        const int v = mask[p], vq = mask[q];
        const bool lf = vq == v && v != ign;
        if (lf) rg_union(par, p, q);
        if (conn8 && y > 0 && y % RG_TH != 0 && !lf) {         // (on a tile's top row the row threads above make these links)
            const int up = p - W, uq = q - W;
            const int vu = mask[up], vuq = mask[uq];
            if (v != ign && vuq == v && vu != v) rg_union(par, p, uq);          // p and its upper left
            if (vq != ign && vu == vq && vuq != vq) rg_union(par, q, up);       // q and its upper right
        }
    }
}

// ---- flatten pass ----------------------------------------------------------------------------------------------------------------------
// Other threads of this launch overwrite parents with roots while this one chases: what it reads is an ancestor either way.
struct FlattenParents {
    const int* p;
    __device__ __forceinline__ int load(int i) const { return p[i]; }
};
__global__ __launch_bounds__(256) void rg_flatten_kernel(int* labels, long long N) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int l = labels[i];
    if (l < 0 || l == (int)i) return;
    const int r = rg_find(FlattenParents{labels}, l);
    if (r != l) labels[i] = r;
}

// ---- sizes -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_sizes_kernel(const int* __restrict__ labels, long long N, int* __restrict__ sizes) {
    __shared__ int e_label[RG_SZ_ENTRIES];
    __shared__ int e_count[RG_SZ_ENTRIES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < RG_SZ_ENTRIES) e_label[tid] = -1;
    __syncthreads();
    const long long base = (long long)blockIdx.x * (RG_SZ_ITERS * 1024);
#pragma unroll 1
    for (int it = 0; it < RG_SZ_ITERS; ++it) {
        int cell[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = base + it * 1024 + k * 256 + tid;
            cell[k] = i < N ? labels[i] : -1;
        }
        // wave-level rounds (wave-uniform control flow): the label of the first lane that still holds one is broadcast, every pixel of
        // the wave with that label is counted by a ballot and retires; the total goes to the wave's LDS entry of this round
#pragma unroll 1
        for (int r = 0; r < RG_SZ_ROUNDS; ++r) {
            const int mine = cell[0] >= 0 ? cell[0] : cell[1] >= 0 ? cell[1] : cell[2] >= 0 ? cell[2] : cell[3];
            const unsigned long long holders = __ballot(mine >= 0);
            if (holders == 0) break;
            const int leader = __ffsll((long long)holders) - 1;
            const int lc = __builtin_amdgcn_readlane(mine, leader);
            int n = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool same = cell[k] == lc;
                n += __popcll(__ballot(same));
                cell[k] = same ? -1 : cell[k];
            }
            if (lane == leader) {
                const int e = (wv * RG_SZ_ITERS + it) * RG_SZ_ROUNDS + r;
                e_label[e] = lc;
                e_count[e] = n;
            }
        }
        // what is left (noise: many labels in one wave) hardly collides
#pragma unroll
        for (int k = 0; k < 4; ++k) if (cell[k] >= 0) atomicAdd(&sizes[cell[k]], 1);
    }
    __syncthreads();
    // merge the block's entries: the first entry of each label adds up all of them and issues the one global atomic
    if (tid < RG_SZ_ENTRIES) {
        const int l = e_label[tid];
        if (l >= 0) {
            bool first = true;
            for (int j = 0; j < tid; ++j) first = first && e_label[j] != l;
            if (first) {
                int n = e_count[tid];
                for (int j = tid + 1; j < RG_SZ_ENTRIES; ++j) n += e_label[j] == l ? e_count[j] : 0;
                atomicAdd(&sizes[l], n);
            }
        }
    }
}

// ---- sieve -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_sieve_bid_kernel(const int* __restrict__ labels, const int* __restrict__ sizes, int H, int W,
                                                           int min_size, unsigned long long* __restrict__ best) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int l = labels[i];
    if (l < 0 || sizes[l] >= min_size) return;
    const int y = (int)(i / W), x = (int)(i % W);
    unsigned long long key = 0;
    const auto look = [&](long long j) {
        const int lj = labels[j];
        if (lj < 0 || lj == l) return;
        const int sj = sizes[lj];
        if (sj < min_size) return;
        const unsigned long long k = (unsigned long long)(unsigned)sj << 32 | (0xFFFFFFFFu - (unsigned)lj);
        key = k > key ? k : key;
    };
    if (y > 0) look(i - W);
    if (x > 0) look(i - 1);
    if (x + 1 < W) look(i + 1);
    if (y + 1 < H) look(i + W);
    if (key) atomicMax(&best[l], key);
}

__global__ __launch_bounds__(256) void rg_sieve_apply_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ labels,
                                                             const int* __restrict__ sizes, long long N, int min_size, int fill,
                                                             const unsigned long long* __restrict__ best, unsigned char* __restrict__ out,
                                                             unsigned long long* __restrict__ n_changed) {
    __shared__ int red[4];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int changed = 0;
    if (i < N) {
        const int v = mask[i], l = labels[i];
        int o = v;
        if (l >= 0 && sizes[l] < min_size) {
            if (fill >= 0) {
                o = fill;
            } else {
                const unsigned long long k = best[l];
                if (k) o = mask[0xFFFFFFFFu - (unsigned)k];          // the winner's root holds the winner's value
            }
        }
        out[i] = (unsigned char)o;
        changed = o != v;
    }
    const int n = __popcll(__ballot(changed));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0 && n_changed) {
        const int tot = red[0] + red[1] + red[2] + red[3];
        if (tot) atomicAdd(n_changed, (unsigned long long)tot);
    }
}

}  // namespace pylc

using namespace pylc;

static bool rg_pixels_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }

extern "C" int pylc_label_regions(const unsigned char* mask, int H, int W, int connectivity, int ignore_index, int* labels, void* stream) {
    PYLC_REQUIRE(mask && labels, "label_regions: mask or labels is NULL");
    PYLC_REQUIRE(connectivity == 4 || connectivity == 8, "label_regions: connectivity=%d (4 or 8)", connectivity);
    PYLC_REQUIRE(rg_pixels_ok(H, W), "label_regions: H=%d W=%d outside 1 <= H*W < 2^31", H, W);
    PYLC_REQUIRE(ignore_index >= -1 && ignore_index <= 255, "label_regions: ignore_index=%d outside -1..255", ignore_index);
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(labels) & 3) == 0, "label_regions: labels is not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    const long long N = (long long)H * W;
    const int tiles_x = cdiv(W, RG_TW), tiles_y = cdiv(H, RG_TH);
    const int conn8 = connectivity == 8;
    hipLaunchKernelGGL(rg_tile_kernel, dim3((unsigned)((long long)tiles_x * tiles_y)), dim3(256), 0, st, mask, H, W, tiles_x, conn8, ignore_index,
                       labels);
    const long long n_row = (long long)(tiles_y - 1) * W, n_col = (long long)(tiles_x - 1) * H;
    if (n_row + n_col > 0)
        hipLaunchKernelGGL(rg_border_kernel, dim3((unsigned)cdiv<long long>(n_row + n_col, 256)), dim3(256), 0, st, mask, H, W, n_row, n_col,
                           conn8, ignore_index, labels);
    if (n_row + n_col > 0)                             // a single tile is flat already
        hipLaunchKernelGGL(rg_flatten_kernel, dim3((unsigned)cdiv<long long>(N, 256)), dim3(256), 0, st, labels, N);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_region_sizes(const int* labels, long long N, int* sizes, void* stream) {
    PYLC_REQUIRE(labels && sizes, "region_sizes: labels or sizes is NULL");
    PYLC_REQUIRE(N >= 1 && N < (1ll << 31), "region_sizes: N=%lld outside 1 <= N < 2^31", N);
    PYLC_REQUIRE(((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(sizes)) & 3) == 0, "region_sizes: a buffer is not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    PYLC_HIP(hipMemsetAsync(sizes, 0, (size_t)N * sizeof(int), st));
    hipLaunchKernelGGL(rg_sizes_kernel, dim3((unsigned)cdiv<long long>(N, RG_SZ_ITERS * 1024)), dim3(256), 0, st, labels, N, sizes);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_sieve_regions(const unsigned char* mask, const int* labels, const int* sizes, int H, int W, int min_size, int ignore_index,
                                  int fill, unsigned long long* best_ws, unsigned char* out, long long* n_changed, void* stream) {
    PYLC_REQUIRE(mask && labels && sizes && out, "sieve_regions: mask, labels, sizes or out is NULL");
    PYLC_REQUIRE(rg_pixels_ok(H, W), "sieve_regions: H=%d W=%d outside 1 <= H*W < 2^31", H, W);
    PYLC_REQUIRE(min_size >= 1, "sieve_regions: min_size=%d below 1", min_size);
    PYLC_REQUIRE(ignore_index >= -1 && ignore_index <= 255, "sieve_regions: ignore_index=%d outside -1..255", ignore_index);
    PYLC_REQUIRE(fill >= -1 && fill <= 255, "sieve_regions: fill=%d outside -1..255 (-1: the neighbour rule)", fill);
    PYLC_REQUIRE(fill >= 0 || best_ws, "sieve_regions: the neighbour rule needs best_ws");
    PYLC_REQUIRE(out != mask, "sieve_regions: out may not alias mask");
    PYLC_REQUIRE(((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(sizes)) & 3) == 0 &&
                 ((reinterpret_cast<uintptr_t>(best_ws) | reinterpret_cast<uintptr_t>(n_changed)) & 7) == 0,
                 "sieve_regions: a buffer is not aligned to its element");
    hipStream_t st = as_stream(stream);
    const long long N = (long long)H * W;
    const unsigned blocks = (unsigned)cdiv<long long>(N, 256);
    if (fill < 0) {
        PYLC_HIP(hipMemsetAsync(best_ws, 0, (size_t)N * 8, st));
        hipLaunchKernelGGL(rg_sieve_bid_kernel, dim3(blocks), dim3(256), 0, st, labels, sizes, H, W, min_size, best_ws);
    }
    hipLaunchKernelGGL(rg_sieve_apply_kernel, dim3(blocks), dim3(256), 0, st, mask, labels, sizes, N, min_size, fill, best_ws, out,
                       reinterpret_cast<unsigned long long*>(n_changed));
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}
