// Distance to the nearest pixel of another class, and the scores of the band along class borders: boundary IoU and trimap counts
// (not in the reference).
//
// d2(p) = min(R*R + 1, min |p - q|^2 over the pixels q of the same image whose value differs from p's); an ignored pixel differs from every
// class and gets -1 itself; the image edge is no border.  The transform is separable and exact in integers:
//
//   column pass   g(x,y)  = min(R + 1, min |y - y'| over y' with m[y',x] != m[y,x])                                    one byte per pixel
//   row pass      d2(x,y) = min(R*R + 1, min over |x - x'| <= R of (x - x')^2 + (m[y,x'] != m[y,x] ? 0 : g(x',y))^2)
//
// (g(x',y) was taken relative to m[y,x']: where that value equals m[y,x] it is the wanted column distance, where it differs the pixel
// (x',y) itself is a q at column distance 0.)
//
// Both passes stage a tile and its R-wide halo in LDS (dynamic: the size follows R) and scan outward from every pixel, at most R steps
// each way, so the work per pixel is bounded by R and not by the image:
//
//   column pass   a 64 x 64 tile plus R rows above and below, as dwords of 4 columns.  A thread owns 4 columns: one ds_read_b32 per step
//                 and direction compares 4 pixels at once (xor, then the zero-byte trick), the step at which a byte first differs is
//                 its g.  The 64 lanes of a wave read 64 consecutive dwords: conflict-free.  It ends when its 4 bytes are all found.
//   row pass      a 128 x 8 tile plus R columns left and right, one 16-bit word value | g << 8 per pixel: ONE ds_read_u16 per candidate.
//                 A lane owns a pixel; consecutive lanes read consecutive words (two lanes per bank dword: a broadcast).  The scan stops
//                 once (x - x')^2 reaches the best value so far -- at the first differing value, whose candidate is exactly that square.
//
// Pixels outside the image are never a q: the scans are bounded by the pixel's distance to the image edge, the LDS cells past the edge
// are filled and never read.  A block belongs to one image of the batch and reads no other.
//
// Counts (pylc_boundary_counts): the row pass of the truth and of the prediction in ONE kernel, whose epilogue counts instead of writing
// the two d2 maps.  A pixel's contribution is a key (truth, prediction, in the truth's band, in the prediction's band); a wave adds up
// each run of equal keys along its row with one ballot (masks are blobs: most of a wave shares one key), the block's LDS counters take the
// runs' totals and the int64 counters one 64-bit atomic per non-zero cell and block.  Above BD_LDS_MAXC classes the C*C + 3C + 1 cells
// are no sensible LDS array and the runs' totals go to the int64 counters directly.  pylc_boundary_counts_maps is the two-map form: the
// same epilogue over two d2 maps written by pylc_boundary_distance (tools/boundary_bench.py times one against the other).
//
// Border weights (pylc_boundary_weights): the row pass with an epilogue that stores table[d2] as a float instead of
// d2 -- the per-pixel weight of a border-weighted loss in the two launches of the distance, with no int32 map written and read back.  The
// profile is the caller's table of R*R + 2 floats (no expf here: the result is a lookup, bit for bit what numpy's table[d2] gives).
// pylc_weights_from_d2 is the one-launch form over a map that exists.
#include "common.h"

namespace pylc {

constexpr int BD_CL_TW = 64, BD_CL_TH = 64;           // column pass tile: 16 dword-columns x 64 rows, a thread takes 4 columns x 4 rows
constexpr int BD_RW_TW = 128, BD_RW_TH = 8;            // row pass tile: a thread takes 1 column x 4 rows
constexpr int BD_MAX_R = 254;                          // g = R + 1 must fit a byte
constexpr int BD_LDS_MAXC = 32;                        // classes up to which a block counts in LDS
constexpr int BD_LDS_CELLS = BD_LDS_MAXC * BD_LDS_MAXC + 3 * BD_LDS_MAXC + 1;
constexpr int BD_KEY_BAD = 1 << 20;
constexpr int BD_COUNT_GRID = 8 * kNumCU;              // blocks of a counting kernel at most: they walk the tiles and flush once

// the value of pixel i as the passes see it: the ignore label where `from` (the truth, for a prediction) holds it
__device__ __forceinline__ int bd_value(const unsigned char* __restrict__ mask, const unsigned char* __restrict__ from, long long i, int ign) {
    int v = mask[i];
    if (from && from[i] == ign) v = ign;
    return v;
}

// ---- column pass -----------------------------------------------------------------------------------------------------------------------
// g: [B][H][Wp] bytes, Wp = W rounded up to 4 and the base 4-byte aligned, so that a thread's 4 columns are one aligned dword
__global__ __launch_bounds__(256) void bd_column_kernel(const unsigned char* __restrict__ mask, const unsigned char* __restrict__ from, int H, int W,
                                                        int Wp, int tiles_x, int tiles_y, int R, int ign, unsigned char* __restrict__ g) {
    extern __shared__ unsigned int bd_lds[];           // (BD_CL_TH + 2 R) rows of 16 dwords
    unsigned int t = blockIdx.x;
    const int tx0 = (int)(t % (unsigned)tiles_x) * BD_CL_TW;
    t /= (unsigned)tiles_x;
    const int ty0 = (int)(t % (unsigned)tiles_y) * BD_CL_TH;
    const long long img = t / (unsigned)tiles_y;
    const unsigned char* m = mask + img * H * W;
    const unsigned char* f = from ? from + img * H * W : nullptr;
    const int tid = threadIdx.x;
    unsigned char* stage = reinterpret_cast<unsigned char*>(bd_lds);
    const int rows = BD_CL_TH + 2 * R;
    for (int i = tid; i < rows * BD_CL_TW; i += 256) {
        const int y = ty0 - R + (i >> 6), x = tx0 + (i & (BD_CL_TW - 1));
        int v = 0;
        if (y >= 0 && y < H && x < W) v = bd_value(m, f, (long long)y * W + x, ign);
        stage[i] = (unsigned char)v;
    }
    __syncthreads();
    const int cx = tid & 15, x0 = tx0 + cx * 4;
    if (x0 >= W) return;
#pragma unroll 1
    for (int k = 0; k < BD_CL_TH / 16; ++k) {
        const int ly = (tid >> 4) + 16 * k, y = ty0 + ly;       // a wave: 4 consecutive rows, 64 consecutive dwords
        if (y >= H) break;
        const unsigned int* col = bd_lds + (ly + R) * 16 + cx;
        const unsigned int me = col[0];
        const int up = y < R ? y : R, dn = H - 1 - y < R ? H - 1 - y : R;     // rows that exist
        const int far = up > dn ? up : dn;
        unsigned int gp = (unsigned)(R + 1) * 0x01010101u, found = 0;
#pragma unroll 1
        for (int d = 1; d <= far && found != 0x80808080u; ++d) {
            unsigned int diff = 0;
            if (d <= up) diff |= col[-d * 16] ^ me;
            if (d <= dn) diff |= col[d * 16] ^ me;
            const unsigned int nz = (diff | ((diff & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;     // bit 7 of every non-zero byte
            const unsigned int fresh = nz & ~found;
            const unsigned int sel = (fresh >> 7) * 0xffu;
            gp = (gp & ~sel) | ((unsigned)d * 0x01010101u & sel);
            found |= nz;
        }
        *reinterpret_cast<unsigned int*>(g + (img * H + y) * Wp + x0) = gp;      // x0 + 3 < Wp: the pitch is a multiple of 4
    }
}

// ---- row pass --------------------------------------------------------------------------------------------------------------------------
// one tile row of value | g << 8 words with its halo, index c <-> column tx0 - R + c
__device__ __forceinline__ void bd_stage_rows(unsigned short* rows, int stride, const unsigned char* __restrict__ m, const unsigned char* __restrict__ f,
                                              const unsigned char* __restrict__ g, int H, int W, int Wp, int tx0, int ty0, int R, int ign) {
    // (one flat loop over the rows' words: at a small radius a row is shorter than the block)
#pragma unroll 4
    for (int i = threadIdx.x; i < BD_RW_TH * stride; i += 256) {
        const int r = i / stride, c = i - r * stride;
        const int y = ty0 + r, x = tx0 - R + c;
        int v = 0;
        if (y < H && x >= 0 && x < W) v = bd_value(m, f, (long long)y * W + x, ign) | (int)g[(long long)y * Wp + x] << 8;
        rows[i] = (unsigned short)v;
    }
}

// d2 of the pixel at word `at` of a staged row (column x of the image); -1 at an ignored pixel
__device__ __forceinline__ int bd_row_d2(const unsigned short* at, int x, int W, int R, int ign) {
    const int w0 = at[0], me = w0 & 0xff, g0 = w0 >> 8;
    if (me == ign) return -1;
    const int cap = R * R + 1;
    int best = g0 * g0 < cap ? g0 * g0 : cap;
    const int lf = x < R ? x : R, rt = W - 1 - x < R ? W - 1 - x : R;        // columns that exist
    const int far = lf > rt ? lf : rt;
#pragma unroll 1
    for (int d = 1; d <= far && d * d < best; ++d) {
        if (d <= lf) {
            const int w = at[-d], gg = (w & 0xff) != me ? 0 : w >> 8, c = d * d + gg * gg;
            best = c < best ? c : best;
        }
        if (d <= rt) {
            const int w = at[d], gg = (w & 0xff) != me ? 0 : w >> 8, c = d * d + gg * gg;
            best = c < best ? c : best;
        }
    }
    return best;
}

// what the row pass does with a pixel's d2: write it, or write the weight it selects (pylc_boundary_weights: no int32 map in between)
struct BdStoreD2 {
    int* __restrict__ d2;
    __device__ __forceinline__ void operator()(long long i, int v) const { d2[i] = v; }
};

// table: float [R*R + 2], indexed by d2 in 0..R*R + 1 (which bd_row_d2 never exceeds); an ignored pixel (-1) weighs 0
struct BdStoreWeight {
    const float* __restrict__ table;
    float* __restrict__ out;
    __device__ __forceinline__ void operator()(long long i, int v) const { out[i] = v < 0 ? 0.f : table[v]; }
};

template <typename Epilogue>
__global__ __launch_bounds__(256) void bd_row_kernel(const unsigned char* __restrict__ mask, const unsigned char* __restrict__ from,
                                                     const unsigned char* __restrict__ g, int H, int W, int Wp, int tiles_x, int tiles_y, int R,
                                                     int ign, Epilogue store) {
    extern __shared__ unsigned short bd_rows[];        // BD_RW_TH rows of BD_RW_TW + 2 R words
    unsigned int t = blockIdx.x;
    const int tx0 = (int)(t % (unsigned)tiles_x) * BD_RW_TW;
    t /= (unsigned)tiles_x;
    const int ty0 = (int)(t % (unsigned)tiles_y) * BD_RW_TH;
    const long long img = t / (unsigned)tiles_y;
    const int stride = BD_RW_TW + 2 * R;
    bd_stage_rows(bd_rows, stride, mask + img * H * W, from ? from + img * H * W : nullptr, g + img * H * Wp, H, W, Wp, tx0, ty0, R, ign);
    __syncthreads();
    const int lx = threadIdx.x & (BD_RW_TW - 1), x = tx0 + lx;
    if (x >= W) return;
#pragma unroll 1
    for (int k = 0; k < BD_RW_TH / 2; ++k) {
        const int r = (threadIdx.x >> 7) + 2 * k, y = ty0 + r;
        if (y >= H) break;
        store((img * H + y) * W + x, bd_row_d2(bd_rows + r * stride + R + lx, x, W, R, ign));
    }
}

// the one-launch form over a d2 map that was written out; a value above R*R + 1 (no map of this radius holds one) reads the last cell
__global__ __launch_bounds__(256) void bd_weights_from_d2_kernel(const int* __restrict__ d2, long long N, int cap, const float* __restrict__ table,
                                                                 float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const int v = d2[i];
        out[i] = v < 0 ? 0.f : table[v < cap ? v : cap];
    }
}

// ---- counts ----------------------------------------------------------------------------------------------------------------------------
// counts: [C*C] cm_band[t * C + p], [C] inter, [C] gband, [C] pband, [1] values outside 0..C-1 that are not the ignore label.
// The key of a pixel: -1 (nothing to add), BD_KEY_BAD, or t | p << 8 | prediction is a class << 16 | in truth's band << 17 | in
// prediction's band << 18.
__device__ __forceinline__ int bd_key(int t, int p, int d2t, int d2p, int C, int R2, int ign) {
    if (t == ign) return -1;                           // only pixels with a labelled truth are counted
    if (t >= C || (p >= C && p != ign)) return BD_KEY_BAD;
    const int pv = p != ign;
    const int in_g = d2t <= R2, in_p = pv && d2p >= 0 && d2p <= R2;
    if (!in_g && !in_p) return -1;
    return t | p << 8 | pv << 16 | in_g << 17 | in_p << 18;
}

template <bool LDSH>
__device__ __forceinline__ void bd_add(unsigned int* hist, unsigned long long* counts, int cell, unsigned n) {
    if constexpr (LDSH) atomicAdd(&hist[cell], n);
    else atomicAdd(&counts[cell], (unsigned long long)n);
}

template <bool LDSH>
__device__ __forceinline__ void bd_apply(unsigned int* hist, unsigned long long* counts, int key, unsigned n, int C) {
    const int CC = C * C;
    if (key == BD_KEY_BAD) {
        bd_add<LDSH>(hist, counts, CC + 3 * C, n);
        return;
    }
    const int t = key & 0xff, p = key >> 8 & 0xff;
    const bool pv = key >> 16 & 1, in_g = key >> 17 & 1, in_p = key >> 18 & 1;
    if (in_g && pv) bd_add<LDSH>(hist, counts, t * C + p, n);
    if (in_g && pv && t == p && in_p) bd_add<LDSH>(hist, counts, CC + t, n);
    if (in_g) bd_add<LDSH>(hist, counts, CC + C + t, n);
    if (in_p) bd_add<LDSH>(hist, counts, CC + 2 * C + p, n);
}

// Every lane of the wave must be here (a lane without a pixel brings -1).  The lanes of a wave are consecutive pixels of one row, and masks
// are blobs: equal keys come in runs.  The first lane of every run adds the run's length -- one shuffle and one ballot per wave, and all
// runs' atomics issue together -- instead of one atomic per pixel on a handful of cells.
template <bool LDSH>
__device__ __forceinline__ void bd_tally(unsigned int* hist, unsigned long long* counts, int key, int C) {
    const int lane = threadIdx.x & 63;
    const int left = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || left != key;
    const unsigned long long heads = __ballot(head);
    if (head && key >= 0) {
        const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = after ? __ffsll((long long)after) : 64 - lane;       // up to the next run's first lane, or the end of the wave
        bd_apply<LDSH>(hist, counts, key, (unsigned)len, C);
    }
}

template <bool LDSH>
__device__ __forceinline__ void bd_hist_clear(unsigned int* hist, int C) {
    if constexpr (LDSH) {
        for (int i = threadIdx.x; i < C * C + 3 * C + 1; i += 256) hist[i] = 0;
        __syncthreads();
    }
}

template <bool LDSH>
__device__ __forceinline__ void bd_hist_flush(const unsigned int* hist, unsigned long long* counts, int C) {
    if constexpr (LDSH) {
        __syncthreads();
        for (int i = threadIdx.x; i < C * C + 3 * C + 1; i += 256)
            if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
    }
}

// the row pass of truth and prediction with the counting epilogue.  At most BD_COUNT_GRID blocks take tiles from a device counter, in
// order, until none is left: the LDS counters are flushed once per block and not once per tile (12288 tiles of a 3072 x 4096 photograph
// would send some 200 000 64-bit atomics to the same hundred addresses), and a block that drew tiles deep inside a region, where every scan
// runs the full radius, draws fewer of them.  No thread leaves before the end: the tally is a wave operation, the flush a block one.
template <bool LDSH>
__global__ __launch_bounds__(256) void bd_row_count_kernel(const unsigned char* __restrict__ truth, const unsigned char* __restrict__ pred,
                                                           const unsigned char* __restrict__ g_t, const unsigned char* __restrict__ g_p, int H, int W,
                                                           int Wp, int tiles_x, int tiles_y, unsigned n_tiles, unsigned int* tile_counter, int R,
                                                           int ign, int C, unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned short bd_rows[];        // truth's rows, then the prediction's
    __shared__ unsigned int hist[LDSH ? BD_LDS_CELLS : 1];
    __shared__ unsigned int next_tile;
    const int stride = BD_RW_TW + 2 * R;
    unsigned short* rows_t = bd_rows;
    unsigned short* rows_p = bd_rows + BD_RW_TH * stride;
    bd_hist_clear<LDSH>(hist, C);
    for (;;) {
        if (threadIdx.x == 0) next_tile = atomicAdd(tile_counter, 1u);
        __syncthreads();
        unsigned int t = next_tile;
        if (t >= n_tiles) break;                       // (the same for every thread of the block)
        const int tx0 = (int)(t % (unsigned)tiles_x) * BD_RW_TW;
        t /= (unsigned)tiles_x;
        const int ty0 = (int)(t % (unsigned)tiles_y) * BD_RW_TH;
        const long long img = t / (unsigned)tiles_y;
        const unsigned char* mt = truth + img * H * W;
        const unsigned char* mp = pred + img * H * W;
        const unsigned char* gt = g_t + img * H * Wp;
        const unsigned char* gp = g_p + img * H * Wp;
        // both masks' rows in one loop (bd_stage_rows twice would wait for the first mask's loads before it issued the second's); where
        // the truth is ignored, so is the prediction
#pragma unroll 4
        for (int i = threadIdx.x; i < BD_RW_TH * stride; i += 256) {
            const int r = i / stride, c = i - r * stride;
            const int y = ty0 + r, x = tx0 - R + c;
            int vt = 0, vp = 0;
            if (y < H && x >= 0 && x < W) {
                const long long mi = (long long)y * W + x, gi = (long long)y * Wp + x;
                const int tv = mt[mi], pv = mp[mi];
                vt = tv | (int)gt[gi] << 8;
                vp = (tv == ign ? ign : pv) | (int)gp[gi] << 8;
            }
            rows_t[i] = (unsigned short)vt;
            rows_p[i] = (unsigned short)vp;
        }
        __syncthreads();
        const int lx = threadIdx.x & (BD_RW_TW - 1), x = tx0 + lx;
#pragma unroll 1
        for (int k = 0; k < BD_RW_TH / 2; ++k) {
            const int r = (threadIdx.x >> 7) + 2 * k, y = ty0 + r;
            int key = -1;
            if (x < W && y < H) {
                const unsigned short* at_t = rows_t + r * stride + R + lx;
                const unsigned short* at_p = rows_p + r * stride + R + lx;
                const int tv = at_t[0] & 0xff, pv = at_p[0] & 0xff;
                if (tv != ign) {
                    const int d2t = bd_row_d2(at_t, x, W, R, ign);
                    const int d2p = bd_row_d2(at_p, x, W, R, ign);
                    key = bd_key(tv, pv, d2t, d2p, C, R * R, ign);
                }
            }
            bd_tally<LDSH>(hist, counts, key, C);
        }
        __syncthreads();                               // before the rows are staged anew and next_tile is drawn again
    }
    bd_hist_flush<LDSH>(hist, counts, C);
}

// the two-map form: the same epilogue over d2 maps that were written out
template <bool LDSH>
__global__ __launch_bounds__(256) void bd_count_maps_kernel(const unsigned char* __restrict__ truth, const unsigned char* __restrict__ pred,
                                                            const int* __restrict__ d2_t, const int* __restrict__ d2_p, long long N, int R, int ign,
                                                            int C, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int hist[LDSH ? BD_LDS_CELLS : 1];
    bd_hist_clear<LDSH>(hist, C);
#pragma unroll 1
    for (long long base = (long long)blockIdx.x * 1024; base < N; base += (long long)gridDim.x * 1024) {     // block-uniform
        // the 16 loads of a thread's 4 pixels are issued before the first tally (a pixel past the end re-reads pixel 0 and is not counted)
        int tv[4], pv[4], dt[4], dp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = base + k * 256 + threadIdx.x, j = i < N ? i : 0;
            tv[k] = truth[j]; pv[k] = pred[j]; dt[k] = d2_t[j]; dp[k] = d2_p[j];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool counted = base + k * 256 + threadIdx.x < N && tv[k] != ign;
            bd_tally<LDSH>(hist, counts, counted ? bd_key(tv[k], pv[k], dt[k], dp[k], C, R * R, ign) : -1, C);
        }
    }
    bd_hist_flush<LDSH>(hist, counts, C);
}

}  // namespace pylc

using namespace pylc;

static int bd_pitch(int W) { return (W + 3) & ~3; }

// the arguments every entry point shares; B * H * W < 2^31 keeps the tile counts inside a grid's x dimension
static int bd_check_shape(const char* who, int B, int H, int W, int radius, int ignore_index) {
    PYLC_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W < (1ll << 31), "%s: B=%d H=%d W=%d outside 1 <= B*H*W < 2^31", who, B, H, W);
    PYLC_REQUIRE(radius >= 1 && radius <= BD_MAX_R, "%s: radius=%d outside 1..%d (the column distance is a byte)", who, radius, BD_MAX_R);
    PYLC_REQUIRE(ignore_index >= -1 && ignore_index <= 255, "%s: ignore_index=%d outside -1..255", who, ignore_index);
    return PYLC_OK;
}

static void bd_launch_column(const unsigned char* mask, const unsigned char* from, int B, int H, int W, int R, int ign, unsigned char* g,
                             hipStream_t st) {
    const int tiles_x = cdiv(W, BD_CL_TW), tiles_y = cdiv(H, BD_CL_TH);
    const size_t lds = (size_t)(BD_CL_TH + 2 * R) * BD_CL_TW;
    hipLaunchKernelGGL(bd_column_kernel, dim3((unsigned)((long long)B * tiles_x * tiles_y)), dim3(256), lds, st, mask, from, H, W, bd_pitch(W),
                       tiles_x, tiles_y, R, ign, g);
}

extern "C" size_t pylc_boundary_workspace_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return 0;
    return 2 * (size_t)B * H * bd_pitch(W) + 16;          // two g maps and the tile counter of the counting kernel
}

extern "C" int pylc_boundary_distance(const unsigned char* mask, int B, int H, int W, int radius, int ignore_index, const unsigned char* ignore_from,
                                      int* d2_out, void* workspace, void* stream) {
    PYLC_REQUIRE(mask && d2_out && workspace, "boundary_distance: mask, d2_out or workspace is NULL");
    if (int rc = bd_check_shape("boundary_distance", B, H, W, radius, ignore_index)) return rc;
    PYLC_REQUIRE(!ignore_from || ignore_index >= 0, "boundary_distance: ignore_from without an ignore_index");
    PYLC_REQUIRE(((reinterpret_cast<uintptr_t>(d2_out) | reinterpret_cast<uintptr_t>(workspace)) & 3) == 0,
                 "boundary_distance: d2_out or workspace is not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    unsigned char* g = static_cast<unsigned char*>(workspace);
    bd_launch_column(mask, ignore_from, B, H, W, radius, ignore_index, g, st);
    const int tiles_x = cdiv(W, BD_RW_TW), tiles_y = cdiv(H, BD_RW_TH);
    const size_t lds = (size_t)BD_RW_TH * (BD_RW_TW + 2 * radius) * sizeof(unsigned short);
    hipLaunchKernelGGL(bd_row_kernel<BdStoreD2>, dim3((unsigned)((long long)B * tiles_x * tiles_y)), dim3(256), lds, st, mask, ignore_from, g, H, W,
                       bd_pitch(W), tiles_x, tiles_y, radius, ignore_index, BdStoreD2{d2_out});
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_boundary_weights(const unsigned char* mask, int B, int H, int W, int radius, int ignore_index, const float* table, float* out,
                                     void* workspace, void* stream) {
    PYLC_REQUIRE(mask && table && out && workspace, "boundary_weights: mask, table, out or workspace is NULL");
    if (int rc = bd_check_shape("boundary_weights", B, H, W, radius, ignore_index)) return rc;
    PYLC_REQUIRE(((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 3) == 0,
                 "boundary_weights: table, out or workspace is not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    unsigned char* g = static_cast<unsigned char*>(workspace);
    bd_launch_column(mask, nullptr, B, H, W, radius, ignore_index, g, st);
    const int tiles_x = cdiv(W, BD_RW_TW), tiles_y = cdiv(H, BD_RW_TH);
    const size_t lds = (size_t)BD_RW_TH * (BD_RW_TW + 2 * radius) * sizeof(unsigned short);
    hipLaunchKernelGGL(bd_row_kernel<BdStoreWeight>, dim3((unsigned)((long long)B * tiles_x * tiles_y)), dim3(256), lds, st, mask,
                       static_cast<const unsigned char*>(nullptr), g, H, W, bd_pitch(W), tiles_x, tiles_y, radius, ignore_index,
                       BdStoreWeight{table, out});
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_weights_from_d2(const int* d2, long long N, int radius, const float* table, float* out, void* stream) {
    PYLC_REQUIRE(d2 && table && out, "weights_from_d2: d2, table or out is NULL");
    PYLC_REQUIRE(N >= 1 && N < (1ll << 31), "weights_from_d2: N=%lld outside 1 <= N < 2^31", N);
    PYLC_REQUIRE(radius >= 1 && radius <= BD_MAX_R, "weights_from_d2: radius=%d outside 1..%d", radius, BD_MAX_R);
    PYLC_REQUIRE(((reinterpret_cast<uintptr_t>(d2) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & 3) == 0,
                 "weights_from_d2: d2, table or out is not 4-byte aligned");
    const long long want = cdiv<long long>(N, 256);
    const unsigned blocks = (unsigned)(want < 8 * kNumCU ? want : 8 * kNumCU);
    hipLaunchKernelGGL(bd_weights_from_d2_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d2, N, radius * radius + 1, table, out);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_boundary_counts(const unsigned char* truth, const unsigned char* pred, int B, int H, int W, int n_classes, int radius,
                                    int ignore_index, unsigned long long* counts, void* workspace, void* stream) {
    PYLC_REQUIRE(truth && pred && counts && workspace, "boundary_counts: truth, pred, counts or workspace is NULL");
    if (int rc = bd_check_shape("boundary_counts", B, H, W, radius, ignore_index)) return rc;
    PYLC_REQUIRE(n_classes >= 1 && n_classes <= 255, "boundary_counts: n_classes=%d outside 1..255", n_classes);
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
                 "boundary_counts: counts is not 8-byte or workspace not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    unsigned char* g_t = static_cast<unsigned char*>(workspace);
    unsigned char* g_p = g_t + (size_t)B * H * bd_pitch(W);
    bd_launch_column(truth, nullptr, B, H, W, radius, ignore_index, g_t, st);
    bd_launch_column(pred, ignore_index >= 0 ? truth : nullptr, B, H, W, radius, ignore_index, g_p, st);
    const int tiles_x = cdiv(W, BD_RW_TW), tiles_y = cdiv(H, BD_RW_TH);
    const unsigned n_tiles = (unsigned)((long long)B * tiles_x * tiles_y);
    const unsigned blocks = n_tiles < (unsigned)BD_COUNT_GRID ? n_tiles : (unsigned)BD_COUNT_GRID;
    const size_t lds = 2 * (size_t)BD_RW_TH * (BD_RW_TW + 2 * radius) * sizeof(unsigned short);
    unsigned int* tile_counter = reinterpret_cast<unsigned int*>(g_p + (size_t)B * H * bd_pitch(W));       // (4-byte aligned: the pitch is)
    PYLC_HIP(hipMemsetAsync(tile_counter, 0, sizeof(unsigned int), st));
    if (n_classes <= BD_LDS_MAXC)
        hipLaunchKernelGGL(bd_row_count_kernel<true>, dim3(blocks), dim3(256), lds, st, truth, pred, g_t, g_p, H, W, bd_pitch(W), tiles_x, tiles_y,
                           n_tiles, tile_counter, radius, ignore_index, n_classes, counts);
    else
        hipLaunchKernelGGL(bd_row_count_kernel<false>, dim3(blocks), dim3(256), lds, st, truth, pred, g_t, g_p, H, W, bd_pitch(W), tiles_x, tiles_y,
                           n_tiles, tile_counter, radius, ignore_index, n_classes, counts);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_boundary_counts_maps(const unsigned char* truth, const unsigned char* pred, const int* d2_truth, const int* d2_pred, long long N,
                                         int n_classes, int radius, int ignore_index, unsigned long long* counts, void* stream) {
    PYLC_REQUIRE(truth && pred && d2_truth && d2_pred && counts, "boundary_counts_maps: a pointer is NULL");
    PYLC_REQUIRE(N >= 1 && N < (1ll << 31), "boundary_counts_maps: N=%lld outside 1 <= N < 2^31", N);
    PYLC_REQUIRE(radius >= 1 && radius <= BD_MAX_R, "boundary_counts_maps: radius=%d outside 1..%d", radius, BD_MAX_R);
    PYLC_REQUIRE(ignore_index >= -1 && ignore_index <= 255, "boundary_counts_maps: ignore_index=%d outside -1..255", ignore_index);
    PYLC_REQUIRE(n_classes >= 1 && n_classes <= 255, "boundary_counts_maps: n_classes=%d outside 1..255", n_classes);
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(d2_truth) | reinterpret_cast<uintptr_t>(d2_pred)) & 3) == 0,
                 "boundary_counts_maps: a buffer is not aligned to its element");
    hipStream_t st = as_stream(stream);
    const long long want = cdiv<long long>(N, 1024);
    const unsigned blocks = (unsigned)(want < BD_COUNT_GRID ? want : BD_COUNT_GRID);
    if (n_classes <= BD_LDS_MAXC)
        hipLaunchKernelGGL(bd_count_maps_kernel<true>, dim3(blocks), dim3(256), 0, st, truth, pred, d2_truth, d2_pred, N, radius, ignore_index,
                           n_classes, counts);
    else
        hipLaunchKernelGGL(bd_count_maps_kernel<false>, dim3(blocks), dim3(256), 0, st, truth, pred, d2_truth, d2_pred, N, radius, ignore_index,
                           n_classes, counts);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}
