// Training tile sets from photographs (the reference's `pylc.py extract`: Extractor.extract -> __split -> class_encode -> profile,
// utils/extract.py:106-231, 279-310; utils/profile.py:92-150), the pixel-sized part on the GPU:
//
//   tile_cut_stats_kernel   cuts the tiles of the grid rows = (H - tile) / stride + 1, cols = (W - tile) / stride + 1 (row-major, the
//                           remainder right and below dropped: torch.unfold(0, t, s).unfold(1, t, s) and the reshape at extract.py:302-308)
//                           out of a planar uint8 image and its class-index mask and, in the same pass over the bytes, sums per tile what
//                           the dataset profile needs: sum x and sum x^2 per channel, and the class histogram of the mask.
//                           With no destination it only sums: the statistics of tiles that already exist (pylc_tile_stats).
//
// Everything is integer arithmetic, so the sums are exact and do not depend on how the work is split.  A tile is cut by several blocks, one
// per band of rows (one photograph gives a few dozen tiles only); a band never holds more than 65 536 pixels per plane, so even the band's
// total of x^2 (<= 65 536 * 255^2 = 4 261 478 400) fits 32 bits and the per-thread and per-wave partials are plain dwords.  The waves add
// theirs to 64-bit LDS accumulators and the block sends one 64-bit atomic add per counter to the zero-initialised outputs.  The histogram
// counts in LDS, every thread in a column of its own (ds_add without a return value and without two lanes on one address: masks are
// blobs, a shared counter would serialise the wave).
//
// A lane moves 16 bytes of a tile row at a time.  Source rows start anywhere (the pitch of a photograph is odd as often as not): the lane
// loads the aligned dwords that hold its 16 bytes, one x4 and one more when the address is not a multiple of 4, and shifts them into place
// (v_alignbyte).  Every dword it touches holds at least one byte of the row, so it lies in the same page as that byte.  The store is one
// 16-byte store when the destination is aligned (always when tile % 16 == 0).  The last group of a row whose tile is no multiple of 16,
// and stores to unaligned rows, go byte by byte.
#include "tile_bytes.h"

namespace pylc {

namespace {

constexpr int kDsAutoBandPixels = 8192;        // the default band: 16 rows of a 512 tile, 32 KB of RGB + mask per block

struct TileGeom {
    const unsigned char* img;                  // plane 0 of tile-grid origin (0, 0)
    const unsigned char* mask;                 // NULL: no mask
    long long img_row_step, img_col_step;      // bytes from one grid row / column of tiles to the next
    long long mask_row_step, mask_col_step;
    long long plane_stride;                    // bytes between the channels of one tile's source
    int pitch;                                 // bytes between source rows
    int cols, first_tile;
    int C, tile, band_rows, n_classes;
};

struct __attribute__((packed, aligned(4))) Dwords4 { unsigned int x, y, z, w; };

// 16 bytes from any address (valid == 16), or the first `valid` of them with zeros behind
__device__ __forceinline__ uint4 load_group(const unsigned char* p, int valid) {
    uint4 v;
    if (valid == 16) {
        const unsigned long long a = (unsigned long long)p;
        const unsigned int sh = (unsigned int)a & 3u;
        const unsigned int* q = reinterpret_cast<const unsigned int*>(a - sh);
        const Dwords4 d = *reinterpret_cast<const Dwords4*>(q);
        v.x = d.x; v.y = d.y; v.z = d.z; v.w = d.w;
        if (sh) {
            const unsigned int e = q[4];       // holds byte 15 of the group
            v.x = __builtin_amdgcn_alignbyte(d.y, d.x, sh);
            v.y = __builtin_amdgcn_alignbyte(d.z, d.y, sh);
            v.z = __builtin_amdgcn_alignbyte(d.w, d.z, sh);
            v.w = __builtin_amdgcn_alignbyte(e, d.w, sh);
        }
    } else {
        unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 15; ++k)
            if (k < valid) w[k >> 2] |= (unsigned int)p[k] << (8 * (k & 3));
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    }
    return v;
}

// grid (n_tiles, bands); img_tiles [n][C][t][t] and mask_tiles [n][t][t] may be NULL (statistics only); sums [n][2][C] (sum x, then
// sum x^2), hist [n][n_classes + 1] (the last bin: every value >= n_classes), both zeroed by the caller and indexed from this launch's
// first tile.
__global__ __launch_bounds__(kDsThreads) void tile_cut_stats_kernel(TileGeom g, unsigned char* __restrict__ img_tiles,
                                                                     unsigned char* __restrict__ mask_tiles,
                                                                     unsigned long long* __restrict__ sums,
                                                                     unsigned long long* __restrict__ hist) {
    __shared__ unsigned int cnt[kDsBins * kDsThreads];
    __shared__ unsigned long long acc[6 + kDsBins];
    const int tid = threadIdx.x;
    const long long n = blockIdx.x;
    const int t = g.tile;
    const int r0 = blockIdx.y * g.band_rows;
    const int nr = g.band_rows < t - r0 ? g.band_rows : t - r0;
    const int G = cdiv(t, 16);
    const int items = nr * G;
    const long long gt = (long long)g.first_tile + n;
    const long long ty = gt / g.cols, tx = gt - ty * g.cols;
    const int bins = g.mask ? g.n_classes + 1 : 0;
    if (tid < 6 + kDsBins) acc[tid] = 0;
    for (int b = 0; b < bins; ++b) cnt[b * kDsThreads + tid] = 0;

    unsigned int s[3] = {0u, 0u, 0u}, ss[3] = {0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c < g.C) {
            const unsigned char* src = g.img + c * g.plane_stride + ty * g.img_row_step + tx * g.img_col_step + (long long)r0 * g.pitch;
            unsigned char* dst = img_tiles ? img_tiles + ((n * g.C + c) * t + r0) * t : nullptr;
            for (int j = tid; j < items; j += kDsThreads) {
                const int r = j / G, x0 = (j - r * G) * 16;
                const int valid = t - x0 < 16 ? t - x0 : 16;
                const uint4 v = load_group(src + (long long)r * g.pitch + x0, valid);
                if (dst) store_group(dst + (long long)r * t + x0, v, valid);
                sum_group(v, s[c], ss[c]);
            }
        }
    }
    if (g.mask) {
        const unsigned char* src = g.mask + ty * g.mask_row_step + tx * g.mask_col_step + (long long)r0 * g.pitch;
        unsigned char* dst = mask_tiles ? mask_tiles + (n * t + r0) * t : nullptr;
        const unsigned int top = (unsigned int)g.n_classes;
        for (int j = tid; j < items; j += kDsThreads) {
            const int r = j / G, x0 = (j - r * G) * 16;
            const int valid = t - x0 < 16 ? t - x0 : 16;
            const uint4 v = load_group(src + (long long)r * g.pitch + x0, valid);
            if (dst) store_group(dst + (long long)r * t + x0, v, valid);
            count_group(v, valid, top, cnt);
        }
    }
    __syncthreads();                                       // acc is zero everywhere
    commit_tile_stats(s, ss, cnt, acc, g.C, bins, n, sums, hist);
}

int launch(const TileGeom& g0, int n_tiles, int band_rows, unsigned char* img_tiles, unsigned char* mask_tiles, unsigned long long* sums,
           unsigned long long* hist, void* stream, const char* who) {
    TileGeom g = g0;
    const int t = g.tile;
    if (band_rows <= 0) {
        band_rows = kDsAutoBandPixels / t;
        band_rows = band_rows < 1 ? 1 : (band_rows > t ? t : band_rows);
    }
    PYLC_REQUIRE(band_rows <= t && (long long)band_rows * t <= kDsBandPixels, "%s: band_rows=%d x tile %d exceeds %d pixels per block", who,
                 band_rows, t, kDsBandPixels);
    g.band_rows = band_rows;
    const int bands = cdiv(t, band_rows);
    PYLC_REQUIRE(bands <= 65535, "%s: %d row bands exceed the launch grid", who, bands);
    hipLaunchKernelGGL(tile_cut_stats_kernel, dim3((unsigned)n_tiles, (unsigned)bands), dim3(kDsThreads), 0, as_stream(stream), g, img_tiles,
                       mask_tiles, sums, hist);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

}  // namespace
}  // namespace pylc

using namespace pylc;

extern "C" int pylc_extract_tiles(const unsigned char* img, int Cimg, int H, int W, const unsigned char* mask, int n_classes, int tile,
                                  int stride, int first_tile, int n_tiles, int band_rows, unsigned char* img_tiles,
                                  unsigned char* mask_tiles, unsigned long long* sums, unsigned long long* hist, void* stream) {
    PYLC_REQUIRE((Cimg == 1 || Cimg == 3) && H > 0 && W > 0, "extract_tiles: bad arguments");
    PYLC_REQUIRE(tile > 0 && tile <= kDsBandPixels && stride > 0, "extract_tiles: tile=%d stride=%d", tile, stride);
    PYLC_REQUIRE(tile <= H && tile <= W, "extract_tiles: tile %d exceeds the image %dx%d (HxW)", tile, H, W);
    PYLC_REQUIRE((long long)H * W * Cimg < (1LL << 31), "extract_tiles: image too large");
    PYLC_REQUIRE(!mask || (n_classes >= 1 && n_classes <= PYLC_MAX_CLASSES), "extract_tiles: n_classes=%d outside 1..%d", n_classes,
                 PYLC_MAX_CLASSES);
    const int rows = (H - tile) / stride + 1, cols = (W - tile) / stride + 1;
    PYLC_REQUIRE(first_tile >= 0 && n_tiles >= 0 && (long long)first_tile + n_tiles <= (long long)rows * cols,
                 "extract_tiles: tiles %d..%lld outside the %dx%d grid", first_tile, (long long)first_tile + n_tiles - 1, rows, cols);
    if (n_tiles == 0) return PYLC_OK;
    PYLC_REQUIRE(img && img_tiles && sums && (!mask || (mask_tiles && hist)), "extract_tiles: a NULL image, tile or statistics pointer");
    TileGeom g;
    g.img = img; g.mask = mask;
    g.img_row_step = g.mask_row_step = (long long)stride * W;
    g.img_col_step = g.mask_col_step = stride;
    g.plane_stride = (long long)H * W;
    g.pitch = W;
    g.cols = cols; g.first_tile = first_tile;
    g.C = Cimg; g.tile = tile; g.band_rows = 0; g.n_classes = n_classes;
    return launch(g, n_tiles, band_rows, img_tiles, mask ? mask_tiles : nullptr, sums, hist, stream, "extract_tiles");
}

extern "C" int pylc_tile_stats(const unsigned char* img_tiles, long long n_tiles, int Cimg, int tile, const unsigned char* mask_tiles,
                               int n_classes, int band_rows, unsigned long long* sums, unsigned long long* hist, void* stream) {
    PYLC_REQUIRE(Cimg == 1 || Cimg == 3, "tile_stats: bad arguments");
    PYLC_REQUIRE(tile > 0 && tile <= kDsBandPixels, "tile_stats: tile=%d", tile);
    PYLC_REQUIRE(n_tiles >= 0 && n_tiles < (1LL << 31), "tile_stats: n_tiles=%lld", n_tiles);
    PYLC_REQUIRE(!mask_tiles || (n_classes >= 1 && n_classes <= PYLC_MAX_CLASSES), "tile_stats: n_classes=%d outside 1..%d", n_classes,
                 PYLC_MAX_CLASSES);
    if (n_tiles == 0) return PYLC_OK;
    PYLC_REQUIRE(img_tiles && sums && (!mask_tiles || hist), "tile_stats: a NULL tile or statistics pointer");
    TileGeom g;
    g.img = img_tiles; g.mask = mask_tiles;
    g.img_row_step = (long long)Cimg * tile * tile;
    g.mask_row_step = (long long)tile * tile;
    g.img_col_step = g.mask_col_step = 0;
    g.plane_stride = (long long)tile * tile;
    g.pitch = tile;
    g.cols = 1; g.first_tile = 0;
    g.C = Cimg; g.tile = tile; g.band_rows = 0; g.n_classes = n_classes;
    return launch(g, (int)n_tiles, band_rows, nullptr, nullptr, sums, hist, stream, "tile_stats");
}
