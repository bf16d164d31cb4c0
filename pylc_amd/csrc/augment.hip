// The augmentation transform of `pylc.py augment` (augment_transform -> perspective_shift + channel_shift, utils/tools.py:452-594; called
// by Augmentor.oversample, utils/augment.py:184-239) on uint8 tiles, with the per-tile statistics of the dataset profile in the same pass.
//
// What the reference does to a float32 image tile and an integer mask tile of side t, given the 3 x 3 matrix M of its four drawn points:
//   1. cv2.warpPerspective(M, INTER_AREA -- which warpPerspective treats as linear -- for the image, INTER_NEAREST for the mask,
//      BORDER_REFLECT_101): per warped pixel (x, y), with Minv = inv(M), all in double and every operation rounded on its own,
//          X0 = Minv00 x + Minv01 y + Minv02, Y0 likewise, W = Minv20 x + Minv21 y + Minv22, W = W ? q / W : 0, fX = X0 W, fY = Y0 W
//      mask  (q = 1):  warped = mask[refl(rint(fY))][refl(rint(fX))]
//      image (q = 32): X = rint(fX), sx = X >> 5, ax = X & 31, likewise Y; the four taps refl(sy), refl(sy + 1) x refl(sx), refl(sx + 1)
//                      weighted by (32 - ax | ax) (32 - ay | ay) / 1024: an integer N <= 255 * 1024 over 1024, exact in fp32.
//   2. crop [30 : t - 30]^2 and cv2.resize back to t: nearest for the mask (s = min(floor(d * scale), t - 61), scale = 1 / (t / (t - 60))
//      in double), and for the image OpenCV's linear kernel in area mode: s = floor(d * scale), f = float((d + 1) - (s + 1) * (t / (t - 60))),
//      f = f <= 0 ? 0 : f - floor(f), (s + 1 >= t - 60: f = 0, s = t - 61), a[s] * (1.0f - f) + a[s + 1] * f along the rows first, then the
//      same down the columns of the row results -- fp32, every multiply and add rounded on its own (no FMA: see DESIGN.md section 5.6).
//   3. np.int16 (truncation), + shift, clip to 0..255, uint8.
//
// One evaluation of the homography serves the image and the mask: 32 / W and 1 / W round alike (a power of two scales exactly), so the
// mask's fX is the image's fX / 32 bit for bit, and the nearest resize reads the same cropped rows and columns s that the linear one does.
//
// augment_kernel: grid (copies, bands of output rows), 256 threads.  A block walks its band in steps of a few output rows.  For each step
// it computes the warped rows the step needs that it has not computed yet -- every warped pixel ONCE: one fp64 homography, four source
// gathers per channel and one for the mask -- into a ring of warped rows in LDS (fp32 per channel, one byte of mask), then runs the two
// fp32 passes from LDS, 16 output bytes per lane, stores them (tile_bytes.h: one 16-byte store where the destination is aligned) and sums
// them like tile_cut_stats_kernel does.  The ring makes the rows two steps share cost nothing, so only a band's first rows are computed by
// two blocks.  The source pixels are gathered from global memory (neighbouring lanes read neighbouring bytes; the tile was just written or
// read and sits in L2).
#include "tile_bytes.h"

#pragma clang fp contract(off)

namespace pylc {

namespace {

constexpr int kAugMinTile = 128;               // the crop needs t - 60 > 0 with margin; the reference's points lie in a 512 tile
constexpr int kAugMaxTile = 1024;              // three warped rows of (t - 60) x (3 fp32 + 1 byte) fit the ring
constexpr int kAugRingWords = 10240;           // 40 KB: 6 warped rows of a 512 RGB tile
constexpr int kAugAutoBandPixels = 16384;      // the default band: 32 rows of a 512 tile
constexpr int kAugCrop = 30;

struct AugArgs {
    const unsigned char* img;                  // [n_src][C][t][t]
    const unsigned char* mask;                 // [n_src][t][t] or NULL
    const int* src_index;                      // [m]
    const double* minv;                        // [m][9]
    const int* shift;                          // [m]
    unsigned char* out_img;                    // [m][C][t][t]
    unsigned char* out_mask;                   // [m][t][t] or NULL
    unsigned long long* sums;                  // [m][2][C] or NULL
    unsigned long long* hist;                  // [m][n_classes + 1] or NULL
    long long n_src;
    int C, tile, band_rows, n_classes, ring_rows;
};

// BORDER_REFLECT_101: p < 0 -> -p, p >= t -> 2t - 2 - p, until in range
__device__ __forceinline__ int refl(int p, int t) {
    if ((unsigned)p < (unsigned)t) return p;
    const int period = 2 * t - 2;
    p = (p < 0 ? -p : p) % period;
    return p < t ? p : period - p;
}

// rint of a coordinate as an int; far-off and NaN coordinates end at +-2^30 (OpenCV saturates at the int range: as far outside any tile)
__device__ __forceinline__ int round_coord(double f) { return (int)rint(fmin(fmax(f, -1073741824.0), 1073741824.0)); }

__global__ __launch_bounds__(kDsThreads) void augment_kernel(AugArgs a) {
    __shared__ unsigned int ring[kAugRingWords];
    __shared__ unsigned int cnt[kDsBins * kDsThreads];
    __shared__ unsigned long long acc[6 + kDsBins];
    __shared__ float res_f[kAugMaxTile];                   // the resize's fraction and cropped index per output row / column
    __shared__ unsigned short res_s[kAugMaxTile];
    const int tid = threadIdx.x;
    const long long n = blockIdx.x;
    const int t = a.tile, wc = t - 2 * kAugCrop, C = a.C;
    const long long src = a.src_index[n];
    if (src < 0 || src >= a.n_src) return;                 // the caller's error; nothing is read or written for this copy
    const int r0 = blockIdx.y * a.band_rows;
    const int r1 = r0 + a.band_rows < t ? r0 + a.band_rows : t;
    const int G = cdiv(t, 16);
    const bool with_mask = a.mask != nullptr;
    const int bins = a.hist ? a.n_classes + 1 : 0;
    const int R = a.ring_rows;
    float* const wimg = reinterpret_cast<float*>(ring);                                    // [C][R][wc]
    unsigned char* const wmask = reinterpret_cast<unsigned char*>(ring + C * R * wc);      // [R][wc]
    const unsigned char* const simg = a.img + src * C * t * t;
    const unsigned char* const smask = with_mask ? a.mask + src * t * t : nullptr;
    double M[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = a.minv[n * 9 + k];
    const int shift = a.shift[n];

    if (tid < 6 + kDsBins) acc[tid] = 0;
    for (int b = 0; b < bins; ++b) cnt[b * kDsThreads + tid] = 0;
    const double inv = (double)t / (double)wc, scale = 1.0 / inv;
    for (int d = tid; d < t; d += kDsThreads) {
        int s = (int)floor(d * scale);
        float f = (float)((double)(d + 1) - (double)(s + 1) * inv);
        f = f <= 0.f ? 0.f : f - floorf(f);
        if (s + 1 >= wc) { f = 0.f; s = wc - 1; }
        res_f[d] = f;
        res_s[d] = (unsigned short)s;
    }
    __syncthreads();

    unsigned int s[3] = {0u, 0u, 0u}, ss[3] = {0u, 0u, 0u};
    int done = -1;                                         // the last warped (cropped) row in the ring
    for (int d0 = r0; d0 < r1;) {
        // the step: output rows d0..d1 whose cropped rows lo..hi fit the ring
        const int lo = res_s[d0];
        int d1 = d0;
        while (d1 + 1 < r1 && min((int)res_s[d1 + 1] + 1, wc - 1) - lo < R) ++d1;
        const int hi = min((int)res_s[d1] + 1, wc - 1);
        const int from = lo > done + 1 ? lo : done + 1;
        for (int i = tid; i < (hi - from + 1) * wc; i += kDsThreads) {
            const int wr = i / wc, wy = from + wr, wx = i - wr * wc;
            const double x = (double)(wx + kAugCrop), y = (double)(wy + kAugCrop);
            const double X0 = (M[0] * x + M[1] * y) + M[2];
            const double Y0 = (M[3] * x + M[4] * y) + M[5];
            double W = (M[6] * x + M[7] * y) + M[8];
            W = W != 0.0 ? 32.0 / W : 0.0;
            const double fX = X0 * W, fY = Y0 * W;
            const int slot = (wy % R) * wc + wx;
            const int X = round_coord(fX), Y = round_coord(fY);
            const int ax = X & 31, ay = Y & 31;
            const int x0 = refl(X >> 5, t), x1 = refl((X >> 5) + 1, t);
            const int y0 = refl(Y >> 5, t) * t, y1 = refl((Y >> 5) + 1, t) * t;
            const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c < C) {
                    const unsigned char* p = simg + (long long)c * t * t;
                    const int N = w00 * p[y0 + x0] + w01 * p[y0 + x1] + w10 * p[y1 + x0] + w11 * p[y1 + x1];
                    wimg[c * R * wc + slot] = (float)N * 0.0009765625f;
                }
            }
            if (with_mask) wmask[slot] = smask[refl(round_coord(fY * 0.03125), t) * t + refl(round_coord(fX * 0.03125), t)];
        }
        done = hi;
        __syncthreads();

        const int items = (d1 - d0 + 1) * G;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < C) {
                const float* plane = wimg + c * R * wc;
                unsigned char* dst = a.out_img + ((n * C + c) * t) * t;
                for (int j = tid; j < items; j += kDsThreads) {
                    const int r = j / G, xg = (j - r * G) * 16, d = d0 + r;
                    const int valid = t - xg < 16 ? t - xg : 16;
                    const int sy = res_s[d];
                    const float fy = res_f[d], gy = 1.0f - fy;
                    const float* ra = plane + (sy % R) * wc;
                    const float* rb = plane + (min(sy + 1, wc - 1) % R) * wc;
                    unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        if (k < valid) {
                            const int sx = res_s[xg + k], sx1 = min(sx + 1, wc - 1);
                            const float fx = res_f[xg + k], gx = 1.0f - fx;
                            const float top = ra[sx] * gx + ra[sx1] * fx;
                            const float bot = rb[sx] * gx + rb[sx1] * fx;
                            const int q = (int)(top * gy + bot * fy) + shift;          // np.int16: towards zero
                            w[k >> 2] |= (unsigned int)(q < 0 ? 0 : (q > 255 ? 255 : q)) << (8 * (k & 3));
                        }
                    }
                    const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
                    store_group(dst + (long long)d * t + xg, v, valid);
                    sum_group(v, s[c], ss[c]);
                }
            }
        }
        if (with_mask) {
            unsigned char* dst = a.out_mask ? a.out_mask + n * t * t : nullptr;
            const unsigned int top = (unsigned int)a.n_classes;
            for (int j = tid; j < items; j += kDsThreads) {
                const int r = j / G, xg = (j - r * G) * 16, d = d0 + r;
                const int valid = t - xg < 16 ? t - xg : 16;
                const unsigned char* row = wmask + ((int)res_s[d] % R) * wc;
                unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < valid) w[k >> 2] |= (unsigned int)row[res_s[xg + k]] << (8 * (k & 3));
                const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
                if (dst) store_group(dst + (long long)d * t + xg, v, valid);
                if (bins) count_group(v, valid, top, cnt);
            }
        }
        __syncthreads();                                   // the next step overwrites ring rows this one read
        d0 = d1 + 1;
    }
    commit_tile_stats(s, ss, cnt, acc, C, bins, n, a.sums, a.hist);
}

}  // namespace
}  // namespace pylc

using namespace pylc;

extern "C" int pylc_augment_tiles(const unsigned char* img_tiles, const unsigned char* mask_tiles, long long n_src, int Cimg, int tile,
                                  const int* src_index, const double* minv, const int* shift, long long m, int band_rows,
                                  unsigned char* out_img, unsigned char* out_mask, int n_classes, unsigned long long* sums,
                                  unsigned long long* hist, void* stream) {
    PYLC_REQUIRE(Cimg == 1 || Cimg == 3, "augment_tiles: Cimg=%d, not 1 or 3", Cimg);
    PYLC_REQUIRE(tile >= kAugMinTile && tile <= kAugMaxTile, "augment_tiles: tile=%d outside %d..%d", tile, kAugMinTile, kAugMaxTile);
    PYLC_REQUIRE(n_src > 0 && m >= 0 && m < (1LL << 31), "augment_tiles: n_src=%lld m=%lld", n_src, m);
    PYLC_REQUIRE(!hist || (n_classes >= 1 && n_classes <= PYLC_MAX_CLASSES), "augment_tiles: n_classes=%d outside 1..%d", n_classes,
                 PYLC_MAX_CLASSES);
    if (band_rows <= 0) {
        band_rows = kAugAutoBandPixels / tile;
        band_rows = band_rows < 1 ? 1 : (band_rows > tile ? tile : band_rows);
    }
    PYLC_REQUIRE(band_rows <= tile && (long long)band_rows * tile <= kDsBandPixels, "augment_tiles: band_rows=%d x tile %d exceeds %d pixels per block",
                 band_rows, tile, kDsBandPixels);
    if (m == 0) return PYLC_OK;
    PYLC_REQUIRE(img_tiles && src_index && minv && shift && out_img, "augment_tiles: a NULL tile, index, matrix, shift or output pointer");
    PYLC_REQUIRE(mask_tiles || (!out_mask && !hist), "augment_tiles: mask output or histogram without mask tiles");
    AugArgs a;
    a.img = img_tiles; a.mask = (out_mask || hist) ? mask_tiles : nullptr;
    a.src_index = src_index; a.minv = minv; a.shift = shift;
    a.out_img = out_img; a.out_mask = out_mask; a.sums = sums; a.hist = hist;
    a.n_src = n_src;
    a.C = Cimg; a.tile = tile; a.band_rows = band_rows; a.n_classes = n_classes;
    const int wc = tile - 2 * kAugCrop;
    a.ring_rows = kAugRingWords * 4 / (wc * (4 * Cimg + 1));           // >= 3 up to kAugMaxTile
    if (a.ring_rows > wc) a.ring_rows = wc;
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)m, (unsigned)cdiv(tile, band_rows)), dim3(kDsThreads), 0, as_stream(stream), a);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}
