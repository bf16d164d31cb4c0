// The tile cutter of full-image inference: ONE kernel behind the five pylc_image_pack_tiles* entry points (DESIGN.md sections 5.4, 5.10).
//
//   tiles [n][tile][tile][4] <- the windows first .. first+n-1 (row-major tile order) of img [Cimg][H][W] (raw 0..255, float or uint8),
//   normalised ((v - m) / s) / 255, channel 3 = 0, one channel copied into three (Extractor.__split utils/extract.py:279-310 +
//   Model.normalize_image models/model.py:416-445, fused).
//
// The geometry is overlap_geom.h's: tile (i, j) of a grid `cols` wide covers the `out` square at o = min(i*stride, n - out) and reads the
// window `pad = (tile - out) / 2` wider on every side, mirrored (reflect-101) beyond the image; flip = 1 reads column tile-1-c0 for
// column c0.  The two grids the entry points offer are cases of it:
//
//   fitted (pylc_image_pack_tiles, _ex, _flip)       out = tile, rows = (H - tile) / stride + 1, cols = (W - tile) / stride + 1, the
//                                                     remainder right and below dropped: the origins i*stride never reach the clamp,
//                                                     the windows never leave the image
//   any size (pylc_image_pack_tiles_reflect, _ex)    rows = overlap_count(H, out, stride), cols = overlap_count(W, out, stride)
//
// Each entry point is its own argument checks, then launch_cut_tiles.  A bandwidth kernel: 1-12 B read, 16 B written per window pixel.
#include <type_traits>

#include "common.h"
#include "overlap_geom.h"

namespace pylc {

namespace {

template <bool U8>
__global__ __launch_bounds__(256) void cut_tiles_kernel(const void* __restrict__ img_, int Cimg, int H, int W, int tile, int out, int stride,
                                                         int cols, int first, int count, int flip, float m0, float m1, float m2,
                                                         float s0, float s1, float s2, float* __restrict__ tiles) {
    typedef typename std::conditional<U8, unsigned char, float>::type T;
    const T* __restrict__ img = static_cast<const T*>(img_);
    const int pad = (tile - out) / 2;
    const long long total = (long long)count * tile * tile;
    const size_t plane = (size_t)H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % tile);
        const long long t = i / tile;
        const int r = (int)(t % tile);
        const int k = first + (int)(t / tile);
        const int cs = flip ? tile - 1 - c0 : c0;
        const int y = reflect101(overlap_origin(k / cols, H, out, stride) - pad + r, H);
        const int x = reflect101(overlap_origin(k % cols, W, out, stride) - pad + cs, W);
        const T* src = img + (size_t)y * W + x;
        const float a = (float)src[0];
        const float b = Cimg == 3 ? (float)src[plane] : a;
        const float c = Cimg == 3 ? (float)src[2 * plane] : a;
        ot_f32x4 v;
        v.x = ((a - m0) / s0) / 255.f;
        v.y = ((b - m1) / s1) / 255.f;
        v.z = ((c - m2) / s2) / 255.f;
        v.w = 0.f;
        *reinterpret_cast<ot_f32x4*>(tiles + 4 * i) = v;
    }
}

// the caller has checked the arguments: every window lies within `pad` of the image, first .. first + n - 1 within the grid
int launch_cut_tiles(const void* img, int is_u8, int Cimg, int H, int W, int tile, int out, int stride, int cols, int first, int n, int flip,
                     const float* mean3, const float* std3, float* tiles, void* stream) {
    const int blocks = ot_grid((long long)n * tile * tile);
    const auto kernel = is_u8 ? cut_tiles_kernel<true> : cut_tiles_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, as_stream(stream), img, Cimg, H, W, tile, out, stride, cols, first, n, flip, mean3[0],
                       mean3[1], mean3[2], std3[0], std3[1], std3[2], tiles);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

bool tile_range_ok(int first, int n, int rows, int cols) { return first >= 0 && n > 0 && (long long)first + n <= (long long)rows * cols; }

// the fitted sliding-window grid (an unfitted image loses its remainder right and below)
int cut_fitted(const char* who, const void* img, int is_u8, int Cimg, int H, int W, int tile, int stride, int first, int n, int flip,
               const float* mean3, const float* std3, float* tiles, void* stream) {
    PYLC_REQUIRE(img && tiles && mean3 && std3 && (Cimg == 1 || Cimg == 3) && tile > 0 && stride > 0 && H >= tile && W >= tile &&
                     (flip == 0 || flip == 1),
                 "%s: bad arguments", who);
    const int rows = (H - tile) / stride + 1, cols = (W - tile) / stride + 1;
    PYLC_REQUIRE(tile_range_ok(first, n, rows, cols), "%s: tile range outside the image", who);
    return launch_cut_tiles(img, is_u8, Cimg, H, W, tile, tile, stride, cols, first, n, flip, mean3, std3, tiles, stream);
}

// the any-size grid of mirrored windows; pad0: tile == out is accepted
int cut_overlap(const char* who, bool pad0, const void* img, int is_u8, int Cimg, int H, int W, int tile, int out, int stride, int first, int n,
                int flip, const float* mean3, const float* std3, float* tiles, void* stream) {
    PYLC_REQUIRE(img && tiles && mean3 && std3 && (Cimg == 1 || Cimg == 3) && (pad0 ? tile >= out : tile > out) && (tile - out) % 2 == 0 &&
                     (flip == 0 || flip == 1),
                 "%s: bad arguments", who);
    if (int rc = overlap_check(who, H, W, out, stride, (tile - out) / 2)) return rc;
    const int rows = overlap_count(H, out, stride), cols = overlap_count(W, out, stride);
    PYLC_REQUIRE(tile_range_ok(first, n, rows, cols), "%s: tiles %d..%d outside the %dx%d grid", who, first, first + n - 1, rows, cols);
    return launch_cut_tiles(img, is_u8, Cimg, H, W, tile, out, stride, cols, first, n, flip, mean3, std3, tiles, stream);
}

}  // namespace
}  // namespace pylc

using namespace pylc;

extern "C" int pylc_image_pack_tiles(const float* img, int Cimg, int H, int W, int tile, int stride, int first_tile, int n_tiles,
                                     const float* mean3, const float* std3, float* out, void* stream) {
    return cut_fitted("image_pack_tiles", img, 0, Cimg, H, W, tile, stride, first_tile, n_tiles, 0, mean3, std3, out, stream);
}

// a uint8 sample converts to the float of the same value exactly, so equal pixel values give bit-identical tiles
extern "C" int pylc_image_pack_tiles_ex(const void* img, int is_u8, int Cimg, int H, int W, int tile, int stride, int first_tile, int n_tiles,
                                        const float* mean3, const float* std3, float* out, void* stream) {
    return cut_fitted(is_u8 ? "image_pack_tiles_ex" : "image_pack_tiles", img, is_u8, Cimg, H, W, tile, stride, first_tile, n_tiles, 0, mean3,
                      std3, out, stream);
}

extern "C" int pylc_image_pack_tiles_flip(const void* img, int is_u8, int Cimg, int H, int W, int tile, int stride, int first_tile, int n_tiles,
                                          const float* mean3, const float* std3, float* out, void* stream, int flip) {
    return cut_fitted("image_pack_tiles_flip", img, is_u8, Cimg, H, W, tile, stride, first_tile, n_tiles, flip, mean3, std3, out, stream);
}

extern "C" int pylc_image_pack_tiles_reflect(const void* img, int is_u8, int Cimg, int H, int W, int tile, int out, int stride, int first_tile,
                                             int n_tiles, const float* mean3, const float* std3, float* tiles, void* stream) {
    return cut_overlap("image_pack_tiles_reflect", false, img, is_u8, Cimg, H, W, tile, out, stride, first_tile, n_tiles, 0, mean3, std3, tiles,
                       stream);
}

extern "C" int pylc_image_pack_tiles_reflect_ex(const void* img, int is_u8, int Cimg, int H, int W, int tile, int out, int stride,
                                                int first_tile, int n_tiles, const float* mean3, const float* std3, float* tiles,
                                                void* stream, int flip) {
    return cut_overlap("image_pack_tiles_reflect_ex", true, img, is_u8, Cimg, H, W, tile, out, stride, first_tile, n_tiles, flip, mean3, std3,
                       tiles, stream);
}
