// The streaming mean-probability blend: overlap_tile.hip's blend -- every pixel's score is the mean of the
// softmax probabilities of the tiles that cover it -- taken batch by batch into one fp32 accumulation image instead of from every logit
// tile at once, for any number of ensemble members, and the mirrored tile cutters of the horizontal-flip member.
//
//   blend_accumulate_kernel<C>  acc[y][x][c] += softmax(tile logits at that pixel)[c] over the batch's tiles that cover the pixel, in
//                               ascending tile index.  Gather form: one lane per pixel of the batch's bounding box, lanes along x, the
//                               pixel's acc vector loaded once, added to in registers and stored once (16-byte accesses, no atomics).
//                               Tile index ascends within a batch and from batch to batch, so after a member's last batch acc holds,
//                               bit for bit, the sums stitch_overlap_kernel forms in registers: independent of the batch size.
//   blend_finalize_kernel<C, 1> p[c] = acc[c] / (members * covering tiles) -- the count comes from the geometry, no count buffer --
//                               class = first maximum; mask (four pixels per lane, one dword), optional probs [C][H][W], conf [H][W].
//                               (blend_finalize.h: multiscale.hip's ensemble finalizer is the same body with one divisor.)
//   pack_tiles_flip_kernel      pack_tiles_kernel / pack_tiles_reflect_kernel with an optional mirror along x (column c0 of a window
//                               reads the window's column tile-1-c0) and pad = 0 allowed.
//
// The geometry is overlap_geom.h's: o_i = min(i*stride, n - out); the fitted sliding-window grid of stitch.hip is the case out = tile
// in which the clamp is never active.  Bandwidth kernels: no LDS, no MFMA.
#include <type_traits>

#include "blend_finalize.h"
#include "common.h"
#include "overlap_geom.h"

namespace pylc {

namespace {

// the pixels [y0, y0 + bh) x [x0, x0 + bw) that the tiles first .. first + count - 1 can touch
struct BlendBox { int y0, x0, bh, bw; };

template <int C>
__global__ __launch_bounds__(256) void blend_accumulate_kernel(const float* __restrict__ logits, BlendGeom g, BlendBox box, int first, int count,
                                                                int flip, float* __restrict__ acc) {
    constexpr int NV = (C + 3) / 4;
    const long long total = (long long)box.bh * box.bw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int by = (int)(i / box.bw);
        const int y = box.y0 + by, x = box.x0 + (int)(i - (long long)by * box.bw);
        const Cover cy = overlap_cover(y, g.H, g.out, g.stride, g.rows);
        const Cover cx = overlap_cover(x, g.W, g.out, g.stride, g.cols);
        ot_f32x4* dst = reinterpret_cast<ot_f32x4*>(acc + ((size_t)y * g.W + x) * g.acc_pitch);
        float a[NV * 4];
        bool loaded = false;
        for (int ia = cy.lo; ia <= cy.hi + cy.last; ++ia) {
            const int ti = ia <= cy.hi ? ia : g.rows - 1;
            const int ly = y - overlap_origin(ti, g.H, g.out, g.stride);
            for (int ib = cx.lo; ib <= cx.hi + cx.last; ++ib) {
                const int tj = ib <= cx.hi ? ib : g.cols - 1;
                const int k = ti * g.cols + tj - first;              // the tile's place in this batch
                if (k < 0 || k >= count) continue;
                if (!loaded) {
#pragma unroll
                    for (int q = 0; q < NV; ++q) {
                        const ot_f32x4 t = dst[q];
                        a[4 * q] = t.x; a[4 * q + 1] = t.y; a[4 * q + 2] = t.z; a[4 * q + 3] = t.w;
                    }
                    loaded = true;
                }
                int lx = x - overlap_origin(tj, g.W, g.out, g.stride);
                lx = flip ? g.out - 1 - lx : lx;
                const ot_f32x4* src = reinterpret_cast<const ot_f32x4*>(logits + (((size_t)k * g.out + ly) * g.out + lx) * g.pitch);
                float v[NV * 4];
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    const ot_f32x4 t = src[q];
                    v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
                }
                // stitch_overlap_kernel's softmax, operation for operation
                float m = v[0];
#pragma unroll
                for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) { v[c] = expf(v[c] - m); s += v[c]; }
                const float inv = 1.f / s;
#pragma unroll
                for (int c = 0; c < C; ++c) a[c] += v[c] * inv;
            }
        }
        if (loaded) {                     // a pixel of the box that no tile of the batch covers is not written
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                ot_f32x4 t;
                t.x = a[4 * q]; t.y = a[4 * q + 1]; t.z = a[4 * q + 2]; t.w = a[4 * q + 3];
                dst[q] = t;
            }
        }
    }
}

// tiles [count][tile][tile][4] <- normalised windows of img [Cimg][H][W] (raw 0..255), tiles first .. first+count-1 of a grid `cols`
// wide whose origins are min(i*stride, n - out), the window `pad` wider on every side and mirrored (reflect-101) beyond the image.
// flip: column c0 of the window is read at tile-1-c0.  pack_tiles_kernel's arithmetic, ((v - m) / s) / 255, channel 3 = 0.
template <bool U8>
__global__ __launch_bounds__(256) void pack_tiles_flip_kernel(const void* __restrict__ img_, int Cimg, int H, int W, int tile, int out, int stride,
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

int launch_pack_flip(const void* img, int is_u8, int Cimg, int H, int W, int tile, int out, int stride, int cols, int first_tile, int n_tiles,
                     int flip, const float* mean3, const float* std3, float* tiles, void* stream) {
    const long long total = (long long)n_tiles * tile * tile;
    hipStream_t st = as_stream(stream);
    if (is_u8)
        hipLaunchKernelGGL(pack_tiles_flip_kernel<true>, dim3(ot_grid(total)), dim3(256), 0, st, img, Cimg, H, W, tile, out, stride, cols,
                           first_tile, n_tiles, flip, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], tiles);
    else
        hipLaunchKernelGGL(pack_tiles_flip_kernel<false>, dim3(ot_grid(total)), dim3(256), 0, st, img, Cimg, H, W, tile, out, stride, cols,
                           first_tile, n_tiles, flip, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], tiles);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

}  // namespace
}  // namespace pylc

using namespace pylc;

// pylc_image_pack_tiles_ex with a mirror: the fitted grid rows = (H - tile) / stride + 1, cols = (W - tile) / stride + 1 (the remainder
// right and below is dropped), whose origins i*stride never reach the clamp of the shared geometry.
extern "C" int pylc_image_pack_tiles_flip(const void* img, int is_u8, int Cimg, int H, int W, int tile, int stride, int first_tile, int n_tiles,
                                          const float* mean3, const float* std3, float* out, void* stream, int flip) {
    PYLC_REQUIRE(img && out && mean3 && std3 && (Cimg == 1 || Cimg == 3) && tile > 0 && stride > 0 && H >= tile && W >= tile &&
                     (flip == 0 || flip == 1),
                 "image_pack_tiles_flip: bad arguments");
    const int rows = (H - tile) / stride + 1, cols = (W - tile) / stride + 1;
    PYLC_REQUIRE(first_tile >= 0 && n_tiles > 0 && (long long)first_tile + n_tiles <= (long long)rows * cols,
                 "image_pack_tiles_flip: tile range outside the image");
    return launch_pack_flip(img, is_u8, Cimg, H, W, tile, tile, stride, cols, first_tile, n_tiles, flip, mean3, std3, out, stream);
}

// pylc_image_pack_tiles_reflect with a mirror, and with tile == out (pad = 0: same-size networks on the any-size grid) accepted
extern "C" int pylc_image_pack_tiles_reflect_ex(const void* img, int is_u8, int Cimg, int H, int W, int tile, int out, int stride,
                                                int first_tile, int n_tiles, const float* mean3, const float* std3, float* tiles,
                                                void* stream, int flip) {
    PYLC_REQUIRE(img && tiles && mean3 && std3 && (Cimg == 1 || Cimg == 3) && tile >= out && (tile - out) % 2 == 0 && (flip == 0 || flip == 1),
                 "image_pack_tiles_reflect_ex: bad arguments");
    if (int rc = overlap_check("image_pack_tiles_reflect_ex", H, W, out, stride, (tile - out) / 2)) return rc;
    const int rows = overlap_count(H, out, stride), cols = overlap_count(W, out, stride);
    PYLC_REQUIRE(first_tile >= 0 && n_tiles > 0 && (long long)first_tile + n_tiles <= (long long)rows * cols,
                 "image_pack_tiles_reflect_ex: tiles %d..%d outside the %dx%d grid", first_tile, first_tile + n_tiles - 1, rows, cols);
    return launch_pack_flip(img, is_u8, Cimg, H, W, tile, out, stride, cols, first_tile, n_tiles, flip, mean3, std3, tiles, stream);
}

extern "C" int pylc_blend_accumulate(const float* logits, int pitch, int first_tile, int n_tiles, int H, int W, int out, int stride, int C,
                                     int flip, float* acc, int acc_pitch, void* stream) {
    PYLC_REQUIRE(logits && pitch >= C && pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0,
                 "blend_accumulate: logits must be 16-B aligned NHWC tiles with a pitch >= C, multiple of 4");
    PYLC_REQUIRE(acc && acc_pitch >= C && acc_pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(acc) & 15) == 0,
                 "blend_accumulate: acc must be a 16-B aligned [H][W][acc_pitch] image with acc_pitch >= C, multiple of 4");
    PYLC_REQUIRE(flip == 0 || flip == 1, "blend_accumulate: flip=%d", flip);
    if (int rc = overlap_check("blend_accumulate", H, W, out, stride, 0)) return rc;
    const int rows = overlap_count(H, out, stride), cols = overlap_count(W, out, stride);
    PYLC_REQUIRE(first_tile >= 0 && n_tiles > 0 && (long long)first_tile + n_tiles <= (long long)rows * cols,
                 "blend_accumulate: tiles %d..%d outside the %dx%d grid", first_tile, first_tile + n_tiles - 1, rows, cols);
    // the bounding box of the batch: its tile rows, and their columns when it lies within one row (else the full width)
    const int last = first_tile + n_tiles - 1;
    const int r0 = first_tile / cols, r1 = last / cols;
    BlendBox box;
    box.y0 = overlap_origin(r0, H, out, stride);
    box.bh = overlap_origin(r1, H, out, stride) + out - box.y0;
    if (r0 == r1) {
        box.x0 = overlap_origin(first_tile % cols, W, out, stride);
        box.bw = overlap_origin(last % cols, W, out, stride) + out - box.x0;
    } else {
        box.x0 = 0;
        box.bw = W;
    }
    const BlendGeom g{H, W, out, stride, rows, cols, pitch, acc_pitch};
    const int blocks = ot_grid((long long)box.bh * box.bw);
    hipStream_t st = as_stream(stream);
#define LAUNCH_BA(CC) hipLaunchKernelGGL((blend_accumulate_kernel<CC>), dim3(blocks), dim3(256), 0, st, logits, g, box, first_tile, n_tiles, flip, acc)
    PYLC_BLEND_SWITCH(C, LAUNCH_BA, "blend_accumulate")
#undef LAUNCH_BA
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_blend_finalize(const float* acc, int acc_pitch, int H, int W, int out, int stride, int C, int members, unsigned char* mask,
                                   float* probs, float* conf, void* stream) {
    PYLC_REQUIRE(acc && mask && acc_pitch >= C && acc_pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(acc) & 15) == 0,
                 "blend_finalize: acc must be a 16-B aligned [H][W][acc_pitch] image with acc_pitch >= C, multiple of 4");
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(mask) & 3) == 0, "blend_finalize: mask must be 4-B aligned");
    PYLC_REQUIRE(members >= 1, "blend_finalize: members=%d", members);
    if (int rc = overlap_check("blend_finalize", H, W, out, stride, 0)) return rc;
    const BlendGeom g{H, W, out, stride, overlap_count(H, out, stride), overlap_count(W, out, stride), 0, acc_pitch};
    const int blocks = ot_grid(cdiv<long long>((long long)H * W, kOtPx));
    hipStream_t st = as_stream(stream);
#define LAUNCH_BF(CC) hipLaunchKernelGGL((blend_finalize_kernel<CC, true>), dim3(blocks), dim3(256), 0, st, acc, g, members, 0.f, mask, probs, conf)
    PYLC_BLEND_SWITCH(C, LAUNCH_BF, "blend_finalize")
#undef LAUNCH_BF
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}
