// The streaming mean-probability blend: overlap_tile.hip's blend -- every pixel's score is the mean of the
// softmax probabilities of the tiles that cover it -- taken batch by batch into one fp32 accumulation image instead of from every logit
// tile at once, for any number of ensemble members (the windows, mirrored ones for the horizontal-flip member included, are cut by
// pack_tiles.hip).
//
//   blend_accumulate_kernel<C>  acc[y][x][c] += softmax(tile logits at that pixel)[c] over the batch's tiles that cover the pixel, in
//                               ascending tile index.  Gather form: one lane per pixel of the batch's bounding box, lanes along x, the
//                               pixel's acc vector loaded once, added to in registers and stored once (16-byte accesses, no atomics).
//                               Tile index ascends within a batch and from batch to batch, so after a member's last batch acc holds,
//                               bit for bit, the sums stitch_overlap_kernel forms in registers: independent of the batch size.
//   blend_finalize_kernel<C, 1> p[c] = acc[c] / (members * covering tiles) -- the count comes from the geometry, no count buffer --
//                               class = first maximum; mask (four pixels per lane, one dword), optional probs [C][H][W], conf [H][W].
//                               (blend_finalize.h: multiscale.hip's ensemble finalizer is the same body with one divisor.)
//
// The window-weighted blend: a tile's term counts wt = win[ly] * win[lx] times, win one table of `out` floats.
//   blend_accumulate_kernel<C, 1, const float*>  the same gather, acc[c] += wt * (softmax term); the same bytes moved, plus the 4 * out B table.
//   blend_window_sums_kernel      one axis' sums of win over the covering tiles: a table of n floats, the separable form of the divisor.
//   blend_finalize_kernel<C, 0, BlendTableDiv>  the same finalizer body, p[c] = acc[c] / (members * (sum_y[y] * sum_x[x])).
// A table of ones gives the plain kernels' bytes: every product and sum is then an exact small integer.
//
// The geometry is overlap_geom.h's: o_i = min(i*stride, n - out); the fitted sliding-window grid of stitch.hip is the case out = tile
// in which the clamp is never active.  Bandwidth kernels: no LDS, no MFMA.
#include "blend_finalize.h"
#include "common.h"
#include "overlap_geom.h"

namespace pylc {

namespace {

// the pixels [y0, y0 + bh) x [x0, x0 + bw) that the tiles first .. first + count - 1 can touch
struct BlendBox { int y0, x0, bh, bw; };

// TEMP: the tile's term is softmax(beta * logits) (pylc_blend_accumulate_t); without it `beta` is not read.
// Win (none, or one const float* after beta; TEMP): the window table of pylc_blend_accumulate_w -- the term is multiplied by
// wt = win[ly] * win[lx], ly and lx the pixel's position inside the placed tile (for the flip member: after the mirrored logits are
// mirrored back).  Without one the parameter list and the code are the plain forms'.
template <int C, bool TEMP, class... Win>
__global__ __launch_bounds__(256) void blend_accumulate_kernel(const float* __restrict__ logits, BlendGeom g, BlendBox box, int first, int count,
                                                                int flip, float* __restrict__ acc, float beta, Win... win) {
    static_assert(sizeof...(Win) <= 1 && !(!TEMP && sizeof...(Win)), "the windowed gather is the temperature form with one table");
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
                [[maybe_unused]] float wt = 1.f;
                if constexpr (sizeof...(Win) == 1) wt = ((win[ly] * win[lx]), ...);        // the placed position: before the read's flip mapping
                lx = flip ? g.out - 1 - lx : lx;
                const ot_f32x4* src = reinterpret_cast<const ot_f32x4*>(logits + (((size_t)k * g.out + ly) * g.out + lx) * g.pitch);
                if constexpr (sizeof...(Win) == 1) softmax_add<C, NV * 4, true, true>(src, a, beta, wt);
                else if constexpr (TEMP) softmax_add<C, NV * 4, true>(src, a, beta);
                else softmax_add<C>(src, a);         // stitch_overlap_kernel's term, operation for operation
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

// sums[y] = the fp32 sum of win[y - o_i] over the tiles i covering coordinate y of an axis of length n, in overlap_cover's visiting
// order (the unclamped tiles ascending, then the clamped last tile); one lane per coordinate.
__global__ __launch_bounds__(256) void blend_window_sums_kernel(const float* __restrict__ win, int n, int out, int stride, int cnt,
                                                                 float* __restrict__ sums) {
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= n) return;
    const Cover c = overlap_cover(y, n, out, stride, cnt);
    float s = 0.f;
    for (int ia = c.lo; ia <= c.hi + c.last; ++ia) {
        const int ti = ia <= c.hi ? ia : cnt - 1;
        s += win[y - overlap_origin(ti, n, out, stride)];
    }
    sums[y] = s;
}

}  // namespace
}  // namespace pylc

using namespace pylc;

// win: NULL for the plain forms, else the window table [out] of pylc_blend_accumulate_w (TEMP then holds)
template <bool TEMP>
static int blend_accumulate_impl(const float* logits, int pitch, int first_tile, int n_tiles, int H, int W, int out, int stride, int C,
                                 int flip, float* acc, int acc_pitch, void* stream, float beta, const float* win = nullptr) {
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
#define LAUNCH_BA(CC) hipLaunchKernelGGL((blend_accumulate_kernel<CC, TEMP>), dim3(blocks), dim3(256), 0, st, logits, g, box, first_tile, n_tiles, flip, acc, beta)
#define LAUNCH_BW(CC) hipLaunchKernelGGL((blend_accumulate_kernel<CC, true, const float*>), dim3(blocks), dim3(256), 0, st, logits, g, box, first_tile, n_tiles, flip, acc, beta, win)
    if constexpr (TEMP) {
        if (win != nullptr) {
            PYLC_FOR_CLASSES(C, LAUNCH_BW, "blend_accumulate")
            PYLC_LAUNCH_CHECK();
            return PYLC_OK;
        }
    }
    PYLC_FOR_CLASSES(C, LAUNCH_BA, "blend_accumulate")
#undef LAUNCH_BW
#undef LAUNCH_BA
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_blend_accumulate(const float* logits, int pitch, int first_tile, int n_tiles, int H, int W, int out, int stride, int C,
                                     int flip, float* acc, int acc_pitch, void* stream) {
    return blend_accumulate_impl<false>(logits, pitch, first_tile, n_tiles, H, W, out, stride, C, flip, acc, acc_pitch, stream, 1.f);
}

extern "C" int pylc_blend_accumulate_t(const float* logits, int pitch, int first_tile, int n_tiles, int H, int W, int out, int stride, int C,
                                       int flip, float* acc, int acc_pitch, void* stream, float inv_temperature) {
    PYLC_REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.4028234e38f, "blend_accumulate_t: inv_temperature must be positive and finite");
    return blend_accumulate_impl<true>(logits, pitch, first_tile, n_tiles, H, W, out, stride, C, flip, acc, acc_pitch, stream, inv_temperature);
}

extern "C" int pylc_blend_accumulate_w(const float* logits, int pitch, int first_tile, int n_tiles, int H, int W, int out, int stride, int C,
                                       int flip, float* acc, int acc_pitch, const float* win, float inv_temperature, void* stream) {
    PYLC_REQUIRE(win && (reinterpret_cast<uintptr_t>(win) & 3) == 0, "blend_accumulate_w: win must be a 4-B aligned table of `out` floats");
    PYLC_REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.4028234e38f, "blend_accumulate_w: inv_temperature must be positive and finite");
    return blend_accumulate_impl<true>(logits, pitch, first_tile, n_tiles, H, W, out, stride, C, flip, acc, acc_pitch, stream, inv_temperature, win);
}

extern "C" int pylc_blend_window_sums(const float* win, int out, int stride, int n, float* sums, void* stream) {
    PYLC_REQUIRE(win && sums, "blend_window_sums: NULL pointer");
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(win) & 3) == 0 && (reinterpret_cast<uintptr_t>(sums) & 3) == 0,
                 "blend_window_sums: win and sums must be 4-B aligned");
    PYLC_REQUIRE(static_cast<const float*>(sums) != win, "blend_window_sums: sums may not alias win");
    if (int rc = overlap_check("blend_window_sums", n, n, out, stride, 0)) return rc;
    hipLaunchKernelGGL(blend_window_sums_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), win, n, out, stride,
                       overlap_count(n, out, stride), sums);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_blend_finalize_w(const float* acc, int acc_pitch, int H, int W, int C, int members, const float* sum_y, const float* sum_x,
                                     unsigned char* mask, float* probs, float* conf, void* stream) {
    PYLC_REQUIRE(acc && mask && acc_pitch >= C && acc_pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(acc) & 15) == 0,
                 "blend_finalize_w: acc must be a 16-B aligned [H][W][acc_pitch] image with acc_pitch >= C, multiple of 4");
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(mask) & 3) == 0, "blend_finalize_w: mask must be 4-B aligned");
    PYLC_REQUIRE(sum_y && sum_x && (reinterpret_cast<uintptr_t>(sum_y) & 3) == 0 && (reinterpret_cast<uintptr_t>(sum_x) & 3) == 0,
                 "blend_finalize_w: sum_y [H] and sum_x [W] must be 4-B aligned tables");
    PYLC_REQUIRE(members >= 1, "blend_finalize_w: members=%d", members);
    PYLC_REQUIRE(H >= 1 && W >= 1, "blend_finalize_w: H=%d W=%d", H, W);
    const BlendGeom g{H, W, 0, 0, 0, 0, 0, acc_pitch};
    const BlendTableDiv div{sum_y, sum_x};
    const int blocks = ot_grid(cdiv<long long>((long long)H * W, kOtPx));
    hipStream_t st = as_stream(stream);
#define LAUNCH_FW(CC) hipLaunchKernelGGL((blend_finalize_kernel<CC, false, BlendTableDiv>), dim3(blocks), dim3(256), 0, st, acc, g, 1, (float)members, mask, probs, conf, div)
    PYLC_FOR_CLASSES(C, LAUNCH_FW, "blend_finalize_w")
#undef LAUNCH_FW
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
    PYLC_FOR_CLASSES(C, LAUNCH_BF, "blend_finalize")
#undef LAUNCH_BF
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}
