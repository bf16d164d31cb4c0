// The multi-scale test-time ensemble on top of the streaming mean-probability blend: the photograph is run at
// several sizes, each size's mean probabilities are resampled to the photograph's size and their weighted mean is taken.
//
//   resize_bilinear_kernel<U8>   dst [Cimg][oh][ow] fp32 <- src [Cimg][H][W] uint8 or fp32, half-pixel-centre bilinear without antialiasing
//                                (F.interpolate(mode='bilinear', align_corners=False)); one destination pixel per lane.
//   blend_resample_kernel<C>     ens[y][x][c] = (add ? ens[y][x][c] : 0) + weight * bilinear(p)[c], p[c] = acc_s[..][c] / (members * covering
//                                tiles) at the four source pixels: blend_finalize_kernel's division, the count from the scaled image's
//                                geometry.  One destination pixel per lane, lanes along x, 16-byte loads of the four source vectors, the
//                                destination vector loaded (add) and stored once; channels C .. ens_pitch-1 are not written.
//   blend_resample_kernel<C, BlendTableDiv>  the same body with the four corner divisors read from the scaled size's window sums.
//   blend_finalize_kernel<C, false> (blend_finalize.h)   p = ens / total_weight, mask, probs, conf as pylc_blend_finalize writes them.
//
// The coordinate rule, per axis (destination length n, source length ns): s = (i + 0.5) * ((double)ns / n) - 0.5 in double, clamped to
// [0, ns - 1]; i0 = floor(s), i1 = min(i0 + 1, ns - 1), f = (float)(s - i0); value (1-fy)*((1-fx)*v00 + fx*v01) + fy*((1-fx)*v10 + fx*v11)
// in fp32, in that order.  ns == n gives s = i exactly, f = 0 and the value v00 bit for bit through the same code: there is no copy
// branch.  Coordinates are double (augment.hip's reason: an fp32 coordinate is off by up to 2.4e-4 px at x = 4096); the ratio is formed
// once on the host, a lane spends one double multiply per axis.  Bandwidth kernels: no LDS, no atomics, no MFMA.
#include <type_traits>

#include "blend_finalize.h"
#include "common.h"
#include "overlap_geom.h"

namespace pylc {

namespace {

struct Axis { int i0, i1; float f; };

// the two source indices and the weight of the second for destination index i; ratio = (double)ns / n
__device__ __forceinline__ Axis bilinear_axis(int i, double ratio, int ns) {
    double s = (i + 0.5) * ratio - 0.5;
    const double hi = (double)(ns - 1);
    s = s < 0.0 ? 0.0 : s;
    s = s > hi ? hi : s;
    Axis a;
    a.i0 = (int)s;                                  // s >= 0: the floor
    a.i1 = a.i0 + 1 < ns ? a.i0 + 1 : ns - 1;
    a.f = (float)(s - (double)a.i0);
    return a;
}

__device__ __forceinline__ float bilinear(float v00, float v01, float v10, float v11, float fx, float fy) {
    return (1.f - fy) * ((1.f - fx) * v00 + fx * v01) + fy * ((1.f - fx) * v10 + fx * v11);
}

template <bool U8>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const void* __restrict__ src_, int Cimg, int H, int W, double ry, double rx,
                                                               float* __restrict__ dst, int oh, int ow) {
    typedef typename std::conditional<U8, unsigned char, float>::type T;
    const T* __restrict__ src = static_cast<const T*>(src_);
    const long long total = (long long)oh * ow;
    const size_t plane = (size_t)H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(i / ow), x = (int)(i - (long long)y * ow);
        const Axis ay = bilinear_axis(y, ry, H), ax = bilinear_axis(x, rx, W);
        const T* r0 = src + (size_t)ay.i0 * W;
        const T* r1 = src + (size_t)ay.i1 * W;
        for (int c = 0; c < Cimg; ++c) {
            const size_t o = c * plane;
            dst[(size_t)c * total + i] = bilinear((float)r0[o + ax.i0], (float)r0[o + ax.i1], (float)r1[o + ax.i0], (float)r1[o + ax.i1], ax.f, ay.f);
        }
    }
}

// Hs, Ws .. cols: the scaled image's blend geometry (BlendGeom's fields); H, W: the ensemble image
struct ResampleGeom { int Hs, Ws, out, stride, rows, cols, src_pitch, H, W, ens_pitch, members, add; double ry, rx; float weight; };

// number of tiles covering coordinate y along an axis (blend_finalize_kernel's factor)
__device__ __forceinline__ int cover_count(int y, int n, int out, int stride, int cnt) {
    const Cover c = overlap_cover(y, n, out, stride, cnt);
    return c.hi + c.last - c.lo + 1;
}

// The channels are walked four at a time: the four corners' 16-byte loads of one quad, its 4 results, the destination's quad.  Every
// 16-byte piece of the five vectors is touched once, and no more than one quad of each is live at a time.
// Tab (none, or one BlendTableDiv after ens): pylc_blend_resample_accumulate_w -- the four corner divisors are
// members * (sum_y[.] * sum_x[.]) from the scaled size's window sums; g.out, g.stride, g.rows and g.cols are then not read.  Without
// one the parameter list and the code are the plain form's.
template <int C, class... Tab>
__global__ __launch_bounds__(256) void blend_resample_kernel(const float* __restrict__ acc, ResampleGeom g, float* __restrict__ ens, Tab... tab) {
    static_assert(sizeof...(Tab) <= 1, "one table divisor at most");
    constexpr int NV = (C + 3) / 4;
    const long long total = (long long)g.H * g.W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(i / g.W), x = (int)(i - (long long)y * g.W);
        const Axis ay = bilinear_axis(y, g.ry, g.Hs), ax = bilinear_axis(x, g.rx, g.Ws);
        float n00, n01, n10, n11;
        if constexpr (sizeof...(Tab) == 1) {
            const float fm = (float)g.members;
            n00 = fm * (tab(ay.i0, ax.i0), ...); n01 = fm * (tab(ay.i0, ax.i1), ...);
            n10 = fm * (tab(ay.i1, ax.i0), ...); n11 = fm * (tab(ay.i1, ax.i1), ...);
        } else {
            const int ny0 = cover_count(ay.i0, g.Hs, g.out, g.stride, g.rows), ny1 = cover_count(ay.i1, g.Hs, g.out, g.stride, g.rows);
            const int nx0 = cover_count(ax.i0, g.Ws, g.out, g.stride, g.cols), nx1 = cover_count(ax.i1, g.Ws, g.out, g.stride, g.cols);
            n00 = (float)(g.members * ny0 * nx0); n01 = (float)(g.members * ny0 * nx1);
            n10 = (float)(g.members * ny1 * nx0); n11 = (float)(g.members * ny1 * nx1);
        }
        const ot_f32x4* s00 = reinterpret_cast<const ot_f32x4*>(acc + ((size_t)ay.i0 * g.Ws + ax.i0) * g.src_pitch);
        const ot_f32x4* s01 = reinterpret_cast<const ot_f32x4*>(acc + ((size_t)ay.i0 * g.Ws + ax.i1) * g.src_pitch);
        const ot_f32x4* s10 = reinterpret_cast<const ot_f32x4*>(acc + ((size_t)ay.i1 * g.Ws + ax.i0) * g.src_pitch);
        const ot_f32x4* s11 = reinterpret_cast<const ot_f32x4*>(acc + ((size_t)ay.i1 * g.Ws + ax.i1) * g.src_pitch);
        float* dst = ens + (size_t)i * g.ens_pitch;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const ot_f32x4 t00 = s00[q], t01 = s01[q], t10 = s10[q], t11 = s11[q];
            float r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (4 * q + k < C)
                    r[k] = g.weight * bilinear(t00[k] / n00, t01[k] / n01, t10[k] / n10, t11[k] / n11, ax.f, ay.f);
            }
            if (4 * q + 4 <= C) {
                ot_f32x4 d = {0.f, 0.f, 0.f, 0.f};
                if (g.add) d = reinterpret_cast<const ot_f32x4*>(dst)[q];
                d.x += r[0]; d.y += r[1]; d.z += r[2]; d.w += r[3];
                reinterpret_cast<ot_f32x4*>(dst)[q] = d;
            } else {                                  // the last, partial quad: channels C .. ens_pitch-1 are neither read nor written
#pragma unroll
                for (int k = 0; k < C - 4 * q; ++k) {
                    float d = 0.f;
                    if (g.add) d = dst[4 * q + k];
                    dst[4 * q + k] = d + r[k];
                }
            }
        }
    }
}

}  // namespace
}  // namespace pylc

using namespace pylc;

extern "C" int pylc_resize_bilinear_image(const void* src, int is_u8, int Cimg, int H, int W, float* dst, int oh, int ow, void* stream) {
    PYLC_REQUIRE(src && dst, "resize_bilinear_image: NULL pointer");
    PYLC_REQUIRE((is_u8 == 0 || is_u8 == 1) && (Cimg == 1 || Cimg == 3), "resize_bilinear_image: is_u8=%d Cimg=%d (uint8 or float32, 1 or 3 channels)",
                 is_u8, Cimg);
    PYLC_REQUIRE(H >= 1 && W >= 1 && oh >= 1 && ow >= 1, "resize_bilinear_image: %dx%d -> %dx%d", H, W, oh, ow);
    PYLC_REQUIRE(static_cast<const void*>(dst) != src, "resize_bilinear_image: dst may not alias src");
    const double ry = (double)H / oh, rx = (double)W / ow;
    const int blocks = ot_grid((long long)oh * ow);
    hipStream_t st = as_stream(stream);
    if (is_u8)
        hipLaunchKernelGGL(resize_bilinear_kernel<true>, dim3(blocks), dim3(256), 0, st, src, Cimg, H, W, ry, rx, dst, oh, ow);
    else
        hipLaunchKernelGGL(resize_bilinear_kernel<false>, dim3(blocks), dim3(256), 0, st, src, Cimg, H, W, ry, rx, dst, oh, ow);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_blend_resample_accumulate(const float* acc_s, int src_pitch, int Hs, int Ws, int out, int stride, int members, float weight,
                                              int C, float* ens, int ens_pitch, int H, int W, int add, void* stream) {
    PYLC_REQUIRE(acc_s && ens, "blend_resample_accumulate: NULL pointer");
    PYLC_REQUIRE(src_pitch >= C && src_pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(acc_s) & 15) == 0,
                 "blend_resample_accumulate: acc_s must be a 16-B aligned [Hs][Ws][src_pitch] image with src_pitch >= C, multiple of 4");
    PYLC_REQUIRE(ens_pitch >= C && ens_pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(ens) & 15) == 0,
                 "blend_resample_accumulate: ens must be a 16-B aligned [H][W][ens_pitch] image with ens_pitch >= C, multiple of 4");
    PYLC_REQUIRE(static_cast<const float*>(ens) != acc_s, "blend_resample_accumulate: ens may not alias acc_s");
    PYLC_REQUIRE(members >= 1, "blend_resample_accumulate: members=%d", members);
    PYLC_REQUIRE(weight > 0.f && weight <= 3.4e38f, "blend_resample_accumulate: weight %g must be positive and finite", (double)weight);
    PYLC_REQUIRE(H >= 1 && W >= 1 && (add == 0 || add == 1), "blend_resample_accumulate: H=%d W=%d add=%d", H, W, add);
    if (int rc = overlap_check("blend_resample_accumulate", Hs, Ws, out, stride, 0)) return rc;
    ResampleGeom g;
    g.Hs = Hs; g.Ws = Ws; g.out = out; g.stride = stride;
    g.rows = overlap_count(Hs, out, stride); g.cols = overlap_count(Ws, out, stride);
    g.src_pitch = src_pitch; g.H = H; g.W = W; g.ens_pitch = ens_pitch; g.members = members; g.add = add;
    g.ry = (double)Hs / H; g.rx = (double)Ws / W; g.weight = weight;
    const int blocks = ot_grid((long long)H * W);
    hipStream_t st = as_stream(stream);
#define LAUNCH_RS(CC) hipLaunchKernelGGL((blend_resample_kernel<CC>), dim3(blocks), dim3(256), 0, st, acc_s, g, ens)
    PYLC_FOR_CLASSES(C, LAUNCH_RS, "blend_resample_accumulate")
#undef LAUNCH_RS
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_blend_resample_accumulate_w(const float* acc_s, int src_pitch, int Hs, int Ws, int members, float weight, int C,
                                                const float* sum_y_s, const float* sum_x_s, float* ens, int ens_pitch, int H, int W, int add,
                                                void* stream) {
    PYLC_REQUIRE(acc_s && ens, "blend_resample_accumulate_w: NULL pointer");
    PYLC_REQUIRE(src_pitch >= C && src_pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(acc_s) & 15) == 0,
                 "blend_resample_accumulate_w: acc_s must be a 16-B aligned [Hs][Ws][src_pitch] image with src_pitch >= C, multiple of 4");
    PYLC_REQUIRE(ens_pitch >= C && ens_pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(ens) & 15) == 0,
                 "blend_resample_accumulate_w: ens must be a 16-B aligned [H][W][ens_pitch] image with ens_pitch >= C, multiple of 4");
    PYLC_REQUIRE(static_cast<const float*>(ens) != acc_s, "blend_resample_accumulate_w: ens may not alias acc_s");
    PYLC_REQUIRE(sum_y_s && sum_x_s && (reinterpret_cast<uintptr_t>(sum_y_s) & 3) == 0 && (reinterpret_cast<uintptr_t>(sum_x_s) & 3) == 0,
                 "blend_resample_accumulate_w: sum_y_s [Hs] and sum_x_s [Ws] must be 4-B aligned tables");
    PYLC_REQUIRE(members >= 1, "blend_resample_accumulate_w: members=%d", members);
    PYLC_REQUIRE(weight > 0.f && weight <= 3.4e38f, "blend_resample_accumulate_w: weight %g must be positive and finite", (double)weight);
    PYLC_REQUIRE(Hs >= 1 && Ws >= 1, "blend_resample_accumulate_w: Hs=%d Ws=%d", Hs, Ws);
    PYLC_REQUIRE(H >= 1 && W >= 1 && (add == 0 || add == 1), "blend_resample_accumulate_w: H=%d W=%d add=%d", H, W, add);
    ResampleGeom g;
    g.Hs = Hs; g.Ws = Ws; g.out = 0; g.stride = 0; g.rows = 0; g.cols = 0;
    g.src_pitch = src_pitch; g.H = H; g.W = W; g.ens_pitch = ens_pitch; g.members = members; g.add = add;
    g.ry = (double)Hs / H; g.rx = (double)Ws / W; g.weight = weight;
    const BlendTableDiv tab{sum_y_s, sum_x_s};
    const int blocks = ot_grid((long long)H * W);
    hipStream_t st = as_stream(stream);
#define LAUNCH_RW(CC) hipLaunchKernelGGL((blend_resample_kernel<CC, BlendTableDiv>), dim3(blocks), dim3(256), 0, st, acc_s, g, ens, tab)
    PYLC_FOR_CLASSES(C, LAUNCH_RW, "blend_resample_accumulate_w")
#undef LAUNCH_RW
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_ensemble_finalize(const float* ens, int pitch, int H, int W, int C, float total_weight, unsigned char* mask, float* probs,
                                      float* conf, void* stream) {
    PYLC_REQUIRE(ens && mask, "ensemble_finalize: NULL pointer");
    PYLC_REQUIRE(pitch >= C && pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(ens) & 15) == 0,
                 "ensemble_finalize: ens must be a 16-B aligned [H][W][pitch] image with pitch >= C, multiple of 4");
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(mask) & 3) == 0, "ensemble_finalize: mask must be 4-B aligned");
    PYLC_REQUIRE(total_weight > 0.f && total_weight <= 3.4e38f, "ensemble_finalize: total_weight %g must be positive and finite", (double)total_weight);
    PYLC_REQUIRE(H >= 1 && W >= 1, "ensemble_finalize: H=%d W=%d", H, W);
    const BlendGeom g{H, W, 0, 0, 0, 0, 0, pitch};
    const int blocks = ot_grid(cdiv<long long>((long long)H * W, kOtPx));
    hipStream_t st = as_stream(stream);
#define LAUNCH_EF(CC) hipLaunchKernelGGL((blend_finalize_kernel<CC, false>), dim3(blocks), dim3(256), 0, st, ens, g, 1, total_weight, mask, probs, conf)
    PYLC_FOR_CLASSES(C, LAUNCH_EF, "ensemble_finalize")
#undef LAUNCH_EF
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}
