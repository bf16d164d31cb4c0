// The finalizer shared by csrc/blend.hip (pylc_blend_finalize, pylc_blend_finalize_w) and csrc/multiscale.hip (pylc_ensemble_finalize):
// one body, the divisor chosen by a template flag or read from the two tables of a trailing BlendTableDiv.
#pragma once
#include "common.h"
#include "overlap_geom.h"

namespace pylc {

namespace {

struct BlendGeom { int H, W, out, stride, rows, cols, pitch, acc_pitch; };

// The separable table form of a pixel's divisor: sum_y[y] * sum_x[x], the per-axis sums of pylc_blend_window_sums --
// two loads and one product where the cover count takes two integer divisions per axis.
struct BlendTableDiv {
    const float* __restrict__ sum_y;
    const float* __restrict__ sum_x;
    __device__ __forceinline__ float operator()(int y, int x) const { return sum_y[y] * sum_x[x]; }
};

// acc [H][W][acc_pitch] -> mask [H][W], probs [C][H][W] (optional), conf [H][W] (optional).  Lane q owns the linear pixels 4q .. 4q+3,
// visited one after the other (stitch_overlap_kernel's rolled loop: an unrolled one spills at C >= 9); the mask leaves as one dword.
// kCover: p[c] = acc[c] / (members * covering tiles), the count from the geometry (the blend).  !kCover: p[c] = acc[c] / total, one
// divisor for every pixel (the ensemble: cover := 1); g.out, g.stride, g.rows, g.cols and members are then not read.
// Div (none, or one BlendTableDiv after conf; !kCover): p[c] = acc[c] / (total * (sum_y[y] * sum_x[x])), the window-weighted blend with
// total = members.  Without one the parameter list and the code are the two forms above.
template <int C, bool kCover, class... Div>
__global__ __launch_bounds__(256) void blend_finalize_kernel(const float* __restrict__ acc, BlendGeom g, int members, float total,
                                                              unsigned char* __restrict__ mask, float* __restrict__ probs,
                                                              float* __restrict__ conf, Div... div) {
    static_assert(sizeof...(Div) <= 1 && !(kCover && sizeof...(Div)), "one divisor: the geometry's count, the total, or total times the tables' product");
    constexpr int NV = (C + 3) / 4;
    const long long npx = (long long)g.H * g.W;
    const long long groups = cdiv<long long>(npx, kOtPx);
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += (long long)gridDim.x * blockDim.x) {
        const long long base = q * kOtPx;
        const int np = npx - base < kOtPx ? (int)(npx - base) : kOtPx;
        unsigned int packed = 0;
#pragma unroll 1
        for (int p = 0; p < np; ++p) {
            const long long i = base + p;
            float fn = total;
            if constexpr (kCover) {
                const int y = (int)(i / g.W), x = (int)(i - (long long)y * g.W);
                const Cover cy = overlap_cover(y, g.H, g.out, g.stride, g.rows);
                const Cover cx = overlap_cover(x, g.W, g.out, g.stride, g.cols);
                const int n = members * (cy.hi + cy.last - cy.lo + 1) * (cx.hi + cx.last - cx.lo + 1);
                fn = (float)n;
            }
            [[maybe_unused]] float ty = 1.f, tx = 1.f;
            if constexpr (sizeof...(Div) == 1) {
                const int y = (int)(i / g.W), x = (int)(i - (long long)y * g.W);
                ((ty = div.sum_y[y], tx = div.sum_x[x]), ...);                  // issued with the loads of acc, multiplied after them
            }
            const ot_f32x4* src = reinterpret_cast<const ot_f32x4*>(acc + (size_t)i * g.acc_pitch);
            float a[NV * 4];
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const ot_f32x4 t = src[k];
                a[4 * k] = t.x; a[4 * k + 1] = t.y; a[4 * k + 2] = t.z; a[4 * k + 3] = t.w;
            }
            if constexpr (sizeof...(Div) == 1) fn = total * (ty * tx);       // after the loads of acc: one wait for the tables and the sums
            int best = 0;
            float bv = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                a[c] = a[c] / fn;
                if (c == 0 || a[c] > bv) { bv = a[c]; best = c; }     // first maximum (np.argmax)
            }
            packed |= (unsigned int)best << (8 * p);
            if (probs != nullptr) {
#pragma unroll
                for (int c = 0; c < C; ++c) probs[(size_t)c * npx + i] = a[c];
            }
            if (conf != nullptr) conf[i] = bv;
        }
        if (np == kOtPx) {
            *reinterpret_cast<unsigned int*>(mask + base) = packed;     // base % 4 == 0: an aligned dword
        } else {
            for (int p = 0; p < np; ++p) mask[base + p] = (unsigned char)(packed >> (8 * p));
        }
    }
}

}  // namespace

}  // namespace pylc
