// Edge-aware refinement of class probabilities: the guided filter (He, Sun, Tang, PAMI 2013) with a one-channel uint8 guide
// (the reference has nothing of the kind).
//
//   luma_u8_kernel          g = (77 R + 150 G + 29 B + 128) >> 8 from a planar uint8 image (a 1-channel image is copied).
//   guided_coeffs_kernel    stage 1, one class per blockIdx.z: the window sums S_g, S_gg (int32, exact), S_p, S_gp (fp32) of the
//                           (2r+1)^2 window clipped to the image, then a_c, b_c.  n * S_gg - S_g^2 is formed in int64; where it is 0
//                           a_c = 0 exactly and b_c = S_p / n.
//   guided_apply_kernel     stage 2, all classes in one block: q_c = (sum a_c / n) * g / 255 + sum b_c / n, first-maximum argmax,
//                           clamped confidence, optional volume.  The running maximum of a pixel lives in LDS between the classes.
//
// One shape for every radius 1..64, the column strip: a block of 8 x 64 threads owns 64 output columns and a run of rows, and walks
// down its rows eight at a time.  Per step: the eight new input rows (64 + 2r columns, zero outside the image) go to LDS; each thread
// forms one horizontal window sum per quantity from those raw values and stores it into a ring of 2r + 8 rows of horizontal sums; each
// thread then forms one vertical window sum per quantity from 2r + 1 ring rows.  Every window sum is therefore the sum of that window's
// own 2r + 1 row sums of 2r + 1 values, in ascending x then ascending y -- nothing is carried from one window to the next, no
// subtraction, no atomics, and two runs give the same bytes.  The ring is dynamic LDS sized by r (stage 1: 16 B per column and row,
// 139 KiB at r = 64, 24 KiB at r = 8), which is what fixes the occupancy at large radii.
#include "common.h"

namespace pylc {

namespace {

constexpr int kRfCols = 64;      // output columns of a strip (threadIdx.x)
constexpr int kRfRows = 8;       // rows per step (threadIdx.y)
constexpr int kRfThreads = kRfCols * kRfRows;
constexpr int kRfMaxLds = 160 * 1024;

__global__ __launch_bounds__(256) void luma_u8_kernel(const unsigned char* __restrict__ img, int ch, long long npx,
                                                       unsigned char* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (long long)gridDim.x * blockDim.x) {
        if (ch == 1) {
            out[i] = img[i];
        } else {
            const int v = 77 * (int)img[i] + 150 * (int)img[npx + i] + 29 * (int)img[2 * npx + i] + 128;
            out[i] = (unsigned char)(v >> 8);
        }
    }
}

struct RefineGeom { int H, W, r, rows_per_block; };

// the pixel count of the window centred on (y, x), clipped to the image
__device__ __forceinline__ int window_count(int y, int x, const RefineGeom& g) {
    const int y0 = y - g.r < 0 ? 0 : y - g.r, y1 = y + g.r > g.H - 1 ? g.H - 1 : y + g.r;
    const int x0 = x - g.r < 0 ? 0 : x - g.r, x1 = x + g.r > g.W - 1 ? g.W - 1 : x + g.r;
    return (y1 - y0 + 1) * (x1 - x0 + 1);
}

__global__ __launch_bounds__(kRfThreads) void guided_coeffs_kernel(const float* __restrict__ p, long long plane_stride, long long row_pitch,
                                                                    const unsigned char* __restrict__ guide, RefineGeom g, float eps,
                                                                    float* __restrict__ a, float* __restrict__ b) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int r = g.r, win = 2 * r + 1, rw = kRfCols + 2 * r, nr = 2 * r + kRfRows;
    // [nr][64] horizontal sums, one 16-byte access each: x = sum p, y = sum g * p (float bits), z = sum g, w = sum g * g
    int4* ring = reinterpret_cast<int4*>(lds_raw);
    float2* raw_p = reinterpret_cast<float2*>(ring + (size_t)nr * kRfCols);         // [8][rw]: (p, g * p)
    unsigned char* raw_g = reinterpret_cast<unsigned char*>(raw_p + kRfRows * rw);  // [8][rw]

    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kRfCols + tx;
    const int c = blockIdx.z;
    const int x0 = blockIdx.x * kRfCols, y0 = blockIdx.y * g.rows_per_block;
    const int rows = g.H - y0 < g.rows_per_block ? g.H - y0 : g.rows_per_block;
    const float* pc = p + (size_t)c * plane_stride;
    const size_t out_plane = (size_t)c * g.H * g.W;
    const int steps = (rows + 2 * r + kRfRows - 1) / kRfRows;
    for (int k = 0; k < steps; ++k) {
        const int yy0 = y0 - r + k * kRfRows;
        for (int i = tid; i < kRfRows * rw; i += kRfThreads) {
            const int rr = i / rw, cc = i - rr * rw;
            const int yy = yy0 + rr, xx = x0 - r + cc;
            const bool in = yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
            const float v = in ? pc[(size_t)yy * row_pitch + xx] : 0.f;
            const unsigned char gv = in ? guide[(size_t)yy * g.W + xx] : (unsigned char)0;
            raw_p[i] = make_float2(v, (float)gv * v);
            raw_g[i] = gv;
        }
        __syncthreads();
        {
            const float2* rp = raw_p + ty * rw + tx;
            const unsigned char* rg = raw_g + ty * rw + tx;
            float sp = 0.f, sgp = 0.f;
            int sg = 0, sgg = 0;
            for (int j = 0; j < win; ++j) {
                const int gi = rg[j];
                const float2 v = rp[j];
                sp += v.x;
                sgp += v.y;
                sg += gi;
                sgg += gi * gi;
            }
            ring[((k * kRfRows + ty) % nr) * kRfCols + tx] = make_int4(__float_as_int(sp), __float_as_int(sgp), sg, sgg);
        }
        __syncthreads();
        const int rel = k * kRfRows + ty - 2 * r;           // the output row whose last window row this step brought, relative to y0
        const int x = x0 + tx;
        if (rel >= 0 && rel < rows && x < g.W) {
            const int y = y0 + rel;
            float sp = 0.f, sgp = 0.f;
            int sg = 0, sgg = 0;
            int row = rel % nr;                             // ring row of image row y - r
            for (int j = 0; j < win; ++j) {
                const int4 h = ring[row * kRfCols + tx];
                sp += __int_as_float(h.x); sgp += __int_as_float(h.y); sg += h.z; sgg += h.w;
                row = row + 1 == nr ? 0 : row + 1;
            }
            const int n = window_count(y, x, g);
            const float nf = (float)n;
            const long long d = (long long)n * sgg - (long long)sg * sg;
            float ac = 0.f, bc = sp / nf;
            if (d != 0) {
                const float var = (float)d / (65025.f * nf * nf);
                const float cov = (nf * sgp - (float)sg * sp) / (255.f * nf * nf);
                const float mean_i = (float)sg / (255.f * nf);
                ac = cov / (var + eps);
                bc = sp / nf - ac * mean_i;
            }
            const size_t o = out_plane + (size_t)y * g.W + x;
            a[o] = ac;
            b[o] = bc;
        }
    }
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }      // a NaN stays a NaN

__global__ __launch_bounds__(kRfThreads) void guided_apply_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                   const unsigned char* __restrict__ guide, RefineGeom g, int C, int clip,
                                                                   unsigned char* __restrict__ mask, float* __restrict__ probs,
                                                                   float* __restrict__ conf) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int r = g.r, win = 2 * r + 1, rw = kRfCols + 2 * r, nr = 2 * r + kRfRows;
    float2* ring = reinterpret_cast<float2*>(lds_raw);                  // [nr][64] horizontal sums of (a, b), one 8-byte access each
    float2* raw = ring + (size_t)nr * kRfCols;                          // [8][rw]: (a, b)
    float* best_v = reinterpret_cast<float*>(raw + kRfRows * rw);       // [rows_per_block][64] the running maximum of q
    unsigned char* best_c = reinterpret_cast<unsigned char*>(best_v + (size_t)g.rows_per_block * kRfCols);   // and its class

    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kRfCols + tx;
    const int x0 = blockIdx.x * kRfCols, y0 = blockIdx.y * g.rows_per_block;
    const int rows = g.H - y0 < g.rows_per_block ? g.H - y0 : g.rows_per_block;
    const size_t npx = (size_t)g.H * g.W;
    const int steps = (rows + 2 * r + kRfRows - 1) / kRfRows;
    for (int c = 0; c < C; ++c) {
        const float* ac = a + (size_t)c * npx;
        const float* bc = b + (size_t)c * npx;
        for (int k = 0; k < steps; ++k) {
            const int yy0 = y0 - r + k * kRfRows;
            for (int i = tid; i < kRfRows * rw; i += kRfThreads) {
                const int rr = i / rw, cc = i - rr * rw;
                const int yy = yy0 + rr, xx = x0 - r + cc;
                const bool in = yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
                const size_t o = (size_t)yy * g.W + xx;
                raw[i] = in ? make_float2(ac[o], bc[o]) : make_float2(0.f, 0.f);
            }
            __syncthreads();
            {
                const float2* rr = raw + ty * rw + tx;
                float sa = 0.f, sb = 0.f;
                for (int j = 0; j < win; ++j) {
                    const float2 v = rr[j];
                    sa += v.x;
                    sb += v.y;
                }
                ring[((k * kRfRows + ty) % nr) * kRfCols + tx] = make_float2(sa, sb);
            }
            __syncthreads();
            const int rel = k * kRfRows + ty - 2 * r;
            const int x = x0 + tx;
            if (rel >= 0 && rel < rows && x < g.W) {
                const int y = y0 + rel;
                float sa = 0.f, sb = 0.f;
                int row = rel % nr;
                for (int j = 0; j < win; ++j) {
                    const float2 h = ring[row * kRfCols + tx];
                    sa += h.x; sb += h.y;
                    row = row + 1 == nr ? 0 : row + 1;
                }
                const float nf = (float)window_count(y, x, g);
                const size_t o = (size_t)y * g.W + x;
                const float q = (sa / nf) * ((float)guide[o] / 255.f) + sb / nf;
                if (probs != nullptr) probs[(size_t)c * npx + o] = clip ? clamp01(q) : q;
                // this pixel is this thread's in every class: its running maximum needs no barrier
                const int s = rel * kRfCols + tx;
                float bv = q;
                int best = c;
                if (c > 0 && !(q > best_v[s])) { bv = best_v[s]; best = best_c[s]; }      // first maximum (np.argmax, blend_finalize.h)
                if (c + 1 < C) {
                    best_v[s] = bv; best_c[s] = (unsigned char)best;
                } else {
                    mask[o] = (unsigned char)best;
                    if (conf != nullptr) conf[o] = clamp01(bv);
                }
            }
        }
    }
}

inline int rows_per_block(int r, int cap) {
    const int want = 8 * r < 64 ? 64 : 8 * r;
    return want > cap ? cap : want;
}

int check_geometry(const char* who, int C, int H, int W, int r) {
    PYLC_REQUIRE(C >= 2 && C <= PYLC_MAX_CLASSES, "%s: n_classes=%d unsupported (2..%d)", who, C, PYLC_MAX_CLASSES);
    PYLC_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "%s: a %d x %d image (need H, W >= 1 and H*W < 2^31)", who, H, W);
    PYLC_REQUIRE(r >= 1 && r <= 64, "%s: radius %d outside [1, 64]", who, r);
    return PYLC_OK;
}

}  // namespace
}  // namespace pylc

using namespace pylc;

extern "C" int pylc_luma_u8(const unsigned char* img, int ch, int H, int W, unsigned char* out, void* stream) {
    PYLC_REQUIRE(img && out, "luma_u8: a NULL image or output");
    PYLC_REQUIRE(ch == 1 || ch == 3, "luma_u8: %d channels (1 or 3)", ch);
    PYLC_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "luma_u8: a %d x %d image (need H, W >= 1 and H*W < 2^31)", H, W);
    const long long npx = (long long)H * W;
    const long long want = cdiv<long long>(npx, 256);
    const int blocks = (int)(want < 16 * kNumCU ? want : 16 * kNumCU);
    hipLaunchKernelGGL(luma_u8_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), img, ch, npx, out);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_guided_coeffs(const float* p, long long plane_stride, long long row_pitch, const unsigned char* g, int C, int H, int W,
                                  int r, float eps, float* a, float* b, void* stream) {
    PYLC_REQUIRE(p && g && a && b, "guided_coeffs: a NULL probability volume, guide or coefficient buffer");
    if (int rc = check_geometry("guided_coeffs", C, H, W, r)) return rc;
    PYLC_REQUIRE(eps >= 1e-6f && eps <= 1.f, "guided_coeffs: eps %g outside [1e-6, 1]", (double)eps);
    PYLC_REQUIRE(row_pitch >= W, "guided_coeffs: row pitch %lld below the width %d", row_pitch, W);
    PYLC_REQUIRE(plane_stride >= (long long)(H - 1) * row_pitch + W, "guided_coeffs: plane stride %lld below one plane of %d rows of pitch %lld",
                 plane_stride, H, row_pitch);
    PYLC_REQUIRE(((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3) == 0,
                 "guided_coeffs: the fp32 buffers must be 4-B aligned");
    const RefineGeom geom{H, W, r, rows_per_block(r, 256)};
    const int nr = 2 * r + kRfRows, rw = kRfCols + 2 * r;
    const int lds = nr * kRfCols * 16 + kRfRows * rw * 9;
    static_assert((2 * 64 + kRfRows) * kRfCols * 16 + kRfRows * (kRfCols + 128) * 9 <= kRfMaxLds, "stage 1 at r = 64 must fit the LDS");
    PYLC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(guided_coeffs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kRfMaxLds));
    const dim3 grid(cdiv(W, kRfCols), cdiv(H, geom.rows_per_block), C);
    hipLaunchKernelGGL(guided_coeffs_kernel, grid, dim3(kRfCols, kRfRows), lds, as_stream(stream), p, plane_stride, row_pitch, g, geom, eps, a, b);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_guided_apply(const float* a, const float* b, const unsigned char* g, int C, int H, int W, int r, int clip,
                                 unsigned char* mask, float* probs, float* conf, void* stream) {
    PYLC_REQUIRE(a && b && g && mask, "guided_apply: a NULL coefficient buffer, guide or mask");
    if (int rc = check_geometry("guided_apply", C, H, W, r)) return rc;
    PYLC_REQUIRE(clip == 0 || clip == 1, "guided_apply: clip=%d (0 or 1)", clip);
    PYLC_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(probs) |
                   reinterpret_cast<uintptr_t>(conf)) & 3) == 0, "guided_apply: the fp32 buffers must be 4-B aligned");
    const RefineGeom geom{H, W, r, rows_per_block(r, 128)};
    const int nr = 2 * r + kRfRows, rw = kRfCols + 2 * r;
    const int lds = nr * kRfCols * 8 + kRfRows * rw * 8 + geom.rows_per_block * kRfCols * 5;
    static_assert((2 * 64 + kRfRows) * kRfCols * 8 + kRfRows * (kRfCols + 128) * 8 + 128 * kRfCols * 5 <= kRfMaxLds,
                  "stage 2 at r = 64 must fit the LDS");
    PYLC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(guided_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kRfMaxLds));
    const dim3 grid(cdiv(W, kRfCols), cdiv(H, geom.rows_per_block), 1);
    hipLaunchKernelGGL(guided_apply_kernel, grid, dim3(kRfCols, kRfRows), lds, as_stream(stream), a, b, g, geom, C, clip, mask, probs, conf);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}
