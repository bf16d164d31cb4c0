// Photograph-side steps of the reference's test path (test.py:23-115) that precede and follow the network, on the GPU:
//
//   resize_area_kernel          cv2.resize(..., INTER_AREA) of a decoded photograph: the --scale step of get_image
//                               (utils/tools.py:77-148) and the fit to the tile grid of adjust_to_tile (utils/tools.py:151-206)
//   class_encode_resize_kernel  cv2.resize(..., INTER_NEAREST) of an RGB mask followed by class_encode (utils/tools.py:412-449):
//                               the ground truth of Evaluator.load (utils/evaluate.py:64-118) and the predicted colour mask
//
// INTER_AREA is OpenCV's general downscale (resizeArea with computeResizeAreaTab).  Per axis, scale = 1 / (dst / src) in double
// (cv::resize passes dst/src, the area path inverts it).  Output d covers [d*scale, d*scale + scale) clipped to the source; the partial
// first and last source cells get fractional weights, slivers of <= 1e-3 are dropped, and every weight is a double quotient by the cell
// width stored as float.  Accumulation is OpenCV's, in fp32: for each contributing source row (ascending), the row's weighted sum over
// the contributing columns (ascending), then acc += beta * rowsum; the byte is cvRound (to nearest, ties to even).  -ffp-contract=off
// (Makefile) keeps every product and sum a separate rounding, as OpenCV's scalar loop has it.  OpenCV's own fast path for integer
// factors (resizeAreaFast: its 2x2 case rounds ties up) is not reproduced: the general weights give the plain box mean there.
//
// The taps of an output coordinate are contiguous source indices s0 .. s0+n-1 whose weights differ only at the ends, so five words
// describe them (AreaTaps).  A block computes the taps of its 8 rows and ~131 columns once into LDS; each lane then produces four
// consecutive bytes of the flat planar output and stores them as one aligned dword.  Below a scale of 6 the tap loops are unrolled to
// ceil(scale) + 1 per axis (resize_area_kernel<K>): with loop bounds the loads of a pixel wait for one another and the kernel is latency-bound.
#include "common.h"

namespace pylc {

namespace {

struct AreaTaps { int s0, n; float a_first, a_mid, a_last; };

// computeResizeAreaTab for output coordinate d along an axis of ssize source pixels (scale >= 1)
__device__ AreaTaps area_taps(int d, int ssize, double scale) {
    const double f1 = d * scale;
    const double f2 = f1 + scale;
    const double cell = fmin(scale, ssize - f1);
    int s2 = (int)floor(f2);
    s2 = s2 < ssize - 1 ? s2 : ssize - 1;
    int s1 = (int)ceil(f1);
    s1 = s1 < s2 ? s1 : s2;
    const bool head = s1 - f1 > 1e-3;
    const bool tail = f2 - s2 > 1e-3;
    const float mid = (float)(1.0 / cell);
    const float ah = head ? (float)((s1 - f1) / cell) : mid;
    const float at = tail ? (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell) : mid;
    AreaTaps t;
    t.s0 = head ? s1 - 1 : s1;
    t.n = (int)head + (s2 - s1) + (int)tail;
    t.a_mid = mid;
    t.a_first = head ? ah : (s2 > s1 ? mid : at);
    t.a_last = tail ? at : (s2 > s1 ? mid : ah);
    return t;
}

__device__ __forceinline__ float area_w(const AreaTaps& t, int k) { return k == 0 ? t.a_first : (k == t.n - 1 ? t.a_last : t.a_mid); }

// one output byte; src points at the channel's first sample.  K > 0: at most K taps per axis (K >= ceil(scale) + 1, which bounds
// computeResizeAreaTab's count), every loop unrolled to K with the missing taps as weight 0 at a valid index -- adding +0 * x to a sum of
// non-negative terms leaves it bit for bit unchanged, and the loads no longer wait for one another.  K = 0: the counts as loop bounds.
template <int K>
__device__ __forceinline__ unsigned int area_pixel(const unsigned char* __restrict__ src, int row_pitch, int px_stride, const AreaTaps& ty,
                                                   const AreaTaps& tx) {
    float acc = 0.f;
    if (K == 0) {
        for (int a = 0; a < ty.n; ++a) {
            const unsigned char* row = src + (size_t)(ty.s0 + a) * row_pitch + (size_t)tx.s0 * px_stride;
            float r = 0.f;
            for (int b = 0; b < tx.n; ++b) r += (float)row[b * px_stride] * area_w(tx, b);
            acc += area_w(ty, a) * r;
        }
    } else {
#pragma unroll
        for (int a = 0; a < K; ++a) {
            const unsigned char* row = src + (size_t)(ty.s0 + (a < ty.n ? a : ty.n - 1)) * row_pitch;
            float r = 0.f;
#pragma unroll
            for (int b = 0; b < K; ++b) {
                const float s = (float)row[(tx.s0 + (b < tx.n ? b : tx.n - 1)) * px_stride];
                r += s * (b < tx.n ? area_w(tx, b) : 0.f);
            }
            acc += (a < ty.n ? area_w(ty, a) : 0.f) * r;
        }
    }
    const int v = (int)__builtin_rintf(acc);
    return (unsigned int)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

constexpr int kRaRows = 8;                    // output rows per block
constexpr int kRaGroups = 32;                 // dword groups per block row: 128 columns
constexpr int kRaCols = 4 * kRaGroups + 3;    // columns a block row can touch (its groups start 0..3 columns into the row)

struct AreaGeom {
    int H, W, C, oh, ow, px_stride, row_pitch, ch_stride;
    double sy, sx;
};

// dst [C][oh][ow] seen as one plane of C*oh rows.  Row Y's first dword-aligned flat offset lies h0 = (-Y*ow) & 3 columns in; lane (r, j) of
// the block owns the four flat bytes from column h0 + 4j of row R0 + r, which for the row's last group run on into the next row (those
// few pixels compute their taps directly).  Each byte stays inside its channel's source plane; only the tensor's last group can be short.
// The taps of the four pixels are gathered first, then their loads and sums run as one straight-line body.  (Flat sizes < 2^31: checked.)
template <int K>
__global__ __launch_bounds__(256) void resize_area_kernel(const unsigned char* __restrict__ src, AreaGeom g, unsigned char* __restrict__ dst) {
    __shared__ AreaTaps xs[kRaCols];
    __shared__ AreaTaps ys[kRaRows];
    const int rows = g.C * g.oh;
    const int R0 = blockIdx.y * kRaRows;
    const int X0 = 4 * kRaGroups * blockIdx.x;
    for (int i = threadIdx.x; i < kRaCols; i += blockDim.x)
        if (X0 + i < g.ow) xs[i] = area_taps(X0 + i, g.W, g.sx);
    if (threadIdx.x < kRaRows && R0 + (int)threadIdx.x < rows) ys[threadIdx.x] = area_taps((R0 + threadIdx.x) % g.oh, g.H, g.sy);
    __syncthreads();
    const int r = threadIdx.x / kRaGroups;
    const int Y = R0 + r;
    if (Y >= rows) return;
    const int row_lin = Y * g.ow;
    const int col0 = ((-row_lin) & 3) + X0 + 4 * (threadIdx.x % kRaGroups);
    if (col0 >= g.ow) return;
    const int lin0 = row_lin + col0;
    const int total = rows * g.ow;
    const int np = total - lin0 < 4 ? total - lin0 : 4;
    const int c0 = Y / g.oh;
    AreaTaps ty[4], tx[4];
    int ch[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int col = col0 + p;
        if (col < g.ow) {
            ty[p] = ys[r];
            tx[p] = xs[col - X0];
            ch[p] = c0;
        } else if (p < np) {
            const int Y2 = (lin0 + p) / g.ow;
            ty[p] = area_taps(Y2 % g.oh, g.H, g.sy);
            tx[p] = area_taps(lin0 + p - Y2 * g.ow, g.W, g.sx);
            ch[p] = Y2 / g.oh;
        } else {                                                   // past the tensor's end: any valid taps, the byte is not stored
            ty[p] = ys[r];
            tx[p] = xs[col0 - X0];
            ch[p] = c0;
        }
    }
    unsigned int packed = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) packed |= area_pixel<K>(src + (size_t)ch[p] * g.ch_stride, g.row_pitch, g.px_stride, ty[p], tx[p]) << (8 * p);
    if (np == 4) {
        *reinterpret_cast<unsigned int*>(dst + lin0) = packed;      // lin0 % 4 == 0: an aligned dword
    } else {
        for (int p = 0; p < np; ++p) dst[lin0 + p] = (unsigned char)(packed >> (8 * p));
    }
}

// out[oy][ox] = class_encode(rgb[min(floor(oy*fy), H-1)][min(floor(ox*fx), W-1)]): the LAST palette index whose colour matches (the
// reference's loop overwrites), `unmatched` when none does (1 is its np.ones).  Four consecutive flat pixels per lane, their twelve loads issued together,
// one dword store.  (Flat sizes < 2^31: checked.)
__global__ __launch_bounds__(256) void class_encode_resize_kernel(const unsigned char* __restrict__ rgb, int H, int W,
                                                                  const unsigned char* __restrict__ palette, int C, unsigned char* __restrict__ out,
                                                                  int oh, int ow, double fy, double fx, unsigned int unmatched) {
    __shared__ unsigned int pal[PYLC_MAX_CLASSES];
    if (threadIdx.x < C) pal[threadIdx.x] = palette[3 * threadIdx.x] | (palette[3 * threadIdx.x + 1] << 8) | (palette[3 * threadIdx.x + 2] << 16);
    __syncthreads();
    const int total = oh * ow;
    const int groups = cdiv(total, 4);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
        const int base = 4 * q;
        const int np = total - base < 4 ? total - base : 4;
        unsigned int colour[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = base + (p < np ? p : 0);
            const int oy = i / ow, ox = i - oy * ow;
            int sy = (int)floor(oy * fy), sx = (int)floor(ox * fx);        // cv2.INTER_NEAREST (resizeNN)
            sy = sy < H - 1 ? sy : H - 1;
            sx = sx < W - 1 ? sx : W - 1;
            const unsigned char* s = rgb + (sy * W + sx) * 3;
            colour[p] = s[0] | (s[1] << 8) | (s[2] << 16);
        }
        unsigned int packed = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            unsigned int cls = unmatched;
            for (int k = 0; k < C; ++k)
                if (pal[k] == colour[p]) cls = k;
            packed |= cls << (8 * p);
        }
        if (np == 4) {
            *reinterpret_cast<unsigned int*>(out + base) = packed;
        } else {
            for (int p = 0; p < np; ++p) out[base + p] = (unsigned char)(packed >> (8 * p));
        }
    }
}

inline int ph_grid(long long n) {
    const long long b = cdiv<long long>(n, 256);
    return (int)(b < 8192 ? (b < 1 ? 1 : b) : 8192);
}

}  // namespace
}  // namespace pylc

using namespace pylc;

extern "C" int pylc_resize_area_u8(const unsigned char* src, int src_planar, int Cimg, int H, int W, unsigned char* dst, int oh, int ow,
                                   void* stream) {
    PYLC_REQUIRE(src && dst && (Cimg == 1 || Cimg == 3) && H > 0 && W > 0 && oh > 0 && ow > 0, "resize_area_u8: bad arguments");
    PYLC_REQUIRE(oh <= H && ow <= W, "resize_area_u8: %dx%d -> %dx%d would upscale (INTER_AREA downscales only here)", H, W, oh, ow);
    PYLC_REQUIRE((long long)H * W * Cimg < (1LL << 31) && (long long)oh * ow * Cimg < (1LL << 31), "resize_area_u8: image too large");
    const int yblocks = cdiv(Cimg * oh, kRaRows);
    PYLC_REQUIRE(yblocks <= 65535, "resize_area_u8: %d output rows exceed the launch grid", oh);
    AreaGeom g;
    g.H = H; g.W = W; g.C = Cimg; g.oh = oh; g.ow = ow;
    g.px_stride = src_planar ? 1 : Cimg;
    g.row_pitch = W * g.px_stride;
    g.ch_stride = src_planar ? H * W : 1;
    g.sy = 1.0 / ((double)oh / H);
    g.sx = 1.0 / ((double)ow / W);
    // taps per axis <= floor(f2) - floor(f1) + 1 <= ceil(scale) + 1
    const int k = (int)ceil(g.sy > g.sx ? g.sy : g.sx) + 1;
    const dim3 grid((unsigned)cdiv(cdiv(ow, 4), kRaGroups), (unsigned)yblocks);
    hipStream_t st = as_stream(stream);
#define LAUNCH_RA(KK) hipLaunchKernelGGL(resize_area_kernel<KK>, grid, dim3(256), 0, st, src, g, dst)
    switch (k) {
        case 2: LAUNCH_RA(2); break; case 3: LAUNCH_RA(3); break; case 4: LAUNCH_RA(4); break; case 5: LAUNCH_RA(5); break;
        case 6: LAUNCH_RA(6); break; case 7: LAUNCH_RA(7); break;
        default: LAUNCH_RA(0); break;
    }
#undef LAUNCH_RA
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_class_encode_resize_ex(const unsigned char* rgb, int H, int W, const unsigned char* palette_rgb, int n_classes,
                                           unsigned char* out, int oh, int ow, int unmatched_value, void* stream) {
    PYLC_REQUIRE(rgb && palette_rgb && out && H > 0 && W > 0 && oh > 0 && ow > 0, "class_encode_resize: bad arguments");
    PYLC_REQUIRE(n_classes >= 1 && n_classes <= PYLC_MAX_CLASSES, "class_encode_resize: n_classes=%d outside 1..%d", n_classes, PYLC_MAX_CLASSES);
    PYLC_REQUIRE(unmatched_value >= 0 && unmatched_value <= 255, "class_encode_resize: unmatched_value=%d outside 0..255", unmatched_value);
    PYLC_REQUIRE((long long)H * W * 3 < (1LL << 31) && (long long)oh * ow < (1LL << 31), "class_encode_resize: image too large");
    const long long groups = cdiv<long long>((long long)oh * ow, 4);
    hipLaunchKernelGGL(class_encode_resize_kernel, dim3(ph_grid(groups)), dim3(256), 0, as_stream(stream), rgb, H, W, palette_rgb, n_classes, out,
                       oh, ow, 1.0 / ((double)oh / H), 1.0 / ((double)ow / W), (unsigned int)unmatched_value);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_class_encode_resize(const unsigned char* rgb, int H, int W, const unsigned char* palette_rgb, int n_classes,
                                        unsigned char* out, int oh, int ow, void* stream) {
    return pylc_class_encode_resize_ex(rgb, H, W, palette_rgb, n_classes, out, oh, ow, 1, stream);      // the reference's np.ones
}
