// The per-step training augmenter: output sample k is source plane set src_index[k] under an inverse affine map
// of six int64 numbers in Q24 fixed point, bilinear (32 steps per axis) for the image with a 256-entry tone table per sample and channel,
// nearest for the mask and its weight map.  Every operation is on integers, so the result is exact, independent of the launch, and a lane
// may walk along a row by ADDING a00 / a10: the sums are the products, bit for bit (tests/_batch_augment.py is the statement).
//
//   X = a00 x + a01 y + a02, Y = a10 x + a11 y + a12                          (int64; pixel centres at integers)
//   image:  sx = X >> 24, fx = (X >> 19) & 31, likewise sy, fy
//           N = (t(sy,sx)(32-fx) + t(sy,sx+1) fx)(32-fy) + (t(sy+1,sx)(32-fx) + t(sy+1,sx+1) fx) fy;  out = lut[(N + 512) >> 10]
//   mask, weights:  mx = (X + 2^23) >> 24, my likewise
//   border: constant (fill[c] / mask_fill / 0.0f outside) or BORDER_REFLECT_101 for any integer index
//
// batch_augment_kernel<C, REFLECT>: grid (samples, bands of output rows), 256 threads.  The block stages its sample's tone tables (768
// bytes; the identity without one) in LDS.  A lane makes a run of 4 adjacent output pixels of one row: one 64-bit multiply-add for the
// run's first coordinate, then additions; per pixel the tap offsets and weights are computed once and serve every channel.  The taps are
// gathers from global memory, two bytes at once for the two taps of a row (the sources were just written or read: they come out of L2 /
// Infinity Cache, as in augment_kernel), issued for every tap -- a tap outside reads a valid offset and is replaced -- so that no branch
// stands between one pixel's gathers and the next one's.  The 4 bytes per plane leave as one dword where the destination is aligned (a
// wave stores 256 contiguous bytes), the 4 weights as one float4.  Why 4 and not tile_bytes.h's group of 16: measured, a run of 16 was
// no faster at the same band (143 us against 143 us for 32 samples of 512^2 RGB + mask) and needs 94-119 VGPRs where this needs 73;
// what paid was more and shorter blocks (the default band) and the two-byte gathers: 82 us.  No atomics, no
// floating point but the copied weights, and no division per pixel (the reflection's remainder is taken only by taps outside the source).
#include "tile_bytes.h"

namespace pylc {

namespace {

constexpr int kBaRun = 4;                        // output pixels per lane and item: one dword per plane (see the kernel's comment)
constexpr int kBaAutoBandPixels = 4096;          // the default band: 8 rows of a 512 output (measured best of 4 .. 128: section 5.26)
constexpr int kBaMaxOut = 16384;                 // with the matrix bounds below, X and Y stay inside int64 (and X >> 24 inside int32)
constexpr int kBaHostChunk = 32;                 // samples per launch when indices or matrices travel as kernel arguments
constexpr long long kBaLinearMax = 1ll << 32;    // |a00|, |a01|, |a10|, |a11| <= 2^32: a magnification of 1/256 at the least
constexpr long long kBaShiftLimit = 1ll << 44;   // |a02|, |a12| < 2^44

struct BaHost {                                  // what a host caller's arrays become: no upload, no allocation
    long long mats[kBaHostChunk][6];
    int src[kBaHostChunk];
};

struct BaArgs {
    const unsigned char* img;                    // [n_src][C][Hs][Ws]
    const unsigned char* mask;                   // [n_src][Hs][Ws] or NULL
    const float* weights;                        // [n_src][Hs][Ws] or NULL
    const int* src_index;                        // device [m], or NULL: host.src
    const long long* mats;                       // device [m][6], or NULL: host.mats
    const unsigned char* lut;                    // device [m][C][256] or NULL
    unsigned char* out_img;                      // [m][C][oh][ow]
    unsigned char* out_mask;                     // [m][oh][ow] or NULL
    float* out_weights;                          // [m][oh][ow] or NULL
    long long n_src, first;                      // this launch makes samples first + blockIdx.x
    int Hs, Ws, oh, ow, band_rows, reflect, mask_fill;
    int fill[3];
    BaHost host;
};

__host__ __device__ inline bool ba_matrix_ok(const long long* a) {
    for (int k = 0; k < 6; ++k) {
        if (a[k] == (-0x7fffffffffffffffll - 1)) return false;
        const long long v = a[k] < 0 ? -a[k] : a[k];
        if ((k % 3 == 2) ? v >= kBaShiftLimit : v > kBaLinearMax) return false;
    }
    return true;
}

// BORDER_REFLECT_101 of any index: period 2(n - 1)
__device__ __forceinline__ int ba_refl(int p, int n) {
    if ((unsigned)p < (unsigned)n) return p;
    const unsigned period = 2u * (unsigned)n - 2u;
    const unsigned q = (p < 0 ? 0u - (unsigned)p : (unsigned)p) % period;
    return q < (unsigned)n ? (int)q : (int)(period - q);
}

// the run's four bytes of one plane: one dword where the destination is aligned and the run whole
__device__ __forceinline__ void store_run(unsigned char* p, unsigned int v, int valid) {
    if (valid == kBaRun && ((unsigned long long)p & 3u) == 0) {
        *reinterpret_cast<unsigned int*>(p) = v;
    } else {
#pragma unroll
        for (int k = 0; k < kBaRun; ++k)
            if (k < valid) p[k] = (unsigned char)(v >> (8 * k));
    }
}

// the index a tap reads and whether the tap lies inside the source: reflected (always inside), or 0 for a tap outside -- valid either way
template <bool REFLECT>
__device__ __forceinline__ int ba_tap(int p, int n, bool& inside) {
    if (REFLECT) {
        inside = true;
        return ba_refl(p, n);
    }
    inside = (unsigned)p < (unsigned)n;
    return inside ? p : 0;
}

template <int C, bool REFLECT>
__global__ __launch_bounds__(kDsThreads) void batch_augment_kernel(BaArgs a) {
    __shared__ unsigned char lut[C * 256];
    const int tid = threadIdx.x;
    const long long n = a.first + blockIdx.x;
    const long long src = a.src_index ? a.src_index[n] : a.host.src[blockIdx.x];
    long long M[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) M[k] = a.mats ? a.mats[n * 6 + k] : a.host.mats[blockIdx.x][k];
    if (src < 0 || src >= a.n_src || !ba_matrix_ok(M)) return;      // the caller's error; nothing is read or written for this sample
    const int Hs = a.Hs, Ws = a.Ws, oh = a.oh, ow = a.ow;
    for (int i = tid; i < C * 256; i += kDsThreads) lut[i] = a.lut ? a.lut[n * C * 256 + i] : (unsigned char)i;
    __syncthreads();

    const long long plane = (long long)Hs * Ws;
    const unsigned char* const simg = a.img + src * C * plane;
    const unsigned char* const smask = a.mask ? a.mask + src * plane : nullptr;
    const float* const sw = a.weights ? a.weights + src * plane : nullptr;
    const int r0 = blockIdx.y * a.band_rows;
    const int r1 = r0 + a.band_rows < oh ? r0 + a.band_rows : oh;
    const int G = cdiv(ow, kBaRun);
    const int items = (r1 - r0) * G;
    const long long oplane = (long long)oh * ow;

    for (int j = tid; j < items; j += kDsThreads) {
        const int r = j / G, xg = (j - r * G) * kBaRun, y = r0 + r;
        const int valid = ow - xg < kBaRun ? ow - xg : kBaRun;
        const long long X0 = M[0] * xg + (M[1] * y + M[2]);
        const long long Y0 = M[3] * xg + (M[4] * y + M[5]);
        const long long at = (long long)y * ow + xg;
        // Every pixel of the run is computed, the ragged last group's beyond `ow` too: their addresses are as valid, only the stores look
        // at `valid`, and the loop has no branch that keeps one pixel's gathers from being issued before the previous pixel's have arrived.
        {
            unsigned int w[C];
#pragma unroll
            for (int c = 0; c < C; ++c) w[c] = 0u;
            long long X = X0, Y = Y0;
#pragma unroll
            for (int k = 0; k < kBaRun; ++k) {
                const int sx = (int)(X >> 24), sy = (int)(Y >> 24);
                const int fx = (int)(X >> 19) & 31, fy = (int)(Y >> 19) & 31;
                bool ix0, ix1, iy0, iy1;
                const int x0 = ba_tap<REFLECT>(sx, Ws, ix0), x1 = ba_tap<REFLECT>(sx + 1, Ws, ix1);
                const int y0 = ba_tap<REFLECT>(sy, Hs, iy0) * Ws, y1 = ba_tap<REFLECT>(sy + 1, Hs, iy1) * Ws;
                // The two taps of a row are neighbours in memory -- reflected indices differ by one at the turning points too, and an inside
                // tap of the constant border is column xl or xl + 1 of xl = clamp(sx, 0, Ws - 2) -- so ONE two-byte load (at any alignment)
                // brings both, and a pixel costs two gather instructions per channel, not four.
                const int xl = REFLECT ? (x0 < x1 ? x0 : x1) : (sx < 0 ? 0 : (sx > Ws - 2 ? Ws - 2 : sx));
                const int s0 = REFLECT || ix0 ? 8 * (x0 - xl) : 0, s1 = REFLECT || ix1 ? 8 * (x1 - xl) : 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const unsigned char* p = simg + c * plane;
                    const int f = a.fill[c];
                    unsigned short top, bot;
                    __builtin_memcpy(&top, p + y0 + xl, 2);
                    __builtin_memcpy(&bot, p + y1 + xl, 2);
                    int t00 = (top >> s0) & 255, t01 = (top >> s1) & 255, t10 = (bot >> s0) & 255, t11 = (bot >> s1) & 255;
                    if (!REFLECT) {
                        t00 = iy0 && ix0 ? t00 : f; t01 = iy0 && ix1 ? t01 : f;
                        t10 = iy1 && ix0 ? t10 : f; t11 = iy1 && ix1 ? t11 : f;
                    }
                    const int N = (t00 * (32 - fx) + t01 * fx) * (32 - fy) + (t10 * (32 - fx) + t11 * fx) * fy;
                    w[c] |= (unsigned int)lut[c * 256 + ((N + 512) >> 10)] << (8 * k);
                }
                X += M[0];
                Y += M[3];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) store_run(a.out_img + (n * C + c) * oplane + at, w[c], valid);
        }
        if (smask || sw) {                                                  // nearest: ONE offset serves the mask and the weight
            unsigned int wm = 0u;
            float wf[kBaRun];
            long long X = X0 + (1ll << 23), Y = Y0 + (1ll << 23);
#pragma unroll
            for (int k = 0; k < kBaRun; ++k) {
                bool inx, iny;
                const int o = ba_tap<REFLECT>((int)(Y >> 24), Hs, iny) * Ws + ba_tap<REFLECT>((int)(X >> 24), Ws, inx);
                const bool in = inx && iny;
                if (smask) {
                    const int v = smask[o];
                    wm |= (unsigned int)(in ? v : a.mask_fill) << (8 * k);
                }
                wf[k] = 0.f;
                if (sw) {
                    const float v = sw[o];
                    wf[k] = in ? v : 0.f;
                }
                X += M[0];
                Y += M[3];
            }
            if (smask) store_run(a.out_mask + n * oplane + at, wm, valid);
            if (sw) {
                float* q = a.out_weights + n * oplane + at;
                if (valid == kBaRun && ((unsigned long long)q & 15u) == 0) {
                    *reinterpret_cast<float4*>(q) = make_float4(wf[0], wf[1], wf[2], wf[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < kBaRun; ++k)
                        if (k < valid) q[k] = wf[k];
                }
            }
        }
    }
}

// whether the device can read p: anything the runtime does not know as device (or managed) memory is the host's
bool ba_on_device(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

}  // namespace
}  // namespace pylc

using namespace pylc;

extern "C" int pylc_batch_augment(const unsigned char* img, const unsigned char* mask, const float* weights, long long n_src, int Cimg,
                                  int Hs, int Ws, const int* src_index, const long long* mats, const unsigned char* lut, long long m,
                                  int oh, int ow, int border, const unsigned char* fill, int mask_fill, int band_rows,
                                  unsigned char* out_img, unsigned char* out_mask, float* out_weights, void* stream) {
    PYLC_REQUIRE(Cimg == 1 || Cimg == 3, "batch_augment: Cimg=%d, not 1 or 3", Cimg);
    PYLC_REQUIRE(Hs >= 2 && Ws >= 2 && (long long)Hs * Ws < (1ll << 31), "batch_augment: source %dx%d (HxW) below 2 or above 2^31 pixels", Hs, Ws);
    PYLC_REQUIRE(oh >= 1 && ow >= 1 && oh <= kBaMaxOut && ow <= kBaMaxOut, "batch_augment: output %dx%d (HxW) outside 1..%d", oh, ow, kBaMaxOut);
    PYLC_REQUIRE(n_src > 0 && m >= 0 && m < (1ll << 31), "batch_augment: n_src=%lld m=%lld", n_src, m);
    PYLC_REQUIRE(border == PYLC_BORDER_CONSTANT || border == PYLC_BORDER_REFLECT, "batch_augment: border=%d, not %d (constant) or %d (reflect)",
                 border, PYLC_BORDER_CONSTANT, PYLC_BORDER_REFLECT);
    PYLC_REQUIRE(mask_fill >= 0 && mask_fill <= 255, "batch_augment: mask_fill=%d outside 0..255", mask_fill);
    PYLC_REQUIRE(border != PYLC_BORDER_CONSTANT || fill, "batch_augment: a constant border without fill values");
    PYLC_REQUIRE((mask != nullptr) == (out_mask != nullptr), "batch_augment: masks and their output come together");
    PYLC_REQUIRE((weights != nullptr) == (out_weights != nullptr), "batch_augment: weights and their output come together");
    PYLC_REQUIRE(((unsigned long long)weights & 3u) == 0 && ((unsigned long long)out_weights & 3u) == 0 && ((unsigned long long)mats & 7u) == 0 &&
                     ((unsigned long long)src_index & 3u) == 0, "batch_augment: a misaligned weight, matrix or index pointer");
    if (m == 0) return PYLC_OK;
    PYLC_REQUIRE(img && src_index && mats && out_img, "batch_augment: a NULL image, index, matrix or output pointer");
    const bool src_dev = ba_on_device(src_index), mats_dev = ba_on_device(mats);
    if (!src_dev)
        for (long long k = 0; k < m; ++k)
            PYLC_REQUIRE(src_index[k] >= 0 && src_index[k] < n_src, "batch_augment: src_index[%lld]=%d outside 0..%lld", k, src_index[k], n_src - 1);
    if (!mats_dev)
        for (long long k = 0; k < m; ++k)
            PYLC_REQUIRE(ba_matrix_ok(mats + k * 6),
                         "batch_augment: matrix %lld outside |a00|,|a01|,|a10|,|a11| <= 2^32 (Q24: a magnification of 1/256) and |a02|,|a12| < 2^44", k);
    if (band_rows <= 0) {
        band_rows = kBaAutoBandPixels / ow;
        band_rows = band_rows < 1 ? 1 : band_rows;
    }
    if (band_rows > oh) band_rows = oh;
    BaArgs a;
    memset(&a, 0, sizeof(a));
    a.img = img; a.mask = mask; a.weights = weights; a.lut = lut;
    a.src_index = src_dev ? src_index : nullptr; a.mats = mats_dev ? mats : nullptr;
    a.out_img = out_img; a.out_mask = out_mask; a.out_weights = out_weights;
    a.n_src = n_src;
    a.Hs = Hs; a.Ws = Ws; a.oh = oh; a.ow = ow; a.band_rows = band_rows;
    a.reflect = border == PYLC_BORDER_REFLECT; a.mask_fill = mask_fill;
    for (int c = 0; c < Cimg; ++c) a.fill[c] = fill ? fill[c] : 0;
    const long long chunk = (src_dev && mats_dev) ? m : kBaHostChunk;      // one launch, unless host arrays travel as kernel arguments
    for (long long first = 0; first < m; first += chunk) {
        const long long count = m - first < chunk ? m - first : chunk;
        a.first = first;
        if (!src_dev) memcpy(a.host.src, src_index + first, count * sizeof(int));
        if (!mats_dev) memcpy(a.host.mats, mats + first * 6, count * 6 * sizeof(long long));
        const dim3 grid((unsigned)count, (unsigned)cdiv(oh, band_rows));
        if (Cimg == 3 && a.reflect) hipLaunchKernelGGL((batch_augment_kernel<3, true>), grid, dim3(kDsThreads), 0, as_stream(stream), a);
        else if (Cimg == 3) hipLaunchKernelGGL((batch_augment_kernel<3, false>), grid, dim3(kDsThreads), 0, as_stream(stream), a);
        else if (a.reflect) hipLaunchKernelGGL((batch_augment_kernel<1, true>), grid, dim3(kDsThreads), 0, as_stream(stream), a);
        else hipLaunchKernelGGL((batch_augment_kernel<1, false>), grid, dim3(kDsThreads), 0, as_stream(stream), a);
        PYLC_LAUNCH_CHECK();
    }
    return PYLC_OK;
}
