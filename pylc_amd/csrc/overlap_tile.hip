// Full-image U-Net inference by the overlap-tile method (U-Net paper, section 3; the geometry the reference records in
// config.py:225-236 -- input_size 512, output_size 324, the image padded by mirroring -- but never wires up: utils/tools.py:209-319
// reconstruct() assumes same-size tiles).  A valid-convolution U-Net maps a `tile` window to the centred `out = tile - 2*pad`
// square, so:
//
//   output-tile origins along an axis of length H:  o_i = min(i*stride, H - out),  i = 0 .. ceil((H - out) / stride)
//   tile (i, j) reads the window [o_i - pad, o_i + out + pad) x [o_j - pad, o_j + out + pad) of the image mirrored at its edges
//   (reflect-101: the edge pixel is not repeated, torch.nn.functional.pad(mode='reflect')); the clamped last tile keeps every
//   window within `pad` of the image, so one reflection suffices (pad < H, pad < W)
//   score of an image pixel = mean of the softmax probabilities of every tile that covers it (equal weights, summed in tile order:
//   rows ascending, then columns -- no atomics, deterministic); class = argmax, first maximum
//
// pack_tiles.hip's cutter cuts and normalises the windows straight from the device image (float or uint8); stitch_overlap_kernel here
// reads each pixel's covering logit tiles (<= ceil(out/stride)+1 per axis) and writes the uint8 mask, optionally the mean
// probabilities [C][H][W] (the reference's mask_fullsized layout).
#include "common.h"
#include "overlap_geom.h"      // the geometry: overlap_count, overlap_origin, overlap_cover, overlap_check; softmax_add

namespace pylc {

namespace {

struct OverlapGeom { int H, W, out, stride, rows, cols, pitch; };

// logits [rows*cols][out][out][pitch] (NHWC tiles, row-major tile order) -> mask [H][W] (uint8), probs [C][H][W] (fp32, optional).
// Lane q owns the linear pixels 4q .. 4q+3 (they may straddle a row or a tile edge: every pixel finds its own covering tiles); the
// pixels are visited one after the other (a rolled loop: an unrolled one holding the four pixels' C means spills at C >= 9), the
// mask bytes are collected and leave as one aligned dword.  probs, an optional extra output, is written per pixel.
template <int C>
__global__ __launch_bounds__(256) void stitch_overlap_kernel(const float* __restrict__ logits, OverlapGeom g, unsigned char* __restrict__ mask,
                                                              float* __restrict__ probs) {
    const long long total = (long long)g.H * g.W;
    const long long groups = cdiv<long long>(total, kOtPx);
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += (long long)gridDim.x * blockDim.x) {
        const long long base = q * kOtPx;
        const int np = total - base < kOtPx ? (int)(total - base) : kOtPx;
        unsigned int packed = 0;
#pragma unroll 1
        for (int p = 0; p < np; ++p) {
            const long long i = base + p;
            const int y = (int)(i / g.W), x = (int)(i - (long long)y * g.W);
            const Cover cy = overlap_cover(y, g.H, g.out, g.stride, g.rows);
            const Cover cx = overlap_cover(x, g.W, g.out, g.stride, g.cols);
            float acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 0.f;
            int n = 0;
            for (int a = cy.lo; a <= cy.hi + cy.last; ++a) {
                const int ti = a <= cy.hi ? a : g.rows - 1;
                const int ly = y - overlap_origin(ti, g.H, g.out, g.stride);
                for (int b = cx.lo; b <= cx.hi + cx.last; ++b) {
                    const int tj = b <= cx.hi ? b : g.cols - 1;
                    const int lx = x - overlap_origin(tj, g.W, g.out, g.stride);
                    const ot_f32x4* src = reinterpret_cast<const ot_f32x4*>(
                        logits + (((size_t)(ti * g.cols + tj) * g.out + ly) * g.out + lx) * g.pitch);
                    softmax_add<C>(src, acc);
                    ++n;
                }
            }
            const float fn = (float)n;
            int best = 0;
            float bv = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                acc[c] = acc[c] / fn;
                if (c == 0 || acc[c] > bv) { bv = acc[c]; best = c; }     // first maximum (np.argmax)
            }
            packed |= (unsigned int)best << (8 * p);
            if (probs != nullptr) {
#pragma unroll
                for (int c = 0; c < C; ++c) probs[(size_t)c * total + i] = acc[c];
            }
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

using namespace pylc;

extern "C" int pylc_stitch_overlap_argmax(const float* logits, int pitch, int n_tiles, int H, int W, int out, int stride, int C,
                                          unsigned char* mask, float* probs, void* stream) {
    PYLC_REQUIRE(logits && mask && pitch >= C && pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0,
                 "stitch_overlap_argmax: logits must be 16-B aligned NHWC tiles with a pitch >= C, multiple of 4");
    if (int rc = overlap_check("stitch_overlap_argmax", H, W, out, stride, 0)) return rc;
    const int rows = overlap_count(H, out, stride), cols = overlap_count(W, out, stride);
    PYLC_REQUIRE((long long)rows * cols == n_tiles, "stitch_overlap_argmax: %d tiles given, the %dx%d grid needs %d", n_tiles, rows, cols,
                 rows * cols);
    const OverlapGeom g{H, W, out, stride, rows, cols, pitch};
    const int blocks = ot_grid(cdiv<long long>((long long)H * W, kOtPx));
    hipStream_t st = as_stream(stream);
#define LAUNCH_OT(CC) hipLaunchKernelGGL((stitch_overlap_kernel<CC>), dim3(blocks), dim3(256), 0, st, logits, g, mask, probs)
    PYLC_FOR_CLASSES(C, LAUNCH_OT, "stitch_overlap_argmax")
#undef LAUNCH_OT
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}
