// The overlap-tile geometry shared by csrc/pack_tiles.hip (the tile cutter), csrc/overlap_tile.hip (the one-shot blend) and
// csrc/blend.hip (the streaming blend):
//
//   output-tile origins along an axis of length n:  o_i = min(i*stride, n - out),  i = 0 .. ceil((n - out) / stride), tiles in
//   row-major order; 1 <= stride <= out <= n.  A fitted image, (n - out) % stride == 0, is the case in which the clamp is never active.
#pragma once
#include "common.h"

namespace pylc {

typedef float ot_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kOtPx = 4;      // consecutive pixels per lane: the mask leaves as one dword per lane

// number of output-tile origins along an axis of length n (n >= out)
__host__ __device__ inline int overlap_count(int n, int out, int stride) { return (n - out + stride - 1) / stride + 1; }

// origin of tile i along an axis of length n
__host__ __device__ __forceinline__ int overlap_origin(int i, int n, int out, int stride) {
    const int o = i * stride;
    return o < n - out ? o : n - out;
}

// tiles covering coordinate y along an axis: the unclamped tiles lo .. hi (origin i*stride), then the clamped last tile cnt-1 when
// y >= n - out.  Visited as a = lo .. hi + last, tile = a <= hi ? a : cnt - 1 (ascending either way; lo <= hi + 1 always).
struct Cover { int lo, hi, last; };
__device__ __forceinline__ Cover overlap_cover(int y, int n, int out, int stride, int cnt) {
    Cover c;
    c.lo = y < out ? 0 : (y - out) / stride + 1;
    const int h = y / stride;
    c.hi = h < cnt - 2 ? h : cnt - 2;
    c.last = y >= n - out ? 1 : 0;
    return c;
}

// acc[c] += softmax(v)[c] for the C logits that start at the 16-byte aligned `src` (pitch >= C rounded up to 4): the per-tile term of the
// mean-probability blend, stated once so that the one-shot and the streaming blend add the same bits in the same order.
// TEMP (pylc_blend_accumulate_t): softmax(beta * v), the exponent taken as (v - max) * beta -- beta = 1 multiplies by
// 1.0f, which is exact, and gives the bytes of the plain form; without TEMP `beta` is not read and the code is the plain form's.
// WIN (pylc_blend_accumulate_w): acc[c] += wt * (v[c] * inv), the plain term times the tile's window weight before the
// add -- wt = 1 is exact again; without WIN `wt` is not read.
template <int C, int N, bool TEMP = false, bool WIN = false>
__device__ __forceinline__ void softmax_add(const ot_f32x4* __restrict__ src, float (&acc)[N], float beta = 1.f, float wt = 1.f) {
    constexpr int NV = (C + 3) / 4;
    float v[NV * 4];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const ot_f32x4 t = src[k];
        v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
    }
    float m = v[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if constexpr (TEMP) v[c] = expf((v[c] - m) * beta);
        else v[c] = expf(v[c] - m);
        s += v[c];
    }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if constexpr (WIN) acc[c] += wt * (v[c] * inv);
        else acc[c] += v[c] * inv;
    }
}

__device__ __forceinline__ int reflect101(int y, int n) {
    y = y < 0 ? -y : y;
    return y >= n ? 2 * (n - 1) - y : y;
}

inline int ot_grid(long long n) {
    const long long b = cdiv<long long>(n, 256);
    return (int)(b < 8192 ? (b < 1 ? 1 : b) : 8192);
}

// the geometry every entry point accepts (pylc_amd/inference.py:overlap_tile_grid raises on the same conditions)
inline int overlap_check(const char* who, int H, int W, int out, int stride, int pad) {
    PYLC_REQUIRE(out > 0 && pad >= 0, "%s: out=%d pad=%d", who, out, pad);
    PYLC_REQUIRE(stride >= 1 && stride <= out, "%s: stride %d outside [1, out=%d]", who, stride, out);
    PYLC_REQUIRE(H >= out && W >= out, "%s: image %dx%d smaller than the output tile %d", who, H, W, out);
    PYLC_REQUIRE(pad < H && pad < W, "%s: pad %d must be below the image size %dx%d (one reflection)", who, pad, H, W);
    return PYLC_OK;
}

}  // namespace pylc
