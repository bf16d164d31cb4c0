// The pixel loader shared by the kernels that stream a network's NHWC logits four pixels per lane: csrc/score.hip (argmax + confusion
// counts) and csrc/calibration.hip (confidence, reliability counts, the NLL grid).
#pragma once
#include "common.h"

namespace pylc {

typedef float score_f4 __attribute__((ext_vector_type(4)));
typedef float score_f2 __attribute__((ext_vector_type(2)));

// the 4 pixels a lane works on: exactly C logits each (no pad lane is loaded: a dead destination register would be reused while its load
// is still in flight and stall the loads behind it) and their targets
template <int C, typename TT>
struct ScorePixels {
    float v[4][C];
    TT t[4];
};

// the 4 pixels of group g: pixel 4 g - off + k.  Pixels outside 0 .. N-1 (the ends of a mask that starts `off` bytes past a dword, the
// tail, a lane past the last group) load the nearest real pixel instead and are never counted or written.
template <int C, typename TT, bool VEC, bool HAS_T>
__device__ __forceinline__ void score_load(ScorePixels<C, TT>& px, const float* __restrict__ logits, int pitch, const TT* __restrict__ target,
                                           long long N, long long first) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        long long q = first + k;
        q = q < 0 ? 0 : (q < N ? q : N - 1);
        const float* row = logits + q * pitch;
        if constexpr (VEC) {                               // rows are 16-byte aligned: 16-byte loads, then what is left of C in one or two
            constexpr int C4 = C / 4 * 4;
#pragma unroll
            for (int c = 0; c < C4; c += 4) {
                const score_f4 f = *reinterpret_cast<const score_f4*>(row + c);
                px.v[k][c] = f.x; px.v[k][c + 1] = f.y; px.v[k][c + 2] = f.z; px.v[k][c + 3] = f.w;
            }
            if constexpr (C - C4 >= 2) {
                const score_f2 f = *reinterpret_cast<const score_f2*>(row + C4);
                px.v[k][C4] = f.x; px.v[k][C4 + 1] = f.y;
            }
            if constexpr ((C - C4) % 2 == 1) px.v[k][C - 1] = row[C - 1];
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) px.v[k][c] = row[c];
        }
        if constexpr (HAS_T) px.t[k] = target[q];
    }
}

}  // namespace pylc
