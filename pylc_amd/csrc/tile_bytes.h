// What the kernels that write uint8 tiles and sum them in the same pass share (dataset.hip, augment.hip): the block shape, the 16-byte
// group store, and the wave / block reduction of the per-tile integer statistics (sum x and sum x^2 per channel, the class histogram).
#pragma once
#include "common.h"

namespace pylc {

constexpr int kDsThreads = 256;
constexpr int kDsBins = PYLC_MAX_CLASSES + 1;
constexpr int kDsBandPixels = 65536;           // pixels per plane and block: 65 536 * 255^2 < 2^32

__device__ __forceinline__ void store_group(unsigned char* p, const uint4& v, int valid) {
    if (valid == 16 && ((unsigned long long)p & 15u) == 0) {
        *reinterpret_cast<uint4*>(p) = v;
    } else {
        const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < valid) p[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// the wave's total of v (it fits 32 bits: see kDsBandPixels) added to a 64-bit LDS accumulator
__device__ __forceinline__ void wave_add(unsigned int v, unsigned long long* acc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(acc, (unsigned long long)v);
}

// s += the bytes of the group, ss += their squares
__device__ __forceinline__ void sum_group(const uint4& v, unsigned int& s, unsigned int& ss) {
    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s = __builtin_amdgcn_sad_u8(w[k], 0u, s);
        ss = __builtin_amdgcn_udot4(w[k], w[k], ss, false);
    }
}

// the first `valid` bytes of the group counted into this thread's own column of cnt [bins][kDsThreads] (ds_add without a return value and
// without two lanes on one address: masks are blobs, a shared counter would serialise the wave); values >= top go to bin top
__device__ __forceinline__ void count_group(const uint4& v, int valid, unsigned int top, unsigned int* cnt) {
    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < valid) {
            const unsigned int b = (w[k >> 2] >> (8 * (k & 3))) & 255u;
            atomicAdd(&cnt[(b < top ? b : top) * kDsThreads + threadIdx.x], 1u);
        }
    }
}

// The block's totals to tile n of sums [n][2][C] and hist [n][bins] (either may be NULL): s / ss per thread and channel, cnt as count_group
// leaves it, acc [6 + kDsBins] zeroed before the __syncthreads() that precedes this call.  One 64-bit atomic add per counter and block.
__device__ __forceinline__ void commit_tile_stats(const unsigned int (&s)[3], const unsigned int (&ss)[3], const unsigned int* cnt,
                                                  unsigned long long* acc, int C, int bins, long long n, unsigned long long* sums,
                                                  unsigned long long* hist) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c < C) {
            wave_add(s[c], &acc[c]);
            wave_add(ss[c], &acc[3 + c]);
        }
    }
    for (int b = 0; b < bins; ++b) wave_add(cnt[b * kDsThreads + tid], &acc[6 + b]);
    __syncthreads();
    if (tid < 6) {
        const int which = tid / 3, c = tid - 3 * which;
        if (sums && c < C && acc[tid]) atomicAdd(&sums[(n * 2 + which) * C + c], acc[tid]);
    } else if (tid < 6 + bins) {
        if (hist && acc[tid]) atomicAdd(&hist[n * bins + (tid - 6)], acc[tid]);
    }
}

}  // namespace pylc
