// Calibration of the confidences the inference paths hand out: reliability counts of a confidence map or straight
// from a network's logits, and the negative log-likelihood of the logits on a grid of inverse temperatures, each in one streaming pass.
//
// Shared definitions (include/pylc_hip.h states them for callers, tests/_calibration.py restates them as the yardstick):
//   bin of a float32 confidence p with B bins:  min(B - 1, (int)(p * (float)B))   -- fp32 product, truncating conversion, p == 1 in the last bin
//   quantised confidence:                       q = (uint32)(p * 16777216.0f)     -- the product is exact, the conversion truncates
//   cells: counts is int64 [3*C*B + 3].  Predicted class c, bin b: (c*B + b)*3 + {0, 1, 2} = pixels, pixels whose target is c, sum of q.
//          Tail 3*C*B + {0, 1, 2} = targets (or, for pylc_reliability_counts, predicted classes) outside 0..C-1 that are not the ignore
//          label, targets equal to the ignore label, confidences that are NaN, infinite or outside [0, 1].  A tail pixel is counted in its
//          tail cell only, in the first one of that order it qualifies for.
// Confidence is summed as integers, so every cell is exact and independent of the order in which pixels arrive, like the project's other
// counters; the price is at most 2^-24 per pixel.
//
// Geometry and counting follow score.hip: a lane takes 4 consecutive pixels, a block of 256 lanes 1024, at most CAL_GRID blocks (one per
// CU) walk the pixels in a grid-stride loop with the next round's loads issued before this round's work.  LDS holds 32-bit pixel and hit
// counters and 64-bit q sums per cell; a block adds one 64-bit global atomic per non-zero number at its end.  Masks are blobs and
// confidences cluster in the top bins, so one LDS atomic per pixel would serialise on a few cells: each wave first reduces in registers
// (the cell of the first lane that still holds one is broadcast, ballots count its pixels and its hits, the q of those pixels is summed
// over the wave, the leader adds three numbers), for at most CAL_ROUNDS rounds and until a round retires fewer than CAL_ROUND_MIN pixels;
// what is left goes to LDS pixel by pixel.
//
// pylc_logits_nll_grid is a different kernel: K * C exponentials per pixel make it arithmetic-bound, so it runs two blocks per CU without
// the ping-pong.  Its sums are floating point and must not depend on arrival order: a thread adds its pixels' fp32 terms into its own fp64
// column of an LDS table, the block folds the columns by a fixed tree, writes K partial sums to the workspace, and a one-wave kernel adds
// the blocks' partial sums in block order into `sums`.  The number of blocks depends on N alone.  No float atomics anywhere.
#include "common.h"
#include "score_pixels.h"

namespace pylc {

constexpr int CAL_MAXB = 32;               // bins at most
constexpr int CAL_MAXK = 32;               // inverse temperatures at most per launch of the NLL grid
constexpr int CAL_GRID = kNumCU;           // counting kernels: one block per CU, 262144 pixels per round of the grid
constexpr int CAL_ROUNDS = 12;             // wave-level rounds at most before the per-pixel LDS atomics
constexpr int CAL_ROUND_MIN = 8;           // a round that retired fewer pixels than this was the last: what is left is scattered
constexpr int CAL_CELLS = PYLC_MAX_CLASSES * CAL_MAXB + 3;
// One block counts at most 1024 * ceil(ceil((N + 3) / 4) / (256 * CAL_GRID)) <= 2^31 + 1024 pixels for N <= 2^39 (which the entry points
// check): below 2^32 for the 32-bit LDS counters, and with q <= 2^24 a 64-bit LDS q sum stays below 2^56.  The global int64 q cell holds
// N * 2^24 <= 2^63 - 2^24 for every N < 2^39 summed over all launches into one `counts`.
constexpr long long CAL_MAX_PIXELS = 1ll << 39;
constexpr int NLL_GRID = 2 * kNumCU;       // NLL grid: two blocks per CU (2 x 64 KiB of LDS)

__device__ __forceinline__ int cal_bin(float p, int B) {
    const int b = (int)(p * (float)B);
    return b < B - 1 ? b : B - 1;
}
__device__ __forceinline__ unsigned cal_q(float p) { return (unsigned)(p * 16777216.0f); }

struct CalLds {
    unsigned int n[CAL_CELLS], hit[CAL_CELLS];
    unsigned long long q[CAL_CELLS];
};

// the cell of one pixel (-1: not a pixel), with `hit` and `q` for a table cell; CB + 0..2 are the tail cells
__device__ __forceinline__ int cal_cell(bool ok, long long t, int cls, float p, int C, int B, bool has_ign, long long ign, bool& hit, unsigned& q) {
    hit = false;
    q = 0;
    if (!ok) return -1;
    const int CB = C * B;
    if (has_ign && t == ign) return CB + 1;
    if ((unsigned long long)t >= (unsigned long long)C || (unsigned)cls >= (unsigned)C) return CB;
    if (!(p >= 0.f && p <= 1.f)) return CB + 2;          // NaN fails both comparisons
    hit = (int)t == cls;
    q = cal_q(p);
    return cls * B + cal_bin(p, B);
}

// Adds the wave's 256 pixels to the block's LDS table.  Every lane of the wave is here (the callers' loops are wave-uniform).
__device__ __forceinline__ void cal_count(int (&cell)[4], const bool (&hit)[4], const unsigned (&q)[4], CalLds& lds) {
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int r = 0; r < CAL_ROUNDS; ++r) {
        const int mine = cell[0] >= 0 ? cell[0] : cell[1] >= 0 ? cell[1] : cell[2] >= 0 ? cell[2] : cell[3];
        const unsigned long long holders = __ballot(mine >= 0);
        if (holders == 0) return;
        const int leader = __ffsll((long long)holders) - 1;
        const int lc = __builtin_amdgcn_readlane(mine, leader);
        int n = 0, h = 0;
        unsigned qs = 0;                                  // a lane's 4 q are below 2^26 + 1, 32 lanes' below 2^32
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool same = cell[k] == lc;
            n += __popcll(__ballot(same));
            h += __popcll(__ballot(same && hit[k]));
            qs += same ? q[k] : 0u;
            cell[k] = same ? -1 : cell[k];
        }
        // the 32-bit sum stays within each half of the wave (xor distances below 32): 32 lanes x 4 x 2^24 = 2^31; the halves meet in 64 bits
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) qs += (unsigned)__shfl_xor((int)qs, o, 64);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)qs, 0), hi = (unsigned)__builtin_amdgcn_readlane((int)qs, 32);
        if (lane == leader) {
            atomicAdd(&lds.n[lc], (unsigned)n);
            if (h) atomicAdd(&lds.hit[lc], (unsigned)h);
            const unsigned long long t = (unsigned long long)lo + hi;
            if (t) atomicAdd(&lds.q[lc], t);
        }
        if (n < CAL_ROUND_MIN) break;                     // (n is wave-uniform)
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (cell[k] >= 0) {
            atomicAdd(&lds.n[cell[k]], 1u);
            if (hit[k]) atomicAdd(&lds.hit[cell[k]], 1u);
            if (q[k]) atomicAdd(&lds.q[cell[k]], (unsigned long long)q[k]);
        }
}

__device__ __forceinline__ void cal_clear(CalLds& lds, int cells) {
    for (int i = threadIdx.x; i < cells; i += 256) { lds.n[i] = 0; lds.hit[i] = 0; lds.q[i] = 0; }
    __syncthreads();
}

// one 64-bit global atomic per non-zero number of the block
__device__ __forceinline__ void cal_flush(const CalLds& lds, int CB, unsigned long long* __restrict__ counts) {
    __syncthreads();
    for (int i = threadIdx.x; i < CB + 3; i += 256) {
        if (!lds.n[i]) continue;
        if (i < CB) {
            atomicAdd(&counts[3 * i], (unsigned long long)lds.n[i]);
            if (lds.hit[i]) atomicAdd(&counts[3 * i + 1], (unsigned long long)lds.hit[i]);
            if (lds.q[i]) atomicAdd(&counts[3 * i + 2], lds.q[i]);
        } else {
            atomicAdd(&counts[3 * CB + (i - CB)], (unsigned long long)lds.n[i]);
        }
    }
}

// ---- pylc_reliability_counts: confidence map + predicted mask + truth mask ------------------------------------------------------------------
template <typename TT>
struct RelPixels {
    float p[4];
    unsigned char c[4];
    TT t[4];
};

// pixels first .. first + 3; pixels outside 0 .. N-1 load the nearest real pixel and are never counted.  VEC: conf is 16-byte and the byte
// masks are 4-byte aligned, so a group that lies inside the maps is one load per map.
template <typename TT, bool VEC>
__device__ __forceinline__ void rel_load(RelPixels<TT>& px, const float* __restrict__ conf, const unsigned char* __restrict__ pred,
                                         const TT* __restrict__ truth, long long N, long long first) {
    if (VEC && first + 3 < N) {
        const score_f4 f = *reinterpret_cast<const score_f4*>(conf + first);
        px.p[0] = f.x; px.p[1] = f.y; px.p[2] = f.z; px.p[3] = f.w;
        const unsigned w = *reinterpret_cast<const unsigned*>(pred + first);
#pragma unroll
        for (int k = 0; k < 4; ++k) px.c[k] = (unsigned char)(w >> (8 * k));
        if constexpr (sizeof(TT) == 1) {
            const unsigned u = *reinterpret_cast<const unsigned*>(truth + first);
#pragma unroll
            for (int k = 0; k < 4; ++k) px.t[k] = (TT)(u >> (8 * k));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) px.t[k] = truth[first + k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            long long i = first + k;
            i = i < N ? i : N - 1;
            px.p[k] = conf[i];
            px.c[k] = pred[i];
            px.t[k] = truth[i];
        }
    }
}

template <typename TT>
__device__ __forceinline__ void rel_work(const RelPixels<TT>& px, long long N, long long first, int C, int B, bool has_ign, long long ign,
                                         CalLds& lds) {
    int cell[4];
    bool hit[4];
    unsigned q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cell[k] = cal_cell(first + k < N, (long long)px.t[k], (int)px.c[k], px.p[k], C, B, has_ign, ign, hit[k], q[k]);
    cal_count(cell, hit, q, lds);
}

template <typename TT, bool VEC>
__global__ __launch_bounds__(256) void reliability_counts_kernel(const float* __restrict__ conf, const unsigned char* __restrict__ pred,
                                                                  const TT* __restrict__ truth, long long N, int C, int B, int has_ign,
                                                                  long long ign, unsigned long long* __restrict__ counts) {
    __shared__ CalLds lds;
    cal_clear(lds, C * B + 3);
    const long long groups = (N + 3) >> 2;
    const long long step = (long long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    RelPixels<TT> a, b;                  // score.hip's ping-pong: `g - lane` is the wave's first group, the loop is wave-uniform
    rel_load<TT, VEC>(a, conf, pred, truth, N, 4 * g);
    while (g - lane < groups) {
        rel_load<TT, VEC>(b, conf, pred, truth, N, 4 * (g + step));
        rel_work<TT>(a, N, 4 * g, C, B, has_ign != 0, ign, lds);
        g += step;
        if (g - lane >= groups) break;
        rel_load<TT, VEC>(a, conf, pred, truth, N, 4 * (g + step));
        rel_work<TT>(b, N, 4 * g, C, B, has_ign != 0, ign, lds);
        g += step;
    }
    cal_flush(lds, C * B, counts);
}

// ---- pylc_logits_reliability: logits -> class, confidence, counts -----------------------------------------------------------------------------
template <int C, typename TT, bool HAS_T>
__device__ __forceinline__ void lrel_work(const ScorePixels<C, TT>& px, long long N, long long first, int B, float beta,
                                          unsigned char* __restrict__ mask, float* __restrict__ conf_out, bool has_ign, long long ign,
                                          CalLds& lds) {
    int cls[4];
    float conf[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int best = 0;
        float bv = px.v[k][0];
#pragma unroll
        for (int c = 1; c < C; ++c) if (px.v[k][c] > bv) { bv = px.v[k][c]; best = c; }     // first maximum (np.argmax)
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += expf((px.v[k][c] - bv) * beta);                    // ascending c; the maximum's term is 1
        cls[k] = best;
        conf[k] = 1.f / s;
        ok[k] = first + k >= 0 && first + k < N;
    }
    const bool full = ok[0] && ok[3];
    if (mask) {
        if (full) {                  // mask + first is dword-aligned by the choice of `off`
            *reinterpret_cast<unsigned int*>(mask + first) = (unsigned)cls[0] | (unsigned)cls[1] << 8 | (unsigned)cls[2] << 16 | (unsigned)cls[3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (ok[k]) mask[first + k] = (unsigned char)cls[k];
        }
    }
    if (conf_out) {
        if (full && (reinterpret_cast<uintptr_t>(conf_out + first) & 15) == 0) {
            score_f4 f;
            f.x = conf[0]; f.y = conf[1]; f.z = conf[2]; f.w = conf[3];
            *reinterpret_cast<score_f4*>(conf_out + first) = f;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (ok[k]) conf_out[first + k] = conf[k];
        }
    }
    if constexpr (HAS_T) {
        int cell[4];
        bool hit[4];
        unsigned q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) cell[k] = cal_cell(ok[k], (long long)px.t[k], cls[k], conf[k], C, B, has_ign, ign, hit[k], q[k]);
        cal_count(cell, hit, q, lds);
    }
}

template <int C, typename TT, bool VEC, bool HAS_T>
__global__ __launch_bounds__(256) void logits_reliability_kernel(const float* __restrict__ logits, int pitch, const TT* __restrict__ target,
                                                                  long long N, int off, int B, float beta, unsigned char* __restrict__ mask,
                                                                  float* __restrict__ conf_out, unsigned long long* __restrict__ counts,
                                                                  int has_ign, long long ign) {
    __shared__ CalLds lds;
    if constexpr (HAS_T) cal_clear(lds, C * B + 3);
    const long long groups = (N + off + 3) >> 2;
    const long long step = (long long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    ScorePixels<C, TT> a, b;             // as logits_score_kernel: the next round's loads are issued before this round's work
    score_load<C, TT, VEC, HAS_T>(a, logits, pitch, target, N, 4 * g - off);
    while (g - lane < groups) {
        score_load<C, TT, VEC, HAS_T>(b, logits, pitch, target, N, 4 * (g + step) - off);
        lrel_work<C, TT, HAS_T>(a, N, 4 * g - off, B, beta, mask, conf_out, has_ign != 0, ign, lds);
        g += step;
        if (g - lane >= groups) break;
        score_load<C, TT, VEC, HAS_T>(a, logits, pitch, target, N, 4 * (g + step) - off);
        lrel_work<C, TT, HAS_T>(b, N, 4 * g - off, B, beta, mask, conf_out, has_ign != 0, ign, lds);
        g += step;
    }
    if constexpr (HAS_T) cal_flush(lds, C * B, counts);
}

template <int C, typename TT, bool HAS_T>
static void lrel_launch(bool vec, int blocks, hipStream_t st, const float* logits, int pitch, const void* target, long long N, int off, int B,
                        float beta, unsigned char* mask, float* conf_out, unsigned long long* counts, int has_ign, long long ign) {
    if (vec)
        hipLaunchKernelGGL((logits_reliability_kernel<C, TT, true, HAS_T>), dim3(blocks), dim3(256), 0, st, logits, pitch,
                           static_cast<const TT*>(target), N, off, B, beta, mask, conf_out, counts, has_ign, ign);
    else
        hipLaunchKernelGGL((logits_reliability_kernel<C, TT, false, HAS_T>), dim3(blocks), dim3(256), 0, st, logits, pitch,
                           static_cast<const TT*>(target), N, off, B, beta, mask, conf_out, counts, has_ign, ign);
}

// ---- pylc_logits_nll_grid ---------------------------------------------------------------------------------------------------------------------
struct NllBetas { float b[CAL_MAXK]; };

inline int nll_blocks(long long N) {
    const long long want = cdiv<long long>((N + 3) >> 2, 256);
    return (int)(want < NLL_GRID ? want : NLL_GRID);
}

template <int C, typename TT, bool VEC>
__global__ __launch_bounds__(256) void nll_grid_kernel(const float* __restrict__ logits, int pitch, const TT* __restrict__ target, long long N,
                                                        NllBetas betas, int K, int has_ign, long long ign, double* __restrict__ workspace,
                                                        unsigned long long* __restrict__ tail) {
    __shared__ double acc[CAL_MAXK][256];              // thread t owns column t: no two threads touch one entry before the fold
    const int tid = threadIdx.x;
    for (int k = 0; k < K; ++k) acc[k][tid] = 0.0;
    unsigned long long n_sum = 0, n_bad = 0, n_ign = 0;
    const long long groups = (N + 3) >> 2;
    const long long step = (long long)gridDim.x * 256;
    for (long long g = (long long)blockIdx.x * 256 + tid; g < groups; g += step) {
        ScorePixels<C, TT> px;
        score_load<C, TT, VEC, true>(px, logits, pitch, target, N, 4 * g);
        float d[4][C], dt[4];
        bool use[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = 4 * g + j < N;
            const long long t = (long long)px.t[j];
            const bool ignored = has_ign && t == ign;
            const bool inside = (unsigned long long)t < (unsigned long long)C;
            use[j] = ok && !ignored && inside;
            n_sum += use[j];
            n_ign += ok && ignored;
            n_bad += ok && !ignored && !inside;
            float m = px.v[j][0];
#pragma unroll
            for (int c = 1; c < C; ++c) m = fmaxf(m, px.v[j][c]);
            dt[j] = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                d[j][c] = px.v[j][c] - m;
                dt[j] = t == c ? d[j][c] : dt[j];
            }
        }
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const float beta = betas.b[k];
            double sum = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) s += expf(d[j][c] * beta);
                const float term = logf(s) - dt[j] * beta;
                sum += use[j] ? (double)term : 0.0;
            }
            acc[k][tid] += sum;
        }
    }
    // fold the 256 columns by a fixed tree, then one partial sum per beta and block
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h)
            for (int k = 0; k < K; ++k) acc[k][tid] += acc[k][tid + h];
    }
    __syncthreads();
    if (tid < K) workspace[(size_t)blockIdx.x * K + tid] = acc[tid][0];
    // the tail is integer: wave sum, one 64-bit atomic per non-zero number per wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_sum += __shfl_xor(n_sum, o, 64);
        n_bad += __shfl_xor(n_bad, o, 64);
        n_ign += __shfl_xor(n_ign, o, 64);
    }
    if ((tid & 63) == 0) {
        if (n_sum) atomicAdd(&tail[0], n_sum);
        if (n_bad) atomicAdd(&tail[1], n_bad);
        if (n_ign) atomicAdd(&tail[2], n_ign);
    }
}

// sums[k] += the blocks' partial sums in block order (one wave, thread k)
__global__ __launch_bounds__(64) void nll_combine_kernel(const double* __restrict__ workspace, int blocks, int K, double* __restrict__ sums) {
    const int k = threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += workspace[(size_t)b * K + k];
    sums[k] += s;
}

template <int C, typename TT>
static void nll_launch(bool vec, int blocks, hipStream_t st, const float* logits, int pitch, const void* target, long long N,
                       const NllBetas& betas, int K, int has_ign, long long ign, double* workspace, unsigned long long* tail) {
    if (vec)
        hipLaunchKernelGGL((nll_grid_kernel<C, TT, true>), dim3(blocks), dim3(256), 0, st, logits, pitch, static_cast<const TT*>(target), N, betas,
                           K, has_ign, ign, workspace, tail);
    else
        hipLaunchKernelGGL((nll_grid_kernel<C, TT, false>), dim3(blocks), dim3(256), 0, st, logits, pitch, static_cast<const TT*>(target), N, betas,
                           K, has_ign, ign, workspace, tail);
}

static int cal_blocks(long long groups) {
    const long long want = cdiv<long long>(groups, 256);
    return (int)(want < CAL_GRID ? want : CAL_GRID);
}

}  // namespace pylc

using namespace pylc;

extern "C" int pylc_reliability_counts(const float* conf, const unsigned char* pred, const void* truth, int truth_bytes, long long N, int C, int B,
                                       int has_ignore, int ignore_index, unsigned long long* counts, void* stream) {
    PYLC_REQUIRE(conf && pred && truth && counts, "reliability_counts: a buffer is NULL");
    PYLC_REQUIRE(C >= 2 && C <= PYLC_MAX_CLASSES, "reliability_counts: n_classes=%d unsupported (2..%d)", C, PYLC_MAX_CLASSES);
    PYLC_REQUIRE(B >= 1 && B <= CAL_MAXB, "reliability_counts: bins=%d outside 1..%d", B, CAL_MAXB);
    PYLC_REQUIRE(N > 0 && N <= CAL_MAX_PIXELS, "reliability_counts: N=%lld outside 1..2^39 (the bound of the block counters)", N);
    PYLC_REQUIRE(truth_bytes == 1 || truth_bytes == 8, "reliability_counts: truth_bytes=%d (1: uint8, 8: int64)", truth_bytes);
    PYLC_REQUIRE(has_ignore == 0 || has_ignore == 1, "reliability_counts: has_ignore=%d", has_ignore);
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(conf) & 3) == 0 && (reinterpret_cast<uintptr_t>(counts) & 7) == 0 &&
                 (truth_bytes != 8 || (reinterpret_cast<uintptr_t>(truth) & 7) == 0), "reliability_counts: a buffer is not aligned to its element");
    const bool vec = (reinterpret_cast<uintptr_t>(conf) & 15) == 0 && (reinterpret_cast<uintptr_t>(pred) & 3) == 0 &&
                     (truth_bytes == 8 || (reinterpret_cast<uintptr_t>(truth) & 3) == 0);
    const int blocks = cal_blocks((N + 3) >> 2);
    hipStream_t st = as_stream(stream);
    const long long ign = ignore_index;
#define LAUNCH_RC(TT, VEC)                                                                                                               \
    hipLaunchKernelGGL((reliability_counts_kernel<TT, VEC>), dim3(blocks), dim3(256), 0, st, conf, pred, static_cast<const TT*>(truth), N, C, B, \
                       has_ignore, ign, counts)
    if (truth_bytes == 8) { if (vec) LAUNCH_RC(long long, true); else LAUNCH_RC(long long, false); }
    else { if (vec) LAUNCH_RC(unsigned char, true); else LAUNCH_RC(unsigned char, false); }
#undef LAUNCH_RC
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

// the checks the two logits entry points share
static int cal_logits_check(const char* who, const float* logits, int pitch, const void* target, int target_bytes, long long N, int C) {
    PYLC_REQUIRE(logits, "%s: logits is NULL", who);
    PYLC_REQUIRE(C >= 2 && C <= PYLC_MAX_CLASSES, "%s: n_classes=%d unsupported (2..%d)", who, C, PYLC_MAX_CLASSES);
    PYLC_REQUIRE(pitch >= C, "%s: pitch=%d below n_classes=%d", who, pitch, C);
    PYLC_REQUIRE(N > 0 && N <= CAL_MAX_PIXELS, "%s: N=%lld outside 1..2^39", who, N);
    PYLC_REQUIRE(target_bytes == 0 || target_bytes == 1 || target_bytes == 8, "%s: target_bytes=%d (0: none, 1: uint8, 8: int64)", who, target_bytes);
    PYLC_REQUIRE((target != nullptr) == (target_bytes != 0), "%s: target and target_bytes=%d disagree", who, target_bytes);
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 3) == 0 && (target_bytes != 8 || (reinterpret_cast<uintptr_t>(target) & 7) == 0),
                 "%s: a buffer is not aligned to its element", who);
    return PYLC_OK;
}

extern "C" int pylc_logits_reliability(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int B,
                                       float inv_temperature, int has_ignore, int ignore_index, unsigned char* mask_out, float* conf_out,
                                       unsigned long long* counts, void* stream) {
    if (int rc = cal_logits_check("logits_reliability", logits, pitch, target, target_bytes, N, C)) return rc;
    PYLC_REQUIRE(mask_out || conf_out || counts, "logits_reliability: mask_out, conf_out and counts are all NULL, nothing to compute");
    PYLC_REQUIRE(B >= 1 && B <= CAL_MAXB, "logits_reliability: bins=%d outside 1..%d", B, CAL_MAXB);
    PYLC_REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.4028234e38f, "logits_reliability: inv_temperature must be positive and finite");
    PYLC_REQUIRE(has_ignore == 0 || has_ignore == 1, "logits_reliability: has_ignore=%d", has_ignore);
    PYLC_REQUIRE(!counts || target, "logits_reliability: counts without target");
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0 && (reinterpret_cast<uintptr_t>(conf_out) & 3) == 0,
                 "logits_reliability: a buffer is not aligned to its element");
    const bool vec = pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    // groups of 4 pixels start where the mask's dwords do; without a mask, where conf_out's 16-byte vectors do
    const int off = mask_out ? (int)(reinterpret_cast<uintptr_t>(mask_out) & 3) : conf_out ? (int)((reinterpret_cast<uintptr_t>(conf_out) >> 2) & 3) : 0;
    const int blocks = cal_blocks((N + off + 3) >> 2);
    hipStream_t st = as_stream(stream);
    const long long ign = ignore_index;
    if (!counts) {                                                                 // maps only: a target, if any, is not read
#define LAUNCH_LR(CC) lrel_launch<CC, unsigned char, false>(vec, blocks, st, logits, pitch, nullptr, N, off, B, inv_temperature, mask_out, conf_out, nullptr, 0, 0)
        PYLC_FOR_CLASSES(C, LAUNCH_LR, "logits_reliability")
#undef LAUNCH_LR
    } else if (target_bytes == 8) {
#define LAUNCH_LR(CC) lrel_launch<CC, long long, true>(vec, blocks, st, logits, pitch, target, N, off, B, inv_temperature, mask_out, conf_out, counts, has_ignore, ign)
        PYLC_FOR_CLASSES(C, LAUNCH_LR, "logits_reliability")
#undef LAUNCH_LR
    } else {
#define LAUNCH_LR(CC) lrel_launch<CC, unsigned char, true>(vec, blocks, st, logits, pitch, target, N, off, B, inv_temperature, mask_out, conf_out, counts, has_ignore, ign)
        PYLC_FOR_CLASSES(C, LAUNCH_LR, "logits_reliability")
#undef LAUNCH_LR
    }
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" size_t pylc_logits_nll_grid_workspace_bytes(long long N, int K) {
    if (N <= 0 || K < 1 || K > CAL_MAXK) return 0;
    return (size_t)nll_blocks(N) * K * sizeof(double);
}

extern "C" int pylc_logits_nll_grid(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, const float* betas,
                                    int K, int has_ignore, int ignore_index, void* workspace, double* sums, long long* tail, void* stream) {
    if (int rc = cal_logits_check("logits_nll_grid", logits, pitch, target, target_bytes, N, C)) return rc;
    PYLC_REQUIRE(target && workspace && sums && tail && betas, "logits_nll_grid: a buffer is NULL");
    PYLC_REQUIRE(K >= 1 && K <= CAL_MAXK, "logits_nll_grid: K=%d outside 1..%d", K, CAL_MAXK);
    PYLC_REQUIRE(has_ignore == 0 || has_ignore == 1, "logits_nll_grid: has_ignore=%d", has_ignore);
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(tail) & 7) == 0, "logits_nll_grid: a buffer is not aligned to its element");
    NllBetas kb;
    for (int k = 0; k < CAL_MAXK; ++k) kb.b[k] = 1.f;
    for (int k = 0; k < K; ++k) {
        PYLC_REQUIRE(betas[k] > 0.f && betas[k] <= 3.4028234e38f, "logits_nll_grid: betas[%d] must be positive and finite", k);
        kb.b[k] = betas[k];
    }
    const bool vec = pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    const int blocks = nll_blocks(N);
    hipStream_t st = as_stream(stream);
    const long long ign = ignore_index;
    double* ws = static_cast<double*>(workspace);
    unsigned long long* tl = reinterpret_cast<unsigned long long*>(tail);
    if (target_bytes == 8) {
#define LAUNCH_NG(CC) nll_launch<CC, long long>(vec, blocks, st, logits, pitch, target, N, kb, K, has_ignore, ign, ws, tl)
        PYLC_FOR_CLASSES(C, LAUNCH_NG, "logits_nll_grid")
#undef LAUNCH_NG
    } else {
#define LAUNCH_NG(CC) nll_launch<CC, unsigned char>(vec, blocks, st, logits, pitch, target, N, kb, K, has_ignore, ign, ws, tl)
        PYLC_FOR_CLASSES(C, LAUNCH_NG, "logits_nll_grid")
#undef LAUNCH_NG
    }
    hipLaunchKernelGGL(nll_combine_kernel, dim3(1), dim3(64), 0, st, ws, blocks, K, sums);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}
