// Hard-pixel mining: the per-pixel loss map nll_n = lse - z_t of a batch of logits, and the exact selection of its k
// largest candidates (bootstrapped / top-k cross-entropy) and / or of every candidate at or above a cap (OHEM's probability threshold) as a
// pixel-weight map for pylc_multiloss_*_w / _ls.  include/pylc_hip.h states the definitions for callers, tests/_mining.py restates them as the
// yardstick.
//
// Selection is a radix select on the float bits: a candidate's value is >= +0 (a -0 counts as +0), and non-negative floats order as their
// uint32 bits, whose top bit is clear.  The 31 bits that are left are taken in three digits of 11 / 10 / 10 bits, most significant first:
//   pass 1  histogram of bits 30..20 of every candidate                       (2048 bins; the fused form takes it in the kernel that computes nll)
//   pass 2  histogram of bits 19..10 of the candidates whose bits 30..20 are the digit pass 1 found      (1024 bins)
//   pass 3  histogram of bits  9..0  of the candidates whose bits 30..10 are the prefix found so far     (1024 bins)
//   apply   tau = min(value of the 31 bits found, cap); writes the weight map, counts the kept pixels, writes info
// A histogram is taken per block in LDS and flushed with one 32-bit integer global atomic per non-empty bin (N < 2^31: no count overflows),
// so it does not depend on the order in which blocks or pixels arrive and the result is bitwise reproducible.  The scan of a finished
// histogram -- find the digit d with count(digits > d) < k <= count(digits >= d), carry k - count(digits > d) on -- is no launch of its own:
// every block of the NEXT kernel does it redundantly at its start (8 KiB of L2-resident counts, one wave), and block 0 records the result
// for the kernel after that.  Four launches and one hipMemsetAsync of the three histograms.
// Every pass reads the STORED float32 map (the caller's nll_out, or the map's room in the workspace), so all passes see the same bits.
//
// Crowded bins: a trained model puts most pixels near nll = 0 and constant logits put every pixel into ONE bin; LDS atomics on equal
// addresses serialise.  As in calibration.hip each wave first combines equal keys in registers -- the key of the first lane that still
// holds one is broadcast, ballots count its holders, the leader adds the count once -- for at most MINE_ROUNDS rounds and until a round
// retires fewer than MINE_ROUND_MIN keys; what is left goes to LDS key by key.  (A histogram per wave would not help: the lanes that
// collide are lanes of one wave.)
//
// Geometry follows calibration.hip: a lane takes 4 consecutive pixels, a block of 256 lanes 1024, and the blocks walk the pixels in a
// grid-stride loop.  The nll kernel runs at most MINE_GRID blocks (one per CU) and issues the next round's loads before this round's work;
// the passes over the stored map are a 16-byte load and a few integer operations per lane and run at most MINE_MAP_GRID blocks.
#include <cfloat>
#include <cmath>

#include "common.h"
#include "score_pixels.h"

namespace pylc {

constexpr int MINE_GRID = kNumCU;          // the nll kernel: one block per CU (it prefetches), 262144 pixels per round of the grid
constexpr int MINE_MAP_GRID = 4 * kNumCU;  // the passes over the stored map: four blocks per CU hide the load latency, 1048576 pixels per round
constexpr int MINE_B1 = 2048;              // bits 30..20
constexpr int MINE_B2 = 1024;              // bits 19..10
constexpr int MINE_B3 = 1024;              // bits  9..0
constexpr int MINE_ROUNDS = 12;            // wave-level rounds at most before the per-key LDS atomics
constexpr int MINE_ROUND_MIN = 8;          // a round that retired fewer keys than this was the last
constexpr long long MINE_MAX_PIXELS = 2147483647ll;
constexpr unsigned MINE_INF_BITS = 0x7F800000u;
// workspace: [hist1 | hist2 | hist3 | state (64 words)] then the map's room.  The memset clears the histograms only.
constexpr size_t MINE_HIST_WORDS = MINE_B1 + MINE_B2 + MINE_B3;
constexpr size_t MINE_STATE_WORDS = 64;
constexpr size_t MINE_HEAD_BYTES = (MINE_HIST_WORDS + MINE_STATE_WORDS) * sizeof(unsigned);     // 16640: a multiple of 256
// state words: block 0 of the kernel that scanned a histogram writes them, the kernels after it read them
enum { ST_NVALID = 0, ST_K = 1, ST_D1 = 2, ST_REM1 = 3, ST_D2 = 8, ST_REM2 = 9 };

struct MineLds {
    unsigned hist[MINE_B1];
    unsigned part[256];
    unsigned res[4];          // digit, remaining rank, total of the scanned histogram, k
};

// ---- what a map value and a weight mean ------------------------------------------------------------------------------------------------------
// weight: 0 takes part, 1 u == 0, 2 negative / NaN / infinite (the PW rules of loss.hip)
__device__ __forceinline__ int mine_weight(float u) {
    if (u == 0.f) return 1;
    return (u > 0.f && u <= FLT_MAX) ? 0 : 2;
}
// a value of the map is a candidate's when it is >= 0 (NaN is not, -0 is and counts as +0)
__device__ __forceinline__ bool mine_is_value(float v) { return v >= 0.f; }
__device__ __forceinline__ unsigned mine_key(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }      // (-0 -> +0; only called on values >= 0)

// ---- counting keys of a wave into the block's histogram -----------------------------------------------------------------------------------------
// cell[k] < 0: nothing to count.  Every lane of the wave is here (the callers' loops are wave-uniform).
__device__ __forceinline__ void mine_count(int (&cell)[4], unsigned* __restrict__ hist) {
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int r = 0; r < MINE_ROUNDS; ++r) {
        const int mine = cell[0] >= 0 ? cell[0] : cell[1] >= 0 ? cell[1] : cell[2] >= 0 ? cell[2] : cell[3];
        const unsigned long long holders = __ballot(mine >= 0);
        if (holders == 0) return;
        const int leader = __ffsll((long long)holders) - 1;
        const int lc = __builtin_amdgcn_readlane(mine, leader);
        int n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool same = cell[k] == lc;
            n += __popcll(__ballot(same));
            cell[k] = same ? -1 : cell[k];
        }
        if (lane == leader) atomicAdd(&hist[lc], (unsigned)n);
        if (n < MINE_ROUND_MIN) break;                    // (n is wave-uniform)
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (cell[k] >= 0) atomicAdd(&hist[cell[k]], 1u);
}

__device__ __forceinline__ void mine_clear(unsigned* __restrict__ hist, int bins) {
    for (int i = threadIdx.x; i < bins; i += 256) hist[i] = 0;
    __syncthreads();
}

// one 32-bit global atomic per non-empty bin of the block
__device__ __forceinline__ void mine_flush(const unsigned* __restrict__ hist, int bins, unsigned* __restrict__ ghist) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256)
        if (hist[i]) atomicAdd(&ghist[i], hist[i]);
}

// k = min(n_valid, max(min_kept, ceil(keep * n_valid))), the product and the ceil in fp64
__device__ __forceinline__ unsigned mine_k(unsigned n_valid, double keep, long long min_kept) {
    const double want = ceil(keep * (double)n_valid);                     // <= n_valid + 1 for keep <= 1
    long long k = (long long)want;
    k = k > min_kept ? k : min_kept;
    return (unsigned)(k < (long long)n_valid ? k : (long long)n_valid);
}

// Scans a finished histogram of BINS counts (every thread of the block is here): finds the digit d with count(> d) < k <= count(>= d) and
// leaves in lds.res: d, k - count(> d), the histogram's total, k.  FIRST: k is computed from the total (the number of candidates);
// otherwise k is given.  k == 0 (or a total below k, which no caller produces): res[0] = 0, res[1] = 0.
template <int BINS, bool FIRST>
__device__ __forceinline__ void mine_scan(const unsigned* __restrict__ ghist, unsigned k, double keep, long long min_kept, MineLds& lds) {
    constexpr int PER = BINS / 256;
    const int tid = threadIdx.x;
    for (int i = tid; i < BINS; i += 256) lds.hist[i] = ghist[i];
    __syncthreads();
    unsigned s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) s += lds.hist[tid * PER + j];
    lds.part[tid] = s;
    __syncthreads();
    if (tid < 64) {
        const unsigned q = lds.part[4 * tid] + lds.part[4 * tid + 1] + lds.part[4 * tid + 2] + lds.part[4 * tid + 3];
        unsigned suf = q;                                 // inclusive suffix sum over the lanes: the count of lanes >= tid
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = (unsigned)__shfl_down((int)suf, o, 64);
            suf += tid + o < 64 ? v : 0u;
        }
        const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)suf, 0);
        if constexpr (FIRST) k = mine_k(total, keep, min_kept);
        const unsigned long long reach = __ballot(k != 0 && suf >= k);     // lanes 0..L: suf does not increase with the lane
        if (reach == 0) {
            if (tid == 0) { lds.res[0] = 0; lds.res[1] = 0; lds.res[2] = total; lds.res[3] = k; }
        } else {
            const int L = 63 - __clzll((long long)reach);
            if (tid == L) {
                unsigned above = suf - q;                 // the count of the bins above this lane's
                const int lo = 4 * tid * PER;
                int b = lo + 4 * PER - 1;
                for (; b > lo; --b) {                     // (the lane's bins hold the k-th: the walk ends inside them)
                    const unsigned h = lds.hist[b];
                    if (above + h >= k) break;
                    above += h;
                }
                lds.res[0] = (unsigned)b; lds.res[1] = k - above; lds.res[2] = total; lds.res[3] = k;
            }
        }
    }
    __syncthreads();
}

// ---- the map's loads and stores ---------------------------------------------------------------------------------------------------------------
// 4 floats at first .. first + 3; vec: p is 16-byte aligned (first is a multiple of 4).  Entries past N - 1 load the last real one.
__device__ __forceinline__ void mine_ld4(float (&v)[4], const float* __restrict__ p, long long N, long long first, bool vec) {
    if (vec && first + 3 < N) {
        const score_f4 f = *reinterpret_cast<const score_f4*>(p + first);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            long long i = first + k;
            i = i < N ? i : N - 1;
            v[k] = p[i];
        }
    }
}

__device__ __forceinline__ void mine_st4(const float (&v)[4], float* __restrict__ p, long long N, long long first, bool vec) {
    if (vec && first + 3 < N) {
        score_f4 f;
        f.x = v[0]; f.y = v[1]; f.z = v[2]; f.w = v[3];
        *reinterpret_cast<score_f4*>(p + first) = f;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (first + k < N) p[first + k] = v[k];
    }
}

// ---- the loss map (and, HIST, the first histogram) ----------------------------------------------------------------------------------------------
template <int C, typename TT>
struct MinePixels {
    ScorePixels<C, TT> s;
    float u[4];
};

template <int C, typename TT, bool VEC>
__device__ __forceinline__ void mine_load(MinePixels<C, TT>& px, const float* __restrict__ logits, int pitch, const TT* __restrict__ target,
                                          const float* __restrict__ pw, long long N, long long first, bool pw_vec) {
    score_load<C, TT, VEC, true>(px.s, logits, pitch, target, N, first);
    if (pw != nullptr) {
        // a group past the end loads the last group's weights (never used)
        mine_ld4(px.u, pw, N, first < N ? first : ((N - 1) & ~3ll), pw_vec);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) px.u[k] = 1.f;
    }
}

// nll of one pixel with the operation order of softmax_px (loss.hip): zmax, sum expf(z - zmax) in ascending c, zmax + logf(sum), minus z_t
template <int C>
__device__ __forceinline__ float mine_nll(const float (&z)[C], int t) {
    float zmax = z[0];
#pragma unroll
    for (int c = 1; c < C; ++c) zmax = fmaxf(zmax, z[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) sum += expf(z[c] - zmax);
    const float lse = zmax + logf(sum);
    float zt = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) zt = (c == t) ? z[c] : zt;
    const float nll = lse - zt;
    return nll == 0.f ? 0.f : nll;                         // -0 -> +0
}

template <int C, typename TT, bool HIST>
__device__ __forceinline__ void mine_nll_work(const MinePixels<C, TT>& px, long long N, long long first, long long ign, float* __restrict__ nll_out,
                                              bool out_vec, unsigned* __restrict__ hist) {
    float v[4];
    int cell[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long t = (long long)px.s.t[k];
        const bool ignored = t == ign;
        const bool inside = (unsigned long long)t < (unsigned long long)C;
        const int w = mine_weight(px.u[k]);
        // the target is judged first: ignored, then bad; then the weight: zero, then bad (loss.hip's PW kernels)
        const float sentinel = ignored ? -1.f : !inside ? -2.f : w == 1 ? -1.f : -2.f;
        const bool takes_part = !ignored && inside && w == 0;
        const float nll = mine_nll<C>(px.s.v[k], inside ? (int)t : 0);
        v[k] = takes_part ? nll : sentinel;
        if constexpr (HIST) cell[k] = (first + k < N && takes_part && mine_is_value(nll)) ? (int)(mine_key(nll) >> 20) : -1;
    }
    if (first < N) mine_st4(v, nll_out, N, first, out_vec);
    if constexpr (HIST) mine_count(cell, hist);
}

template <int C, typename TT, bool VEC, bool HIST>
__global__ __launch_bounds__(256) void mine_nll_kernel(const float* __restrict__ logits, int pitch, const TT* __restrict__ target, long long N,
                                                        long long ign, const float* __restrict__ pw, int pw_vec, float* __restrict__ nll_out,
                                                        int out_vec, unsigned* __restrict__ ghist, unsigned long long* __restrict__ info) {
    __shared__ unsigned hist[HIST ? MINE_B1 : 1];
    if constexpr (HIST) {
        mine_clear(hist, MINE_B1);
        if (blockIdx.x == 0 && threadIdx.x == 0) info[2] = 0;             // the apply kernel's blocks add their kept pixels into it
    }
    const long long groups = (N + 3) >> 2;
    const long long step = (long long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    MinePixels<C, TT> a, b;              // calibration.hip's ping-pong: `g - lane` is the wave's first group, the loop is wave-uniform
    mine_load<C, TT, VEC>(a, logits, pitch, target, pw, N, 4 * g, pw_vec != 0);
    while (g - lane < groups) {
        mine_load<C, TT, VEC>(b, logits, pitch, target, pw, N, 4 * (g + step), pw_vec != 0);
        mine_nll_work<C, TT, HIST>(a, N, 4 * g, ign, nll_out, out_vec != 0, hist);
        g += step;
        if (g - lane >= groups) break;
        mine_load<C, TT, VEC>(a, logits, pitch, target, pw, N, 4 * (g + step), pw_vec != 0);
        mine_nll_work<C, TT, HIST>(b, N, 4 * g, ign, nll_out, out_vec != 0, hist);
        g += step;
    }
    if constexpr (HIST) mine_flush(hist, MINE_B1, ghist);
}

// ---- the passes over a stored map -------------------------------------------------------------------------------------------------------------
// PASS 1: the first histogram of a map that was given (pylc_hard_select); 2 and 3: scan the histogram before, count the next digit of the
// candidates that carry the prefix.  pw (may be NULL): a value >= 0 counts only under a weight that takes part (a map this library wrote
// says so itself, so the fused form passes NULL).
template <int PASS>
__global__ __launch_bounds__(256) void mine_hist_kernel(const float* __restrict__ nll, long long N, const float* __restrict__ pw, int vec,
                                                         double keep, long long min_kept, unsigned* __restrict__ ws,
                                                         unsigned long long* __restrict__ info) {
    __shared__ MineLds lds;
    unsigned* h1 = ws;
    unsigned* h2 = ws + MINE_B1;
    unsigned* h3 = ws + MINE_B1 + MINE_B2;
    unsigned* state = ws + MINE_HIST_WORDS;
    unsigned prefix = 0;
    if constexpr (PASS == 1) {
        if (blockIdx.x == 0 && threadIdx.x == 0) info[2] = 0;
    } else if constexpr (PASS == 2) {
        mine_scan<MINE_B1, true>(h1, 0, keep, min_kept, lds);
        const unsigned d1 = lds.res[0], rem = lds.res[1], n_valid = lds.res[2], k = lds.res[3];
        __syncthreads();
        if (blockIdx.x == 0 && threadIdx.x == 0) { state[ST_NVALID] = n_valid; state[ST_K] = k; state[ST_D1] = d1; state[ST_REM1] = rem; }
        if (k == 0) return;                               // nothing is selected by rank: the later passes have nothing to find
        prefix = d1;
    } else {
        const unsigned k = state[ST_K], d1 = state[ST_D1];
        mine_scan<MINE_B2, false>(h2, k == 0 ? 0u : state[ST_REM1], 0.0, 0, lds);
        const unsigned d2 = lds.res[0], rem = lds.res[1];
        __syncthreads();
        if (blockIdx.x == 0 && threadIdx.x == 0) { state[ST_D2] = d2; state[ST_REM2] = rem; }
        if (k == 0) return;
        prefix = (d1 << 10) | d2;
    }
    constexpr int BINS = PASS == 1 ? MINE_B1 : PASS == 2 ? MINE_B2 : MINE_B3;
    unsigned* ghist = PASS == 1 ? h1 : PASS == 2 ? h2 : h3;
    mine_clear(lds.hist, BINS);
    const long long groups = (N + 3) >> 2;
    const long long step = (long long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g - lane < groups; g += step) {      // wave-uniform
        float v[4], u[4] = {1.f, 1.f, 1.f, 1.f};
        const long long first = 4 * g < N ? 4 * g : ((N - 1) & ~3ll);
        mine_ld4(v, nll, N, first, vec != 0);
        if (pw != nullptr) mine_ld4(u, pw, N, first, vec != 0);
        int cell[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool cand = 4 * g + j < N && mine_is_value(v[j]) && mine_weight(u[j]) == 0;
            const unsigned key = mine_key(v[j]);
            if constexpr (PASS == 1) cell[j] = cand ? (int)(key >> 20) : -1;
            else if constexpr (PASS == 2) cell[j] = (cand && (key >> 20) == prefix) ? (int)((key >> 10) & 1023u) : -1;
            else cell[j] = (cand && (key >> 10) == prefix) ? (int)(key & 1023u) : -1;
        }
        mine_count(cell, lds.hist);
    }
    mine_flush(lds.hist, BINS, ghist);
}

// scans the last histogram, then writes the weight map and info
__global__ __launch_bounds__(256) void mine_apply_kernel(const float* __restrict__ nll, long long N, const float* __restrict__ pw, int vec,
                                                          unsigned cap_bits, float* __restrict__ out, const unsigned* __restrict__ ws,
                                                          unsigned long long* __restrict__ info) {
    __shared__ MineLds lds;
    const unsigned* h3 = ws + MINE_B1 + MINE_B2;
    const unsigned* state = ws + MINE_HIST_WORDS;
    const unsigned n_valid = state[ST_NVALID], k = state[ST_K];
    mine_scan<MINE_B3, false>(h3, k == 0 ? 0u : state[ST_REM2], 0.0, 0, lds);
    const unsigned tau_k = k == 0 ? MINE_INF_BITS : (state[ST_D1] << 20) | (state[ST_D2] << 10) | lds.res[0];
    // without a candidate nothing is compared with tau: it is reported as +inf whatever the cap
    const unsigned tau = n_valid == 0 ? MINE_INF_BITS : (tau_k < cap_bits ? tau_k : cap_bits);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        info[0] = n_valid;
        info[1] = k;
        info[3] = tau;
    }
    unsigned kept = 0;
    const long long groups = (N + 3) >> 2;
    const long long step = (long long)gridDim.x * 256;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += step) {
        float v[4], u[4] = {1.f, 1.f, 1.f, 1.f}, o[4];
        mine_ld4(v, nll, N, 4 * g, vec != 0);
        if (pw != nullptr) mine_ld4(u, pw, N, 4 * g, vec != 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int w = mine_weight(u[j]);
            if (v[j] == -1.f) {
                o[j] = 0.f;                               // ignored, or of weight zero
            } else if (mine_is_value(v[j]) && w != 2) {
                const bool keep_it = w == 0 && mine_key(v[j]) >= tau;
                o[j] = keep_it ? u[j] : 0.f;              // (a value under a weight of zero is no candidate: 0)
                kept += keep_it && 4 * g + j < N;
            } else {
                o[j] = u[j];                              // -2, NaN, another negative, a bad weight: the loss that follows must see it
            }
        }
        mine_st4(o, out, N, 4 * g, vec != 0);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) kept += (unsigned)__shfl_xor((int)kept, s, 64);
    if ((threadIdx.x & 63) == 0 && kept != 0) atomicAdd(&info[2], (unsigned long long)kept);
}

static int mine_blocks(long long N, int grid = MINE_GRID) {
    const long long want = cdiv<long long>((N + 3) >> 2, 256);
    return (int)(want < grid ? want : grid);
}

template <int C, typename TT, bool HIST>
static void mine_nll_launch(bool vec, int blocks, hipStream_t st, const float* logits, int pitch, const void* target, long long N, long long ign,
                            const float* pw, int pw_vec, float* nll_out, int out_vec, unsigned* ghist, unsigned long long* info) {
    if (vec)
        hipLaunchKernelGGL((mine_nll_kernel<C, TT, true, HIST>), dim3(blocks), dim3(256), 0, st, logits, pitch, static_cast<const TT*>(target), N,
                           ign, pw, pw_vec, nll_out, out_vec, ghist, info);
    else
        hipLaunchKernelGGL((mine_nll_kernel<C, TT, false, HIST>), dim3(blocks), dim3(256), 0, st, logits, pitch, static_cast<const TT*>(target), N,
                           ign, pw, pw_vec, nll_out, out_vec, ghist, info);
}

template <int C, typename... Args>
static void mine_nll_pick(bool hist, int target_bytes, Args... args) {
    if (hist && target_bytes == 8) mine_nll_launch<C, long long, true>(args...);
    else if (hist) mine_nll_launch<C, unsigned char, true>(args...);
    else if (target_bytes == 8) mine_nll_launch<C, long long, false>(args...);
    else mine_nll_launch<C, unsigned char, false>(args...);
}

}  // namespace pylc

using namespace pylc;

static bool mine_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks of the logits side, as pylc_multiloss_stats_w states them
static int mine_logits_check(const char* who, const float* logits, int pitch, const void* target, int target_bytes, long long N, int C,
                             const float* pixel_weights) {
    PYLC_REQUIRE(C >= 2 && C <= PYLC_MAX_CLASSES, "%s: n_classes=%d unsupported (2..%d)", who, C, PYLC_MAX_CLASSES);
    PYLC_REQUIRE(target_bytes == 1 || target_bytes == 8, "%s: target_bytes=%d (1: uint8, 8: int64)", who, target_bytes);
    PYLC_REQUIRE(target, "%s: target is NULL", who);
    PYLC_REQUIRE(pitch >= C, "%s: pitch=%d below n_classes=%d", who, pitch, C);
    PYLC_REQUIRE(N > 0 && N <= MINE_MAX_PIXELS, "%s: N=%lld outside 1..2^31-1", who, N);
    PYLC_REQUIRE(logits, "%s: logits is NULL", who);
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 3) == 0 && (target_bytes != 8 || (reinterpret_cast<uintptr_t>(target) & 7) == 0) &&
                     (reinterpret_cast<uintptr_t>(pixel_weights) & 3) == 0,
                 "%s: a buffer is not aligned to its element", who);
    return PYLC_OK;
}

// the checks of the selection side
static int mine_select_check(const char* who, long long N, const float* pixel_weights, double keep, long long min_kept, float nll_cap,
                             const float* out, const long long* info, const void* workspace) {
    PYLC_REQUIRE(N > 0 && N <= MINE_MAX_PIXELS, "%s: N=%lld outside 1..2^31-1", who, N);
    PYLC_REQUIRE(keep >= 0.0 && keep <= 1.0, "%s: keep=%g outside [0, 1]", who, keep);                   // NaN fails both
    PYLC_REQUIRE(min_kept >= 0, "%s: min_kept=%lld is negative", who, min_kept);
    PYLC_REQUIRE(nll_cap >= 0.f, "%s: nll_cap=%g is negative or NaN", who, (double)nll_cap);
    PYLC_REQUIRE(!(keep == 0.0 && min_kept == 0 && nll_cap == INFINITY), "%s: keep=0, min_kept=0 and no cap select nothing", who);
    PYLC_REQUIRE(out && info && workspace, "%s: out, info or workspace is NULL", who);
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(info) & 7) == 0 && mine_al16(workspace) &&
                     (reinterpret_cast<uintptr_t>(pixel_weights) & 3) == 0,
                 "%s: a buffer is not aligned to its element (the workspace to 16 bytes)", who);
    return PYLC_OK;
}

extern "C" size_t pylc_mining_workspace_bytes(long long N) {
    if (N <= 0 || N > MINE_MAX_PIXELS) return 0;
    return MINE_HEAD_BYTES + (((size_t)N * sizeof(float) + 255) & ~(size_t)255);
}

static int mine_nll_dispatch(bool hist, const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                             const float* pw, float* nll_out, unsigned* ghist, unsigned long long* info, hipStream_t st) {
    const bool vec = pitch % 4 == 0 && mine_al16(logits);
    const int blocks = mine_blocks(N);
    const long long ign = ignore_index;
    const int pw_vec = mine_al16(pw), out_vec = mine_al16(nll_out);
#define LAUNCH_MN(CC) \
    mine_nll_pick<CC>(hist, target_bytes, vec, blocks, st, logits, pitch, target, N, ign, pw, pw_vec, nll_out, out_vec, ghist, info)
    PYLC_FOR_CLASSES(C, LAUNCH_MN, "mining")
#undef LAUNCH_MN
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

// passes 2, 3 and apply over a stored map whose first histogram is taken; pw_hist: the weights the histogram passes judge candidates by
static int mine_finish(const float* nll, long long N, const float* pw_hist, const float* pw, double keep, long long min_kept, float nll_cap,
                       float* out, unsigned long long* info, unsigned* ws, hipStream_t st) {
    const int blocks = mine_blocks(N, MINE_MAP_GRID);
    const int vec_h = mine_al16(nll) && mine_al16(pw_hist);
    const int vec_a = mine_al16(nll) && mine_al16(pw) && mine_al16(out);
    unsigned cap_bits;
    const float cap = nll_cap + 0.f;                                       // -0 -> +0
    memcpy(&cap_bits, &cap, sizeof(cap_bits));
    hipLaunchKernelGGL(mine_hist_kernel<2>, dim3(blocks), dim3(256), 0, st, nll, N, pw_hist, vec_h, keep, min_kept, ws, info);
    PYLC_LAUNCH_CHECK();
    hipLaunchKernelGGL(mine_hist_kernel<3>, dim3(blocks), dim3(256), 0, st, nll, N, pw_hist, vec_h, keep, min_kept, ws, info);
    PYLC_LAUNCH_CHECK();
    hipLaunchKernelGGL(mine_apply_kernel, dim3(blocks), dim3(256), 0, st, nll, N, pw, vec_a, cap_bits, out, ws, info);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_pixel_nll(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                              const float* pixel_weights, float* nll_out, void* stream) {
    if (int rc = mine_logits_check("pixel_nll", logits, pitch, target, target_bytes, N, C, pixel_weights)) return rc;
    PYLC_REQUIRE(nll_out && (reinterpret_cast<uintptr_t>(nll_out) & 3) == 0, "pixel_nll: nll_out is NULL or not 4-byte aligned");
    return mine_nll_dispatch(false, logits, pitch, target, target_bytes, N, C, ignore_index, pixel_weights, nll_out, nullptr, nullptr,
                             as_stream(stream));
}

extern "C" int pylc_hard_select(const float* nll, long long N, const float* pixel_weights, double keep, long long min_kept, float nll_cap,
                                float* out, long long* info, void* workspace, void* stream) {
    if (int rc = mine_select_check("hard_select", N, pixel_weights, keep, min_kept, nll_cap, out, info, workspace)) return rc;
    PYLC_REQUIRE(nll && (reinterpret_cast<uintptr_t>(nll) & 3) == 0, "hard_select: nll is NULL or not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    unsigned* ws = static_cast<unsigned*>(workspace);
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    PYLC_HIP(hipMemsetAsync(ws, 0, MINE_HIST_WORDS * sizeof(unsigned), st));
    hipLaunchKernelGGL(mine_hist_kernel<1>, dim3(mine_blocks(N, MINE_MAP_GRID)), dim3(256), 0, st, nll, N, pixel_weights,
                       (int)(mine_al16(nll) && mine_al16(pixel_weights)), keep, min_kept, ws, inf);
    PYLC_LAUNCH_CHECK();
    return mine_finish(nll, N, pixel_weights, pixel_weights, keep, min_kept, nll_cap, out, inf, ws, st);
}

extern "C" int pylc_hard_pixel_weights(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                                       const float* pixel_weights, double keep, long long min_kept, float nll_cap, float* nll_out, float* out,
                                       long long* info, void* workspace, void* stream) {
    if (int rc = mine_logits_check("hard_pixel_weights", logits, pitch, target, target_bytes, N, C, pixel_weights)) return rc;
    if (int rc = mine_select_check("hard_pixel_weights", N, pixel_weights, keep, min_kept, nll_cap, out, info, workspace)) return rc;
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(nll_out) & 3) == 0, "hard_pixel_weights: nll_out is not 4-byte aligned");
    hipStream_t st = as_stream(stream);
    unsigned* ws = static_cast<unsigned*>(workspace);
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    float* map = nll_out ? nll_out : reinterpret_cast<float*>(static_cast<char*>(workspace) + MINE_HEAD_BYTES);
    PYLC_HIP(hipMemsetAsync(ws, 0, MINE_HIST_WORDS * sizeof(unsigned), st));
    if (int rc = mine_nll_dispatch(true, logits, pitch, target, target_bytes, N, C, ignore_index, pixel_weights, map, ws, inf, st)) return rc;
    // the map says itself which pixels take part (a value >= 0 was written under a weight that does): the histogram passes read no weights
    return mine_finish(map, N, nullptr, pixel_weights, keep, min_kept, nll_cap, out, inf, ws, st);
}
