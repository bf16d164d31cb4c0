// Validation scores: from the network's NHWC logits straight to class bytes and confusion counts, in one pass.
//
// What a validation pass otherwise needs for the same matrix is an argmax that writes an int64 mask (8 B per pixel out, 8 B back in) and
// pylc_confusion_matrix on it: two launches and 16 extra bytes per pixel.  Here a pixel's logits are read once, its class is the FIRST
// maximum (the strict `>` scan of stitch_argmax_kernel, numpy's argmax), and cell target * C + class of an integer matrix is counted --
// exact, and independent of the order in which pixels arrive.
//
// Geometry: a lane takes 4 consecutive pixels (one dword of the class mask wherever that dword is aligned), a block of 256 lanes 1024,
// and at most SCORE_GRID blocks walk the pixels in a grid-stride loop.  With one block per CU there is one wave per SIMD, so the loads of
// the NEXT round are issued before the current round is worked on (two register sets, ping-pong): the memory pipe stays busy while the
// wave compares and counts.
//
// Counting: 32-bit counters in LDS, one 64-bit global atomic per non-zero cell per block (as confusion_kernel).  Masks are blobs, so the
// 256 pixels of a wave's round mostly share one or two cells and one LDS atomic per pixel would serialise on them (section 5.6 has the same
// finding for the tile histogram).  Each wave therefore first reduces in registers: the cell of the first lane that still holds one is
// broadcast, a ballot per pixel slot finds every pixel of the wave with that cell, the leader adds the population count, those pixels
// retire.  SCORE_ROUNDS such rounds clear a blob mask; what is left after them (uniformly random cells: ~80 distinct ones) goes to LDS with
// one atomic per pixel, where it hardly collides.  Either way every pixel is added exactly once.
//
// pylc_logits_score_ex is the same kernel with one more cell: a target equal to the ignore label is counted in cell
// C*C + 1 instead of the matrix or the out-of-range cell C*C.  The label is a kernel argument; without it the extra cell stays empty and is
// not written back.
#include "common.h"
#include "score_pixels.h"

namespace pylc {

constexpr int SCORE_MAXC = PYLC_MAX_CLASSES;
constexpr int SCORE_GRID = kNumCU;         // blocks at most: one per CU, 262144 pixels per round of the grid
constexpr int SCORE_ROUNDS = 4;            // wave-level rounds before the per-pixel LDS atomics
// One block counts at most 1024 * ceil(ceil((N + 3) / 4) / (256 * SCORE_GRID)) pixels into its 32-bit LDS counters: below 2^32 for every
// N <= 2^39, which the entry point checks (2^39 pixels of logits are 2 TiB at the smallest pitch).
constexpr long long SCORE_MAX_PIXELS = 1ll << 39;

// has_ign: a target equal to `ign` (compared after widening) goes to cell C*C + 1 instead of the matrix or the bad cell C*C
template <int C, typename TT, bool HAS_T>
__device__ __forceinline__ void score_work(const ScorePixels<C, TT>& px, long long N, long long first, unsigned char* __restrict__ mask,
                                           unsigned int* hist, bool has_ign, long long ign) {
    int cls[4], cell[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int best = 0;
        float bv = px.v[k][0];
#pragma unroll
        for (int c = 1; c < C; ++c) if (px.v[k][c] > bv) { bv = px.v[k][c]; best = c; }     // first maximum (np.argmax)
        cls[k] = best;
        ok[k] = first + k >= 0 && first + k < N;
    }
    if (mask) {
        if (ok[0] && ok[3]) {        // mask + first is dword-aligned by the choice of `off`
            *reinterpret_cast<unsigned int*>(mask + first) = (unsigned)cls[0] | (unsigned)cls[1] << 8 | (unsigned)cls[2] << 16 | (unsigned)cls[3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (ok[k]) mask[first + k] = (unsigned char)cls[k];
        }
    }
    if constexpr (!HAS_T) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long t = (unsigned long long)(long long)px.t[k];        // a negative int64 target is out of range too
        const bool ignored = has_ign && (long long)px.t[k] == ign;
        cell[k] = !ok[k] ? -1 : ignored ? C * C + 1 : (t < (unsigned long long)C ? (int)t * C + cls[k] : C * C);
    }
    // wave-level rounds: every lane of the wave is here (the caller's loop is wave-uniform), retired pixels hold -1
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int r = 0; r < SCORE_ROUNDS; ++r) {
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
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) if (cell[k] >= 0) atomicAdd(&hist[cell[k]], 1u);
}

// HAS_T: a target and counts are given (else mask only: TT is not used)
template <int C, typename TT, bool VEC, bool HAS_T>
__global__ __launch_bounds__(256) void logits_score_kernel(const float* __restrict__ logits, int pitch, const TT* __restrict__ target, long long N,
                                                            int off, unsigned char* __restrict__ mask, unsigned long long* __restrict__ counts,
                                                            int has_ign, long long ign) {
    __shared__ unsigned int hist[C * C + 2];
    if constexpr (HAS_T) {
        for (int i = threadIdx.x; i < C * C + 2; i += 256) hist[i] = 0;
        __syncthreads();
    }
    const long long groups = (N + off + 3) >> 2;
    const long long step = (long long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    // `g - lane` is the wave's first group: the loop conditions are the same for the 64 lanes of a wave
    ScorePixels<C, TT> a, b;
    // The next round's loads are issued unconditionally (a round past the end re-reads the last pixel: indices are clamped), so that the
    // number of loads in flight is the same on every path and the waits in score_work count past them instead of draining them.
    score_load<C, TT, VEC, HAS_T>(a, logits, pitch, target, N, 4 * g - off);
    while (g - lane < groups) {
        score_load<C, TT, VEC, HAS_T>(b, logits, pitch, target, N, 4 * (g + step) - off);
        score_work<C, TT, HAS_T>(a, N, 4 * g - off, mask, hist, has_ign != 0, ign);
        g += step;
        if (g - lane >= groups) break;
        score_load<C, TT, VEC, HAS_T>(a, logits, pitch, target, N, 4 * (g + step) - off);
        score_work<C, TT, HAS_T>(b, N, 4 * g - off, mask, hist, has_ign != 0, ign);
        g += step;
    }
    if constexpr (HAS_T) {
        __syncthreads();
        for (int i = threadIdx.x; i < C * C + 1 + has_ign; i += 256)      // (cell C*C + 1 exists in `counts` only with has_ign, and is only then used)
            if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
    }
}

template <int C, typename TT, bool HAS_T>
static void score_launch(bool vec, int blocks, hipStream_t st, const float* logits, int pitch, const void* target, long long N, int off,
                         unsigned char* mask, unsigned long long* counts, int has_ign, long long ign) {
    if (vec)
        hipLaunchKernelGGL((logits_score_kernel<C, TT, true, HAS_T>), dim3(blocks), dim3(256), 0, st, logits, pitch, static_cast<const TT*>(target),
                           N, off, mask, counts, has_ign, ign);
    else
        hipLaunchKernelGGL((logits_score_kernel<C, TT, false, HAS_T>), dim3(blocks), dim3(256), 0, st, logits, pitch, static_cast<const TT*>(target),
                           N, off, mask, counts, has_ign, ign);
}

}  // namespace pylc

using namespace pylc;

static int logits_score_impl(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, unsigned char* mask,
                             unsigned long long* counts, int has_ign, long long ign, void* stream) {
    PYLC_REQUIRE(logits, "logits_score: logits is NULL");
    PYLC_REQUIRE(mask || counts, "logits_score: mask and counts are both NULL, nothing to compute");
    PYLC_REQUIRE(C >= 2 && C <= SCORE_MAXC, "logits_score: n_classes=%d unsupported (2..%d)", C, SCORE_MAXC);
    PYLC_REQUIRE(pitch >= C, "logits_score: pitch=%d below n_classes=%d", pitch, C);
    PYLC_REQUIRE(N > 0 && N <= SCORE_MAX_PIXELS, "logits_score: N=%lld outside 1..2^39 (the bound of the 32-bit block counters)", N);
    PYLC_REQUIRE(target_bytes == 0 || target_bytes == 1 || target_bytes == 8, "logits_score: target_bytes=%d (0: none, 1: uint8, 8: int64)",
                 target_bytes);
    PYLC_REQUIRE((target != nullptr) == (target_bytes != 0), "logits_score: target and target_bytes=%d disagree", target_bytes);
    PYLC_REQUIRE(!counts || target, "logits_score: counts without target");
    PYLC_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 3) == 0 && (reinterpret_cast<uintptr_t>(counts) & 7) == 0 &&
                 (target_bytes != 8 || (reinterpret_cast<uintptr_t>(target) & 7) == 0), "logits_score: a buffer is not aligned to its element");
    const bool vec = pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    const int off = mask ? (int)(reinterpret_cast<uintptr_t>(mask) & 3) : 0;      // groups of 4 pixels start where the mask's dwords do
    const long long groups = (N + off + 3) >> 2;
    const long long want = cdiv<long long>(groups, 256);
    const int blocks = (int)(want < SCORE_GRID ? want : SCORE_GRID);
    hipStream_t st = as_stream(stream);
    if (!counts) {                                                                 // mask only: a target, if any, is not read
#define LAUNCH_SC(CC) score_launch<CC, unsigned char, false>(vec, blocks, st, logits, pitch, nullptr, N, off, mask, nullptr, 0, 0)
        PYLC_FOR_CLASSES(C, LAUNCH_SC, "logits_score")
#undef LAUNCH_SC
    } else if (target_bytes == 8) {
#define LAUNCH_SC(CC) score_launch<CC, long long, true>(vec, blocks, st, logits, pitch, target, N, off, mask, counts, has_ign, ign)
        PYLC_FOR_CLASSES(C, LAUNCH_SC, "logits_score")
#undef LAUNCH_SC
    } else {
#define LAUNCH_SC(CC) score_launch<CC, unsigned char, true>(vec, blocks, st, logits, pitch, target, N, off, mask, counts, has_ign, ign)
        PYLC_FOR_CLASSES(C, LAUNCH_SC, "logits_score")
#undef LAUNCH_SC
    }
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_logits_score(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, unsigned char* mask,
                                 unsigned long long* counts, void* stream) {
    return logits_score_impl(logits, pitch, target, target_bytes, N, C, mask, counts, 0, 0, stream);
}

extern "C" int pylc_logits_score_ex(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, unsigned char* mask,
                                    int ignore_index, unsigned long long* counts, void* stream) {
    return logits_score_impl(logits, pitch, target, target_bytes, N, C, mask, counts, 1, (long long)ignore_index, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Evaluation: confusion matrix of class-index masks (replaces the sklearn passes over ~1e7-pixel flattened arrays in
// utils/metrics.py:64-88; the scores are simple functions of the n_cls x n_cls count matrix).  Integer counts in LDS,
// merged with 64-bit integer atomics: exact and order-independent.  Evaluator.validate()'s coverage quirk
// (utils/evaluate.py:171-174: the first n_classes pixels of both arrays are overwritten with 0..n_classes-1) is applied
// on the fly when force_coverage != 0.
// ---------------------------------------------------------------------------------------------------------------------
namespace pylc {
// IGN: pixels whose true label equals `ignore` (compared after widening) or lies outside 0..C-1 are left out of the matrix and counted in
// skipped[1] / skipped[0].  Without IGN a pixel with either label out of range is dropped silently, as before.
template <typename TT, typename TP, bool IGN>
__global__ __launch_bounds__(256) void confusion_kernel(const TT* __restrict__ yt, const TP* __restrict__ yp, long long n, int C,
                                                         int force_coverage, unsigned long long* __restrict__ cm, long long ignore,
                                                         unsigned long long* __restrict__ skipped) {
    __shared__ unsigned int hist[SCORE_MAXC * SCORE_MAXC + 2];
    for (int i = threadIdx.x; i < C * C + 2; i += 256) hist[i] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if constexpr (IGN) {
            long long tl = (long long)yt[i];
            int p = (int)yp[i];
            if (force_coverage && i < C) { tl = i; p = (int)i; }
            if (tl == ignore) atomicAdd(&hist[C * C + 1], 1u);
            else if ((unsigned long long)tl >= (unsigned long long)C) atomicAdd(&hist[C * C], 1u);
            else if ((unsigned)p < (unsigned)C) atomicAdd(&hist[(int)tl * C + p], 1u);
        } else {
            int t = (int)yt[i], p = (int)yp[i];
            if (force_coverage && i < C) { t = (int)i; p = (int)i; }
            if ((unsigned)t < (unsigned)C && (unsigned)p < (unsigned)C) atomicAdd(&hist[t * C + p], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256)
        if (hist[i]) atomicAdd(&cm[i], (unsigned long long)hist[i]);
    if constexpr (IGN) {
        if (skipped != nullptr && threadIdx.x < 2 && hist[C * C + threadIdx.x]) atomicAdd(&skipped[threadIdx.x], (unsigned long long)hist[C * C + threadIdx.x]);
    }
}

template <bool IGN>
static void confusion_launch(const void* y_true, int true_bytes, const void* y_pred, int pred_bytes, long long n, int C, int force_coverage,
                             unsigned long long* cm, long long ignore, unsigned long long* skipped, hipStream_t st) {
    const long long want = cdiv<long long>(n, 256);
    const int blocks = (int)(want < 1024 ? want : 1024);
    if (true_bytes == 1 && pred_bytes == 1)
        hipLaunchKernelGGL((confusion_kernel<unsigned char, unsigned char, IGN>), dim3(blocks), dim3(256), 0, st, (const unsigned char*)y_true,
                           (const unsigned char*)y_pred, n, C, force_coverage, cm, ignore, skipped);
    else if (true_bytes == 8 && pred_bytes == 1)
        hipLaunchKernelGGL((confusion_kernel<long long, unsigned char, IGN>), dim3(blocks), dim3(256), 0, st, (const long long*)y_true,
                           (const unsigned char*)y_pred, n, C, force_coverage, cm, ignore, skipped);
    else if (true_bytes == 1 && pred_bytes == 8)
        hipLaunchKernelGGL((confusion_kernel<unsigned char, long long, IGN>), dim3(blocks), dim3(256), 0, st, (const unsigned char*)y_true,
                           (const long long*)y_pred, n, C, force_coverage, cm, ignore, skipped);
    else
        hipLaunchKernelGGL((confusion_kernel<long long, long long, IGN>), dim3(blocks), dim3(256), 0, st, (const long long*)y_true,
                           (const long long*)y_pred, n, C, force_coverage, cm, ignore, skipped);
}
}  // namespace pylc

template <bool IGN>
static int confusion_impl(const char* who, const void* y_true, int true_bytes, const void* y_pred, int pred_bytes, long long n, int C,
                          int force_coverage, unsigned long long* cm, long long ignore, unsigned long long* skipped, void* stream) {
    PYLC_REQUIRE(y_true && y_pred && cm && n > 0 && C >= 2 && C <= SCORE_MAXC, "%s: bad arguments", who);
    PYLC_REQUIRE((true_bytes == 1 || true_bytes == 8) && (pred_bytes == 1 || pred_bytes == 8), "%s: masks must be uint8 or int64", who);
    confusion_launch<IGN>(y_true, true_bytes, y_pred, pred_bytes, n, C, force_coverage, cm, ignore, skipped, as_stream(stream));
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_confusion_matrix(const void* y_true, int true_bytes, const void* y_pred, int pred_bytes, long long n, int C,
                                     int force_coverage, unsigned long long* cm /* [C*C], zeroed by the caller */, void* stream) {
    return confusion_impl<false>("confusion_matrix", y_true, true_bytes, y_pred, pred_bytes, n, C, force_coverage, cm, 0, nullptr, stream);
}

extern "C" int pylc_confusion_matrix_ex(const void* y_true, int true_bytes, const void* y_pred, int pred_bytes, long long n, int C,
                                        int force_coverage, unsigned long long* cm /* [C*C], zeroed by the caller */, int ignore_index,
                                        unsigned long long* n_skipped /* [2]: bad, ignored; ADDED into; may be NULL */, void* stream) {
    return confusion_impl<true>("confusion_matrix_ex", y_true, true_bytes, y_pred, pred_bytes, n, C, force_coverage, cm, (long long)ignore_index,
                                n_skipped, stream);
}
