// Fused MultiLoss head: weighted/unweighted cross-entropy + Dice + Focal in ONE per-pixel pass forward
// (3 + 3C partial sums) and ONE per-pixel pass backward (closed form).
//
// Replaces models/modules/loss.py: ce_loss :66-69, dice_loss :137-146, focal_loss :174-189, forward :107-112
// (the reference runs 3 softmaxes + 2 one-hots + ~20 elementwise passes over B*C*H*W).
// logits are NHWC [N pixels][pitch]; one thread owns one pixel (its C logits are contiguous).
//
// Ignore label (pylc_multiloss_*_ex): the kernels are templates over the target's width (TT: int64 or uint8, read at
// any byte address) and IGN.  With IGN a pixel is VALID when its target, widened to 64 bits, is not `ignore` and lies in 0..C-1; every
// other pixel is skipped before its logits row is loaded (unpainted regions are blobs: whole waves skip), contributes to no sum, is never
// used as an index, and gets an all-zero gradient row.  A valid pixel runs the very same per-pixel code as without IGN, in the same
// thread of the same grid, so <int64, IGN = false> (the entry points without _ex) is the code as it was, and the _ex path with nothing
// skipped gives the same bits.  The number of valid pixels is not passed in: it is the sum of the class counts stats[3 + 2C + c], taken in
// double from the (all-reduced) statistics.  Those counts are exact as long as a class holds at most 2^24 = 16 777 216 valid pixels
// globally: a thread's and a block's partial counts are sums of ones in fp32 (exact below 2^24 per block, i.e. for N < 2^34),
// column_sum_kernel adds the <= 1024 block partials in fp64 (exact), and only the final store of a class total to the fp32 stats (and a
// data-parallel all-reduce of it) rounds -- to nearest, relative error <= 2^-25 per class beyond 2^24 pixels in it.
//
// Pixel weights (pylc_multiloss_*_w): PW adds a float weight u_n per pixel, read next to the target and before the
// logits row.  A pixel takes part when its target is valid as above AND 0 < u_n <= FLT_MAX; u_n == 0 is skipped like an ignored pixel, a
// negative, NaN or infinite u_n is skipped and counted in n_bad (the target is judged first: an ignored target is never counted, whatever
// its weight).  u is ONE extra factor: u * w in the CE sum and its denominator, u on every Dice and Focal addend, gs * u on the gradient
// row, so stats[1] = sum u w, the class counts are sum u o_c and their sum is sum u -- what finalize_ex and the backward divide by already.
// Multiplying by exactly 1.0f changes no bit (the library is built with -ffp-contract=off and no existing operation is re-associated), so
// u == 1 gives the bits of the _ex path; PW = false is the code as it was.  The exactness argument above holds as written whenever every
// weight is 1; with other weights the class counts are fp32 sums of non-integers and round like every other sum of the statistics
// (a block partial's relative error grows with the pixels a thread adds, as for sum p_c).
#include <cfloat>

#include "common.h"

namespace pylc {

constexpr int MAXC = PYLC_MAX_CLASSES;
constexpr float kFlAlpha = 0.25f;   // config.py:207
constexpr float kFlEps = 1e-8f;     // loss.py:50
constexpr float kDiceSmooth = 1.f;  // config.py:204
constexpr int kLossBlocks = 1024;

template <int C>
__device__ __forceinline__ void softmax_px(const float* __restrict__ z, float (&p)[C], float& lse) {
    float zmax = z[0];
#pragma unroll
    for (int c = 1; c < C; ++c) zmax = fmaxf(zmax, z[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(z[c] - zmax); sum += p[c]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
    lse = zmax + logf(sum);
}

// partial[block][3 + 3C]
// n_bad (IGN only, may be NULL): the number of skipped pixels that are not `ignore` is ADDED into it
// PW (needs IGN): pw[n] weighs pixel n, see above; without PW pw is not read
template <int C, typename TT, bool IGN, bool PW>
__global__ __launch_bounds__(256) void multiloss_stats_kernel(const float* __restrict__ logits, int pitch, const TT* __restrict__ target,
                                                              long long N, const float* __restrict__ cw, float* __restrict__ partial,
                                                              long long ignore, unsigned long long* __restrict__ n_bad,
                                                              const float* __restrict__ pw) {
    static_assert(IGN || !PW, "pixel weights ride on the ignore path");
    __shared__ float red[4];
    float acc[3 + 3 * C];
#pragma unroll
    for (int k = 0; k < 3 + 3 * C; ++k) acc[k] = 0.f;
    unsigned int bad = 0;
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        const long long tl = (long long)target[n];
        float u = 1.f;
        if constexpr (PW) u = pw[n];
        if constexpr (IGN) {
            if (tl == ignore) continue;
            if ((unsigned long long)tl >= (unsigned long long)C) { ++bad; continue; }
        }
        if constexpr (PW) {
            if (u == 0.f) continue;
            if (!(u > 0.f && u <= FLT_MAX)) { ++bad; continue; }      // negative, NaN, infinite
        }
        float z[C], p[C], lse;
        const float* src = logits + n * pitch;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = src[c];
        softmax_px<C>(z, p, lse);
        const int t = (int)tl;
        float zt = 0.f, pt = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const bool is = (c == t);
            zt = is ? z[c] : zt;
            pt = is ? p[c] : pt;
            if constexpr (PW) {
                const float up = u * p[c];
                acc[3 + c] += is ? up : 0.f;
                acc[3 + C + c] += up;
                acc[3 + 2 * C + c] += is ? u : 0.f;
            } else {
                acc[3 + c] += is ? p[c] : 0.f;        // I_c
                acc[3 + C + c] += p[c];               // sum p_c
                acc[3 + 2 * C + c] += is ? 1.f : 0.f; // count_c
            }
        }
        const float w = cw != nullptr ? cw[t] : 1.f;
        const float q = pt + kFlEps;
        const float omq = 1.f - q;
        if constexpr (PW) {
            const float uw = u * w;
            acc[0] += uw * (lse - zt);
            acc[1] += uw;
            acc[2] += u * (-kFlAlpha * omq * omq * logf(q));
        } else {
            acc[0] += w * (lse - zt);                 // -log p_t via log-sum-exp (exact for saturated pixels)
            acc[1] += w;
            acc[2] += -kFlAlpha * omq * omq * logf(q);
        }
    }
    float* dst = partial + (size_t)blockIdx.x * (3 + 3 * C);
#pragma unroll
    for (int k = 0; k < 3 + 3 * C; ++k) {
        const float s = block_sum_256(acc[k], red);
        if (threadIdx.x == 0) dst[k] = s;
    }
    if constexpr (IGN) {
        if (n_bad != nullptr) {
            unsigned long long wave_bad = 0;
            for (int l = 0; l < 64; ++l) wave_bad += (unsigned)__shfl((int)bad, l, 64);
            if ((threadIdx.x & 63) == 0 && wave_bad != 0) atomicAdd(n_bad, wave_bad);
        }
    }
}

// the number of valid pixels of (all-reduced) stats: the sum of the class counts, in double
__device__ __forceinline__ double stats_n_valid(const float* __restrict__ stats, int C) {
    double n = 0.0;
    for (int c = 0; c < C; ++c) n += (double)stats[3 + 2 * C + c];
    return n;
}

// FROM_STATS: n is the valid count of the stats (the argument is not used); a zero count or weight sum gives 0, never a division by zero
template <bool FROM_STATS>
__global__ void multiloss_finalize_kernel(const float* __restrict__ stats, double n, int C, float w_ce, float w_d, float w_f,
                                          float* __restrict__ losses) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double ce, fl;
    if constexpr (FROM_STATS) {
        n = stats_n_valid(stats, C);
        ce = stats[1] > 0.f ? (double)stats[0] / (double)stats[1] : 0.0;
        fl = n > 0.0 ? (double)stats[2] / n : 0.0;
    } else {
        ce = (double)stats[0] / (double)stats[1];
        fl = (double)stats[2] / n;
    }
    double dsc = 0.0;
    for (int c = 0; c < C; ++c) {
        const double I = stats[3 + c], K = (double)stats[3 + C + c] + (double)stats[3 + 2 * C + c];
        dsc += 1.0 - (2.0 * I + kDiceSmooth) / (K + kDiceSmooth);
    }
    dsc /= C;
    losses[0] = (float)(w_ce * ce + w_d * dsc + w_f * fl);
    losses[1] = (float)ce;
    losses[2] = (float)dsc;
    losses[3] = (float)fl;
}

typedef float loss_f4 __attribute__((ext_vector_type(4)));

// IGN: inv_n is not used (1 / the valid count of `stats` instead, rounded as the host rounds 1 / n_global for the plain form); skipped
// pixels write a zero row of Cstore floats -- with 16-byte stores when zero16 (dpitch % 4 == 0 and an aligned base, so Cstore % 4 == 0)
// PW (needs IGN): a pixel whose weight is not in (0, FLT_MAX] is skipped too; the others' rows are scaled by gs * u
template <int C, typename TT, bool IGN, bool PW>
__global__ __launch_bounds__(256) void multiloss_bwd_kernel(const float* __restrict__ logits, int pitch, const TT* __restrict__ target,
                                                            long long N, const float* __restrict__ cw, const float* __restrict__ stats,
                                                            float inv_n, float w_ce, float w_d, float w_f,
                                                            const float* __restrict__ grad_scale, float* __restrict__ dlogits, int dpitch,
                                                            int Cstore, unsigned* __restrict__ amax_out, long long ignore, int zero16,
                                                            const float* __restrict__ pw) {
    static_assert(IGN || !PW, "pixel weights ride on the ignore path");
    // per-class Dice coefficients: dL_d/dp_c(n) = -[2 o_c (K_c + s) - (2 I_c + s)] / (K_c + s)^2 / C = o_c * A_c + B_c
    float dA[C], dB[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float I = stats[3 + c], K = stats[3 + C + c] + stats[3 + 2 * C + c];
        const float den = K + kDiceSmooth;
        dA[c] = -2.f / den / (float)C;
        dB[c] = (2.f * I + kDiceSmooth) / (den * den) / (float)C;
    }
    const float gs = grad_scale != nullptr ? grad_scale[0] : 1.f;
    float ce_norm;
    if constexpr (IGN) {
        const double nv = stats_n_valid(stats, C);
        inv_n = nv > 0.0 ? (float)(1.0 / nv) : 0.f;
        ce_norm = stats[1] > 0.f ? w_ce / stats[1] : 0.f;
    } else {
        ce_norm = w_ce / stats[1];             // unweighted: stats[1] = N
    }
    float gmax = 0.f;                          // max |dlogits|: the range the conv backward that receives them scales its operand with
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        const long long tl = (long long)target[n];
        float gsu = gs;
        bool skip_u = false;
        if constexpr (PW) {
            const float u = pw[n];
            skip_u = !(u > 0.f && u <= FLT_MAX);
            gsu = gs * u;
        }
        if constexpr (IGN) {
            if (tl == ignore || (unsigned long long)tl >= (unsigned long long)C || skip_u) {
                float* zrow = dlogits + n * dpitch;
                if (zero16) {
                    for (int c = 0; c < Cstore; c += 4) *reinterpret_cast<loss_f4*>(zrow + c) = loss_f4{0.f, 0.f, 0.f, 0.f};
                } else {
                    for (int c = 0; c < Cstore; ++c) zrow[c] = 0.f;
                }
                continue;
            }
        }
        float z[C], p[C], lse;
        const float* src = logits + n * pitch;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = src[c];
        softmax_px<C>(z, p, lse);
        const int t = (int)tl;
        float pt = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) pt = (c == t) ? p[c] : pt;
        const float w = cw != nullptr ? cw[t] : 1.f;
        // focal: f'(q) = alpha*gamma*(1-q)*log q - alpha*(1-q)^2/q, dq/dz_c = p_t (o_c - p_c)
        const float q = pt + kFlEps, omq = 1.f - q;
        const float fprime = kFlAlpha * 2.f * omq * logf(q) - kFlAlpha * omq * omq / q;
        const float fcoef = w_f * inv_n * fprime * pt;
        // dice through softmax: p_c (g_c - sum_k g_k p_k)
        float gdot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) gdot += ((c == t ? dA[c] : 0.f) + dB[c]) * p[c];
        float* dst = dlogits + n * dpitch;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float o = (c == t) ? 1.f : 0.f;
            const float gc = (c == t ? dA[c] : 0.f) + dB[c];
            const float d = ce_norm * w * (p[c] - o) + w_d * p[c] * (gc - gdot) + fcoef * (o - p[c]);
            dst[c] = gsu * d;
            gmax = fmaxf(gmax, fabsf(gsu * d));
        }
        for (int c = C; c < Cstore; ++c) dst[c] = 0.f;     // channel padding up to the pitch stays zero
    }
    if (amax_out != nullptr) amax_commit(gmax, amax_out);
}

// ---- soft targets (pylc_multiloss_*_soft, pylc_multiloss_*_ls) ----------------------------------------------------
// A pair of kernels of their own next to the <C, TT, IGN, PW> ones, which stay as they are: the target of pixel n is a ROW q of C
// non-negative floats, kept in registers next to z and p, and every term is its one-hot form with o_c replaced by q_c.  The row comes from
// one of three sources (SRC): a float32 [B,C,H,W] volume read in place through its four strides (the planar case reads consecutive
// addresses in consecutive lanes, class by class), teacher logits read the same way and put through softmax_px at inverse temperature
// `par`, or a hard target (TT, judged as by the kernels above) smoothed by `par`.  The pixel weight is a run-time NULL test here (one
// uniform branch; 1.0f is the multiplicative identity bit for bit), so the sources do not double the instantiations.
// Forward arithmetic, ordered so that a one-hot row reproduces the statistics of the PW kernel above bit for bit: the CE addend of a class is
// ((u w_c) q_c)(lse - z_c), the Dice one (u p_c) q_c, the count one u q_c, Focal is u * sum_c q_c f(x_c); the per-pixel sums start from
// +0 and a one-hot row adds +-0 in every class but one, which changes no bit (-ffp-contract=off, nothing re-associated).
enum { kSoftProbs = 0, kSoftLogits = 1, kSoftSmooth = 2 };

struct SoftSrc {
    const void* ptr;              // float volume / teacher logits, or the hard target
    long long sb, sc, sh, sw;     // strides of the volume in elements
    long long HW;                 // pixels of one image
    int W;
    int small;                    // N < 2^32: the pixel index splits with 32-bit divisions
    float par;                    // kSoftLogits: 1 / T; kSoftSmooth: the smoothing
    long long ignore;             // kSoftSmooth
};

// q of pixel n.  0: the row takes part; 1: skipped silently (a row that sums to 0, an ignored target); 2: skipped and counted
template <int C, int SRC, typename TT>
__device__ __forceinline__ int soft_row(const SoftSrc& s, long long n, float (&q)[C]) {
    if constexpr (SRC == kSoftSmooth) {
        const long long tl = (long long)static_cast<const TT*>(s.ptr)[n];
        if (tl == s.ignore) return 1;
        if ((unsigned long long)tl >= (unsigned long long)C) return 2;
        const float off = s.par / (float)C, on = (1.f - s.par) + off;      // smoothing 0: exactly 1 and 0
        const int t = (int)tl;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = (c == t) ? on : off;
        return 0;
    } else {
        long long b, y, x;
        if (s.small) {
            const unsigned nb = (unsigned)n / (unsigned)s.HW, r = (unsigned)n - nb * (unsigned)s.HW, ny = r / (unsigned)s.W;
            b = nb, y = ny, x = r - ny * (unsigned)s.W;
        } else {
            b = n / s.HW;
            const long long r = n - b * s.HW;
            y = r / s.W, x = r - y * s.W;
        }
        const float* src = static_cast<const float*>(s.ptr) + b * s.sb + y * s.sh + x * s.sw;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = src[c * s.sc];
        bool bad = false;
        if constexpr (SRC == kSoftProbs) {
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                bad |= !(q[c] >= 0.f && q[c] <= FLT_MAX);                   // negative, NaN, infinite
                sum += q[c];
            }
            if (bad) return 2;
            return sum == 0.f ? 1 : 0;                                     // non-negative addends: zero only when every entry is
        } else {
            float t[C], lse;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                t[c] = s.par * q[c];
                bad |= !(fabsf(t[c]) <= FLT_MAX);
            }
            if (bad) return 2;
            softmax_px<C>(t, q, lse);
            return 0;
        }
    }
}

// the weight of pixel n (pw == NULL: 1).  0: takes part; 1: u == 0; 2: negative, NaN, infinite
__device__ __forceinline__ int soft_weight(const float* __restrict__ pw, long long n, float& u) {
    u = 1.f;
    if (pw == nullptr) return 0;
    u = pw[n];
    if (u == 0.f) return 1;
    return (u > 0.f && u <= FLT_MAX) ? 0 : 2;
}

template <int C, int SRC, typename TT>
__global__ __launch_bounds__(256) void multiloss_stats_soft_kernel(const float* __restrict__ logits, int pitch, SoftSrc s, long long N,
                                                                   const float* __restrict__ cw, const float* __restrict__ pw,
                                                                   float* __restrict__ partial, unsigned long long* __restrict__ n_bad) {
    __shared__ float red[4];
    float acc[3 + 3 * C];
#pragma unroll
    for (int k = 0; k < 3 + 3 * C; ++k) acc[k] = 0.f;
    unsigned int bad = 0;
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        float q[C], u;
        const int row = soft_row<C, SRC, TT>(s, n, q);                    // the row is judged first, as the target is
        if (row != 0) { bad += row == 2; continue; }
        const int wt = soft_weight(pw, n, u);
        if (wt != 0) { bad += wt == 2; continue; }
        float z[C], p[C], lse;
        const float* src = logits + n * pitch;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = src[c];
        softmax_px<C>(z, p, lse);
        float ce = 0.f, den = 0.f, fl = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float up = u * p[c];
            acc[3 + c] += up * q[c];                  // I_c
            acc[3 + C + c] += up;                     // sum u p_c
            acc[3 + 2 * C + c] += u * q[c];           // sum u q_c
            const float uwq = (u * (cw != nullptr ? cw[c] : 1.f)) * q[c];
            ce += uwq * (lse - z[c]);
            den += uwq;
            const float x = p[c] + kFlEps, omx = 1.f - x;
            fl += q[c] * (-kFlAlpha * omx * omx * logf(x));
        }
        acc[0] += ce;
        acc[1] += den;
        acc[2] += u * fl;
    }
    float* dst = partial + (size_t)blockIdx.x * (3 + 3 * C);
#pragma unroll
    for (int k = 0; k < 3 + 3 * C; ++k) {
        const float v = block_sum_256(acc[k], red);
        if (threadIdx.x == 0) dst[k] = v;
    }
    if (n_bad != nullptr) {
        unsigned long long wave_bad = 0;
        for (int l = 0; l < 64; ++l) wave_bad += (unsigned)__shfl((int)bad, l, 64);
        if ((threadIdx.x & 63) == 0 && wave_bad != 0) atomicAdd(n_bad, wave_bad);
    }
}

// per pixel, times grad_scale * u:
//   CE    ce_norm (W p_c - w_c q_c),  W = sum_k w_k q_k
//   Dice  w_d p_c (g_c - sum_k g_k p_k),  g_c = q_c A_c + B_c
//   Focal w_f inv_n p_c (q_c f'(x_c) - sum_k q_k f'(x_k) p_k),  f'(x) = alpha gamma (1 - x) log x - alpha (1 - x)^2 / x
// inv_n = 1 / sum of the class counts = 1 / sum u q, as on the IGN path; skipped pixels write a zero row as there.
template <int C, int SRC, typename TT>
__global__ __launch_bounds__(256) void multiloss_bwd_soft_kernel(const float* __restrict__ logits, int pitch, SoftSrc s, long long N,
                                                                 const float* __restrict__ cw, const float* __restrict__ pw,
                                                                 const float* __restrict__ stats, float w_ce, float w_d, float w_f,
                                                                 const float* __restrict__ grad_scale, float* __restrict__ dlogits, int dpitch,
                                                                 int Cstore, unsigned* __restrict__ amax_out, int zero16) {
    float dA[C], dB[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float I = stats[3 + c], K = stats[3 + C + c] + stats[3 + 2 * C + c];
        const float den = K + kDiceSmooth;
        dA[c] = -2.f / den / (float)C;
        dB[c] = (2.f * I + kDiceSmooth) / (den * den) / (float)C;
    }
    const float gs = grad_scale != nullptr ? grad_scale[0] : 1.f;
    const double nv = stats_n_valid(stats, C);
    const float fscale = w_f * (nv > 0.0 ? (float)(1.0 / nv) : 0.f);
    const float ce_norm = stats[1] > 0.f ? w_ce / stats[1] : 0.f;
    float gmax = 0.f;
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        float q[C], u;
        if (soft_row<C, SRC, TT>(s, n, q) != 0 || soft_weight(pw, n, u) != 0) {
            float* zrow = dlogits + n * dpitch;
            if (zero16) {
                for (int c = 0; c < Cstore; c += 4) *reinterpret_cast<loss_f4*>(zrow + c) = loss_f4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (int c = 0; c < Cstore; ++c) zrow[c] = 0.f;
            }
            continue;
        }
        const float gsu = gs * u;
        float z[C], p[C], lse;
        const float* src = logits + n * pitch;
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = src[c];
        softmax_px<C>(z, p, lse);
        float fq[C];                                   // q_c f'(x_c)
        float wsum = 0.f, gdot = 0.f, fdot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            wsum += (cw != nullptr ? cw[c] : 1.f) * q[c];
            gdot += (q[c] * dA[c] + dB[c]) * p[c];
            const float x = p[c] + kFlEps, omx = 1.f - x;
            fq[c] = q[c] * (kFlAlpha * 2.f * omx * logf(x) - kFlAlpha * omx * omx / x);
            fdot += fq[c] * p[c];
        }
        float* dst = dlogits + n * dpitch;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float w = cw != nullptr ? cw[c] : 1.f;
            const float d = ce_norm * (wsum * p[c] - w * q[c]) + w_d * p[c] * ((q[c] * dA[c] + dB[c]) - gdot) + fscale * p[c] * (fq[c] - fdot);
            dst[c] = gsu * d;
            gmax = fmaxf(gmax, fabsf(gsu * d));
        }
        for (int c = C; c < Cstore; ++c) dst[c] = 0.f;
    }
    if (amax_out != nullptr) amax_commit(gmax, amax_out);
}

}  // namespace pylc

using namespace pylc;

extern "C" size_t pylc_multiloss_workspace_floats(long long N, int C) {
    (void)N;
    return (size_t)kLossBlocks * (3 + 3 * (size_t)C);
}

// ---- the launchers: one per kernel family (hard / soft targets) and direction, the runtime variant chosen inside -----------------------------
template <int CC>
static void stats_launch(int blocks, hipStream_t st, const float* logits, int pitch, const void* target, int target_bytes, bool ign, long long N,
                         long long ignore, const float* cw, const float* pw, float* workspace, unsigned long long* n_bad) {
#define STATS_K(TT, IGN, PW)                                                                                                                            \
    hipLaunchKernelGGL((multiloss_stats_kernel<CC, TT, IGN, PW>), dim3(blocks), dim3(256), 0, st, logits, pitch, static_cast<const TT*>(target), N, cw, \
                       workspace, ignore, n_bad, pw)
    if (!ign) STATS_K(long long, false, false);
    else if (pw != nullptr && target_bytes == 8) STATS_K(long long, true, true);
    else if (pw != nullptr) STATS_K(unsigned char, true, true);
    else if (target_bytes == 8) STATS_K(long long, true, false);
    else STATS_K(unsigned char, true, false);
#undef STATS_K
}

template <int CC>
static void stats_soft_launch(int blocks, hipStream_t st, const float* logits, int pitch, const SoftSrc& src, int kind, int target_bytes, long long N,
                              const float* cw, const float* pw, float* workspace, unsigned long long* n_bad) {
#define STATS_K(SRC, TT) \
    hipLaunchKernelGGL((multiloss_stats_soft_kernel<CC, SRC, TT>), dim3(blocks), dim3(256), 0, st, logits, pitch, src, N, cw, pw, workspace, n_bad)
    if (kind == kSoftProbs) STATS_K(kSoftProbs, float);
    else if (kind == kSoftLogits) STATS_K(kSoftLogits, float);
    else if (target_bytes == 8) STATS_K(kSoftSmooth, long long);
    else STATS_K(kSoftSmooth, unsigned char);
#undef STATS_K
}

// what the two backward families share: the cleared range word, the grid and how a row of dlogits is stored
struct BwdGeom {
    int blocks, Cstore, zero16;
};

static int bwd_geom(long long N, int C, const float* dlogits, int dpitch, unsigned int* amax_bits, hipStream_t st, BwdGeom& g) {
    if (amax_bits != nullptr) PYLC_HIP(hipMemsetAsync(amax_bits, 0, sizeof(unsigned), st));
    g.blocks = (int)(cdiv<long long>(N, 256) < 4096 ? cdiv<long long>(N, 256) : 4096);
    g.Cstore = ((C + 3) & ~3) <= dpitch ? ((C + 3) & ~3) : C;
    g.zero16 = dpitch % 4 == 0 && (reinterpret_cast<uintptr_t>(dlogits) & 15) == 0;      // then Cstore = roundup4(C) <= dpitch
    return PYLC_OK;
}

template <int CC>
static void bwd_launch(const BwdGeom& g, hipStream_t st, const float* logits, int pitch, const void* target, int target_bytes, bool ign, long long N,
                       long long ignore, const float* cw, const float* pw, const float* stats, float inv_n, float w_ce, float w_dice, float w_focal,
                       const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits) {
#define BWD_K(TT, IGN, PW)                                                                                                                             \
    hipLaunchKernelGGL((multiloss_bwd_kernel<CC, TT, IGN, PW>), dim3(g.blocks), dim3(256), 0, st, logits, pitch, static_cast<const TT*>(target), N, cw, \
                       stats, inv_n, w_ce, w_dice, w_focal, grad_scale, dlogits, dpitch, g.Cstore, amax_bits, ignore, g.zero16, pw)
    if (!ign) BWD_K(long long, false, false);
    else if (pw != nullptr && target_bytes == 8) BWD_K(long long, true, true);
    else if (pw != nullptr) BWD_K(unsigned char, true, true);
    else if (target_bytes == 8) BWD_K(long long, true, false);
    else BWD_K(unsigned char, true, false);
#undef BWD_K
}

template <int CC>
static void bwd_soft_launch(const BwdGeom& g, hipStream_t st, const float* logits, int pitch, const SoftSrc& src, int kind, int target_bytes,
                            long long N, const float* cw, const float* pw, const float* stats, float w_ce, float w_dice, float w_focal,
                            const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits) {
#define BWD_K(SRC, TT)                                                                                                                        \
    hipLaunchKernelGGL((multiloss_bwd_soft_kernel<CC, SRC, TT>), dim3(g.blocks), dim3(256), 0, st, logits, pitch, src, N, cw, pw, stats, w_ce, \
                       w_dice, w_focal, grad_scale, dlogits, dpitch, g.Cstore, amax_bits, g.zero16)
    if (kind == kSoftProbs) BWD_K(kSoftProbs, float);
    else if (kind == kSoftLogits) BWD_K(kSoftLogits, float);
    else if (target_bytes == 8) BWD_K(kSoftSmooth, long long);
    else BWD_K(kSoftSmooth, unsigned char);
#undef BWD_K
}

static int stats_blocks(long long N) { return (int)(cdiv<long long>(N, 256) < kLossBlocks ? cdiv<long long>(N, 256) : kLossBlocks); }

// after the statistics kernel of either family: its launch check, then the per-block rows of the workspace summed into stats
static int stats_finish(const float* workspace, int blocks, int C, float* stats, hipStream_t st) {
    PYLC_LAUNCH_CHECK();
    const int K = 3 + 3 * C;
    hipLaunchKernelGGL(column_sum_kernel, dim3(cdiv(K, 8)), dim3(256), 0, st, workspace, blocks, K, stats);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

static int multiloss_stats_impl(const float* logits, int pitch, const void* target, int target_bytes, bool ign, long long N, int C, long long ignore,
                                const float* cw, const float* pw, float* stats, float* workspace, unsigned long long* n_bad, void* stream) {
    hipStream_t st = as_stream(stream);
    const int blocks = stats_blocks(N);
#define LAUNCH_STATS(CC) stats_launch<CC>(blocks, st, logits, pitch, target, target_bytes, ign, N, ignore, cw, pw, workspace, n_bad)
    PYLC_FOR_CLASSES(C, LAUNCH_STATS, "multiloss")
#undef LAUNCH_STATS
    return stats_finish(workspace, blocks, C, stats, st);
}

static int multiloss_stats_soft_impl(const float* logits, int pitch, const SoftSrc& src, int kind, int target_bytes, long long N, int C,
                                     const float* cw, const float* pw, float* stats, float* workspace, unsigned long long* n_bad, void* stream) {
    hipStream_t st = as_stream(stream);
    const int blocks = stats_blocks(N);
#define LAUNCH_STATS(CC) stats_soft_launch<CC>(blocks, st, logits, pitch, src, kind, target_bytes, N, cw, pw, workspace, n_bad)
    PYLC_FOR_CLASSES(C, LAUNCH_STATS, "multiloss")
#undef LAUNCH_STATS
    return stats_finish(workspace, blocks, C, stats, st);
}

static int multiloss_bwd_impl(const float* logits, int pitch, const void* target, int target_bytes, bool ign, long long N, int C, long long ignore,
                              const float* cw, const float* pw, const float* stats, double n_global, float w_ce, float w_dice, float w_focal,
                              const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits, void* stream) {
    hipStream_t st = as_stream(stream);
    BwdGeom g;
    if (int rc = bwd_geom(N, C, dlogits, dpitch, amax_bits, st, g)) return rc;
    const float inv_n = ign ? 0.f : (float)(1.0 / n_global);
#define LAUNCH_BWD(CC)                                                                                                                          \
    bwd_launch<CC>(g, st, logits, pitch, target, target_bytes, ign, N, ignore, cw, pw, stats, inv_n, w_ce, w_dice, w_focal, grad_scale, dlogits, \
                   dpitch, amax_bits)
    PYLC_FOR_CLASSES(C, LAUNCH_BWD, "multiloss")
#undef LAUNCH_BWD
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

static int multiloss_bwd_soft_impl(const float* logits, int pitch, const SoftSrc& src, int kind, int target_bytes, long long N, int C,
                                   const float* cw, const float* pw, const float* stats, float w_ce, float w_dice, float w_focal,
                                   const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits, void* stream) {
    hipStream_t st = as_stream(stream);
    BwdGeom g;
    if (int rc = bwd_geom(N, C, dlogits, dpitch, amax_bits, st, g)) return rc;
#define LAUNCH_BWD(CC)                                                                                                                           \
    bwd_soft_launch<CC>(g, st, logits, pitch, src, kind, target_bytes, N, cw, pw, stats, w_ce, w_dice, w_focal, grad_scale, dlogits, dpitch, \
                        amax_bits)
    PYLC_FOR_CLASSES(C, LAUNCH_BWD, "multiloss")
#undef LAUNCH_BWD
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

// ---- the argument rules of the _ex, _w, _ls and _soft entry points, in the order each of them states them; `who` names the entry point ------
static bool loss_aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

// a hard target: class count, smoothing (0 where the entry point has none), element size, pointer
static int hard_target_check(const char* who, int C, float smoothing, const void* target, int target_bytes) {
    PYLC_REQUIRE(C >= 2 && C <= MAXC, "%s: n_classes=%d unsupported (2..%d)", who, C, MAXC);
    PYLC_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "%s: smoothing=%g outside [0, 1)", who, (double)smoothing);
    PYLC_REQUIRE(target_bytes == 1 || target_bytes == 8, "%s: target_bytes=%d (1: uint8, 8: int64)", who, target_bytes);
    PYLC_REQUIRE(target, "%s: target is NULL", who);
    return PYLC_OK;
}

// a soft volume: class count, kind, temperature, pointer, extents and strides
static int soft_volume_check(const char* who, int C, int kind, float inv_T, const float* soft, int H, int W, long long N, long long stride_b,
                             long long stride_c, long long stride_h, long long stride_w) {
    PYLC_REQUIRE(C >= 2 && C <= MAXC, "%s: n_classes=%d unsupported (2..%d)", who, C, MAXC);
    PYLC_REQUIRE(kind == kSoftProbs || kind == kSoftLogits, "%s: kind=%d (0: probabilities, 1: teacher logits)", who, kind);
    PYLC_REQUIRE(inv_T > 0.f && inv_T <= FLT_MAX, "%s: inv_T=%g is not a positive finite number", who, (double)inv_T);
    PYLC_REQUIRE(soft, "%s: soft is NULL", who);
    PYLC_REQUIRE(H > 0 && W > 0, "%s: H=%d or W=%d is not positive", who, H, W);
    PYLC_REQUIRE(N > 0 && N % ((long long)H * W) == 0, "%s: N=%lld is not a positive multiple of H*W=%lld", who, N, (long long)H * W);
    PYLC_REQUIRE(stride_b >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, "%s: a stride is negative (%lld, %lld, %lld, %lld)", who,
                 stride_b, stride_c, stride_h, stride_w);
    return PYLC_OK;
}

// the statistics side.  hard: `target` holds labels of target_bytes each, whose rules come first; otherwise it is a float volume
// (target_bytes 4) that soft_volume_check has passed
static int stats_check(const char* who, bool hard, float smoothing, const float* logits, int pitch, const void* target, int target_bytes,
                       long long N, int C, const float* pw, const float* stats, const float* workspace, const unsigned long long* n_bad) {
    if (int rc = hard ? hard_target_check(who, C, smoothing, target, target_bytes) : PYLC_OK) return rc;
    PYLC_REQUIRE(pitch >= C, "%s: pitch=%d below n_classes=%d", who, pitch, C);
    PYLC_REQUIRE(N > 0, "%s: N=%lld is not positive", who, N);
    PYLC_REQUIRE(logits && stats && workspace, "%s: logits, stats or workspace is NULL", who);
    PYLC_REQUIRE(loss_aligned(target, target_bytes) && loss_aligned(n_bad, 8) && loss_aligned(pw, 4), "%s: a buffer is not aligned to its element",
                 who);
    return PYLC_OK;
}

// the backward side, likewise; all of it comes before amax_bits is cleared
static int bwd_check(const char* who, bool hard, float smoothing, const float* logits, int pitch, const void* target, int target_bytes,
                     long long N, int C, const float* pw, const float* stats, const float* dlogits, int dpitch) {
    if (int rc = hard ? hard_target_check(who, C, smoothing, target, target_bytes) : PYLC_OK) return rc;
    PYLC_REQUIRE(pitch >= C && dpitch >= C, "%s: pitch=%d or dpitch=%d below n_classes=%d", who, pitch, dpitch, C);
    PYLC_REQUIRE(N > 0, "%s: N=%lld is not positive", who, N);
    PYLC_REQUIRE(logits && stats && dlogits, "%s: logits, stats or dlogits is NULL", who);
    if (!hard) PYLC_REQUIRE(loss_aligned(target, 4) && loss_aligned(pw, 4), "%s: a buffer is not aligned to its element", who);
    PYLC_REQUIRE(loss_aligned(target, target_bytes), "%s: an int64 target is not 8-byte aligned", who);
    PYLC_REQUIRE(loss_aligned(pw, 4), "%s: pixel_weights is not 4-byte aligned", who);
    return PYLC_OK;
}

static SoftSrc soft_volume(const float* soft, long long sb, long long sc, long long sh, long long sw, long long N, int H, int W, float inv_T) {
    SoftSrc s{};
    s.ptr = soft, s.sb = sb, s.sc = sc, s.sh = sh, s.sw = sw, s.HW = (long long)H * W, s.W = W, s.small = N < (1ll << 32), s.par = inv_T;
    return s;
}

static SoftSrc soft_smooth(const void* target, float smoothing, long long ignore) {
    SoftSrc s{};
    s.ptr = target, s.par = smoothing, s.ignore = ignore, s.HW = 1, s.W = 1;
    return s;
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
extern "C" int pylc_multiloss_stats(const float* logits, int pitch, const int64_t* target, long long N, int C, const float* cw, float* stats,
                                    float* workspace, void* stream) {
    PYLC_REQUIRE(C >= 2 && C <= MAXC, "multiloss_stats: n_classes=%d unsupported (2..%d)", C, MAXC);
    PYLC_REQUIRE(logits && target && stats && workspace && N > 0 && pitch >= C, "multiloss_stats: bad arguments");
    return multiloss_stats_impl(logits, pitch, target, 8, false, N, C, 0, cw, nullptr, stats, workspace, nullptr, stream);
}

extern "C" int pylc_multiloss_stats_ex(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                                       const float* cw, float* stats, float* workspace, unsigned long long* n_bad, void* stream) {
    if (int rc = stats_check("multiloss_stats_ex", true, 0.f, logits, pitch, target, target_bytes, N, C, nullptr, stats, workspace, n_bad)) return rc;
    return multiloss_stats_impl(logits, pitch, target, target_bytes, true, N, C, (long long)ignore_index, cw, nullptr, stats, workspace, n_bad, stream);
}

// pixel_weights == NULL: the very instantiations of _ex
extern "C" int pylc_multiloss_stats_w(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                                      const float* cw, const float* pixel_weights, float* stats, float* workspace, unsigned long long* n_bad,
                                      void* stream) {
    if (int rc = stats_check("multiloss_stats_w", true, 0.f, logits, pitch, target, target_bytes, N, C, pixel_weights, stats, workspace, n_bad))
        return rc;
    return multiloss_stats_impl(logits, pitch, target, target_bytes, true, N, C, (long long)ignore_index, cw, pixel_weights, stats, workspace, n_bad,
                                stream);
}

extern "C" int pylc_multiloss_finalize(const float* stats, double n_global, int C, float w_ce, float w_dice, float w_focal, float* losses,
                                       void* stream) {
    PYLC_REQUIRE(stats && losses && n_global > 0 && C >= 2 && C <= MAXC, "multiloss_finalize: bad arguments");
    hipLaunchKernelGGL(multiloss_finalize_kernel<false>, dim3(1), dim3(64), 0, as_stream(stream), stats, n_global, C, w_ce, w_dice, w_focal, losses);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_multiloss_finalize_ex(const float* stats, int C, float w_ce, float w_dice, float w_focal, float* losses, void* stream) {
    PYLC_REQUIRE(C >= 2 && C <= MAXC, "multiloss_finalize_ex: n_classes=%d unsupported (2..%d)", C, MAXC);
    PYLC_REQUIRE(stats && losses, "multiloss_finalize_ex: stats or losses is NULL");
    hipLaunchKernelGGL(multiloss_finalize_kernel<true>, dim3(1), dim3(64), 0, as_stream(stream), stats, 0.0, C, w_ce, w_dice, w_focal, losses);
    PYLC_LAUNCH_CHECK();
    return PYLC_OK;
}

extern "C" int pylc_multiloss_bwd(const float* logits, int pitch, const int64_t* target, long long N, int C, const float* cw,
                                  const float* stats, double n_global, float w_ce, float w_dice, float w_focal, const float* grad_scale,
                                  float* dlogits, int dpitch, unsigned int* amax_bits, void* stream) {
    PYLC_REQUIRE(C >= 2 && C <= MAXC, "multiloss_bwd: n_classes=%d unsupported (2..%d)", C, MAXC);      // before amax_bits is cleared
    PYLC_REQUIRE(logits && target && stats && dlogits && N > 0 && pitch >= C && dpitch >= C && n_global > 0, "multiloss_bwd: bad arguments");
    return multiloss_bwd_impl(logits, pitch, target, 8, false, N, C, 0, cw, nullptr, stats, n_global, w_ce, w_dice, w_focal, grad_scale, dlogits, dpitch,
                              amax_bits, stream);
}

extern "C" int pylc_multiloss_bwd_ex(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                                     const float* cw, const float* stats, float w_ce, float w_dice, float w_focal, const float* grad_scale,
                                     float* dlogits, int dpitch, unsigned int* amax_bits, void* stream) {
    if (int rc = bwd_check("multiloss_bwd_ex", true, 0.f, logits, pitch, target, target_bytes, N, C, nullptr, stats, dlogits, dpitch)) return rc;
    return multiloss_bwd_impl(logits, pitch, target, target_bytes, true, N, C, (long long)ignore_index, cw, nullptr, stats, 1.0, w_ce, w_dice, w_focal,
                              grad_scale, dlogits, dpitch, amax_bits, stream);
}

extern "C" int pylc_multiloss_bwd_w(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                                    const float* cw, const float* pixel_weights, const float* stats, float w_ce, float w_dice, float w_focal,
                                    const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits, void* stream) {
    if (int rc = bwd_check("multiloss_bwd_w", true, 0.f, logits, pitch, target, target_bytes, N, C, pixel_weights, stats, dlogits, dpitch)) return rc;
    return multiloss_bwd_impl(logits, pitch, target, target_bytes, true, N, C, (long long)ignore_index, cw, pixel_weights, stats, 1.0, w_ce, w_dice,
                              w_focal, grad_scale, dlogits, dpitch, amax_bits, stream);
}

extern "C" int pylc_multiloss_stats_soft(const float* logits, int pitch, long long N, int H, int W, int C, const float* soft, long long stride_b,
                                         long long stride_c, long long stride_h, long long stride_w, int kind, float inv_T, const float* cw,
                                         const float* pixel_weights, float* stats, float* workspace, unsigned long long* n_bad, void* stream) {
    const char* who = "multiloss_stats_soft";
    if (int rc = soft_volume_check(who, C, kind, inv_T, soft, H, W, N, stride_b, stride_c, stride_h, stride_w)) return rc;
    if (int rc = stats_check(who, false, 0.f, logits, pitch, soft, 4, N, C, pixel_weights, stats, workspace, n_bad)) return rc;
    return multiloss_stats_soft_impl(logits, pitch, soft_volume(soft, stride_b, stride_c, stride_h, stride_w, N, H, W, inv_T), kind, 4, N, C, cw,
                                     pixel_weights, stats, workspace, n_bad, stream);
}

extern "C" int pylc_multiloss_bwd_soft(const float* logits, int pitch, long long N, int H, int W, int C, const float* soft, long long stride_b,
                                       long long stride_c, long long stride_h, long long stride_w, int kind, float inv_T, const float* cw,
                                       const float* pixel_weights, const float* stats, float w_ce, float w_dice, float w_focal,
                                       const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits, void* stream) {
    const char* who = "multiloss_bwd_soft";
    if (int rc = soft_volume_check(who, C, kind, inv_T, soft, H, W, N, stride_b, stride_c, stride_h, stride_w)) return rc;
    if (int rc = bwd_check(who, false, 0.f, logits, pitch, soft, 4, N, C, pixel_weights, stats, dlogits, dpitch)) return rc;
    return multiloss_bwd_soft_impl(logits, pitch, soft_volume(soft, stride_b, stride_c, stride_h, stride_w, N, H, W, inv_T), kind, 4, N, C, cw,
                                   pixel_weights, stats, w_ce, w_dice, w_focal, grad_scale, dlogits, dpitch, amax_bits, stream);
}

extern "C" int pylc_multiloss_stats_ls(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                                       const float* cw, const float* pixel_weights, float smoothing, float* stats, float* workspace,
                                       unsigned long long* n_bad, void* stream) {
    if (int rc = stats_check("multiloss_stats_ls", true, smoothing, logits, pitch, target, target_bytes, N, C, pixel_weights, stats, workspace, n_bad))
        return rc;
    return multiloss_stats_soft_impl(logits, pitch, soft_smooth(target, smoothing, (long long)ignore_index), kSoftSmooth, target_bytes, N, C, cw,
                                     pixel_weights, stats, workspace, n_bad, stream);
}

extern "C" int pylc_multiloss_bwd_ls(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                                     const float* cw, const float* pixel_weights, float smoothing, const float* stats, float w_ce, float w_dice,
                                     float w_focal, const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits, void* stream) {
    if (int rc = bwd_check("multiloss_bwd_ls", true, smoothing, logits, pitch, target, target_bytes, N, C, pixel_weights, stats, dlogits, dpitch))
        return rc;
    return multiloss_bwd_soft_impl(logits, pitch, soft_smooth(target, smoothing, (long long)ignore_index), kSoftSmooth, target_bytes, N, C, cw,
                                   pixel_weights, stats, w_ce, w_dice, w_focal, grad_scale, dlogits, dpitch, amax_bits, stream);
}
