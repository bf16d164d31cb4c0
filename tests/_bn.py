"""Training-mode and synchronised BatchNorm stated in float64 torch, from the formulas of include/pylc_hip.h and DESIGN.md section 5 (not
from the kernels), with the first-order worst-case rounding bounds that tests/test_bn_abi_gpu.py uses as tolerances and the inputs both
that file and tests/test_cpu_bn_ref.py run on.  Every tensor is [M rows][C channels].  Not a test module.

The bounds.  u = 2^-24 is the unit round-off of fp32; every bound is a sum of (number of fp32 roundings on the path) x u x (magnitude of the
rounded quantity), to first order in u.  What the library documents about its arithmetic, and what the bounds rely on:
  * a per-channel sum is taken per row slab: products rounded to fp32, kRowBatch = 4 rows summed in fp32, batch sums folded in fp64, ONE
    rounding to the fp32 per-slab partial; the partials are combined in fp64 and rounded ONCE to the fp32 sum;
  * the coefficient math (mean, variance, invstd) runs in fp64 on those fp32 sums and rounds each result once;
  * the elementwise passes evaluate their documented expression in fp32, one rounding per operation.
"""
import collections

import numpy as np
import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
REFINE_RATIO = 64.0          # include/pylc_hip.h: "a channel whose mean^2 exceeds 64 var ... is re-measured in a second pass"
REFINE_FLOOR = 1e-5


# ---- the operation -------------------------------------------------------------------------------------------------------------------------
def stats64(y):
    """Per-channel (sum y, sum y^2, sum |y|, n) of y[M][C] in fp64."""
    y = y.double()
    return y.sum(0), (y * y).sum(0), y.abs().sum(0), float(y.shape[0])


Coeffs = collections.namedtuple('Coeffs', 'mean var invstd scale shift unbiased')


def eps64(eps):
    """The eps the kernels see: a float argument widened to double."""
    return float(np.float32(eps))


def coeffs64(S1, S2, n, gamma, beta, eps, clamp, K=None):
    """From the moments of (y - K) over n values: mean = K + S1/n, biased variance, invstd = (var + eps)^-1/2 or (clamp) max(var, eps)^-1/2,
    scale = gamma invstd, shift = beta - mean scale, and the unbiased variance of the running update (var n/(n-1) for n > 1, else var)."""
    S1, S2, gamma, beta = S1.double(), S2.double(), gamma.double(), beta.double()
    mk = S1 / n
    var = (S2 / n - mk * mk).clamp(min=0.0)
    mean = mk if K is None else K.double() + mk
    e = eps64(eps)
    invstd = var.clamp(min=e).rsqrt() if clamp else (var + e).rsqrt()
    scale = gamma * invstd
    return Coeffs(mean, var, invstd, scale, beta - mean * scale, var * n / (n - 1.0) if n > 1 else var)


def running64(old, new, momentum):
    return (1.0 - momentum) * old.double() + momentum * new.double()


def backward64(dout, mask, y, mean, invstd, gamma, n_global, sums=None):
    """g = dout * mask (mask None: no ReLU), xhat = (y - mean) invstd at the GIVEN mean / invstd, (sum g xhat, sum g) over these rows, and
    dy = gamma invstd (g - sum_g / n - xhat sum_gx / n) with `sums` = (sum g xhat, sum g) when given (all-reduced, or what a kernel stage
    was handed), else the local ones.  Returns (g, sgx, sg, dy, xhat)."""
    g = dout.double() if mask is None else dout.double() * mask.double()
    xh = (y.double() - mean.double()) * invstd.double()
    sgx, sg = (g * xh).sum(0), g.sum(0)
    ux, us = (sgx, sg) if sums is None else (sums[0].double(), sums[1].double())
    dy = gamma.double() * invstd.double() * (g - us / n_global - xh * ux / n_global)
    return g, sgx, sg, dy, xh


def unpack_relu_bits(mask_bytes, m, c):
    """The 1-bit ReLU mask of PylcBnExtra.relu_mask as bool [m, c]: with cv = c / 4 the channel quad, byte (row * C/4 + cv) / 2 holds the
    nibbles of two adjacent quads -- the even quad in the low nibble, the odd one in the high nibble -- and bit k of a nibble is channel
    4 cv + k."""
    assert c % 8 == 0 and mask_bytes.numel() == m * c // 8
    b = mask_bytes.reshape(m, c // 8).to(torch.int32)
    nib = torch.stack((b & 15, b >> 4), dim=2).reshape(m, c // 4)                  # one nibble per (row, quad)
    bits = torch.stack([(nib >> k) & 1 for k in range(4)], dim=2).reshape(m, c)
    return bits.bool()


def _sqrt_nm1(n):
    return max(n - 1.0, 1.0) ** 0.5          # the bound formulas take sqrt(n - 1); one value (n = 1) has the factor 1


def samuelson_bound64(gamma, beta, n, extra, mul):
    """bound_out of the finalize kernels: (max_c (|gamma_c| sqrt(n - 1) + |beta_c|) + extra) mul -- |xhat| <= sqrt(n - 1) (Samuelson)."""
    return float(((gamma.double().abs() * _sqrt_nm1(n) + beta.double().abs()).max() + extra) * mul)


def dy_bound64(gamma, invstd, g_amax, sums, n):
    """dy_bound_out / pylc_bn_bwd_bound: max_c |gamma invstd| (max|g| + |sum g| / n + sqrt(n - 1) |sum g xhat| / n); sums = (sgx, sg)."""
    k = (gamma.double() * invstd.double()).abs()
    return float((k * (g_amax + sums[1].double().abs() / n + _sqrt_nm1(n) * sums[0].double().abs() / n)).max())


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------------
def d_sums(S2, SA):
    """(dS1, dS2).  sum y^2: the product (1 rounding), the 4-row fp32 batch sum (3 additions), the slab partial (1), the column sum (1):
    6u sum y^2.  sum y: the same path without the product: 5u sum |y|."""
    return 5 * U * SA, 6 * U * S2


def needs_refine(S1, S2, n):
    """The header's predicate on the moments of (y - K); returns (refined, borderline): within 1e-3 of the threshold the fp32 sums of the
    kernel may decide either way, and a test must not depend on such a channel."""
    mk = S1 / n
    var = (S2 / n - mk * mk).clamp(min=0.0)
    r = mk * mk / (REFINE_RATIO * (var + REFINE_FLOOR))
    return r > 1.0, (r - 1.0).abs() < 2.5e-4


def d_var(S1, S2, SA, n, refined=None):
    """dvar of var = S2/n - (S1/n)^2:  dS2/n + 2 |S1/n| dS1/n.  A refined channel is re-measured as sum (y - m)^2 with fp32 differences
    (one rounding each, exact where Sterbenz applies) and fp64 sums: 4u var + u |mean| sqrt(var).  Both carry the cancellation of the fp64
    subtraction itself, 4 x 2^-53 S2/n (seen only where var < 1e-9 mean^2: one row per rank, a constant channel)."""
    mk = S1 / n
    var = (S2 / n - mk * mk).clamp(min=0.0)
    dS1, dS2 = d_sums(S2, SA)
    d = dS2 / n + 2 * mk.abs() * dS1 / n
    if refined is not None:
        d = torch.where(refined, 4 * U * var + U * mk.abs() * var.sqrt(), d)
    return d + 4 * U64 * S2 / n


def d_invstd_rel(dvar, var, eps, clamp):
    """d invstd / invstd = 1/2 dvar / (var + eps) + u (the rounding of the result); clamp: 1/2 dvar / max(var, eps) + u above eps and no
    error of the kernel's below it -- there it stores (float)(1 / sqrt((double)eps)), which the tests compare bit-wise; u is that
    rounding.  Channels with |var - eps| <= dvar may fall on either side: `clamp_ambiguous` names them."""
    e = eps64(eps)
    if not clamp:
        return 0.5 * dvar / (var + e) + U
    return torch.where(var > e, 0.5 * dvar / var.clamp(min=e), torch.zeros_like(var)) + U


def clamp_ambiguous(dvar, var, eps):
    return (var - eps64(eps)).abs() <= dvar


def d_mean(S1, SA, n, mean, refined=None):
    """mean = K + S1/n: dS1/n and the rounding of the result.  A refined channel's S1 = n m + sum (y - m) carries fp32 differences only."""
    d = 5 * U * SA / n
    if refined is not None:
        # fp32 differences from an fp32 m (u |y - m| each where Sterbenz does not apply, |y - m| <= |y| + |m|), summed in fp64
        d = torch.where(refined, 2 * U * SA / n, d)
    return d + U * mean.abs()


def d_scale(scale, rel_invstd):
    """scale = gamma * invstd_f in fp32: the error of invstd and one product."""
    return scale.abs() * (rel_invstd + U)


def d_shift(co, dmean, dscale):
    """shift = beta - mean_f * scale_f: the errors of both factors, the product (u) and the difference (u)."""
    return co.mean.abs() * dscale + co.scale.abs() * dmean + U * (co.mean * co.scale).abs() + U * co.shift.abs()


def d_running(old, new, dnew, momentum):
    """(1 - momentum) * old + momentum * new in fp32.  On the first term: 1 - momentum, the product, the sum (3u); on the second: `new`
    rounded to fp32 (the variance; the mean's rounding is in dnew already), the product, the sum (3u)."""
    a, b = ((1.0 - momentum) * old.double()).abs(), (momentum * new.double()).abs()
    return momentum * dnew + 3 * U * a + 3 * U * b


def apply_bound(y, scale, shift, res=None):
    """|out - ref| <= 3u (|y scale| + |shift| + |res|): the product, the sum with shift, the sum with the residual, each at most u of a
    partial result that the three magnitudes bound.  The reference takes the kernel's own fp32 scale / shift; ReLU is 1-Lipschitz."""
    b = (y.double() * scale.double()).abs() + shift.double().abs()
    return 3 * U * (b if res is None else b + res.double().abs())


def d_bwd_sums(g, xh, extra_adds=0):
    """(d sum g xhat, d sum g).  xhat = (y - mean) invstd: 2 roundings; g xhat: 1; then the summation path of d_sums (3 + 1 + 1): 8
    counted, and the bound is set at 9u sum |g xhat| -- one u over the count for what first order leaves out.  sum g: 5u sum |g|.
    extra_adds: fp32 additions of per-rank sums in rank order (each u of a partial sum)."""
    a, b = (g * xh).abs().sum(0), g.abs().sum(0)
    return (9 + extra_adds) * U * a, (5 + extra_adds) * U * b


def dy_elem_bound(gamma, invstd, g, sgx, sg, xh, n):
    """|dy - ref| <= 8u |gamma invstd| (|g| + |sum g|/n + |xhat| |sum g xhat|/n):  k = gamma invstd (1), 1/n as a float (1), sum * 1/n (1),
    xhat (2), xhat * sgx (1), two subtractions (2 between them on the partial results), the product with k (1) -- no term carries more than 8."""
    k = (gamma.double() * invstd.double()).abs()
    return 8 * U * k * (g.abs() + sg.double().abs() / n + xh.abs() * sgx.double().abs() / n)


# ---- slab geometry (row slabs of at least 8 rows per row lane, at most 512 slabs) -----------------------------------------------
def slab_rows(m, c, max_slabs=512):
    cv = c // 4
    rl = 256 // min(cv, 256)
    rps = max(-(-m // max_slabs), rl * 8)
    return -(-rps // rl) * rl


def emulate_sums32(y):
    """The documented accumulation in numpy: per-slab partials of y and of the fp32 products y*y, summed in fp64 and rounded to fp32;
    the partials combined in fp64 and rounded to fp32.  Returns (S1, S2) as float64 arrays holding fp32 values."""
    a = y.detach().cpu().numpy().astype(np.float32)
    m, c = a.shape
    rps = slab_rows(m, c)
    p1 = [a[r:r + rps].astype(np.float64).sum(0).astype(np.float32) for r in range(0, m, rps)]
    p2 = [(a[r:r + rps] * a[r:r + rps]).astype(np.float64).sum(0).astype(np.float32) for r in range(0, m, rps)]
    s1 = np.sum(np.stack(p1).astype(np.float64), 0).astype(np.float32).astype(np.float64)
    s2 = np.sum(np.stack(p2).astype(np.float64), 0).astype(np.float32).astype(np.float64)
    return torch.from_numpy(s1), torch.from_numpy(s2)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
# (M, C, extra pitch): the smallest shapes that reach each branch of the slab walk
SHAPES = [(1000, 64, 0),       # ragged last slab, 16 row lanes
          (363, 48, 4),        # all pitches != C
          (75, 20, 0),         # odd vector count: 5 columns, 51 row lanes, one idle thread
          (72, 728, 0),        # 182 columns, one row lane
          (40, 1536, 0),       # PARTIAL second column pass (Xception exit flow)
          (32, 2048, 4),       # two full column passes
          (5, 256, 0),         # fewer rows than one row batch
          (2, 8, 0),           # smallest legal training input
          (40000, 8, 0)]       # 128 row lanes, 40 slabs

Inputs = collections.namedtuple('Inputs', 'y gamma beta dout res rm rv')


def make_inputs(m, c, seed=4):
    """y = 2 N(0,1) + offset_c with the offsets spread over [-15, 15] (mean^2 / var from 0 to ~56, below the refinement threshold of 64
    for all but the shortest columns); gamma = 1 + 0.1 N; beta = 0.1 N; dout = N(0,1) with per-channel scales spread over 2^-6 .. 2^6 (a
    max-norm tolerance would hide the small channels); residual N(0,1); running statistics 0.1 N and 1 + 0.1 |N|.  fp32, on the CPU."""
    g = torch.Generator().manual_seed(9000 + 13 * m + c + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    y = 2.0 * r(m, c) + torch.linspace(-15.0, 15.0, c)
    dout = r(m, c) * torch.exp2(torch.linspace(-6.0, 6.0, c))
    return Inputs(y, 1 + 0.1 * r(c), 0.1 * r(c), dout, r(m, c), 0.1 * r(c), 1 + 0.1 * r(c).abs())


def _grid(t):
    return torch.round(t * 4096.0) / 4096.0


SyncInputs = collections.namedtuple('SyncInputs', 'y t K gamma beta dout shards')


def make_sync16(shards, seed=0):
    """The 16-channel SyncBN case; shards = rows per rank.  Channels: 0-7 well-conditioned; 8 mean = 1000 sigma on every rank; 9 rank means
    alternate +-50 sigma; 10 mean 20 sigma on rank 0 only; 11 the constant 0.25; 12 sigma^2 ~ 1e-6; 13 sigma^2 ~ 1.6e-5; 14-15 y = t + K
    with K = 5 + |N| and t ~ 0.5 N, both on a 2^-12 grid and |y| < 8, so that y is exact in fp32 and `t` (y - K, what the sums are taken
    over with stat_shift) and y describe the same numbers.  Returns y, t (= y with channels 14-15 replaced by t), K (0 elsewhere), ..."""
    m = sum(shards)
    g = torch.Generator().manual_seed(7000 + 31 * m + len(shards) + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    y = r(m, 16)
    y[:, :8] = 2.0 * y[:, :8] + torch.linspace(-3.0, 3.0, 8)
    rank = torch.cat([torch.full((s,), float(k)) for k, s in enumerate(shards)])
    y[:, 8] += 1000.0
    y[:, 9] += 50.0 * (1.0 - 2.0 * (rank % 2))
    y[:, 10] += 20.0 * (rank == 0).float()
    y[:, 11] = 0.25
    y[:, 12] *= 1e-3
    y[:, 13] *= 4e-3
    K = torch.zeros(16)
    K[14:] = _grid((5.0 + r(2).abs()).clamp(max=6.5))
    t = y.clone()
    t[:, 14:] = _grid((0.5 * r(m, 2)).clamp(-1.25, 1.25))
    y[:, 14:] = t[:, 14:] + K[14:]
    dout = r(m, 16) * torch.exp2(torch.linspace(-6.0, 6.0, 16))
    return SyncInputs(y, t, K, 1 + 0.1 * r(16), 0.1 * r(16), dout, tuple(shards))
