"""The yardstick of hard-pixel mining, numpy only: the loss map in fp64 and in float32, a derived bound on the
distance of a float32 evaluation from the fp64 one, and the selection written out on a float32 map with np.sort.  The CPU suite
(tests/test_cpu_mining.py) proves these against independent statements; the GPU suite (tests/test_mining_gpu.py) compares the kernels
with them -- the maps within the bound, the selection bit for bit."""
import math

import numpy as np

U = 2.0 ** -24                  # unit roundoff of float32 (round to nearest): one operation's relative error, half an ulp
INF_BITS = 0x7F800000
FLT_MAX = float(np.finfo(np.float32).max)

# The maximum errors of the device's single-precision functions, in ulp, as ROCm's HIP math API reference tabulates them.
EXPF_ULP = 1.0
LOGF_ULP = 2.0


def _chain(z, t, dtype):
    """lse - z_t with the operation order of the loss head: zmax, sum exp(z - zmax) in ascending c, zmax + log(sum).  z [N, C], t [N] class
    indices (any integer type; an index outside 0..C-1 takes class 0: its pixel is never a candidate).  Returns (nll, lse)."""
    z = np.asarray(z, dtype=dtype)
    n, c = z.shape
    t = np.asarray(t).astype(np.int64)
    t = np.where((t >= 0) & (t < c), t, 0)
    with np.errstate(all='ignore'):
        zmax = z[:, 0].copy()
        for k in range(1, c):
            zmax = np.fmax(zmax, z[:, k])                    # fmaxf: a NaN entry is passed over here and poisons the sum below
        s = np.zeros(n, dtype=dtype)
        for k in range(c):
            s = (s + np.exp((z[:, k] - zmax).astype(dtype)).astype(dtype)).astype(dtype)
        lse = (zmax + np.log(s).astype(dtype)).astype(dtype)
        nll = (lse - z[np.arange(n), t]).astype(dtype)
    nll = np.where(nll == 0, dtype(0), nll)                  # -0 counts as +0
    return nll, lse


def nll_ref(z, t):
    """The loss map in fp64 (of the float32 logits as they are)."""
    return _chain(z, t, np.float64)[0]


def nll_f32(z, t):
    """The same chain in float32 numpy."""
    return _chain(z, t, np.float32)[0]


def nll_bound(z, t):
    """A per-pixel bound on |float32 evaluation - fp64 evaluation| of the chain, from its operation count, to first order in u = 2^-24 (the
    second-order terms are covered by the factor 1 + 2^-10, the fp64 side's own error by the last term).  An error of E ulp is at most
    2 E u relative.  With d_c = z_c - zmax <= 0, S = sum_c exp(d_c) in [1, C]:
      one subtraction per class     d_c carries a relative error u, which exp turns into the relative error |d_c| u of exp(d_c)
      one expf per class            relative error 2 EXPF_ULP u
      the sum of C terms            C - 1 additions, each u relative to a partial sum that is at most S
        => S carries the relative error  rho <= [2 EXPF_ULP + (C - 1)] u + u sum_c |d_c| exp(d_c) / S
           and |d| exp(d) <= 1 / e, the maximum's own term has d = 0 and S >= 1:  sum_c |d_c| exp(d_c) / S <= (C - 1) / e
      one logf                      log(S (1 + rho)) = log S + rho to first order; the function's own error 2 LOGF_ULP u |log S|, log S <= log C
      two additions                 lse = zmax + log S: u |lse|;  nll = lse - z_t: u |nll|
    Sum:  u [2 EXPF_ULP + (C - 1)(1 + 1 / e) + 2 LOGF_ULP log C + |lse| + |nll|].
    Rows whose fp64 value is not finite get the bound 0: they are compared exactly (+inf) or as NaN."""
    z = np.asarray(z)
    c = z.shape[1]
    nll, lse = _chain(z, t, np.float64)
    with np.errstate(all='ignore'):
        b = U * (2.0 * EXPF_ULP + (c - 1) * (1.0 + 1.0 / math.e) + 2.0 * LOGF_ULP * math.log(c) + np.abs(lse) + np.abs(nll))
        b = b * (1.0 + 2.0 ** -10) + 2.0 ** -50 * (1.0 + np.abs(lse) + np.abs(nll))
    return np.where(np.isfinite(nll), b, 0.0)


# ---- the inputs both suites use ------------------------------------------------------------------------------------------------------------------
# Sizes come from the kernels' geometry (csrc/mining.hip): a lane takes 4 pixels, a block 1024; the nll kernel runs at most 256 blocks
# (a round of its grid is 262144 pixels), the passes over the stored map at most 1024 (1048576).
BLOCK = 1024
NLL_ROUND = 256 * BLOCK
MAP_ROUND = 1024 * BLOCK
SMALL_SIZES = [1, 3, 63, 65, 255, 257, BLOCK - 1, BLOCK + 1]
NLL_SIZES = SMALL_SIZES + [NLL_ROUND + 5, 2 * NLL_ROUND + 1027]
MAP_SIZES = SMALL_SIZES + [MAP_ROUND + 5, 2 * MAP_ROUND + 1027]
CLASSES = (2, 9, 16)


def logits_and_targets(c, n, seed=0):
    """(z float32 [n, c], t int64 [n] in 0..c-1) with planted rows among normal ones: saturated rows whose nll is exactly 0, rows spread over
    +-30, rows with a NaN, a +inf, a -inf at the target (nll = +inf, a candidate) and all -inf."""
    rs = np.random.RandomState(7000 + 31 * c + seed + n % 9973)
    z = (rs.standard_normal((n, c)) * 3.0).astype(np.float32)
    t = rs.randint(0, c, n).astype(np.int64)
    idx = np.arange(n)
    sat = idx % 7 == 2                                       # the target's logit far above the rest: sum = 1, log = 0, lse = zmax
    z[sat] = -200.0
    z[sat, t[sat]] = 200.0
    spread = idx % 7 == 4
    z[spread] = rs.uniform(-30.0, 30.0, (int(spread.sum()), c)).astype(np.float32)
    for r, kind in ((11, 'nan'), (23, 'pinf'), (37, 'ninf_t'), (41, 'ninf_all'), (12, 'nan_t')):
        rows = idx[(idx % 53 == r % 53) & ~sat]
        if kind == 'nan':
            z[rows, (rows + 1) % c] = np.nan
        elif kind == 'nan_t':
            z[rows, t[rows]] = np.nan
        elif kind == 'pinf':
            z[rows, rows % c] = np.inf
        elif kind == 'ninf_t':
            z[rows, t[rows]] = -np.inf
        else:
            z[rows] = -np.inf
    return z, t


def targets_with(t, c, ignore, as_uint8, seed=0):
    """The targets with runs of the ignore label 255 (ignore=True) and a few labels outside 0..c-1 planted, as uint8 or int64."""
    rs = np.random.RandomState(8100 + seed + t.size % 9973)
    t = t.copy()
    n = t.size
    if ignore:
        runs = (np.arange(n) // 5) % 4 == 1
        t[runs & (rs.rand(n) < 0.9)] = 255
    bad = np.arange(n) % 61 == 17
    t[bad] = 200 if as_uint8 else np.where(np.arange(n)[bad] % 2 == 0, -3, 77)
    return t.astype(np.uint8) if as_uint8 else t


def weights_for(n, seed=0):
    """float32 weights in [0.5, 2) with zeros, NaN, negative and infinite entries planted"""
    rs = np.random.RandomState(8200 + seed + n % 9973)
    u = rs.uniform(0.5, 2.0, n).astype(np.float32)
    i = np.arange(n)
    u[i % 13 == 3] = 0.0
    u[i % 97 == 5] = np.nan
    u[i % 89 == 7] = -1.0
    u[i % 101 == 9] = np.inf
    u[i % 103 == 10] = -0.0
    return u


def weight_class(u):
    """0: takes part (0 < u <= FLT_MAX); 1: u == 0; 2: negative, NaN, infinite -- the rules of the weighted loss head"""
    u = np.asarray(u, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        ok = (u > 0) & (u <= np.float32(FLT_MAX))
    return np.where(u == 0, 1, np.where(ok, 0, 2))


def expected_map(nll, t, c, ignore_index=None, weights=None):
    """What pylc_pixel_nll writes given the chain's values: nll where the pixel takes part, -1 at ignored pixels and pixels of weight 0, -2 at
    bad ones; the target is judged first.  Returns (map, takes_part)."""
    t = np.asarray(t).astype(np.int64)
    ignored = np.zeros(t.shape, bool) if ignore_index is None else t == int(ignore_index)
    inside = (t >= 0) & (t < c)
    w = np.zeros(t.shape, np.int64) if weights is None else weight_class(weights)
    part = ~ignored & inside & (w == 0)
    sentinel = np.where(ignored, -1.0, np.where(~inside, -2.0, np.where(w == 1, -1.0, -2.0)))
    return np.where(part, nll, sentinel), part


def compute_k(n_valid, keep, min_kept):
    """k = min(n_valid, max(min_kept, ceil(keep * n_valid))) in Python floats (an IEEE double product, as on the device)"""
    return min(int(n_valid), max(int(min_kept), int(math.ceil(float(keep) * int(n_valid)))))


def bits_of(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def select_ref(nll, keep, min_kept, cap, weights=None):
    """The selection on a float32 map (any shape).  keep in [0, 1], min_kept >= 0, cap a float32 >= 0 (+inf: none), weights float32 of the
    map's shape or None.  A value >= 0 (-0 included, as +0) under a weight that takes part is a candidate; tau_k is the k-th largest
    candidate value -- read from np.sort of the candidates' uint32 bits --, +inf for k == 0; tau = min(tau_k, cap), and +inf when there is
    no candidate.  Output: the weight (1 without weights) at candidates with value >= tau, 0 at the other candidates, at -1 and where a
    value >= 0 sits under a weight of 0; the weight passed through unchanged everywhere else (-2, NaN, another negative, a bad weight).
    Returns (out float32 of the map's shape, info int64 [4] = n_valid, k, kept, bits of tau)."""
    v = np.ascontiguousarray(nll, dtype=np.float32)
    shape = v.shape
    v = v.reshape(-1)
    u = np.ones(v.size, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    w = weight_class(u)
    with np.errstate(invalid='ignore'):
        is_value = v >= 0
    cand = is_value & (w == 0)
    key = v.view(np.uint32) & np.uint32(0x7FFFFFFF)
    n_valid = int(cand.sum())
    k = compute_k(n_valid, keep, min_kept)
    tau_k = INF_BITS if k == 0 else int(np.sort(key[cand])[n_valid - k])
    cap_bits = bits_of(np.float32(cap) + np.float32(0))
    tau = INF_BITS if n_valid == 0 else min(tau_k, cap_bits)
    kept = cand & (key >= np.uint32(tau))
    out = u.copy()                                            # everything else: passed through
    out[is_value & (w != 2)] = 0
    out[kept] = u[kept]
    out[v == np.float32(-1)] = 0
    return out.reshape(shape), np.array([n_valid, k, int(kept.sum()), tau], dtype=np.int64)
