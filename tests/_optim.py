"""Global-norm clipping, AdamW and SGD with momentum stated in float64 numpy, from the formulas of include/pylc_hip.h and the comments of
pylc_amd/csrc/optim.hip, with the same updates in float32 numpy in the kernels' operation order, the first-order worst-case rounding bounds
that tests/test_optim_abi_gpu.py uses as tolerances, and the inputs both that file and tests/test_cpu_optim_ref.py run on (DESIGN.md
section 5.18).  Not a test module.

The statement.  The hyper-parameters are taken AS THE float32 VALUES THE ABI RECEIVES (0.9 is 0.89999998...), and the bias corrections as
the host computes them: bc1 = (float)(1 - pow((double)beta1, step)), bc2_sqrt = (float)sqrt(1 - pow((double)beta2, step)).  The comparison
then measures the kernel's rounding and not the rounding of 0.9.
    c  = coef (1 when NULL)                      gg = g c
    p' = p (1 - lr wd)                           m' = b1 m + (1 - b1) gg          v' = b2 v + (1 - b2) gg^2
    den = sqrt(v') / bc2_sqrt + eps              p'' = p' - (lr / bc1) (m' / den)
    SGD: buf' = gg at step 1 WHATEVER buf held, else mu buf + gg;  p' = p - lr buf'
    clip: norm = sqrt(sum g^2), coef = min(1, max_norm / (norm + 1e-6f))

The bounds.  u = 2^-24, the unit round-off of fp32; every bound is a sum of (number of fp32 roundings on the path) x u x (magnitude of the
rounded quantity), to first order in u.  They rely on what the library's build guarantees: no contraction into fused multiply-adds
(-ffp-contract=off), a correctly rounded fp32 divide and square root (hipcc's default), one rounding per operation.  Under the same
guarantees the float32 model is expected to agree with the kernels bit for bit.
"""
import collections
import math

import numpy as np

U = 2.0 ** -24
f32 = np.float32
EPS_NORM = float(f32(1e-6))           # the kernel adds 1e-6f
NORM_BLOCKS = 1024                    # kNormBlocks: pylc_sqnorm_workspace_floats
STEP_BLOCKS = 4096                    # the block cap of pylc_adamw_step / pylc_sgd_step
ADAM_CHUNK = 8192                     # floats per chunk of pylc_adamw_step_ranges


def _h(x):
    """A hyper-parameter as the ABI receives it: rounded to float32, widened to a Python float."""
    return float(f32(x))


def host_bc(b1, b2, step):
    """(bc1, bc2_sqrt) as float32, computed as pylc_adamw_step does on the host."""
    bc1 = 1.0 - math.pow(_h(b1), float(step))
    bc2 = 1.0 - math.pow(_h(b2), float(step))
    return f32(bc1), f32(math.sqrt(bc2))


# ---- the operation, float64 -------------------------------------------------------------------------------------------------------------------
def clip_ref(g, max_norm):
    """(norm, coef) in fp64."""
    norm = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    return norm, min(1.0, _h(max_norm) / (norm + EPS_NORM))


MUTANTS = ('beta2', 'beta1', 'no_bias_correction', 'eps_inside_sqrt', 'no_decay', 'coupled_decay', 'coef_ignored')


def adamw_ref(p, g, m, v, coef, lr, b1, b2, eps, wd, step, mutant=None):
    """(p, m, v) after one step, fp64.  coef: None or the float32 clip coefficient.  mutant: one of MUTANTS -- a wrong AdamW that the bounds
    must be able to tell from the right one (tests/test_cpu_optim_ref.py)."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = _h(lr), _h(b1), _h(b2), _h(eps), _h(wd)
    bc1, bc2s = (float(x) for x in host_bc(b1, b2, step))
    c = 1.0 if coef is None else float(f32(coef))
    if mutant == 'beta2':
        b2 = _h(0.99) if b2 == _h(0.999) else b2 * 0.99
    if mutant == 'beta1':
        b1 = _h(0.5) if b1 == _h(0.9) else b1 * 0.5 + 0.05
    if mutant == 'no_bias_correction':
        bc1, bc2s = 1.0, 1.0
    if mutant == 'coef_ignored':
        c = 1.0
    gg = g * c
    if mutant == 'coupled_decay':
        gg = gg + wd * p
    p1 = p if mutant in ('no_decay', 'coupled_decay') else p * (1.0 - lr * wd)
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    den = np.sqrt(v1 / (bc2s * bc2s) + eps) if mutant == 'eps_inside_sqrt' else np.sqrt(v1) / bc2s + eps
    return p1 - (lr / bc1) * (m1 / den), m1, v1


def sgd_ref(p, g, buf, coef, lr, mu, step, mutant=None):
    """(p, buf) after one step, fp64; buf = g c at step 1 whatever buf held.  mutant 'no_reset': the buffer is not reset at step 1."""
    p, g, buf = (a.astype(np.float64) for a in (p, g, buf))
    c = 1.0 if coef is None else float(f32(coef))
    gg = g * c
    b = gg if (step == 1 and mutant != 'no_reset') else _h(mu) * buf + gg
    return p - _h(lr) * b, b


# ---- the same updates in float32, one operation per line, in the kernels' order ----------------------------------------------------------------
# adamw_kernel's vector path (four elements per thread) and its scalar tail (n % 4 elements, block 0) evaluate the same expression per
# element, and so does adamw_ranges_kernel: one model covers all of them.  sgd_kernel is scalar throughout.
def adamw_f32(p, g, m, v, coef, lr, b1, b2, eps, wd, step):
    lr, b1, b2, eps, wd, one = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd), f32(1)
    bc1, bc2s = host_bc(b1, b2, step)
    c = one if coef is None else f32(coef)
    step_size = lr / bc1
    gg = g * c
    decay = one - lr * wd
    pp = p * decay
    t1 = b1 * m
    t2 = (one - b1) * gg
    mm = t1 + t2
    t3 = b2 * v
    t4 = (one - b2) * gg
    t4 = t4 * gg
    vv = t3 + t4
    den = np.sqrt(vv)
    den = den / bc2s
    den = den + eps
    q = mm / den
    q = step_size * q
    pp = pp - q
    assert pp.dtype == mm.dtype == vv.dtype == np.float32
    return pp, mm, vv


def sgd_f32(p, g, buf, coef, lr, mu, step):
    c = f32(1) if coef is None else f32(coef)
    gg = g * c
    if step == 1:
        b = gg
    else:
        b = f32(mu) * buf
        b = b + gg
    q = f32(lr) * b
    pp = p - q
    assert pp.dtype == b.dtype == np.float32
    return pp, b


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------------------
def norm_trips(n):
    """L: how many four-element vectors a thread of sqnorm_partial_kernel sums -- the launch is min(ceil((n/4 + 1) / 256), 1024) blocks of
    256 threads striding over n/4 vectors."""
    n4 = n // 4
    blocks = min(-(-(n4 + 1) // 256), NORM_BLOCKS)
    return max(-(-n4 // (blocks * 256)), 0), blocks


def norm_bound(norm, n):
    """|out2[0] - norm|.  Every term of the sum of squares is non-negative, so a relative error per term carries over to the sum.  A term's
    path: its square (1 rounding), the three additions inside a vector (3), L additions into the thread's running sum, one more for the
    tail element that thread may add (1), the 64-wide shuffle tree (6), the four wave sums (3): (14 + L) u.  The combine of the block
    partials runs in fp64 (2^-53 per addition: nothing at this scale).  The square root halves the relative error; the cast to fp32 adds u:
    norm ((14 + L) / 2 + 1) u."""
    L, _ = norm_trips(n)
    return norm * ((14 + L) / 2.0 + 1.0) * U


def coef_bound(norm, dnorm, max_norm):
    """|out2[1] - coef| when the clip is active: coef = max_norm / (norm + 1e-6f): the norm's error, the addition (u), the division (u)."""
    coef = _h(max_norm) / (norm + EPS_NORM)
    return coef * (dnorm / (norm + EPS_NORM) + 2 * U)


AdamBounds = collections.namedtuple('AdamBounds', 'p m v')


def adamw_bounds(p, g, m, v, coef, lr, b1, b2, eps, wd, step):
    """Per-element |kernel - adamw_ref| for p, m, v.
      gg = g c: u.
      m' = b1 m + (1 - b1) gg: the first product u |b1 m|; the second carries gg (u), 1 - b1 (u) and the product (u); the sum u |m'| <= u
           of both magnitudes: 2u |b1 m| + 4u |(1 - b1) gg|.  The sum can cancel, so the bound is in the magnitudes of the terms, not in |m'|.
      v' = b2 v + (1 - b2) gg gg: non-negative terms.  First product u; second: 1 - b2 (u), gg twice (2u), two products (2u); the sum u:
           2u b2 v + 6u (1 - b2) gg^2.
      den = sqrt(v') / bc2_sqrt + eps: r = sqrt(v') / bc2_sqrt carries dv' / (2 v') + u (sqrt) + u (divide); the sum u den.
      q = m' / den: dm' / den + |q| (dden / den + u).           upd = (lr / bc1) q: that ratio (u) and the product (u).
      p' = p (1 - lr wd): lr wd rounded (u lr wd), the difference (u), the product (u |p'|).       p'' = p' - upd: u |p''|."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = _h(lr), _h(b1), _h(b2), _h(eps), _h(wd)
    bc1, bc2s = (float(x) for x in host_bc(b1, b2, step))
    c = 1.0 if coef is None else float(f32(coef))
    gg = g * c
    a1, a2 = np.abs(b1 * m), np.abs((1.0 - b1) * gg)
    m1 = b1 * m + (1.0 - b1) * gg
    dm = 2 * U * a1 + 4 * U * a2
    v1 = b2 * v + (1.0 - b2) * gg * gg
    dv = 2 * U * b2 * v + 6 * U * (1.0 - b2) * gg * gg
    r = np.sqrt(v1) / bc2s
    den = r + eps
    with np.errstate(invalid='ignore', divide='ignore'):
        rel_v = np.where(v1 > 0, dv / np.where(v1 > 0, v1, 1.0), 0.0)
    dden = r * (0.5 * rel_v + 2 * U) + U * den
    q = m1 / den
    dq = dm / den + np.abs(q) * (dden / den + U)
    ss = lr / bc1
    upd = ss * q
    dupd = ss * dq + 2 * U * np.abs(upd)
    decay = 1.0 - lr * wd
    p0 = p * decay
    dp0 = np.abs(p) * U * (lr * wd + decay) + U * np.abs(p0)
    p1 = p0 - upd
    return AdamBounds(dp0 + dupd + U * np.abs(p1), dm, dv)


def sgd_bounds(p, g, buf, coef, lr, mu, step):
    """(dp, dbuf).  gg = g c: u.  buf' = mu buf + gg: the product u |mu buf|, gg's u, the sum u (|mu buf| + |gg|); step 1: gg alone.
    p' = p - lr buf': lr dbuf', the product (u) and the difference (u |p'|)."""
    p, g, buf = (a.astype(np.float64) for a in (p, g, buf))
    c = 1.0 if coef is None else float(f32(coef))
    gg = g * c
    if step == 1:
        b, db = gg, U * np.abs(gg)
    else:
        t = _h(mu) * buf
        b, db = t + gg, 2 * U * (np.abs(t) + np.abs(gg))
    q = _h(lr) * b
    return _h(lr) * db + U * np.abs(q) + U * np.abs(p - q), db


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
# what |g c| is planted at: 0 (with v = m = 0: den = eps, update 0), both sides of eps = 1e-8 (and far below eps = 1e-3), and large.  Every
# planted |g c| is 0 or at least 1e-15, so that (g c)^2 (1 - b2) >= 1e-33 is a NORMAL float32 (and so are (1 - b1) g c and the update):
# no assertion rests on how the device treats subnormals.
PLANT_GC = (0.0, 1e-15, 1e-9, 1e-8, 1e-7, 1e3)

AdamInputs = collections.namedtuple('AdamInputs', 'p g m v planted')


def plant_positions(n, k):
    """k positions spread over [0, n), always with the last three elements (the scalar tail when n % 4 == 3) and element 0."""
    if n <= k:
        return list(range(n))
    pos = sorted(set([(j * n) // k for j in range(k - 3)] + [n - 3, n - 2, n - 1]))
    return pos


def adamw_inputs(n, step, coef, seed=0):
    """p = 0.5 N(0,1), g = 0.01 N(0,1); step > 1: m = 0.005 N(0,1), v = 1e-4 U(0.1, 2), else zeros.  Planted, cycling through the kinds
    (fewer elements than kinds: as many as fit, starting at |g c| = eps = 1e-8, so that n = 1 is not the all-zero element): the PLANT_GC values as g = value / c with alternating sign, m = v = 0 and p = 0
    there (an update of size lr stands against no |p|); p = +-1e3 and p = 0 beside ordinary g, m, v."""
    r = np.random.RandomState(1000 + 7 * seed + (n % 9973) + 31 * step)
    p = (0.5 * r.standard_normal(n)).astype(np.float32)
    g = (0.01 * r.standard_normal(n)).astype(np.float32)
    if step > 1:
        m = (0.005 * r.standard_normal(n)).astype(np.float32)
        v = (1e-4 * r.uniform(0.1, 2.0, n)).astype(np.float32)
    else:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    c = 1.0 if coef is None else float(f32(coef))
    kinds = len(PLANT_GC) + 3
    pos = plant_positions(n, 4 * kinds)
    for j, i in enumerate(pos):
        k = (j + seed + (3 if n < kinds else 0)) % kinds
        if k < len(PLANT_GC):
            g[i] = f32((PLANT_GC[k] / c) * (1 if j % 2 else -1))
            m[i] = v[i] = 0.0
            p[i] = 1e3 if PLANT_GC[k] == 1e3 else 0.0
        elif k == len(PLANT_GC):
            p[i] = 1e3
        elif k == len(PLANT_GC) + 1:
            p[i] = -1e3
        else:
            p[i] = 0.0
    assert ((v == 0) <= (m == 0)).all()
    gc = np.abs(g.astype(np.float64) * c)
    assert ((gc == 0) | (gc >= 0.99e-15)).all()
    return AdamInputs(p, g, m, v, pos)


#              step, (beta1, beta2),  eps, (lr, wd),    coef, n
BIG_N = 4 * (STEP_BLOCKS * 256) + 3075          # past the 4096-block cap (a second grid-stride trip) with a 3-element tail
ADAMW_CASES = [(1, (0.9, 0.999), 1e-8, (1e-4, 5e-5), 0.37, 100003),
               (2, (0.5, 0.9), 1e-3, (1e-2, 0.1), None, 7),
               (7, (0.0, 0.999), 1e-8, (1e-2, 0.0), 1.0, 4),
               (1000, (0.9, 0.999), 1e-8, (1e-2, 0.1), 0.37, BIG_N),
               (200000, (0.9, 0.999), 1e-3, (1e-4, 5e-5), None, 3),
               (1, (0.5, 0.9), 1e-8, (1e-2, 0.1), 1.0, 1),
               (2, (0.9, 0.999), 1e-8, (1e-2, 0.1), 0.37, 100003),
               (7, (0.9, 0.999), 1e-8, (1e-2, 0.0), None, 100003),
               (1, (0.9, 0.999), 1e-3, (1e-2, 0.1), 0.37, 7)]


def adamw_case_args(case):
    step, (b1, b2), eps, (lr, wd), coef, n = case
    return dict(coef=coef, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, step=step)


SgdInputs = collections.namedtuple('SgdInputs', 'p g buf')


def sgd_inputs(n, seed=0):
    """p = 0.5 N(0,1) with exact zeros and +-1e3 planted, g = 0.01 N(0,1), buf = 0.05 N(0,1): a DIRTY buffer, which step 1 must ignore."""
    r = np.random.RandomState(2000 + seed + (n % 9973))
    p = (0.5 * r.standard_normal(n)).astype(np.float32)
    g = (0.01 * r.standard_normal(n)).astype(np.float32)
    buf = (0.05 * r.standard_normal(n)).astype(np.float32)
    for j, i in enumerate(plant_positions(n, 12)):
        p[i] = (0.0, 1e3, -1e3)[(j + seed) % 3]
    return SgdInputs(p, g, buf)


#            step, coef,  mu,  n
SGD_CASES = [(1, None, 0.9, 5),
             (1, 0.37, 0.9, 100003),
             (2, 0.37, 0.9, STEP_BLOCKS * 256 + 9),          # one thread per element, 4096 blocks: the last 9 take a second trip
             (3, None, 0.0, 1),
             (2, None, 0.9, 100003),
             (3, 0.37, 0.0, 5),
             (1, 0.37, 0.0, 1)]

CLIP_NS = (1, 2, 3, 4, 5, 1023, 100003, 2 * 1048576 + 3)        # the last: 2 x (1024 x 256) vectors + 3, so the stride loop wraps


def norm_inputs(n, seed=0):
    """g = 0.01 N(0,1) with heavy elements of 0.06 x the norm of the rest at: element 0, the last element of the last whole vector,
    every tail slot, and the first element of a thread's second grid-stride trip (when there is one).  Returns (g, heavy positions)."""
    r = np.random.RandomState(3000 + seed + (n % 9973))
    g = (0.01 * r.standard_normal(n)).astype(np.float32)
    n4 = n // 4
    L, blocks = norm_trips(n)
    heavy = {0} | set(range(4 * n4, n))
    if n4:
        heavy.add(4 * n4 - 1)
    if L > 1:
        heavy.add(4 * blocks * 256)
    heavy = sorted(heavy)
    rest = np.ones(n, bool)
    rest[heavy] = False
    base = math.sqrt(float((g[rest].astype(np.float64) ** 2).sum())) if rest.any() else 0.01
    for j, i in enumerate(heavy):
        g[i] = f32(0.06 * max(base, 0.01) * (1 if j % 2 else -1))
    return g, heavy
