"""The numpy yardstick of the calibration kernels (csrc/calibration.hip), checked on the CPU by
tests/test_cpu_calibration.py and used by tests/test_calibration_gpu.py.

Definitions restated (include/pylc_hip.h):
  bin of a float32 confidence p with B bins:  min(B - 1, int(p * float32(B))), the product in fp32, the conversion truncating
  quantised confidence:                       q = uint32(p * 2^24) -- the product is exact, the conversion truncates
  counts: int64 [3*C*B + 3]; predicted class c, bin b: (c*B + b)*3 + {0, 1, 2} = pixels, pixels whose target is c, sum of q; the tail
          3*C*B + {0, 1, 2} = targets (or predicted classes) outside 0..C-1 that are not the ignore label, ignored targets, confidences that
          are NaN, infinite or outside [0, 1]; a tail pixel is counted in its tail cell only (ignore label first, then in that order)."""
import numpy as np

from tests import _regions as R

Q_ONE = np.float32(16777216.0)


# ---- fp32 models, bit for bit ------------------------------------------------------------------------------------------------------------
def bin_of(p, bins):
    """float32 confidences in [0, 1] -> int bins"""
    p = np.asarray(p, np.float32)
    prod = (p * np.float32(bins)).astype(np.float32)
    return np.minimum(bins - 1, prod.astype(np.int64))


def q_of(p):
    p = np.asarray(p, np.float32)
    return (p * Q_ONE).astype(np.float32).astype(np.int64)


def n_cells(c, bins):
    return 3 * c * bins + 3


def counts_ref(conf, pred, truth, c, bins, ignore_index=None):
    """the cell layout applied to flat arrays: float32 conf, integer pred and truth"""
    conf = np.asarray(conf, np.float32).reshape(-1)
    pred = np.asarray(pred).reshape(-1).astype(np.int64)
    truth = np.asarray(truth).reshape(-1).astype(np.int64)
    out = np.zeros(n_cells(c, bins), np.int64)
    ignored = truth == ignore_index if ignore_index is not None else np.zeros(truth.shape, bool)
    outside = ~ignored & ((truth < 0) | (truth >= c) | (pred < 0) | (pred >= c))
    with np.errstate(invalid='ignore'):
        good_conf = (conf >= 0) & (conf <= 1)               # NaN fails both
    bad = ~ignored & ~outside & ~good_conf
    out[3 * c * bins:] = outside.sum(), ignored.sum(), bad.sum()
    use = ~ignored & ~outside & good_conf
    p, k, t = conf[use], pred[use], truth[use]
    cell = k * bins + bin_of(p, bins)
    out[:3 * c * bins:3] = np.bincount(cell, minlength=c * bins)
    out[1:3 * c * bins:3] = np.bincount(cell[k == t], minlength=c * bins)
    qsum = np.zeros(c * bins, np.int64)
    np.add.at(qsum, cell, q_of(p))
    out[2:3 * c * bins:3] = qsum
    return out


def scores_ref(counts, c, bins):
    """ece / mce / class_ece of a count vector, written independently of pylc_amd.calibration.reliability_scores"""
    cells = np.asarray(counts, np.float64)[:3 * c * bins].reshape(c, bins, 3)

    def ece(t):
        n = t[:, 0].sum()
        e, m = 0.0, 0.0
        for k in range(bins):
            if t[k, 0] > 0:
                gap = abs(t[k, 1] / t[k, 0] - t[k, 2] / 2.0 ** 24 / t[k, 0])
                e += t[k, 0] / n * gap
                m = max(m, gap)
        return e, m
    e, m = ece(cells.sum(0))
    return {'ece': e, 'mce': m, 'class_ece': [ece(cells[k])[0] if cells[k, :, 0].sum() > 0 else 0.0 for k in range(c)]}


def conf_f32(z, beta=1.0):
    """the kernel's arithmetic in numpy fp32: first maximum, conf = 1 / sum_c exp((z_c - z_max) * beta), ascending c.  z: [N, C] float32.
    (numpy's fp32 exp is not the device's expf bit for bit: this model is for scale, the GPU test compares against fp64.)"""
    z = np.asarray(z, np.float32)
    m = z.max(1, keepdims=True)
    s = np.zeros(z.shape[0], np.float32)
    for k in range(z.shape[1]):
        s = (s + np.exp(((z[:, k:k + 1] - m) * np.float32(beta)).astype(np.float32))[:, 0]).astype(np.float32)
    return z.argmax(1).astype(np.uint8), (np.float32(1) / s).astype(np.float32)


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------------
def conf_f64(z, beta=1.0):
    """float64 softmax maximum of float32 logits z [N, C] at inverse temperature beta (beta as the fp32 number the kernel gets)"""
    d = (np.asarray(z, np.float64) - np.asarray(z, np.float64).max(1, keepdims=True)) * float(np.float32(beta))
    return 1.0 / np.exp(d).sum(1)


def nll_terms_f64(z, target, beta):
    """per-pixel log sum_c exp((z_c - z_max) beta) - (z_t - z_max) beta in float64, for targets inside the classes; and max_c |beta (z_c - z_max)|"""
    z = np.asarray(z, np.float64)
    d = (z - z.max(1, keepdims=True)) * float(np.float32(beta))
    term = np.log(np.exp(d).sum(1)) - d[np.arange(z.shape[0]), target]
    return term, np.abs(d).max(1)


def nll_bound(z, target, beta):
    """The sum over pixels of the per-pixel bound on |term_fp32 - term_fp64|:
    (C + 8) * 2^-23 * (1 + term64) + 2^-22 * max_c |beta (z_c - z_max)|.
    C rounded exponentials and their sum, the logarithm and the final subtraction are relative to the term (the first part); the fp32
    products beta * (z_c - z_max), inside the exponentials and in the target's term, are relative to their own size (the second)."""
    term, amax = nll_terms_f64(z, target, beta)
    c = np.asarray(z).shape[1]
    return float(((c + 8) * 2.0 ** -23 * (1.0 + term) + 2.0 ** -22 * amax).sum())


def nll_sums_ref(z, target, betas, c, ignore_index=None):
    """(float64 sums [K], tail [3], bound [K]) of logits z [N, C] and integer targets [N]"""
    target = np.asarray(target).reshape(-1).astype(np.int64)
    ignored = target == ignore_index if ignore_index is not None else np.zeros(target.shape, bool)
    outside = ~ignored & ((target < 0) | (target >= c))
    use = ~ignored & ~outside
    zz, tt = np.asarray(z)[use], target[use]
    sums = np.array([nll_terms_f64(zz, tt, b)[0].sum() for b in betas])
    bound = np.array([nll_bound(zz, tt, b) for b in betas])
    return sums, np.array([use.sum(), outside.sum(), ignored.sum()], np.int64), bound


def default_betas(k=33, lo=0.25, hi=4.0):
    b = np.exp(np.linspace(np.log(lo), np.log(hi), k))
    if k % 2 == 1 and lo * hi == 1.0:
        b[k // 2] = 1.0
    return b


def fit_temperature(betas, sums, n):
    """pure numpy: the vertex of the parabola through the three grid points around the smallest mean NLL, in log beta (Lagrange form)"""
    x, y = np.log(np.asarray(betas, np.float64)), np.asarray(sums, np.float64) / n
    i = int(np.argmin(y))
    if i == 0 or i == len(y) - 1:
        return {'temperature': float(1.0 / np.exp(x[i])), 'nll': float(y[i]), 'at_edge': True}
    a, b, c = np.polyfit(x[i - 1:i + 2] - x[i], y[i - 1:i + 2], 2)
    xv = -b / (2 * a)
    return {'temperature': float(np.exp(-(xv + x[i]))), 'nll': float(c - b * b / (4 * a)), 'at_edge': False}


# ---- input makers ------------------------------------------------------------------------------------------------------------------------
def blob_mask(n, c, seed=0):
    """a flat blob mask of n pixels: rows of tests/_regions.blobs (runs of one class, as real masks have)"""
    w = 64
    h = -(-n // w)
    return R.blobs(max(h, 16), w, c, seed=seed, radius=5).reshape(-1)[:n].copy()


def logits(n, c, scale=3.0, seed=0):
    return (np.random.default_rng(seed).standard_normal((n, c)) * scale).astype(np.float32)


def sampled(n, c, s, seed=0, spread=2.5):
    """(logits, labels): labels SAMPLED from softmax(t), logits handed out as s * t, so that the true temperature is s"""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((n, c)) * spread
    p = np.exp(t - t.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    u = rng.random(n)
    labels = np.minimum((p.cumsum(1) < u[:, None]).sum(1), c - 1).astype(np.uint8)
    return (s * t).astype(np.float32), labels
