"""Calibration of the confidences the inference paths hand out (csrc/calibration.hip): reliability counts on the
device -- from a confidence map and two masks, or straight from a network's logits --, the expected / maximum calibration error as closed
forms of those counts on the host, the negative log-likelihood of the logits on a grid of inverse temperatures in one pass, and the
single temperature fitted to that grid.  Nothing pixel-sized goes to the host.

Definitions (include/pylc_hip.h): the bin of a float32 confidence p with B bins is min(B - 1, int(p * float32(B))) with the product in
fp32; the confidence is summed as the integer q = uint32(p * 2^24), so every count and sum is exact and independent of pixel order.
counts is int64 [3*C*B + 3]: for predicted class c and bin b the entries (c*B + b)*3 + {0, 1, 2} are pixels, pixels whose target is c and
the sum of q; the last three are out-of-range targets, ignored targets and confidences that are NaN, infinite or outside [0, 1]."""
import ctypes

import numpy as np
import torch

from . import lib as L
from .lib import lib, check, ptr, stream

MAX_BINS = 32
MAX_BETAS = 32          # per launch of pylc_logits_nll_grid; nll_grid() splits a longer grid
Q_ONE = 16777216.0      # 2^24: the quantisation of a confidence


def n_cells(n_classes, bins):
    return 3 * int(n_classes) * int(bins) + 3


def _check_bins(bins):
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError('calibration bins must be an int in 1..%d, got %r' % (MAX_BINS, bins))
    return int(bins)


def _check_counts(counts, cells, device):
    if counts is None:
        return torch.zeros(cells, device=device, dtype=torch.int64)
    if counts.dtype != torch.int64 or counts.numel() != cells or not counts.is_contiguous():
        raise ValueError('counts must be a contiguous int64 tensor of %d entries' % cells)
    return counts


def _check_target(target, n, device, what='target'):
    if target.dtype not in (torch.uint8, torch.int64):
        raise TypeError('%s must be uint8 or int64 class indices, got %s' % (what, target.dtype))
    if target.numel() != n:
        raise ValueError('%s %s does not cover %d pixels' % (what, tuple(target.shape), n))
    return target.to(device, non_blocking=True).contiguous()


def _ignore_args(ignore_index):
    return (0, 0) if ignore_index is None else (1, int(ignore_index))


def reliability_counts(conf, pred, truth, n_classes, bins=15, ignore_index=None, counts=None):
    """Reliability counts of a confidence map against a predicted and a true mask ([H,W] or [B,H,W]: conf float32, pred uint8, truth uint8 or
    int64; what segment_photo(..., return_confidence=True) and photo.encode_mask leave on the device) in one launch.  `counts` (int64
    [3*n_classes*bins + 3], device) is ADDED into; a zeroed one is allocated when none is passed.  Returns counts."""
    L.init()
    bins = _check_bins(bins)
    if conf.dim() not in (2, 3) or conf.dtype != torch.float32:
        raise ValueError('conf must be a float32 [H,W] or [B,H,W] map, got %s %s' % (conf.dtype, tuple(conf.shape)))
    if pred.dtype != torch.uint8 or pred.shape != conf.shape:
        raise ValueError('pred must be a uint8 mask of conf\'s shape %s, got %s %s' % (tuple(conf.shape), pred.dtype, tuple(pred.shape)))
    if truth.shape != conf.shape:
        raise ValueError('truth %s does not match conf %s' % (tuple(truth.shape), tuple(conf.shape)))
    n = conf.numel()
    conf, pred = conf.contiguous(), pred.contiguous()
    truth = _check_target(truth, n, conf.device, 'truth')
    counts = _check_counts(counts, n_cells(n_classes, bins), conf.device)
    has_ign, ign = _ignore_args(ignore_index)
    check(lib.pylc_reliability_counts(ptr(conf), ptr(pred), ptr(truth), truth.element_size(), n, int(n_classes), bins, has_ign, ign, ptr(counts),
                                      stream()))
    return counts


def _logits(logits):
    from . import ops
    if logits.dim() != 4:
        raise ValueError('expected [B,C,H,W] logits, got %s' % (tuple(logits.shape),))
    x = ops.as_nhwc(logits)
    b, c, h, w = x.shape
    return x, ops.pitch_of(x), b, c, h, w


def _inv_temperature(temperature):
    if temperature is None:
        return 1.0
    t = float(temperature)
    if not (t > 0.0 and t != float('inf')):
        raise ValueError('temperature must be a positive finite number, got %r' % (temperature,))
    return 1.0 / t


def logits_reliability(logits, target=None, bins=15, temperature=None, ignore_index=None, counts=None, return_mask=False, return_confidence=False):
    """Reliability counts (and / or the class mask and the confidence map) of a batch of logits [B,C,H,W] as a net returns them, in ONE launch
    and without a host synchronisation: the class of a pixel is the first maximum of its logits, its confidence
    1 / sum_c exp((z_c - z_max) / temperature) in fp32 (temperature None: 1).  target [B,H,W], uint8 or int64; `counts` (int64
    [3*C*bins + 3], device) is ADDED into, a zeroed one is allocated when none is passed.  Returns counts (None without a target), or the tuple
    (counts[, mask][, conf]) with return_mask (uint8 [B,H,W]) / return_confidence (float32 [B,H,W], the very floats that were binned)."""
    L.init()
    bins = _check_bins(bins)
    beta = _inv_temperature(temperature)
    if target is None and counts is not None:
        raise ValueError('counts need a target')
    if target is None and not (return_mask or return_confidence):
        raise ValueError('neither a target nor return_mask / return_confidence: nothing to compute')
    x, pitch, b, c, h, w = _logits(logits)
    n = b * h * w
    tbytes = 0
    if target is not None:
        target = _check_target(target, n, x.device)
        tbytes = target.element_size()
        counts = _check_counts(counts, n_cells(c, bins), x.device)
    mask = torch.empty((b, h, w), device=x.device, dtype=torch.uint8) if return_mask else None
    conf = torch.empty((b, h, w), device=x.device, dtype=torch.float32) if return_confidence else None
    has_ign, ign = _ignore_args(ignore_index)
    check(lib.pylc_logits_reliability(ptr(x), pitch, ptr(target), tbytes, n, c, bins, beta, has_ign, ign, ptr(mask), ptr(conf), ptr(counts),
                                      stream()))
    if not (return_mask or return_confidence):
        return counts
    return (counts,) + ((mask,) if return_mask else ()) + ((conf,) if return_confidence else ())


def default_betas(k=33, lo=0.25, hi=4.0):
    """k log-spaced inverse temperatures from lo to hi (float64 array); for odd k and lo * hi == 1 the middle one is exactly 1."""
    k = int(k)
    if k < 3 or not 0.0 < lo < hi:
        raise ValueError('default_betas: k >= 3 and 0 < lo < hi, got k=%r lo=%r hi=%r' % (k, lo, hi))
    b = np.exp(np.linspace(np.log(lo), np.log(hi), k))
    b[0], b[-1] = lo, hi
    if k % 2 == 1 and lo * hi == 1.0:
        b[k // 2] = 1.0
    return b


def nll_grid(logits, target, betas, ignore_index=None, sums=None, tail=None):
    """Sum over the pixels of logits [B,C,H,W] whose target is a class of the negative log-likelihood of softmax(beta * logits), for every
    beta of `betas` (positive floats, host) in one pass over the logits per 32 betas (a longer grid is split into equal parts: the kernel
    takes at most 32 by value).  The per-pixel term is fp32, the sums are fp64, bitwise reproducible (no float atomics).  sums (float64
    [len(betas)], device) and tail (int64 [3], device: pixels summed, out-of-range targets, ignored targets) are ADDED into; zeroed ones are
    allocated when none are passed.  Returns (sums, tail)."""
    L.init()
    betas = np.asarray(betas, dtype=np.float32).reshape(-1)
    k = betas.size
    if k < 1 or not np.all(np.isfinite(betas) & (betas > 0)):
        raise ValueError('betas must be positive finite numbers, got %r' % (betas,))
    x, pitch, b, c, h, w = _logits(logits)
    n = b * h * w
    target = _check_target(target, n, x.device)
    if sums is None:
        sums = torch.zeros(k, device=x.device, dtype=torch.float64)
    elif sums.dtype != torch.float64 or sums.numel() != k or not sums.is_contiguous():
        raise ValueError('sums must be a contiguous float64 tensor of %d entries' % k)
    if tail is None:
        tail = torch.zeros(3, device=x.device, dtype=torch.int64)
    elif tail.dtype != torch.int64 or tail.numel() != 3 or not tail.is_contiguous():
        raise ValueError('tail must be a contiguous int64 tensor of 3 entries')
    has_ign, ign = _ignore_args(ignore_index)
    parts = -(-k // MAX_BETAS)
    per = -(-k // parts)
    for first in range(0, k, per):
        kk = min(per, k - first)
        ws = torch.empty(max(1, lib.pylc_logits_nll_grid_workspace_bytes(n, kk) // 8), device=x.device, dtype=torch.float64)
        part_tail = tail if first == 0 else torch.zeros_like(tail)           # every part sees the same pixels: count them once
        arr = (ctypes.c_float * kk)(*[float(v) for v in betas[first:first + kk]])
        check(lib.pylc_logits_nll_grid(ptr(x), pitch, ptr(target), target.element_size(), n, c, arr, kk, has_ign, ign, ptr(ws),
                                       sums.data_ptr() + 8 * first, ptr(part_tail), stream()))
    return sums, tail


# ---- host side: closed forms of the counts ---------------------------------------------------------------------------------------------
def _host(a, dtype):
    return np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=dtype).reshape(-1)


def _table_scores(t):
    """(ece, mce, n) of one [B,3] table of (pixels, hits, sum of q)"""
    n = t[:, 0].sum()
    if n == 0:
        return 0.0, 0.0, 0.0
    full = t[:, 0] > 0
    cnt = np.where(full, t[:, 0], 1.0)
    gap = np.where(full, np.abs(t[:, 1] / cnt - t[:, 2] / Q_ONE / cnt), 0.0)
    return float((t[:, 0] / n * gap).sum()), float(gap.max()), float(n)


def reliability_scores(counts, n_classes, bins):
    """Scores of reliability counts, on the host in float64: 'ece' = sum_b n_b / n * |acc_b - conf_b| of the table summed over the classes,
    'mce' the largest such gap among its non-empty bins, 'class_ece' [C] the same of every predicted class's own table (0 for a class
    never predicted), 'accuracy', 'mean_confidence', 'table' [B,3] (n, accuracy, mean confidence; 0 in an empty bin), 'n' the pixels
    counted and 'ignored'.  Raises ValueError when the counts hold an out-of-range target or a confidence outside [0, 1]."""
    c, b = int(n_classes), _check_bins(bins)
    host = _host(counts, np.int64)
    if host.size != n_cells(c, b):
        raise ValueError('counts has %d entries, %d classes x %d bins need %d' % (host.size, c, b, n_cells(c, b)))
    outside, ignored, bad = (int(v) for v in host[3 * c * b:])
    if outside:
        raise ValueError('%d pixels hold a target or a predicted class outside 0..%d' % (outside, c - 1))
    if bad:
        raise ValueError('%d confidences are NaN, infinite or outside [0, 1]' % bad)
    cells = host[:3 * c * b].reshape(c, b, 3).astype(np.float64)
    total = cells.sum(0)
    ece, mce, n = _table_scores(total)
    full = total[:, 0] > 0
    cnt = np.where(full, total[:, 0], 1.0)
    table = np.stack([total[:, 0], np.where(full, total[:, 1] / cnt, 0.0), np.where(full, total[:, 2] / Q_ONE / cnt, 0.0)], axis=1)
    return {'ece': ece, 'mce': mce, 'class_ece': [_table_scores(cells[k])[0] for k in range(c)],
            'accuracy': float(total[:, 1].sum() / n) if n else 0.0, 'mean_confidence': float(total[:, 2].sum() / Q_ONE / n) if n else 0.0,
            'table': table, 'n': int(n), 'ignored': ignored}


def fit_temperature(betas, sums, n):
    """The temperature that minimises the mean NLL sums / n sampled on the grid `betas` of inverse temperatures (ascending):
    {'temperature', 'nll', 'nll_at_1', 'at_edge'}.  The mean NLL of softmax(beta * z) is convex in beta (a log-sum-exp of functions linear
    in beta minus a linear one), so the grid's smallest value brackets the minimum between its two neighbours, and the fit is the vertex of
    the parabola through those three points, taken in log beta; 'nll' is the parabola's value there.  When the smallest value is the first
    or last grid point the minimum lies outside the grid: at_edge=True and that point's temperature and value are returned.  'nll_at_1' is
    the grid's value at beta = 1 (interpolated in log beta when 1 is not a grid point)."""
    betas, y = _host(betas, np.float64), _host(sums, np.float64)
    if betas.size != y.size or betas.size < 3 or not np.all(np.diff(betas) > 0) or betas[0] <= 0:
        raise ValueError('fit_temperature needs at least 3 ascending positive betas and as many sums')
    if not n > 0:
        raise ValueError('fit_temperature: no pixel was summed (n=%r)' % (n,))
    y = y / float(n)
    x = np.log(betas)
    at_1 = float(np.interp(0.0, x, y))
    i = int(np.argmin(y))
    if i == 0 or i == y.size - 1:
        return {'temperature': float(1.0 / betas[i]), 'nll': float(y[i]), 'nll_at_1': at_1, 'at_edge': True}
    x0, x1, x2 = x[i - 1:i + 2]
    y0, y1, y2 = y[i - 1:i + 2]
    d1, d2 = (y1 - y0) / (x1 - x0), (y2 - y1) / (x2 - x1)
    curv = (d2 - d1) / (x2 - x0)                      # half the second derivative of the parabola
    if curv <= 0:                                     # three equal values (a flat stretch of the grid): keep the grid point
        return {'temperature': float(1.0 / betas[i]), 'nll': float(y1), 'nll_at_1': at_1, 'at_edge': False}
    xv = 0.5 * (x0 + x1) - d1 / (2.0 * curv)
    yv = y0 + d1 * (xv - x0) + curv * (xv - x0) * (xv - x1)
    return {'temperature': float(np.exp(-xv)), 'nll': float(yv), 'nll_at_1': at_1, 'at_edge': False}
