"""The statement of pylc_amd.boundary in numpy.  numpy only: the GPU tests must not depend on a library nobody has
checked on the GPU machine.

Boundary distance of a class mask m (uint8 [H,W] or [B,H,W], every image on its own), radius R in 1..254:
    d2(p) = min(R*R + 1, min over pixels q of the same image with m[q] != m[p] of |p - q|^2)          (int32)
A pixel equal to ignore_index is a q for every class and gets -1 itself; only real pixels are q (the image edge is no border).
distance_ref computes it in the separable form, brute_ref (tests/test_cpu_boundary.py's yardstick) by the all-pairs search:
    column pass   g(x,y)  = min(R + 1, min |y - y'| over y' with m[y',x] != m[y,x])
    row pass      d2(x,y) = min(R*R + 1, min over |x - x'| <= R of (x - x')^2 + (m[y,x'] != m[y,x] ? 0 : g(x',y))^2)
Band: labelled pixels with d2 <= R*R.

Counts of a (truth, prediction) pair, int64 [C*C + 3C + 1] = cm_band [C,C], inter [C], gband [C], pband [C], outside [1].  Where the truth
is ignored the prediction is ignored too, before its distances are taken; only pixels with a labelled truth are counted.  A pixel whose
truth is >= C, or whose prediction is >= C and not the ignore label, adds to `outside` and to nothing else.  Of the others:
gband[t] += in truth's band; and where the prediction is not the ignore label: cm_band[t, p] += in truth's band,
pband[p] += in prediction's band, inter[t] += (t == p and in both bands)."""
import numpy as np


def _distance_one(m, R, ign):
    """m: int16 [H,W] with ignored pixels already holding ign (or ign = -1: none)"""
    h, w = m.shape
    g = np.full((h, w), R + 1, np.int64)
    for d in range(1, min(R, h - 1) + 1):
        differ = m[d:] != m[:-d]
        np.minimum(g[d:], np.where(differ, d, R + 1), out=g[d:])
        np.minimum(g[:-d], np.where(differ, d, R + 1), out=g[:-d])
    best = np.minimum(R * R + 1, g * g)
    for d in range(1, min(R, w - 1) + 1):
        differ = m[:, d:] != m[:, :-d]
        np.minimum(best[:, d:], d * d + np.where(differ, 0, g[:, :-d]) ** 2, out=best[:, d:])
        np.minimum(best[:, :-d], d * d + np.where(differ, 0, g[:, d:]) ** 2, out=best[:, :-d])
    best[m == ign] = -1
    return best.astype(np.int32)


def _effective(mask, ignore_index, ignore_from):
    m = np.asarray(mask).astype(np.int16)
    if ignore_from is not None:
        assert ignore_index is not None
        m = np.where(np.asarray(ignore_from) == ignore_index, np.int16(ignore_index), m)
    return m


def distance_ref(mask, R, ignore_index=None, ignore_from=None):
    assert 1 <= R <= 254
    m = _effective(mask, ignore_index, ignore_from)
    ign = -1 if ignore_index is None else int(ignore_index)
    if m.ndim == 2:
        return _distance_one(m, R, ign)
    return np.stack([_distance_one(k, R, ign) for k in m])


def brute_ref(mask, R, ignore_index=None):
    """the definition itself: all pairs of one [H,W] image"""
    m = np.asarray(mask).astype(np.int64)
    h, w = m.shape
    yy, xx = np.mgrid[0:h, 0:w]
    yy, xx, v = yy.reshape(-1), xx.reshape(-1), m.reshape(-1)
    dist = (yy[:, None] - yy[None, :]) ** 2 + (xx[:, None] - xx[None, :]) ** 2
    dist = np.where(v[:, None] != v[None, :], dist, R * R + 1)
    d2 = np.minimum(R * R + 1, dist.min(1))
    if ignore_index is not None:
        d2[v == ignore_index] = -1
    return d2.reshape(h, w).astype(np.int32)


def band_ref(mask, R, ignore_index=None):
    d2 = distance_ref(mask, R, ignore_index)
    return (d2 >= 0) & (d2 <= R * R)


def n_cells(c):
    return c * c + 3 * c + 1


def counts_ref(truth, pred, c, R, ignore_index=None):
    t, p = np.asarray(truth).astype(np.int64), np.asarray(pred).astype(np.int64)
    ign = -1 if ignore_index is None else int(ignore_index)
    d2t = distance_ref(truth, R, ignore_index)
    d2p = distance_ref(pred, R, ignore_index, ignore_from=truth if ignore_index is not None else None)
    labelled = t != ign
    bad = labelled & ((t >= c) | ((p >= c) & (p != ign)))
    ok = labelled & ~bad
    pv = ok & (p != ign)
    in_g = ok & (d2t >= 0) & (d2t <= R * R)
    in_p = pv & (d2p >= 0) & (d2p <= R * R)
    out = np.zeros(n_cells(c), np.int64)
    sel = in_g & pv
    out[:c * c] = np.bincount(t[sel] * c + p[sel], minlength=c * c)
    both = sel & in_p & (t == p)
    out[c * c:c * c + c] = np.bincount(t[both], minlength=c)
    out[c * c + c:c * c + 2 * c] = np.bincount(t[in_g], minlength=c)
    out[c * c + 2 * c:c * c + 3 * c] = np.bincount(p[in_p], minlength=c)
    out[-1] = int(bad.sum())
    return out


def split_counts(counts, c):
    """-> cm_band [C,C], inter, gband, pband [C], outside"""
    k = np.asarray(counts).reshape(-1)
    return k[:c * c].reshape(c, c), k[c * c:c * c + c], k[c * c + c:c * c + 2 * c], k[c * c + 2 * c:c * c + 3 * c], int(k[-1])


def scores_ref(counts, c):
    """class_boundary_iou, its gband-weighted mean and its plain mean over the classes with gband + pband > 0 (float64)"""
    _, inter, gband, pband, _ = (np.asarray(a, np.float64) if not isinstance(a, int) else a for a in split_counts(counts, c))
    union = gband + pband - inter
    iou = np.where(union > 0, inter / np.maximum(union, 1), 0.0)
    present = gband + pband > 0
    w = np.where(present, gband, 0.0)
    return {'class_boundary_iou': iou, 'boundary_iou': float((iou * w).sum() / w.sum()) if w.sum() > 0 else 0.0,
            'boundary_iou_mean': float(iou[present].mean()) if present.any() else 0.0}


def default_radius_ref(h, w, ratio=0.02):
    return min(254, max(1, int(round(ratio * np.sqrt(float(h * h + w * w))))))


def scatter_ignore(mask, frac=0.1, seed=0, value=255):
    """the mask with `frac` of its pixels replaced by the ignore value"""
    out = np.array(mask, copy=True)
    out[np.random.default_rng(seed).random(out.shape) < frac] = value
    return out
