"""Scores along class borders: the distance of every pixel to the nearest pixel of another class, the band it defines, boundary IoU
(Cheng et al., CVPR 2021) and the trimap scores of the DeepLab papers, on the device (csrc/boundary.hip; the reference has
nothing of the kind).

d2(p) = min(R*R + 1, min |p - q|^2 over the pixels q of p's image with mask[q] != mask[p]): the squared Euclidean distance, saturated one
above R*R.  A pixel equal to `ignore_index` differs from every class and gets -1 itself; the image edge is no border.  A labelled pixel is
in its mask's band when d2 <= R*R.  Everything is integer work: a numpy statement of the rules (tests/_boundary.py) is compared bit for bit.

Counts of a (truth, prediction) pair, int64 [C*C + 3C + 1]: cm_band [C,C] over the truth's band (the trimap confusion matrix), then
inter / gband / pband [C] each, then one cell for values outside 0..C-1 that are not the ignore label.  Where the truth is ignored the
prediction counts as ignored before its distances are taken; only pixels with a labelled truth are counted.

Border weights: border_profile is a table over d2, border_weights the float32 map table[d2] of a mask (0 at ignored
pixels) in the distance's two launches -- the per-pixel weights of ops.multiloss(pixel_weights=) and Meta.border_weight."""
import math

import numpy as np
import torch

from . import lib as L
from . import metrics
from .lib import lib, check, ptr, stream
from .regions import _on_device

MAX_RADIUS = 254            # the column distance R + 1 is a byte (csrc/boundary.hip)


def default_radius(h, w, ratio=0.02):
    """The boundary-IoU paper's band: `ratio` (2 %) of the image diagonal, at least 1 and at most MAX_RADIUS."""
    return min(MAX_RADIUS, max(1, int(round(ratio * math.sqrt(h * h + w * w)))))


def n_cells(n_classes):
    return n_classes * n_classes + 3 * n_classes + 1


def _check_radius(radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise TypeError('radius must be an int, got %r' % (radius,))
    if not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError('radius=%d outside 1..%d' % (radius, MAX_RADIUS))
    return int(radius)


def _check_ignore(ignore_index):
    if ignore_index is not None and not 0 <= int(ignore_index) <= 255:
        raise ValueError('ignore_index=%r does not fit a uint8 mask (0..255)' % (ignore_index,))
    return -1 if ignore_index is None else int(ignore_index)


def _check_classes(n_classes):
    if not 1 <= int(n_classes) <= 255:
        raise ValueError('n_classes=%r outside 1..255' % (n_classes,))
    return int(n_classes)


def _check_mask(mask, what='a mask'):
    """-> (B, H, W) of a uint8 [H,W] or [B,H,W] tensor"""
    if not torch.is_tensor(mask) or mask.dtype != torch.uint8:
        raise TypeError('%s must be a uint8 tensor, got %s' % (what, mask.dtype if torch.is_tensor(mask) else type(mask).__name__))
    if mask.dim() not in (2, 3) or mask.numel() == 0:
        raise ValueError('%s must be [H,W] or [B,H,W] with at least one pixel, got %s' % (what, tuple(mask.shape)))
    if mask.numel() >= 2 ** 31:
        raise ValueError('%s must have fewer than 2^31 pixels, got %s' % (what, tuple(mask.shape)))
    return (1,) + tuple(mask.shape) if mask.dim() == 2 else tuple(mask.shape)


def _workspace(b, h, w, device):
    return torch.empty((lib.pylc_boundary_workspace_bytes(b, h, w) // 4,), device=device, dtype=torch.int32)


def boundary_distance(mask, radius, ignore_index=None, ignore_from=None):
    """Device uint8 [H,W] or [B,H,W] -> int32 of the same shape: d2 as above, -1 at pixels equal to ignore_index.  ignore_from: a second
    mask of the same shape whose pixels equal to ignore_index count as ignored here too (how a prediction is measured under a truth)."""
    radius, ign = _check_radius(radius), _check_ignore(ignore_index)
    b, h, w = _check_mask(mask)
    if ignore_from is not None:
        if ignore_index is None:
            raise ValueError('ignore_from needs an ignore_index')
        if _check_mask(ignore_from, 'ignore_from') != (b, h, w) or ignore_from.dim() != mask.dim():
            raise ValueError('ignore_from %s does not match the mask %s' % (tuple(ignore_from.shape), tuple(mask.shape)))
        ignore_from = _on_device(ignore_from, 'ignore_from')
    mask = _on_device(mask, 'a mask')
    L.init()
    d2 = torch.empty(mask.shape, device=mask.device, dtype=torch.int32)
    ws = _workspace(b, h, w, mask.device)
    check(lib.pylc_boundary_distance(ptr(mask), b, h, w, radius, ign, ptr(ignore_from), ptr(d2), ptr(ws), stream()))
    return d2


def boundary_band(mask, radius, ignore_index=None):
    """Device uint8 mask -> bool of the same shape: the labelled pixels within `radius` of a pixel of another class."""
    d2 = boundary_distance(mask, radius, ignore_index)
    return (d2 >= 0) & (d2 <= int(radius) * int(radius))


def border_profile(radius, w0=10.0, sigma=5.0):
    """The weight table of a border-weighted loss, float32 numpy [R*R + 2], indexed by d2: 1 + w0 exp(-d2 / (2 sigma^2))
    for d2 <= R*R (the U-Net paper's profile over one distance), computed in float64 and rounded once; the saturated last cell (no other
    class within R) is 1.  w0 >= 0, sigma > 0."""
    radius = _check_radius(radius)
    w0, sigma = float(w0), float(sigma)
    if not (math.isfinite(w0) and w0 >= 0.0):
        raise ValueError('w0=%r must be a finite number >= 0' % (w0,))
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError('sigma=%r must be a finite number > 0' % (sigma,))
    d2 = np.arange(radius * radius + 2, dtype=np.float64)
    table = 1.0 + w0 * np.exp(-d2 / (2.0 * sigma * sigma))
    table[-1] = 1.0
    return table.astype(np.float32)


def _check_table(table, radius, device):
    """-> contiguous float32 device tensor [R*R + 2] of a numpy array or tensor"""
    cells = radius * radius + 2
    if isinstance(table, np.ndarray):
        table = torch.from_numpy(np.ascontiguousarray(table))
    if not torch.is_tensor(table) or table.dtype != torch.float32 or table.dim() != 1 or table.numel() != cells:
        raise ValueError('a weight table of radius %d must be float32 [%d] (border_profile)' % (radius, cells))
    return table.to(device).contiguous()


def border_weights(mask, radius, table=None, w0=10.0, sigma=5.0, ignore_index=None):
    """Device uint8 [H,W] or [B,H,W] -> float32 of the same shape: table[d2] of boundary_distance(mask, radius, ignore_index), 0 at pixels
    equal to ignore_index -- the per-pixel weights of ops.multiloss(pixel_weights=).  table: float32 [R*R + 2] (numpy or tensor; a device
    tensor is used as it is), by default border_profile(radius, w0, sigma).  Two launches, the int32 distance map is never written."""
    radius, ign = _check_radius(radius), _check_ignore(ignore_index)
    b, h, w = _check_mask(mask)
    if table is None:
        table = border_profile(radius, w0, sigma)
    mask = _on_device(mask, 'a mask')
    table = _check_table(table, radius, mask.device)
    L.init()
    out = torch.empty(mask.shape, device=mask.device, dtype=torch.float32)
    ws = _workspace(b, h, w, mask.device)
    check(lib.pylc_boundary_weights(ptr(mask), b, h, w, radius, ign, ptr(table), ptr(out), ptr(ws), stream()))
    return out


def weights_from_distance(d2, radius, table):
    """border_weights for a distance map that exists: device int32 d2 = boundary_distance(mask, radius, ...) -> float32 table[d2], 0 where
    d2 < 0.  One launch."""
    radius = _check_radius(radius)
    if not torch.is_tensor(d2) or d2.dtype != torch.int32 or d2.numel() == 0 or d2.numel() >= 2 ** 31:
        raise ValueError('a distance map must be a non-empty int32 tensor (boundary_distance)')
    d2 = _on_device(d2, 'd2')
    table = _check_table(table, radius, d2.device)
    L.init()
    out = torch.empty(d2.shape, device=d2.device, dtype=torch.float32)
    check(lib.pylc_weights_from_d2(ptr(d2), d2.numel(), radius, ptr(table), ptr(out), stream()))
    return out


def _check_pair(y_true, y_pred, n_classes, radius, ignore_index, counts):
    c, radius, ign = _check_classes(n_classes), _check_radius(radius), _check_ignore(ignore_index)
    shape = _check_mask(y_true, 'y_true')
    if _check_mask(y_pred, 'y_pred') != shape or y_pred.dim() != y_true.dim():
        raise ValueError('y_pred %s does not match y_true %s' % (tuple(y_pred.shape), tuple(y_true.shape)))
    y_true, y_pred = _on_device(y_true, 'y_true'), _on_device(y_pred, 'y_pred')
    if y_pred.device != y_true.device:
        raise ValueError('y_true and y_pred are on different devices')
    if counts is None:
        counts = torch.zeros(n_cells(c), device=y_true.device, dtype=torch.int64)
    elif (not torch.is_tensor(counts) or counts.dtype != torch.int64 or counts.numel() != n_cells(c) or not counts.is_contiguous()
          or counts.device != y_true.device):
        raise ValueError('counts must be a contiguous int64 tensor of %d entries on the masks\' device' % n_cells(c))
    return y_true, y_pred, shape, c, radius, ign, counts


def boundary_counts(y_true, y_pred, n_classes, radius, ignore_index=None, counts=None):
    """The band counts of a device uint8 mask pair ([H,W] or [B,H,W]) as int64 [C*C + 3C + 1] on the device: ADDED into `counts` when one
    is passed, else into a zeroed one.  Three launches, nothing is read back."""
    y_true, y_pred, (b, h, w), c, radius, ign, counts = _check_pair(y_true, y_pred, n_classes, radius, ignore_index, counts)
    L.init()
    ws = _workspace(b, h, w, y_true.device)
    check(lib.pylc_boundary_counts(ptr(y_true), ptr(y_pred), b, h, w, c, radius, ign, ptr(counts), ptr(ws), stream()))
    return counts


def boundary_counts_from_maps(y_true, y_pred, d2_true, d2_pred, n_classes, radius, ignore_index=None, counts=None):
    """boundary_counts for a pair whose distance maps exist already: d2_true = boundary_distance(y_true, radius, ignore_index), d2_pred =
    boundary_distance(y_pred, radius, ignore_index, ignore_from=y_true).  One launch."""
    y_true, y_pred, _, c, radius, ign, counts = _check_pair(y_true, y_pred, n_classes, radius, ignore_index, counts)
    for d2 in (d2_true, d2_pred):
        if not torch.is_tensor(d2) or d2.dtype != torch.int32 or d2.shape != y_true.shape:
            raise ValueError('a distance map must be an int32 tensor of the masks\' shape (boundary_distance)')
    d2_true, d2_pred = _on_device(d2_true, 'd2_true'), _on_device(d2_pred, 'd2_pred')
    L.init()
    check(lib.pylc_boundary_counts_maps(ptr(y_true), ptr(y_pred), ptr(d2_true), ptr(d2_pred), y_true.numel(), c, radius, ign, ptr(counts),
                                        stream()))
    return counts


def boundary_scores(counts, n_classes):
    """boundary_counts' numbers (device or host) -> {'boundary_iou', 'boundary_iou_mean', 'class_boundary_iou', 'trimap_iou', 'trimap_f1',
    'trimap_mcc', 'band_px'} in host float64.  class_boundary_iou[c] = inter / (gband + pband - inter), 0 where that is 0 / 0;
    boundary_iou is its mean weighted by gband over the classes with gband + pband > 0 (metrics.scores' weighting rule),
    boundary_iou_mean the unweighted mean over the same classes; the trimap scores are metrics.scores of cm_band.  An empty band scores 0.
    Pixels counted outside 0..n_classes-1 are a ValueError."""
    c = _check_classes(n_classes)
    host = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts).reshape(-1)
    if host.size != n_cells(c):
        raise ValueError('counts of %d classes have %d entries, got %d' % (c, n_cells(c), host.size))
    host = host.astype(np.int64)
    outside = int(host[-1])
    if outside:
        raise ValueError('%d pixels hold a truth or prediction outside 0..%d' % (outside, c - 1))
    cm = host[:c * c].reshape(c, c)
    inter, gband, pband = (host[c * c + k * c:c * c + (k + 1) * c].astype(np.float64) for k in range(3))
    union = gband + pband - inter
    iou = np.where(union > 0, inter / np.maximum(union, 1), 0.0)
    present = gband + pband > 0
    w = np.where(present, gband, 0.0)
    band_px = int(cm.sum())
    tri = metrics.scores(cm) if band_px else {'iou': 0.0, 'f1': 0.0, 'mcc': 0.0}
    return {'boundary_iou': float((iou * w).sum() / w.sum()) if w.sum() > 0 else 0.0,
            'boundary_iou_mean': float(iou[present].mean()) if present.any() else 0.0,
            'class_boundary_iou': iou, 'trimap_iou': tri['iou'], 'trimap_f1': tri['f1'], 'trimap_mcc': tri['mcc'], 'band_px': band_px}
