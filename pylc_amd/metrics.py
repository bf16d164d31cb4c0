"""Evaluation scores on the GPU: one confusion-matrix kernel over the class-index masks, then the reference's scores
(utils/metrics.py:64-88 via sklearn: weighted F1, weighted Jaccard = the headline "mIoU", Matthews correlation,
row-normalised confusion matrix) as closed forms of the n_cls x n_cls count matrix -- instead of several sklearn passes
over ~1e7-pixel flattened host arrays (utils/evaluate.py:131-176)."""
import numpy as np
import torch

from . import lib as L
from .lib import lib, check, ptr, stream


def confusion_matrix(y_true, y_pred, n_classes, force_coverage=True, ignore_index=None, skipped=None):
    """int64 [n_classes, n_classes] counts (device) for uint8 / int64 masks of equal size.  With ignore_index, pixels whose true label
    equals it or lies outside 0..n_classes-1 are left out; `skipped` (int64 [2] device tensor, optional) has their numbers (out of
    range, ignored) ADDED into it."""
    L.init()
    yt, yp = y_true.contiguous().reshape(-1), y_pred.contiguous().reshape(-1)
    if yt.numel() != yp.numel():
        raise ValueError('mask sizes differ: %d vs %d' % (yt.numel(), yp.numel()))
    for t in (yt, yp):
        if t.dtype not in (torch.uint8, torch.int64):
            raise TypeError('masks must be uint8 or int64 class indices, got %s' % t.dtype)
    cm = torch.zeros(n_classes * n_classes, device=yt.device, dtype=torch.int64)
    if ignore_index is None:
        if skipped is not None:
            raise ValueError('skipped counts need an ignore_index')
        check(lib.pylc_confusion_matrix(ptr(yt), yt.element_size(), ptr(yp), yp.element_size(), yt.numel(), n_classes,
                                        int(force_coverage), ptr(cm), stream()))
    else:
        if skipped is not None and (skipped.dtype != torch.int64 or skipped.numel() != 2 or not skipped.is_contiguous()):
            raise ValueError('skipped must be a contiguous int64 tensor of 2 entries')
        check(lib.pylc_confusion_matrix_ex(ptr(yt), yt.element_size(), ptr(yp), yp.element_size(), yt.numel(), n_classes,
                                           int(force_coverage), ptr(cm), int(ignore_index), ptr(skipped), stream()))
    return cm.view(n_classes, n_classes)


def scores(cm):
    """{'f1', 'iou', 'mcc', 'cmatrix'} from a count matrix (host float64 arithmetic on n_cls^2 numbers)."""
    cm = np.asarray(cm.cpu() if torch.is_tensor(cm) else cm, np.float64)
    tp, support, predicted, n = np.diag(cm), cm.sum(1), cm.sum(0), cm.sum()
    w = np.where((support + predicted) > 0, support, 0.0)
    f1 = np.where(support + predicted > 0, 2 * tp / np.maximum(support + predicted, 1), 0.0)           # zero_division=0
    iou = np.where(support + predicted - tp > 0, tp / np.maximum(support + predicted - tp, 1), 0.0)
    c_tp, c_pp, c_tt = tp.sum() * n - (support * predicted).sum(), n * n - (predicted ** 2).sum(), n * n - (support ** 2).sum()
    mcc = 0.0 if c_pp * c_tt == 0 else c_tp / np.sqrt(c_tt * c_pp)
    norm = np.divide(cm, support[:, None], out=np.zeros_like(cm), where=support[:, None] > 0)
    return {'f1': float((f1 * w).sum() / w.sum()), 'iou': float((iou * w).sum() / w.sum()), 'mcc': float(mcc), 'cmatrix': norm}


def evaluate(y_true, y_pred, n_classes, ignore_index=None):
    """Evaluator.evaluate() (utils/evaluate.py:131-148) minus the plotting / report printing; with ignore_index, over the pixels whose true
    label is a class other than it."""
    return scores(confusion_matrix(y_true, y_pred, n_classes, force_coverage=True, ignore_index=ignore_index))


# ---- validation scores while training: logits -> counts in one launch (csrc/score.hip) ---------------------------
def logits_confusion(logits, target=None, counts=None, return_mask=False, ignore_index=None):
    """Confusion counts (and / or the class mask) of a batch of logits [B,C,H,W] as a net returns them, in ONE launch and without a host
    synchronisation: the class of a pixel is the first maximum of its logits (numpy's argmax).  target [B,H,W], uint8 or int64 class
    indices: counts[t * C + p] += 1, and counts[C * C] counts the pixels whose target lies outside 0..C-1.  `counts` (int64 [C*C + 1],
    device) is ADDED into; a zeroed one is allocated when none is passed.  Returns counts (None without a target), or (counts, mask) with
    return_mask, mask uint8 [B,H,W].  With ignore_index, counts has C*C + 2 entries: a target equal to the index adds to counts[C*C + 1]
    (and not to the matrix, even for an index inside 0..C-1), counts[C*C] keeps the other out-of-range ones."""
    from . import ops
    L.init()
    if logits.dim() != 4:
        raise ValueError('expected [B,C,H,W] logits, got %s' % (tuple(logits.shape),))
    b, c, h, w = logits.shape
    n = b * h * w
    if target is None and counts is not None:
        raise ValueError('counts need a target')
    if target is None and not return_mask:
        raise ValueError('neither a target nor return_mask: nothing to compute')
    x = ops.as_nhwc(logits)
    pitch = ops.pitch_of(x)
    tbytes = 0
    if target is not None:
        if target.dtype not in (torch.uint8, torch.int64):
            raise TypeError('target must be uint8 or int64 class indices, got %s' % target.dtype)
        if target.numel() != n:
            raise ValueError('target %s does not match logits %s' % (tuple(target.shape), tuple(logits.shape)))
        target = target.to(x.device, non_blocking=True).contiguous()
        tbytes = target.element_size()
        cells = c * c + (1 if ignore_index is None else 2)
        if counts is None:
            counts = torch.zeros(cells, device=x.device, dtype=torch.int64)
        elif counts.dtype != torch.int64 or counts.numel() != cells or not counts.is_contiguous():
            raise ValueError('counts must be a contiguous int64 tensor of %d entries' % cells)
    mask = torch.empty((b, h, w), device=x.device, dtype=torch.uint8) if return_mask else None
    if ignore_index is None or target is None:
        check(lib.pylc_logits_score(ptr(x), pitch, ptr(target), tbytes, n, c, ptr(mask), ptr(counts), stream()))
    else:
        check(lib.pylc_logits_score_ex(ptr(x), pitch, ptr(target), tbytes, n, c, ptr(mask), int(ignore_index), ptr(counts), stream()))
    return (counts, mask) if return_mask else counts


def per_class(cm):
    """{'iou', 'f1', 'support'}: [C] arrays of a count matrix, with scores()'s zero-division rules (a class neither present nor predicted
    scores 0); scores()'s 'iou' and 'f1' are their support-weighted means."""
    cm = np.asarray(cm.cpu() if torch.is_tensor(cm) else cm, np.float64)
    tp, support, predicted = np.diag(cm), cm.sum(1), cm.sum(0)
    f1 = np.where(support + predicted > 0, 2 * tp / np.maximum(support + predicted, 1), 0.0)
    iou = np.where(support + predicted - tp > 0, tp / np.maximum(support + predicted - tp, 1), 0.0)
    return {'iou': iou, 'f1': f1, 'support': support}


class ScoreLog:
    """Validation scores next to the loss log: add() accumulates the confusion counts of every validation batch on the device (one launch,
    no host read), close() turns them into one row per validation pass -- the only D2H copy -- and tracks the best weighted IoU."""

    def __init__(self, n_classes, ignore_index=None, boundary_radius=None, calibration_bins=None):
        self.n_classes = int(n_classes)
        self.ignore_index = None if ignore_index is None else int(ignore_index)      # targets equal to it are dropped and reported as 'ignored'
        # with a radius, add() also counts the band along class borders (boundary.boundary_counts on the mask of the same launch) and the
        # rows gain 'boundary_iou', 'trimap_iou' and 'class_boundary_iou' (DESIGN.md 5.14); without one nothing changes
        self.boundary_radius = None
        if boundary_radius is not None:
            from . import boundary
            self.boundary_radius = boundary._check_radius(boundary_radius)
            boundary._check_classes(self.n_classes)
            boundary._check_ignore(self.ignore_index)
        self.boundary_counts = None        # int64 [C*C + 3C + 1], allocated with `counts`
        # with bins, add() also takes the batch's reliability counts at temperature 1 (one launch) and its NLL on calibration.default_betas()
        # (33 betas: two launches), and the rows gain 'ece', 'mce', 'nll', 'class_ece' and the pass's fitted 'temperature' (DESIGN.md 5.20);
        # without, nothing changes
        self.calibration_bins = None
        self.reliability_counts = None     # int64 [3*C*bins + 3]
        self.nll_sums = None               # float64 [len(betas)]
        self.nll_tail = None               # int64 [3]
        if calibration_bins is not None:
            self.set_calibration(calibration_bins)
        self.counts = None                 # int64 [C*C + 1] (+ 1 with an ignore label), allocated where the first logits live
        self.last_counts = None            # host int64 [C,C] of the last closed pass (summed over the group)
        self.rows = []
        self.best_iou, self.is_best = 0.0, False

    def _zeros(self, device):
        return torch.zeros(self.n_classes * self.n_classes + (1 if self.ignore_index is None else 2), device=device, dtype=torch.int64)

    def set_calibration(self, bins):
        """Switch the calibration rows on for the passes to come (a log taken up from a checkpoint starts without them)."""
        from . import calibration
        self.calibration_bins = calibration._check_bins(bins)
        self.betas = calibration.default_betas()
        self.reliability_counts = self.nll_sums = self.nll_tail = None

    def _calibration_zeros(self, device):
        from . import calibration
        self.reliability_counts = torch.zeros(calibration.n_cells(self.n_classes, self.calibration_bins), device=device, dtype=torch.int64)
        self.nll_sums = torch.zeros(len(self.betas), device=device, dtype=torch.float64)
        self.nll_tail = torch.zeros(3, device=device, dtype=torch.int64)

    def add(self, logits, target):
        if logits.shape[1] != self.n_classes:
            raise ValueError('ScoreLog of %d classes got logits with %d' % (self.n_classes, logits.shape[1]))
        if self.counts is None:
            self.counts = self._zeros(logits.device)
        if self.calibration_bins is not None:
            from . import calibration
            if self.reliability_counts is None:
                self._calibration_zeros(logits.device)
            calibration.logits_reliability(logits, target, self.calibration_bins, counts=self.reliability_counts, ignore_index=self.ignore_index)
            calibration.nll_grid(logits, target, self.betas, self.ignore_index, sums=self.nll_sums, tail=self.nll_tail)
        if self.boundary_radius is None:
            logits_confusion(logits, target, counts=self.counts, ignore_index=self.ignore_index)
            return
        from . import boundary
        _, mask = logits_confusion(logits, target, counts=self.counts, return_mask=True, ignore_index=self.ignore_index)
        if self.boundary_counts is None:
            self.boundary_counts = torch.zeros(boundary.n_cells(self.n_classes), device=mask.device, dtype=torch.int64)
        # (a target outside 0..255 wraps here; the launch above has counted it in the out-of-range cell, which close() raises on)
        truth = target.to(mask.device, non_blocking=True).reshape(mask.shape).to(torch.uint8)
        boundary.boundary_counts(truth, mask, self.n_classes, self.boundary_radius, self.ignore_index, counts=self.boundary_counts)

    def close(self, it, epoch, group=None):
        """End of a validation pass: the counts (summed over `group` when given -- a collective every rank must reach) become a row
        {'iter', 'epoch', 'f1', 'iou', 'mcc', 'class_iou', 'class_f1', 'support'} (with an ignore label also 'ignored', the number of
        dropped pixels; with a boundary radius also 'boundary_iou', 'trimap_iou', 'class_boundary_iou'); the device counts are zeroed
        for the next pass.  With calibration bins the row also has 'ece', 'mce', 'class_ece', 'nll' (the mean negative log-likelihood at
        temperature 1) and 'temperature' (calibration.fit_temperature of this pass; the grid's end when the minimum lies outside it).
        Returns the row, or None when no valid pixel was added."""
        c = self.n_classes
        if self.counts is None:
            self.counts = self._zeros('cpu')           # a rank that saw no batch still takes part in the collective
        if group is not None:
            from .runtime import runtime
            runtime.sync_all_reduce(self.counts, group)           # int64: carried by the torch group (the native communicator takes floats)
        bhost = None
        if self.boundary_radius is not None:
            from . import boundary
            if self.boundary_counts is None:
                self.boundary_counts = torch.zeros(boundary.n_cells(c), device=self.counts.device, dtype=torch.int64)
            if group is not None:
                runtime.sync_all_reduce(self.boundary_counts, group)
            bhost = self.boundary_counts.to('cpu', copy=True)
            self.boundary_counts.zero_()
        rhost = None
        if self.calibration_bins is not None:
            if self.reliability_counts is None:
                self._calibration_zeros(self.counts.device)
            if group is not None:                                   # int64 and fp64: carried by the torch group, as the confusion counts
                for t in (self.reliability_counts, self.nll_sums, self.nll_tail):
                    runtime.sync_all_reduce(t, group)
            rhost = [t.to('cpu', copy=True) for t in (self.reliability_counts, self.nll_sums, self.nll_tail)]
            for t in (self.reliability_counts, self.nll_sums, self.nll_tail):
                t.zero_()
        host = self.counts.to('cpu', copy=True)                    # the one D2H copy of a validation pass (two with a boundary radius)
        self.counts.zero_()
        outside = int(host[c * c])
        if outside:
            raise ValueError('%d validation targets lie outside 0..%d' % (outside, c - 1))
        cm = host[:c * c].view(c, c).clone()
        self.last_counts = cm
        if int(cm.sum()) == 0:
            self.is_best = False
            return None
        s, pc = scores(cm), per_class(cm)
        row = {'iter': int(it), 'epoch': int(epoch), 'f1': s['f1'], 'iou': s['iou'], 'mcc': s['mcc'],
               'class_iou': [float(v) for v in pc['iou']], 'class_f1': [float(v) for v in pc['f1']], 'support': [int(v) for v in pc['support']]}
        if self.ignore_index is not None:
            row['ignored'] = int(host[c * c + 1])
        if bhost is not None:
            b = boundary.boundary_scores(bhost, c)
            row.update(boundary_iou=b['boundary_iou'], trimap_iou=b['trimap_iou'], class_boundary_iou=[float(v) for v in b['class_boundary_iou']])
        if rhost is not None:
            from . import calibration
            r = calibration.reliability_scores(rhost[0], c, self.calibration_bins)
            fit = calibration.fit_temperature(self.betas, rhost[1], int(rhost[2][0]))
            row.update(ece=r['ece'], mce=r['mce'], class_ece=[float(v) for v in r['class_ece']], nll=fit['nll_at_1'],
                       temperature=fit['temperature'])
        self.rows.append(row)
        self.is_best = row['iou'] > self.best_iou
        if self.is_best:
            self.best_iou = row['iou']
        return row

    def save(self, path):
        import json
        import os
        tmp = path + '.tmp.%d' % os.getpid()
        with open(tmp, 'w') as f:
            json.dump({'n_classes': self.n_classes, 'best_iou': float(self.best_iou), 'rows': self.rows}, f)
        os.replace(tmp, path)

    def load(self, path):
        """Take up rows and best_iou from a file written by save(); False when there is none."""
        import json
        import os
        if not os.path.exists(path):
            return False
        with open(path) as f:
            data = json.load(f)
        if int(data['n_classes']) != self.n_classes:
            raise ValueError('%s holds scores of %d classes, this log has %d' % (path, data['n_classes'], self.n_classes))
        self.rows, self.best_iou, self.is_best = list(data['rows']), float(data['best_iou']), False
        return True
