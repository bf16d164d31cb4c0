"""Epoch driver of the HIP path -- the counterpart of the reference's train.py:72-156 loop body (train_epoch, validate,
StepLR stepping, checkpoint on every validation + best-model copy on a new best validation Dice).  The CLI / HDF5 set-up
above that loop (train.py:22-70) is out of scope: callers pass any re-iterable of (img, mask) batches, e.g. a list or a
factory returning a pylc_amd.data.TileFeeder."""
import os

import torch


def _batches(src):
    return src() if callable(src) else src


def train_epoch(model, batches):
    """train.py:95-122."""
    model.net.train()
    for x, y in _batches(batches):
        model.train(x, y)
    return model


def validate(model, batches, save_dir=None):
    """train.py:125-156: eval-mode pass, log, checkpoint."""
    model.net.eval()
    with torch.no_grad():
        for x, y in _batches(batches):
            model.eval(x, y)
        model.log()
        if save_dir is not None:
            model.save(save_dir)
    return model


def _validate_calibrated(model, batches, save_dir, calibrated):
    """validate(); with calibration, the pass's fitted temperature goes into model.meta.temperature before the checkpoint is written."""
    if not calibrated:
        return validate(model, batches, save_dir)
    validate(model, batches, None)
    rows = model.scores.rows
    if rows and rows[-1].get('iter') == model.iter and rows[-1].get('temperature') is not None:
        model.meta.temperature = float(rows[-1]['temperature'])
    if save_dir is not None:
        model.save(save_dir)
    return model


def trainer(model, train_batches, valid_batches, n_epochs, save_dir=None, score=False, best_by='dice', boundary_radius=None,
            calibration_bins=None):
    """train.py:72-92, including its resume quirk `range(offset, n_epochs - offset)`.
    score: every validation pass also logs weighted F1 / IoU / MCC and the per-class scores (metrics.ScoreLog -> scores.json next to
    losses.pth); best_by: 'dice' (the reference's rule) or 'iou' (needs score) picks what the best-model copy follows.
    boundary_radius (needs score): the rows also carry boundary IoU and the trimap IoU of the band of that many pixels.
    calibration_bins (needs score): the rows also carry 'ece', 'mce', 'nll', 'class_ece' and the pass's fitted 'temperature' (DESIGN.md 5.20),
    which is stored in model.meta.temperature after every validation pass (and so in the checkpoints) for temperature='meta' at inference."""
    if boundary_radius is not None and not score:
        raise ValueError('boundary_radius needs score=True')
    if calibration_bins is not None and not score:
        raise ValueError('calibration_bins needs score=True')
    if score and model.scores is None:
        from .metrics import ScoreLog
        model.scores = ScoreLog(model.meta.n_classes, getattr(model.meta, 'ignore_index', None), boundary_radius=boundary_radius,
                                calibration_bins=calibration_bins)
    calibrated = calibration_bins is not None
    if calibrated and model.scores.calibration_bins != calibration_bins:          # a log that a resume or the caller made without them
        model.scores.set_calibration(calibration_bins)
    model.best_by = best_by
    model.net.train()
    offset = model.epoch
    for epoch in range(offset, n_epochs - offset):
        model.loss.lr += [(model.iter, model.get_lr())]
        if epoch == 0:
            _validate_calibrated(model, valid_batches, save_dir, calibrated)
        train_epoch(model, train_batches)
        _validate_calibrated(model, valid_batches, save_dir, calibrated)
        model.sched.step()
        model.epoch += 1
    return model
