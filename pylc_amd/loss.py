"""MultiLoss on the fused HIP loss head -- same constructor, attributes and callables as the reference's
models/modules/loss.py:23-216 (the duck-typed `crit` contract of models/model.py:196-209,317-319,360-362)."""
import numpy as np
import torch
from torch import nn

from . import ops
from .runtime import runtime


class MultiLoss(nn.Module):
    """MultiLoss(loss_weights={'weighted','weights','ce','dice','focal'}, schema={'n_classes','class_codes','class_labels'}, ignore_index=None,
    label_smoothing=0.0, hard_mining=None).

    ignore_index (an int, not in the reference): pixels whose target equals it are left out of all three terms and get a zero gradient;
    targets may then be uint8 or int64.  Any other target outside 0..n_classes-1 is skipped too and counted in `.bad_targets` (an int64
    [1] device tensor, read by Model.log).

    pixel_weights (every callable's optional third argument; not in the reference): a float32 [B,H,W] device map
    u_n, one weight per pixel, e.g. boundary.border_weights(target, ...) or a confidence map.  Each term becomes its u-weighted form
    (CE = sum u w_t nll / sum u w_t, Dice over u-weighted sums, Focal = sum u f / sum u); u_n == 0 leaves the pixel out, negative, NaN
    and infinite weights are left out and counted in `.bad_targets`.  None: the paths without weights, unchanged.

    Soft targets (not in the reference): a float32 4-D `target` [B,C,H,W] is a probability volume -- a row q_n of C
    non-negative numbers per pixel in place of a class index, every term with the one-hot row replaced by q (CE = sum u w_c q_c (-log p_c)
    / sum u w_c q_c, Dice with I_c = sum u p_c q_c and counts sum u q_c, Focal = sum u sum_c q_c f(p_c) / sum u sum_c q_c).  The volume is
    read in place through its strides (a window view of a whole photograph's volume costs no copy) and is used as given: rows are NOT
    renormalised; a row that sums to 0 leaves its pixel out (ignore_index does not apply), a row with a negative, NaN or infinite entry is
    left out and counted in `.bad_targets`.  distill(pred, teacher_logits, temperature) takes q = softmax(teacher_logits / temperature)
    in the kernel.  label_smoothing (0 <= eps < 1) smooths HARD targets in forward() only, q_c = (1 - eps) o_c + eps / C; ce_loss,
    dice_loss, focal_loss and all_losses -- the validation terms -- stay unsmoothed.

    hard_mining (not in the reference): None, or {'keep':, 'min_kept':, 'thresh':} with every key optional and at
    least one of keep (a fraction in (0, 1]: bootstrapped / top-k cross-entropy) and thresh (a probability in (0, 1): OHEM) present.  In
    forward() only and on hard targets only, mining.hard_pixel_weights(pred, target, ...) -- computed from the detached logits and from the
    pixel_weights that were passed -- takes the place of those pixel_weights, and the call goes on as forward(pred, target, mined_map) does;
    label_smoothing applies as it does to any weighted call.  A pixel weight is one factor on EVERY term, so all three terms see the
    mined map, Dice and Focal included: for mining on the cross-entropy alone set the other two loss weights to 0.  The pixels are ranked
    by the plain -log p_t, not by the class-weighted loss.  ce_loss, dice_loss, focal_loss, all_losses and distill stay unmined; a soft
    target together with hard_mining raises ValueError (the ranking needs a class index).  `.mined` holds the last call's info tensor
    (int64 [4], device: candidates, k, kept pixels, the bits of the threshold).

    forward(pred, target) -> 0-d tensor (ce_w*CE + dice_w*Dice + focal_w*Focal) with grad; side effects
    .ce / .dsc / .fl hold the three terms (loss.py:107-112).  One kernel pass computes all three."""

    def __init__(self, loss_weights, schema, ignore_index=None, label_smoothing=0.0, hard_mining=None):
        super().__init__()
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.label_smoothing = float(label_smoothing)
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError('label_smoothing must lie in [0, 1), got %r' % (label_smoothing,))
        from . import mining
        self.hard_mining = mining.check_spec(hard_mining)
        self.mined = None
        self.bad_targets = None
        self.n_classes = schema['n_classes']
        self.codes = schema.get('class_codes')
        self.categories = schema.get('class_labels')
        self.weighted = bool(loss_weights['weighted'])
        w = loss_weights.get('weights')
        # the reference crashes on weights=None (loss.py:46,60-61); here None means uniform weights
        w = np.ones(self.n_classes, np.float32) if w is None else np.asarray(w, np.float32)
        if w.shape != (self.n_classes,):
            raise ValueError('class weights must have length n_classes=%d' % self.n_classes)
        self.register_buffer('weights', torch.from_numpy(w.copy()))
        self.dsc_weight = float(loss_weights['dice'])
        self.ce_weight = float(loss_weights['ce'])
        self.fl_weight = float(loss_weights['focal'])
        self.eps = 1e-8
        self.ce = self.dsc = self.fl = 0.

    def _check(self, pred, target):
        if not torch.is_tensor(pred):
            raise TypeError('Input type is not a torch.Tensor. Got {}'.format(type(pred)))
        if pred.dim() != 4 or pred.size(1) != self.n_classes:
            raise ValueError('Invalid input shape, we expect Bx{}xHxW. Got: {}'.format(self.n_classes, tuple(pred.shape)))
        if pred.size(0) != target.size(0) or pred.size(2) != target.size(1) or pred.size(3) != target.size(2):
            raise ValueError('Expected prediction {} to match target {}.'.format(tuple(pred.shape), tuple(target.shape)))
        if pred.device != target.device:
            raise ValueError('input and target must be in the same device. Got: {} and {}'.format(pred.device, target.device))

    def _bad(self, pred):
        if self.bad_targets is None or self.bad_targets.device != pred.device:
            self.bad_targets = torch.zeros(1, dtype=torch.int64, device=pred.device)
        return self.bad_targets

    def _all(self, pred, target, w_ce, w_d, w_f, pixel_weights=None, smoothing=0.0):
        if torch.is_tensor(target) and target.dim() == 4 and target.is_floating_point():
            return self._soft(pred, target, 'probs', 1.0, w_ce, w_d, w_f, pixel_weights)
        self._check(pred, target)
        cw = self.weights if self.weighted else None
        if smoothing != 0.0:
            return ops.multiloss(pred, target, cw, w_ce, w_d, w_f, runtime.sync_group, self.ignore_index, self._bad(pred), pixel_weights,
                                 label_smoothing=smoothing)
        if self.ignore_index is None and pixel_weights is None:
            return ops.multiloss(pred, target, cw, w_ce, w_d, w_f, runtime.sync_group)
        return ops.multiloss(pred, target, cw, w_ce, w_d, w_f, runtime.sync_group, self.ignore_index, self._bad(pred), pixel_weights)

    def _soft(self, pred, soft, kind, temperature, w_ce, w_d, w_f, pixel_weights=None):
        if not torch.is_tensor(pred):
            raise TypeError('Input type is not a torch.Tensor. Got {}'.format(type(pred)))
        if pred.dim() != 4 or pred.size(1) != self.n_classes:
            raise ValueError('Invalid input shape, we expect Bx{}xHxW. Got: {}'.format(self.n_classes, tuple(pred.shape)))
        if not torch.is_tensor(soft) or soft.dtype != torch.float32 or tuple(soft.shape) != tuple(pred.shape):
            raise ValueError('Expected a float32 soft target of the prediction\'s shape {}. Got: {}'.format(
                tuple(pred.shape), (soft.dtype, tuple(soft.shape)) if torch.is_tensor(soft) else type(soft)))
        if pred.device != soft.device:
            raise ValueError('input and target must be in the same device. Got: {} and {}'.format(pred.device, soft.device))
        cw = self.weights if self.weighted else None
        return ops.multiloss(pred, None, cw, w_ce, w_d, w_f, runtime.sync_group, None, self._bad(pred), pixel_weights, soft_target=soft,
                             soft_kind=kind, temperature=temperature)

    def forward(self, pred, target, pixel_weights=None):
        if self.hard_mining is not None:
            if torch.is_tensor(target) and target.dim() == 4 and target.is_floating_point():
                raise ValueError('hard_mining ranks pixels by the loss of their class index: it cannot be combined with a soft target')
            from . import mining
            self._check(pred, target)
            pixel_weights, self.mined = mining.hard_pixel_weights(pred, target, ignore_index=self.ignore_index, pixel_weights=pixel_weights,
                                                                  **self.hard_mining)
        losses = self._all(pred, target, self.ce_weight, self.dsc_weight, self.fl_weight, pixel_weights, self.label_smoothing)
        self.ce, self.dsc, self.fl = losses[1].detach(), losses[2].detach(), losses[3].detach()
        return losses[0]

    def distill(self, pred, teacher_logits, temperature=1.0, pixel_weights=None):
        """forward() against q = softmax(teacher_logits / temperature), float32 [B,C,H,W] read in place and softened in the kernel.  Only
        the teacher is softened: pred is not divided by the temperature and the loss is not multiplied by its square."""
        losses = self._soft(pred, teacher_logits, 'logits', temperature, self.ce_weight, self.dsc_weight, self.fl_weight, pixel_weights)
        self.ce, self.dsc, self.fl = losses[1].detach(), losses[2].detach(), losses[3].detach()
        return losses[0]

    # the validation path calls the three terms separately (model.py:360-362)
    def ce_loss(self, pred, target, pixel_weights=None):
        return self._all(pred, target, 1.0, 0.0, 0.0, pixel_weights)[0]

    def dice_loss(self, pred, target, pixel_weights=None):
        return self._all(pred, target, 0.0, 1.0, 0.0, pixel_weights)[0]

    def focal_loss(self, pred, target, pixel_weights=None):
        return self._all(pred, target, 0.0, 0.0, 1.0, pixel_weights)[0]

    def all_losses(self, pred, target, pixel_weights=None):
        """(total, ce, dice, focal) as one [4] tensor from a single pass."""
        return self._all(pred, target, self.ce_weight, self.dsc_weight, self.fl_weight, pixel_weights)

    def print_settings(self):
        hline = '_' * 40
        print('{:30s}{:<10s}'.format('Loss', 'Weight'))
        print(hline)
        print('{:30s}{:<10f}'.format('Cross-entropy', self.ce_weight))
        print('\tCE losses {}weighted by class.'.format('' if self.weighted else 'not '))
        print('{:30s}{:<10f}'.format('Dice Coefficient', self.dsc_weight))
        print('{:30s}{:<10f}'.format('Focal Loss', self.fl_weight))
        if self.codes and self.categories:
            print('\n{:8s}{:22s}{:<10s}'.format('Class', 'Label', 'Weight'))
            print(hline)
            for i, w in enumerate(self.weights.tolist()):
                print('{:8s}{:22s}{:<10f}'.format(str(self.codes[i]), str(self.categories[i]), w))
