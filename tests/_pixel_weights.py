"""The fp64 statement of the loss head with a weight per pixel, in torch and differentiable: what the GPU suite
(tests/test_pixel_weights_gpu.py) compares pylc_multiloss_stats_w / _bwd_w with, proven in tests/test_cpu_pixel_weights.py against the
statement of the ignore label (tests/test_cpu_ignore_label.masked_multiloss) and against F.cross_entropy."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.test_cpu_ignore_label import valid_pixels


def taking_part(target, u, n_classes, ignore_index):
    """bool [..]: the target is valid (a class index, not the ignore label) and 0 < u <= FLT_MAX"""
    u = torch.as_tensor(u)
    return valid_pixels(target, n_classes, ignore_index) & (u > 0) & (u <= float(np.finfo(np.float32).max))


def weighted_multiloss(logits, target, u, ignore, weights=(0.5, 0.5, 0.5), cw=None):
    """(total, ce, dice, focal) of [B,C,H,W] logits over the pixels of target [B,H,W] that take part, each with its weight u [B,H,W]:

      CE    = sum u w_t (-log p_t) / sum u w_t
      Dice  = mean over all C classes of 1 - (2 I_c + 1) / (sum u p_c + count_c + 1),  I_c = sum u o_c p_c,  count_c = sum u o_c
      Focal = sum u f_n / sum u,  f_n = -0.25 (1 - q)^2 log q,  q = p_t + 1e-8

    Pixels that do not take part are removed (their weight is never multiplied: a NaN weight leaves no trace); with none, everything is 0."""
    c = logits.shape[1]
    z = logits.permute(0, 2, 3, 1).reshape(-1, c)
    t = target.reshape(-1).long()
    u = torch.as_tensor(u).reshape(-1)
    keep = taking_part(t, u, c, ignore)
    z, t, u = z[keep], t[keep], u[keep].to(z.dtype)
    if z.shape[0] == 0:
        zero = logits.sum() * 0
        return zero, zero, zero, zero
    logp = F.log_softmax(z, dim=1)
    p = logp.exp()
    nll = -logp.gather(1, t[:, None])[:, 0]
    w = torch.ones_like(nll) if cw is None else cw.to(z.dtype)[t]
    ce = (u * w * nll).sum() / (u * w).sum()
    onehot = F.one_hot(t, c).to(z.dtype)
    inter = (u[:, None] * p * onehot).sum(0)
    card = (u[:, None] * p).sum(0) + (u[:, None] * onehot).sum(0)
    dsc = (1 - (2 * inter + 1.0) / (card + 1.0)).mean()
    q = p.gather(1, t[:, None])[:, 0] + 1e-8
    fl = (u * (-0.25 * (1 - q) ** 2 * torch.log(q))).sum() / u.sum()
    return weights[0] * ce + weights[1] * dsc + weights[2] * fl, ce, dsc, fl
