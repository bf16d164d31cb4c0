"""The fp64 statement of the loss head against soft targets, in torch and differentiable: what the GPU suite
(tests/test_soft_targets_gpu.py) compares pylc_multiloss_*_soft / _ls with, proven in tests/test_cpu_soft_targets.py against
F.cross_entropy with probability targets and label smoothing, against the statement of the pixel weights on one-hot rows, and against the
closed-form gradient."""
import numpy as np
import torch
import torch.nn.functional as F

FLT_MAX = float(np.finfo(np.float32).max)


def _rows(x):
    """[B,C,H,W] -> [N,C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def bad_rows(q):
    """bool [N] of q [B,C,H,W]: a row with a negative, NaN or infinite entry (skipped AND counted)"""
    r = _rows(torch.as_tensor(q))
    return ~((r >= 0) & (r <= FLT_MAX)).all(1)


def taking_part(q, u=None):
    """bool [N] of q [B,C,H,W] and u [B,H,W] (None: ones): every entry of the row is finite and >= 0, the row's sum is > 0, and
    0 < u <= FLT_MAX"""
    r = _rows(torch.as_tensor(q))
    ok = ~bad_rows(q)
    ok = ok & (torch.where(ok[:, None], r, torch.zeros_like(r)).double().sum(1) > 0)
    if u is not None:
        u = torch.as_tensor(u).reshape(-1)
        ok = ok & (u > 0) & (u <= FLT_MAX)
    return ok


def smoothed_rows(t, n_classes, eps, ignore):
    """float64 [B,C,H,W]: (1 - eps) one_hot(t) + eps / C of a hard target t [B,H,W], with eps as the float32 the kernel receives; a pixel
    that is ignored or out of range gets a row of zeros, which takes no part"""
    e = float(np.float32(eps))
    t = t.long()
    valid = (t >= 0) & (t < n_classes)
    if ignore is not None:
        valid = valid & (t != ignore)
    onehot = F.one_hot(torch.where(valid, t, torch.zeros_like(t)), n_classes).double()
    q = (1.0 - e) * onehot + e / n_classes
    return (q * valid[..., None]).permute(0, 3, 1, 2)


def teacher_rows(t, temperature):
    """float64 [B,C,H,W]: softmax(inv_T * t) over the classes with inv_T = 1 / temperature as the float32 the kernel receives; a pixel
    with a non-finite inv_T * t entry gets a row of NaN (a bad row)"""
    inv = float(np.float32(1.0 / float(temperature)))
    s = t.double() * inv
    fine = (s.float().abs() <= FLT_MAX).all(1, keepdim=True)
    q = torch.softmax(torch.where(fine, s, torch.zeros_like(s)), dim=1)
    return torch.where(fine, q, torch.full_like(q, float('nan')))


def soft_multiloss(z, q, u=None, weights=(0.5, 0.5, 0.5), cw=None):
    """(total, ce, dice, focal) of [B,C,H,W] logits z against the rows q [B,C,H,W] over the pixels that take part, each with its weight
    u [B,H,W] (None: 1), with p = softmax(z), x = p + 1e-8, f(x) = -0.25 (1 - x)^2 log x:

      CE    = sum_n sum_c u w_c q_c (-log p_c) / sum_n sum_c u w_c q_c
      Dice  = mean over the C classes of 1 - (2 I_c + 1) / (sum u p_c + sum u q_c + 1),  I_c = sum u p_c q_c
      Focal = sum_n u sum_c q_c f(x_c) / sum_n u sum_c q_c

    q is used as given (never renormalised) and carries no gradient.  Pixels that take no part are removed; with none, everything is 0."""
    c = z.shape[1]
    keep = taking_part(q, u)
    zr = _rows(z)[keep]
    qr = _rows(torch.as_tensor(q))[keep].to(zr.dtype).detach()
    ur = torch.ones(zr.shape[0], dtype=zr.dtype) if u is None else torch.as_tensor(u).reshape(-1)[keep].to(zr.dtype)
    if zr.shape[0] == 0:
        zero = z.sum() * 0
        return zero, zero, zero, zero
    logp = F.log_softmax(zr, dim=1)
    p = logp.exp()
    w = torch.ones(c, dtype=zr.dtype) if cw is None else cw.to(zr.dtype)
    uwq = ur[:, None] * w[None, :] * qr
    ce = (uwq * -logp).sum() / uwq.sum()
    up = ur[:, None] * p
    uq = ur[:, None] * qr
    inter = (up * qr).sum(0)
    card = up.sum(0) + uq.sum(0)
    dsc = (1 - (2 * inter + 1.0) / (card + 1.0)).mean()
    x = p + 1e-8
    fl = (uq * (-0.25 * (1 - x) ** 2 * torch.log(x))).sum() / uq.sum()
    return weights[0] * ce + weights[1] * dsc + weights[2] * fl, ce, dsc, fl
