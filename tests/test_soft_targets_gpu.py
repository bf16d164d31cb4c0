"""Soft targets in the loss head on the GPU (-m gpu): pylc_multiloss_stats_soft / _bwd_soft (a probability volume or
teacher logits, read through four strides) and pylc_multiloss_stats_ls / _bwd_ls (a smoothed hard target) with pylc_multiloss_finalize_ex, on
the inputs of tests/test_ignore_label_gpu.py.

  1  against the fp64 statement tests/_soft_targets.soft_multiloss within the bounds the project holds this kernel family to: 2e-6 max(1, |x|)
     per loss term, 1e-5 of the largest gradient entry, 1e-6 on the sum of the class counts.  The per-pixel arithmetic adds at most C fp32
     roundings to terms no larger than before and a thread still adds at most two pixels, so the bounds are conditions, not new numbers.
  2  layouts: planar, channels-last at pitch C and round4(C), a batch slice, a base offset of one float, a row of windows of a larger [C,H,W]
     volume -- each equal to its contiguous copy bit for bit.
  3  the one-hot limit: a one-hot volume and _ls with smoothing 0 give the statistics and the four losses of _w bit for bit.
  4  validity: bad rows skipped and counted, an all-zero volume gives exact zeros, logits of +-80 stay finite.
  5  two shards with very different sum u q.
  6  the Python layers against the C ABI, bit for bit; opcheck; the defaults stay on the present path.
  7  Model.train with soft targets, teacher logits and Meta.label_smoothing on a U-Net (cropped target) and DeepLab/ResNet-101.

Every comparison with a bound prints its figures next to it (lines `ST1` .. `ST7` under `pytest -s`)."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _data as D
from tests._soft_targets import bad_rows, smoothed_rows, soft_multiloss, taking_part, teacher_rows
from tests.test_cpu_ignore_label import ignore_blobs, masked_multiloss
from tests.test_ignore_label_gpu import (CLASS_COUNTS, GRAD_REL, HALF, LOSS_REL, SHAPES, _as_target, _check_rows, _ex, _grad_nchw, _logits,
                                         _loss_err, _pitches, _rows, _target, r4)
from tests.test_ops_gpu import rel_err
from tests.test_pixel_weights_gpu import COUNT_REL, NO_IGNORE, _same, _w, _weights

pytestmark = pytest.mark.gpu

TEMPERATURES = (0.5, 1.0, 1.7)
SMOOTHINGS = (0.05, 0.2)


# ---- inputs and the fp64 statement, computed once and only read ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _volume(shape_id, c, kind):
    """float32 [B,C,H,W]: 'dirichlet' rows of gamma(0.5) variates divided by their sum in float32 (Dirichlet-like; sums are 1 up to
    rounding and are used as they are), 'zero_rows' the same with about 30 % all-zero rows in blobs, 'teacher' logits of scale 2,
    'onehot' the one-hot rows of the 'blobs30' target with all-zero rows where it is ignored"""
    b, h, w = SHAPES[shape_id]
    rs = np.random.RandomState(950 + c + b * h)
    if kind == 'teacher':
        return torch.from_numpy((rs.standard_normal((b, c, h, w)) * 2).astype(np.float32))
    if kind == 'onehot':
        return smoothed_rows(_target(shape_id, c, 'blobs30', 255), c, 0.0, 255).float().contiguous()
    g = rs.gamma(0.5, 1.0, (b, c, h, w)).astype(np.float32) + np.float32(1e-6)
    q = torch.from_numpy(g / g.sum(1, keepdims=True, dtype=np.float32))
    if kind == 'zero_rows':
        cell = 2 if h < 16 else 4 if h < 100 else 16
        q = q * (~ignore_blobs(951 + c, (b, h, w), 0.3, cell=cell))[:, None].float()
    return q.contiguous()


def _source_rows(shape_id, c, source):
    """the rows q [B,C,H,W] the kernel is to see, in float64, for a source ('probs', volume kind) / ('logits', T) / ('ls', eps, ignore)"""
    if source[0] == 'probs':
        return _volume(shape_id, c, source[1]).double()
    if source[0] == 'logits':
        return teacher_rows(_volume(shape_id, c, 'teacher'), source[1])
    return smoothed_rows(_target(shape_id, c, 'blobs30', source[2]), c, source[1], source[2])


@functools.lru_cache(maxsize=None)
def _want(shape_id, c, source, kind_u, weighted):
    """the statement in fp64: ([total, ce, dice, focal], d total / d logits, bool [N] taking part, sum u q)"""
    z, q = _logits(shape_id, c), _source_rows(shape_id, c, source)
    u = None if kind_u is None else _weights(shape_id, c, kind_u)
    cw = torch.from_numpy(D.class_weights(c)).double() if weighted else None
    zr = z.double().requires_grad_(True)
    out = soft_multiloss(zr, q, u, HALF, cw)
    out[0].backward()
    part = taking_part(q, u)
    qr = q.permute(0, 2, 3, 1).reshape(-1, c)[part]
    sum_uq = float((qr.sum(1) * (1.0 if u is None else u.reshape(-1)[part].double())).sum())
    return [v.item() for v in out], zr.grad.detach(), part, sum_uq


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
def _soft(dev, rows, pitch, soft, kind, temperature, c, cw, pw, dpitch, weights=HALF, stats_in=None):
    """pylc_multiloss_stats_soft -> _finalize_ex -> _bwd_soft on a device tensor `soft` [B,C,H,W] of any strides:
    (stats, losses, dlogits [N, dpitch] NaN-prefilled, amax bits, n_bad)"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    b, cc, h, w = soft.shape
    n = b * h * w
    assert cc == c and soft.dtype == torch.float32 and soft.is_cuda and rows.shape[0] == n
    assert pw is None or (pw.dtype == torch.float32 and pw.numel() == n and pw.is_contiguous())
    inv_t = 1.0 / temperature
    strides = [int(v) for v in soft.stride()]
    k = {'probs': 0, 'logits': 1}[kind]
    stats = torch.full((3 + 3 * c,), float('nan'), device=dev)
    ws = torch.empty(lib.pylc_multiloss_workspace_floats(n, c), device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib.pylc_multiloss_stats_soft(ptr(rows), pitch, n, h, w, c, ptr(soft), *strides, k, inv_t, ptr(cw), ptr(pw), ptr(stats), ptr(ws), ptr(bad),
                                        stream()))
    use = stats if stats_in is None else stats_in
    losses = torch.full((4,), float('nan'), device=dev)
    check(lib.pylc_multiloss_finalize_ex(ptr(use), c, *weights, ptr(losses), stream()))
    dl = torch.full((n, dpitch), float('nan'), device=dev)
    amax = torch.full((1,), -1, dtype=torch.int32, device=dev)
    check(lib.pylc_multiloss_bwd_soft(ptr(rows), pitch, n, h, w, c, ptr(soft), *strides, k, inv_t, ptr(cw), ptr(pw), ptr(use), *weights, None, ptr(dl),
                                      dpitch, ptr(amax), stream()))
    return stats, losses, dl, amax, bad


def _ls(dev, rows, pitch, target, c, ignore, cw, pw, eps, dpitch, weights=HALF, stats_in=None):
    """pylc_multiloss_stats_ls -> _finalize_ex -> _bwd_ls: (stats, losses, dlogits [N, dpitch] NaN-prefilled, amax bits, n_bad)"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    n = target.numel()
    stats = torch.full((3 + 3 * c,), float('nan'), device=dev)
    ws = torch.empty(lib.pylc_multiloss_workspace_floats(n, c), device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib.pylc_multiloss_stats_ls(ptr(rows), pitch, ptr(target), target.element_size(), n, c, ignore, ptr(cw), ptr(pw), eps, ptr(stats), ptr(ws),
                                      ptr(bad), stream()))
    use = stats if stats_in is None else stats_in
    losses = torch.full((4,), float('nan'), device=dev)
    check(lib.pylc_multiloss_finalize_ex(ptr(use), c, *weights, ptr(losses), stream()))
    dl = torch.full((n, dpitch), float('nan'), device=dev)
    amax = torch.full((1,), -1, dtype=torch.int32, device=dev)
    check(lib.pylc_multiloss_bwd_ls(ptr(rows), pitch, ptr(target), target.element_size(), n, c, ignore, ptr(cw), ptr(pw), eps, ptr(use), *weights,
                                    None, ptr(dl), dpitch, ptr(amax), stream()))
    return stats, losses, dl, amax, bad


def _run(dev, shape_id, c, source, rows, pitch, cw, pw, dpitch, target_kind='u8', **kw):
    """one source through its entry points"""
    if source[0] == 'probs':
        return _soft(dev, rows, pitch, _volume(shape_id, c, source[1]).to(dev), 'probs', 1.0, c, cw, pw, dpitch, **kw)
    if source[0] == 'logits':
        return _soft(dev, rows, pitch, _volume(shape_id, c, 'teacher').to(dev), 'logits', source[1], c, cw, pw, dpitch, **kw)
    td = _as_target(dev, _target(shape_id, c, 'blobs30', source[2]), target_kind)
    return _ls(dev, rows, pitch, td, c, source[2], cw, pw, source[1], dpitch, **kw)


# ---- 1: against the fp64 statement -----------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    k = 0
    for shape_id in SHAPES:
        for c in CLASS_COUNTS:
            for weighted in (False, True):
                out.append(pytest.param(shape_id, c, weighted, k, id='%s-C%d-%s' % (shape_id, c, 'w' if weighted else 'u')))
                k += 1
    return out


def _sources(k):
    """(source, pixel-weight map or None, target kind): every source in every case; temperatures, smoothings, target kinds, ignore labels
    and the maps go round with k so that every one meets every C, with and without class weights"""
    kinds = (('i64', -100), ('i64', 255), ('u8', 255), ('u8odd', 255))
    (ka, ia), (kb, ib) = kinds[k % 4], kinds[(k + 2) % 4]
    return ((('probs', 'dirichlet'), None if k % 2 else 'uniform', None),
            (('probs', 'zero_rows'), 'uniform' if k % 2 else None, None),
            (('logits', TEMPERATURES[k % 3]), None if (k // 2) % 2 else 'border', None),
            (('ls', SMOOTHINGS[0], ia), 'border' if k % 2 else None, ka),
            (('ls', SMOOTHINGS[1], ib), None if k % 2 else 'uniform', kb))


@pytest.mark.parametrize('shape_id,c,weighted,k', _cases())
def test_soft_loss_head_against_the_fp64_statement(dev, shape_id, c, weighted, k):
    z = _logits(shape_id, c)
    cw = torch.from_numpy(D.class_weights(c)).to(dev) if weighted else None
    for i, (source, kind_u, tkind) in enumerate(_sources(k)):
        pitch, dpitch = _pitches(c)[(k + i) % 3], _pitches(c)[(k + i + 1) % 3]
        want, g, part, sum_uq = _want(shape_id, c, source, kind_u, weighted)
        rows = _rows(dev, z, pitch)
        pw = None if kind_u is None else _weights(shape_id, c, kind_u).reshape(-1).to(dev)
        stats, losses, dl, amax, bad = _run(dev, shape_id, c, source, rows, pitch, cw, pw, dpitch, tkind or 'u8')
        torch.cuda.synchronize()
        el, eg = _loss_err(losses.cpu().tolist(), want), rel_err(_grad_nchw(dl, shape_id, c), g)
        ec = abs(float(stats[3 + 2 * c:].double().sum()) - sum_uq) / sum_uq
        print('ST1 %s C %2d %s %-22s u %-7s pitch %2d/%2d taking part %6d sum uq %.6g: losses %.3g (bound %.3g)  grad %.3g (bound %.3g)  '
              'sum of counts %.3g (bound %.3g)' % (shape_id, c, 'w' if weighted else 'u', source[:2], kind_u, pitch, dpitch, int(part.sum()), sum_uq,
                                                   el, LOSS_REL, eg, GRAD_REL, ec, COUNT_REL))
        if not (el < LOSS_REL and eg < GRAD_REL):        # the yardstick: the hard-label kernel on the same logits against its fp64 statement
            t = _target(shape_id, c, 'blobs30', 255)
            ref = masked_multiloss(z.double().requires_grad_(True), t, 255, HALF, None if cw is None else cw.cpu().double())
            ex = _ex(dev, rows, pitch, _as_target(dev, t, 'u8'), c, 255, cw, dpitch)
            print('ST1   _ex on the same logits: losses %.3g' % _loss_err(ex[1].cpu().tolist(), [v.item() for v in ref]))
        assert el < LOSS_REL and eg < GRAD_REL and ec < COUNT_REL
        assert int(bad) == 0 and 0 < int(part.sum()) and (source[1] in ('dirichlet',) or source[0] == 'logits' or int(part.sum()) < part.numel())
        _check_rows(dl, c, dpitch, ~part)
        assert amax.view(torch.float32).item() == dl[:, :c].abs().max().item()


# ---- 2: layouts ----------------------------------------------------------------------------------------------------------------------------------
def _layouts(dev, q):
    """(name, a device view with the values of q [B,C,H,W] in that layout)"""
    b, c, h, w = q.shape
    qd = q.to(dev)
    out = [('planar', qd.contiguous())]
    out.append(('channels_last', qd.contiguous(memory_format=torch.channels_last)))
    buf = torch.full((b, h, w, r4(c) + 4), float('nan'), device=dev)
    buf[..., :c] = qd.permute(0, 2, 3, 1)
    out.append(('nhwc_pitch', buf[..., :c].permute(0, 3, 1, 2)))
    buf = torch.full((2 * b + 1, c * h * w + 37), float('nan'), device=dev)
    view = buf[1:2 * b + 1:2, :c * h * w].view(b, c, h, w)
    view.copy_(qd)
    out.append(('batch_slice', view))
    buf = torch.full((b * c * h * w + 1,), float('nan'), device=dev)
    view = buf[1:].view(b, c, h, w)
    view.copy_(qd)
    assert view.data_ptr() % 16 == 4
    out.append(('offset_one_float', view))
    return out


def _window_row(dev, shape_id, c, kind):
    """a row of B windows [B,C,H,W] cut out of a larger [C, H + 5, Wbig] volume with a stride below W (the windows overlap):
    probs.unfold(1, H, 3).unfold(2, W, S)[:, 1].permute(1, 0, 2, 3)"""
    b, h, w = SHAPES[shape_id]
    s = max(1, w - 3)
    big_w = (b - 1) * s + w + 2
    rs = np.random.RandomState(960 + c + h)
    if kind == 'logits':
        vol = torch.from_numpy((rs.standard_normal((c, h + 5, big_w)) * 2).astype(np.float32))
    else:
        g = rs.gamma(0.5, 1.0, (c, h + 5, big_w)).astype(np.float32) + np.float32(1e-6)
        vol = torch.from_numpy(g / g.sum(0, keepdims=True, dtype=np.float32))
        vol[:, 4:4 + max(1, h // 3)] = 0                               # rows of zeros inside every window
        vol[0, 3 + h // 2, ::5] = -1.0                                 # and bad rows
    view = vol.to(dev).unfold(1, h, 3).unfold(2, w, s)[:, 1].permute(1, 0, 2, 3)
    assert tuple(view.shape) == (b, c, h, w) and not view.is_contiguous()
    return view


@pytest.mark.parametrize('c', CLASS_COUNTS)
def test_layouts_equal_the_contiguous_copy_bit_for_bit(dev, c):
    cw = torch.from_numpy(D.class_weights(c)).to(dev)
    for shape_id in ('35px', '2880px') + (('270336px',) if c == 9 else ()):
        z = _logits(shape_id, c)
        pitch = r4(c)
        rows = _rows(dev, z, pitch)
        pw = _weights(shape_id, c, 'uniform').reshape(-1).to(dev)
        for kind, vol, temp in (('probs', 'zero_rows', 1.0), ('logits', 'teacher', 1.7)):
            q = _volume(shape_id, c, vol).clone()
            if kind == 'probs':
                q[0, c - 1, 2, ::3] = -0.5                              # bad rows: n_bad is compared too
            else:
                q[0, 0, 1, ::4] = float('inf')
            lay = _layouts(dev, q)
            ref = _soft(dev, rows, pitch, lay[0][1], kind, temp, c, cw, pw, pitch)
            assert int(ref[4]) > 0 and torch.isfinite(ref[1]).all()
            for name, view in lay[1:]:
                _same(_soft(dev, rows, pitch, view, kind, temp, c, cw, pw, pitch), ref, (shape_id, kind, name))
            win = _window_row(dev, shape_id, c, kind)
            got, want = (_soft(dev, rows, pitch, v, kind, temp, c, None, None, pitch) for v in (win, win.contiguous()))
            _same(got, want, (shape_id, kind, 'windows'))
            assert torch.isfinite(got[1]).all() and float(got[3].view(torch.float32)) > 0 and (kind == 'logits' or int(got[4]) > 0)


# ---- 3: the one-hot limit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CLASS_COUNTS)
@pytest.mark.parametrize('shape_id', list(SHAPES))
def test_one_hot_rows_and_zero_smoothing_give_the_bits_of_the_weighted_kernels(dev, shape_id, c):
    z = _logits(shape_id, c)
    t = _target(shape_id, c, 'blobs30', 255)
    onehot = _volume(shape_id, c, 'onehot').to(dev)
    skipped = (t == 255).reshape(-1)
    cwd = torch.from_numpy(D.class_weights(c)).to(dev)
    worst = 0.0
    for i, pitch in enumerate(_pitches(c)):
        rows = _rows(dev, z, pitch)
        for cw in (None, cwd):
            for kind_u in (None, 'uniform', 'border'):
                pw = None if kind_u is None else _weights(shape_id, c, kind_u).reshape(-1).to(dev)
                ref = _w(dev, rows, pitch, _as_target(dev, t, 'u8'), c, 255, cw, pw, pitch)          # (a NULL map: the kernels of _ex)
                cands = [('volume', _soft(dev, rows, pitch, onehot, 'probs', 1.0, c, cw, pw, pitch))]
                for tk in ('i64', 'u8', 'u8odd'):
                    cands.append(('ls0 ' + tk, _ls(dev, rows, pitch, _as_target(dev, t, tk), c, 255, cw, pw, 0.0, pitch)))
                gmax = float(ref[2][:, :c].abs().max())
                for name, got in cands:
                    _same(got, ref, (name, pitch, kind_u, cw is not None), parts=(0, 1, 4))
                    eg = float((got[2][:, :c] - ref[2][:, :c]).abs().max()) / gmax
                    worst = max(worst, eg)
                    assert eg < GRAD_REL, (name, eg)
                    assert got[3].view(torch.float32).item() == got[2][:, :c].abs().max().item() > 0
                    part = ~skipped if pw is None else ~skipped & (pw.cpu() > 0)
                    _check_rows(got[2], c, pitch, ~part)
        # no ignore value at all
        if i == 0:
            tn = _as_target(dev, _target(shape_id, c, 'none', 255), 'i64')
            _same(_ls(dev, rows, pitch, tn, c, NO_IGNORE, cwd, None, 0.0, pitch), _ex(dev, rows, pitch, tn, c, 255, cwd, pitch), 'no ignore',
                  parts=(0, 1, 4))
    print('ST3 %s C %2d: statistics and losses bit for bit; backward against _w %.3g of the largest entry (bound %.3g)' % (shape_id, c, worst, GRAD_REL))


# ---- 4: validity -----------------------------------------------------------------------------------------------------------------------------------
def test_bad_rows_are_skipped_and_counted(dev):
    c, shape_id = 9, '2880px'
    z = _logits(shape_id, c)
    cwh = torch.from_numpy(D.class_weights(c))
    u = _weights(shape_id, c, 'uniform')
    rs = np.random.RandomState(970)
    for kind in ('probs', 'logits'):
        q = _volume(shape_id, c, 'zero_rows' if kind == 'probs' else 'teacher').clone()
        rowsq = q.permute(0, 2, 3, 1).reshape(-1, c)                    # (a copy: written back below)
        live = torch.nonzero(rowsq.abs().sum(1) > 0).reshape(-1)
        pick = live[torch.from_numpy(rs.permutation(live.numel())[:90])]
        values = (-1.0, float('nan'), float('inf'), float('-inf'), -1e-30) if kind == 'probs' else (float('inf'), float('-inf'), float('nan'))
        for j, v in enumerate(values):
            rowsq[pick[j::len(values)], (j * 2) % c] = v
        q = rowsq.reshape(q.shape[0], q.shape[2], q.shape[3], c).permute(0, 3, 1, 2).contiguous()
        rows64 = q.double() if kind == 'probs' else teacher_rows(q, 1.7)
        assert int(bad_rows(rows64).sum()) == pick.numel()
        u_bad = u.clone()
        u_bad.reshape(-1)[pick[:7]] = float('nan')                       # on a bad row: the row is judged first, the pixel is counted once
        zero_row = torch.nonzero(rowsq.abs().sum(1) == 0).reshape(-1)
        u_bad.reshape(-1)[zero_row[:5]] = -1.0                            # on a row of zeros: skipped silently, whatever its weight
        zr = z.double().requires_grad_(True)
        out = soft_multiloss(zr, rows64, u_bad, HALF, cwh.double())
        out[0].backward()
        part = taking_part(rows64, u_bad)
        stats, losses, dl, amax, bad = _soft(dev, _rows(dev, z, 12), 12, q.to(dev), kind, 1.7, c, cwh.to(dev), u_bad.reshape(-1).to(dev), 12)
        el, eg = _loss_err(losses.cpu().tolist(), [v.item() for v in out]), rel_err(_grad_nchw(dl, shape_id, c), zr.grad)
        print('ST4 bad rows %s: n_bad %d of %d  losses %.3g (bound %.3g)  grad %.3g (bound %.3g)' % (kind, int(bad), pick.numel(), el, LOSS_REL, eg,
                                                                                                 GRAD_REL))
        assert int(bad) == pick.numel() and el < LOSS_REL and eg < GRAD_REL and torch.isfinite(stats).all()
        _check_rows(dl, c, 12, ~part)
    # _ls counts bad targets and bad weights in the one counter, as _w does
    t = _target(shape_id, c, 'blobs30', 255).clone()
    lab = torch.nonzero((t != 255).reshape(-1)).reshape(-1)
    t.reshape(-1)[lab[:5]] = 12
    ub = u.clone()
    ub.reshape(-1)[lab[10:13]] = float('inf')
    got = _ls(dev, _rows(dev, z, 12), 12, _as_target(dev, t, 'u8'), c, 255, None, ub.reshape(-1).to(dev), 0.1, 12)
    assert int(got[4]) == 8 and torch.isfinite(got[1]).all()


@pytest.mark.parametrize('c', [2, 9, 16])
def test_an_all_zero_volume_gives_exact_zeros_and_saturated_logits_stay_finite(dev, c):
    shape_id = '2880px'
    b, h, w = SHAPES[shape_id]
    z = _logits(shape_id, c)
    zero = torch.zeros((b, c, h, w), device=dev)
    for pitch in _pitches(c):
        stats, losses, dl, amax, bad = _soft(dev, _rows(dev, z, pitch), pitch, zero, 'probs', 1.0, c, None, None, pitch)
        assert losses.cpu().tolist() == [0.0, 0.0, 0.0, 0.0] and int(amax) == 0 and int(bad) == 0
        assert torch.equal(stats.cpu(), torch.zeros(3 + 3 * c))
        _check_rows(dl, c, pitch, torch.ones(b * h * w, dtype=torch.bool))
    # logits of +-80: p underflows to 0 in most classes, x = 1e-8 there
    sat = torch.where(_logits(shape_id, c) > 0, torch.tensor(80.0), torch.tensor(-80.0))
    cw = torch.from_numpy(D.class_weights(c)).to(dev)
    pw = _weights(shape_id, c, 'uniform').reshape(-1).to(dev)
    rows = _rows(dev, sat, r4(c))
    td = _as_target(dev, _target(shape_id, c, 'blobs30', 255), 'u8')
    for got in (_soft(dev, rows, r4(c), _volume(shape_id, c, 'dirichlet').to(dev), 'probs', 1.0, c, cw, pw, r4(c)),
                _soft(dev, rows, r4(c), sat.to(dev), 'logits', 0.5, c, cw, pw, r4(c)),
                _ls(dev, rows, r4(c), td, c, 255, cw, pw, 0.2, r4(c))):
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all() and torch.isfinite(got[2][:, :c]).all() and int(got[4]) == 0
        assert float(got[1][0]) > 0 and got[3].view(torch.float32).item() == got[2][:, :c].abs().max().item()


# ---- 5: two shards -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [2, 9, 16])
def test_two_shards_with_very_different_target_sums(dev, c):
    """MultiLossFn's wire format with a group: the statistics of two half batches, added, and each half's backward on the sum.  The second
    half's rows are a thousandth of the first's (q is used as given): a pixel count in place of sum u q would be wrong by a factor of two."""
    shape_id = '2880px'
    b, h, w = SHAPES[shape_id]
    z = _logits(shape_id, c)
    q = _volume(shape_id, c, 'zero_rows').clone()
    q[1] *= 1e-3
    u = _weights(shape_id, c, 'uniform')
    cwh = torch.from_numpy(D.class_weights(c))
    zr = z.double().requires_grad_(True)
    out = soft_multiloss(zr, q.double(), u, HALF, cwh.double())
    out[0].backward()
    want = [v.item() for v in out]
    pitch = r4(c)
    rows, qd, cw, ud = _rows(dev, z, pitch), q.to(dev), cwh.to(dev), u.reshape(-1).to(dev)
    n = h * w
    half = [(rows[i * n:(i + 1) * n], qd[i:i + 1], ud[i * n:(i + 1) * n]) for i in range(2)]
    parts = [_soft(dev, r, pitch, qq, 'probs', 1.0, c, cw, uu, pitch)[0] for r, qq, uu in half]
    sums = [float(p[3 + 2 * c:].double().sum()) for p in parts]
    assert sums[0] > 200 * sums[1] > 0
    stats = parts[0] + parts[1]
    halves = [_soft(dev, r, pitch, qq, 'probs', 1.0, c, cw, uu, pitch, stats_in=stats) for r, qq, uu in half]
    single = _soft(dev, rows, pitch, qd, 'probs', 1.0, c, cw, ud, pitch)
    dl = torch.cat([halves[0][2], halves[1][2]])
    el = max(_loss_err(hv[1].cpu().tolist(), want) for hv in halves)
    eg = rel_err(_grad_nchw(dl, shape_id, c), zr.grad)
    es, egs = _loss_err(single[1].cpu().tolist(), want), rel_err(_grad_nchw(single[2], shape_id, c), zr.grad)
    print('ST5 two shards C %2d, sum uq %.6g + %.6g: losses %.3g (bound %.3g)  grad %.3g (bound %.3g); one batch: losses %.3g  grad %.3g'
          % (c, sums[0], sums[1], el, LOSS_REL, eg, GRAD_REL, es, egs))
    assert el < LOSS_REL and eg < GRAD_REL and es < LOSS_REL and egs < GRAD_REL


# ---- 6: the Python layers ----------------------------------------------------------------------------------------------------------------------------
def _leaf(dev, z):
    return z.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)


def test_python_layers_agree_with_the_c_abi(dev):
    import pylc_amd  # noqa: F401
    from pylc_amd import lib as L, ops
    from pylc_amd.loss import MultiLoss
    from torch.library import opcheck
    c, shape_id = 9, '2880px'
    z = _logits(shape_id, c)
    u = _weights(shape_id, c, 'uniform').to(dev)
    cw = torch.from_numpy(D.class_weights(c)).to(dev)
    rows = _rows(dev, z, 12)
    lw = {'weighted': True, 'weights': D.class_weights(c), 'ce': 0.5, 'dice': 0.5, 'focal': 0.5}
    crit = MultiLoss(lw, {'n_classes': c}, ignore_index=255).to(dev)
    for kind, vol, temp in (('probs', 'zero_rows', 1.0), ('logits', 'teacher', 1.7)):
        q = _volume(shape_id, c, vol).clone()
        q[0, 0, 0, :3] = float('nan')                                    # three bad rows
        q = q.to(dev).contiguous(memory_format=torch.channels_last)      # a layout of its own: read in place
        abi = _soft(dev, rows, 12, q, kind, temp, c, cw, u.reshape(-1), 12)
        g_abi = _grad_nchw(abi[2], shape_id, c)
        res = []
        zd, bad = _leaf(dev, z), torch.zeros(1, dtype=torch.int64, device=dev)
        losses = ops.multiloss(zd, None, cw, *HALF, None, None, bad, u, soft_target=q, soft_kind=kind, temperature=temp)
        losses[0].backward()
        res.append((losses.detach(), zd.grad))
        assert int(bad) == 3
        zd = _leaf(dev, z)
        crit.bad_targets = None
        total = crit(zd, q, u) if kind == 'probs' else crit.distill(zd, q, temp, u)
        total.backward()
        res.append((torch.stack([total.detach(), crit.ce, crit.dsc, crit.fl]), zd.grad))
        assert int(crit.bad_targets) == 3
        if kind == 'probs':
            assert torch.equal(crit.all_losses(zd.detach(), q, u), abi[1])
            for name, k in (('ce_loss', 1), ('dice_loss', 2), ('focal_loss', 3)):
                assert torch.equal(getattr(crit, name)(zd.detach(), q, u), abi[1][k])
        zd = _leaf(dev, z)
        losses, stats, nbad = torch.ops.pylc_hip.multiloss_soft(zd, q, kind, temp, u, cw, *HALF)
        losses[0].backward()
        res.append((losses.detach(), zd.grad))
        assert torch.equal(stats, abi[0]) and int(nbad) == 3
        for i, (lo, g) in enumerate(res):
            assert torch.equal(lo, abi[1]) and torch.equal(g, g_abi), (kind, i)
        # without pixel weights
        zd = _leaf(dev, z)
        losses, stats, nbad = torch.ops.pylc_hip.multiloss_soft(zd, q, kind, temp, None, None, *HALF)
        assert torch.equal(losses, _soft(dev, rows, 12, q, kind, temp, c, None, None, 12)[1])
    # label smoothing: MultiLoss.forward alone is smoothed
    t8 = _target(shape_id, c, 'blobs30', 255).to(torch.uint8).to(dev)
    smooth = MultiLoss(lw, {'n_classes': c}, ignore_index=255, label_smoothing=0.1).to(dev)
    abi = _ls(dev, rows, 12, t8.reshape(-1), c, 255, cw, u.reshape(-1), float(np.float32(0.1)), 12)
    zd = _leaf(dev, z)
    total = smooth(zd, t8, u)
    total.backward()
    assert torch.equal(torch.stack([total.detach(), smooth.ce, smooth.dsc, smooth.fl]), abi[1]) and torch.equal(zd.grad, _grad_nchw(abi[2], shape_id, c))
    zd = _leaf(dev, z)
    losses = ops.multiloss(zd, t8.long(), cw, *HALF, None, 255, None, u, label_smoothing=0.1)
    assert torch.equal(losses, abi[1])
    plain_w = _w(dev, rows, 12, t8.reshape(-1), c, 255, cw, u.reshape(-1), 12)
    assert torch.equal(smooth.all_losses(zd.detach(), t8, u), plain_w[1]) and not torch.equal(plain_w[1], abi[1])
    assert torch.equal(smooth.ce_loss(zd.detach(), t8, u), plain_w[1][1])
    # no ignore_index and no weights: INT32_MIN goes down
    tn = _target(shape_id, c, 'none', 255).to(dev)
    nomark = MultiLoss(dict(lw, weighted=False), {'n_classes': c}, label_smoothing=0.1).to(dev)
    want = _ls(dev, rows, 12, tn.reshape(-1), c, NO_IGNORE, None, None, float(np.float32(0.1)), 12)
    assert torch.equal(nomark(zd.detach(), tn), want[1][0])
    # the defaults leave ops.multiloss on its present path: the bits of a direct _ex / _w call
    zd = _leaf(dev, z)
    losses = ops.multiloss(zd, t8, cw, *HALF, None, 255, None, u)
    losses[0].backward()
    assert torch.equal(losses, plain_w[1]) and torch.equal(zd.grad, _grad_nchw(plain_w[2], shape_id, c))
    ex = _ex(dev, rows, 12, t8.reshape(-1), c, 255, cw, 12)
    zd = _leaf(dev, z)
    losses = ops.multiloss(zd, t8, cw, *HALF, None, 255)
    losses[0].backward()
    assert torch.equal(losses, ex[1]) and torch.equal(zd.grad, _grad_nchw(ex[2], shape_id, c))
    # refusals
    q = _volume(shape_id, c, 'dirichlet').to(dev)
    zd = zd.detach()
    for bad_q in (q.double(), q[:1], q[:, :8], q.cpu(), q.reshape(-1)):
        with pytest.raises(L.PylcError, match='soft_target'):
            ops.multiloss(zd, None, cw, *HALF, soft_target=bad_q)
    with pytest.raises(L.PylcError, match='soft_kind'):
        ops.multiloss(zd, None, cw, *HALF, soft_target=q, soft_kind='labels')
    for temp in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(L.PylcError, match='temperature'):
            ops.multiloss(zd, None, cw, *HALF, soft_target=q, soft_kind='logits', temperature=temp)
    with pytest.raises(L.PylcError, match='label_smoothing'):
        ops.multiloss(zd, None, cw, *HALF, soft_target=q, label_smoothing=0.1)
    with pytest.raises(L.PylcError, match='target=None'):
        ops.multiloss(zd, t8, cw, *HALF, soft_target=q)
    with pytest.raises(L.PylcError, match='ignore_index'):
        ops.multiloss(zd, None, cw, *HALF, None, 255, soft_target=q)
    for eps in (1.0, -0.5):
        with pytest.raises(L.PylcError, match='label_smoothing'):
            ops.multiloss(zd, t8, cw, *HALF, label_smoothing=eps)
    with pytest.raises(L.PylcError, match='pixel_weights'):
        ops.multiloss(zd, None, cw, *HALF, pixel_weights=u[:1], soft_target=q)
    zs = _leaf(dev, _logits('35px', c))
    qs, us = _volume('35px', c, 'dirichlet').to(dev), _weights('35px', c, 'uniform').to(dev)
    for kind, pw in (('probs', us), ('logits', None)):
        opcheck(torch.ops.pylc_hip.multiloss_soft.default, (zs, qs, kind, 1.7, pw, cw, 0.5, 0.5, 0.5),
                test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration'))


def test_one_rank_group_equals_no_group(dev):
    import torch.distributed as dist
    from pylc_amd import ops
    c, shape_id = 9, '2880px'
    z, q = _logits(shape_id, c), _volume(shape_id, c, 'zero_rows').to(dev)
    u = _weights(shape_id, c, 'uniform').to(dev)
    t8 = _target(shape_id, c, 'blobs30', 255).to(torch.uint8).to(dev)

    def run(group):
        out = []
        for kw in ({'soft_target': q}, {'soft_target': _volume(shape_id, c, 'teacher').to(dev), 'soft_kind': 'logits', 'temperature': 1.7},
                   {'label_smoothing': 0.1}):
            zd = _leaf(dev, z)
            smooth = 'label_smoothing' in kw
            losses = ops.multiloss(zd, t8 if smooth else None, None, *HALF, group, 255 if smooth else None, None, u, **kw)
            losses[0].backward()
            out += [losses.detach(), zd.grad]
        return out
    want = run(None)
    assert not dist.is_initialized()
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group('gloo', init_method='file://' + os.path.join(tmp, 'store'), rank=0, world_size=1)
        try:
            got = run(dist.group.WORLD)
            ops.check_equal_shards()
        finally:
            dist.destroy_process_group()
    assert len(got) == 6 and all(torch.equal(a, b) for a, b in zip(got, want))


# ---- 7: the whole step -------------------------------------------------------------------------------------------------------------------------------
def _model(dev, arch, c, **meta):
    import oracle
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    runtime.dropout_enabled = False
    backbone = 'resnet' if arch == 'deeplab' else None
    model = Model(Meta(arch=arch, backbone=backbone or 'resnet', ch=3, n_classes=c, weighted=True, weights=D.class_weights(c).tolist(), **meta),
                  dev).build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec(arch, backbone, c, 3), salt=5))
    seen = {}
    forward, distill = model.crit.forward, model.crit.distill

    def spy(pred, target, pixel_weights=None):
        seen['logits'], seen['target'], seen['u'], seen['how'] = pred.detach().clone(), target, pixel_weights, 'forward'
        return forward(pred, target, pixel_weights)

    def spy_distill(pred, teacher, temperature=1.0, pixel_weights=None):
        seen['logits'], seen['target'], seen['u'], seen['how'], seen['T'] = pred.detach().clone(), teacher, pixel_weights, 'distill', temperature
        return distill(pred, teacher, temperature, pixel_weights)
    model.crit.forward, model.crit.distill = spy, spy_distill
    return model, seen


def _sampled(model):
    return [p.detach().reshape(-1)[::97].clone() for p in model.net.parameters()]


def _terms(model):
    return torch.stack((model.crit.ce, model.crit.dsc, model.crit.fl))


@pytest.mark.parametrize('arch', ['deeplab', 'unet'])
def test_network_step_with_soft_targets(dev, arch):
    from pylc_amd import ops
    c = 9
    b, hw = (2, 64) if arch == 'deeplab' else (1, 256)
    x = D.tiles(980, b, 3, hw, hw)
    y = D.blob_masks(981, b, hw, hw, c, cell=8)
    cw = torch.from_numpy(D.class_weights(c)).to(dev)
    rs = np.random.RandomState(982)
    # a whole "photograph's" volume [C, hw + 6, Wbig] and a row of B overlapping windows of it
    s = hw - 8
    g = rs.gamma(0.5, 1.0, (c, hw + 6, (b - 1) * s + hw + 3)).astype(np.float32) + np.float32(1e-6)
    vol = torch.from_numpy(g / g.sum(0, keepdims=True, dtype=np.float32)).to(dev)
    vol[:, 100 % hw:(100 % hw) + 9, 5:40] = 0                                # a region the caller leaves out
    win = vol.unfold(1, hw, 3).unfold(2, hw, s)[:, 1].permute(1, 0, 2, 3)
    assert tuple(win.shape) == (b, c, hw, hw) and not win.is_contiguous()
    (mv, sv), (mc, sc), (mh, sh), (mo, so) = (_model(dev, arch, c) for _ in range(4))
    # Model.train(x, q) is its hand composition: net forward, the cropped VIEW of q, ops.multiloss(soft_target=)
    loss_v = mv.train(x, win)
    qc = mv._soft_target(win)
    lg = sv['logits']
    assert sv['how'] == 'forward' and tuple(qc.shape) == tuple(lg.shape) and sv['target'].data_ptr() == qc.data_ptr() and sv['u'] is None
    assert arch != 'unet' or qc.shape[2] == hw - 2 * mv.meta.pad_size
    hand = ops.multiloss(lg, None, cw, *HALF, None, None, None, None, soft_target=qc)
    assert torch.equal(hand[0], loss_v) and torch.equal(hand[1:], _terms(mv))
    ref = soft_multiloss(lg.double().cpu(), qc.double().cpu(), None, HALF, cw.double().cpu())
    el = _loss_err(hand.cpu().tolist(), [v.item() for v in ref])
    print('ST7 %s: losses of the step against fp64 %.3g (bound %.3g), %d of %d pixels take part' % (
        arch, el, LOSS_REL, int(taking_part(qc.cpu()).sum()), qc.shape[0] * qc.shape[2] * qc.shape[3]))
    assert el < LOSS_REL
    # a window view == its contiguous copy, from identical initial states
    loss_c = mc.train(x, win.contiguous())
    assert torch.equal(loss_c, loss_v) and torch.equal(_terms(mc), _terms(mv))
    for p, q in zip(_sampled(mc), _sampled(mv)):
        assert torch.equal(p, q)
    # one-hot rows against the hard target, from identical initial states
    loss_h, loss_o = mh.train(x, y), mo.train(x, F.one_hot(y, c).permute(0, 3, 1, 2).float())
    eo = _loss_err([float(loss_o)] + _terms(mo).cpu().tolist(), [float(loss_h)] + _terms(mh).cpu().tolist())
    print('ST7 %s: one-hot volume against the hard target: losses %.3g (bound %.3g)' % (arch, eo, LOSS_REL))
    assert eo < LOSS_REL and so['target'].dtype == torch.float32 and sh['target'].dtype == torch.int64
    # teacher logits at the temperature of the checkpoint; pixel weights cropped like the target
    teacher = torch.from_numpy((rs.standard_normal((b, c, hw, hw)) * 2).astype(np.float32)).to(dev)
    conf = torch.from_numpy(rs.rand(b, hw, hw).astype(np.float32)).to(dev)
    with pytest.raises(ValueError, match='meta.temperature is unset'):
        mv.train(x, teacher, soft='logits', temperature='meta')
    mv.meta.temperature = 1.7
    loss_t = mv.train(x, teacher, pixel_weights=conf, soft='logits', temperature='meta')
    assert sv['how'] == 'distill' and sv['T'] == 1.7 and torch.equal(sv['u'], mv.crop_target(conf))
    hand = ops.multiloss(sv['logits'], None, cw, *HALF, None, None, None, sv['u'], soft_target=mv._soft_target(teacher), soft_kind='logits',
                         temperature=1.7)
    assert torch.equal(hand[0], loss_t) and torch.equal(hand[1:], _terms(mv))
    other = ops.multiloss(sv['logits'], None, cw, *HALF, None, None, None, sv['u'], soft_target=mv._soft_target(teacher), soft_kind='logits')
    assert not torch.equal(other, hand)
    torch.cuda.synchronize()
    for m in (mv, mc, mo):
        assert all(torch.isfinite(p).all() for p in m.net.parameters())
        m.log()                                           # no bad row was counted
    # border_weight needs a mask: what build() sets up for Meta.border_weight refuses a soft target before anything is launched
    mc.meta.border_weight = {'w0': 10.0, 'sigma': 2.0, 'radius': 3}
    mc._border = mc._border_table(mc.meta)
    before = mc.iter
    with pytest.raises(ValueError, match='border_weight'):
        mc.train(x, win)
    assert mc.iter == before


@pytest.mark.parametrize('arch', ['deeplab', 'unet'])
def test_network_step_with_label_smoothing(dev, arch):
    from pylc_amd import ops
    c = 9
    b, hw = (2, 64) if arch == 'deeplab' else (1, 256)
    x = D.tiles(990, b, 3, hw, hw)
    y = D.blob_masks(991, b, hw, hw, c, cell=8)
    y[ignore_blobs(992, (b, hw, hw), 0.3, cell=8)] = 255
    y8 = y.to(torch.uint8)
    cw = torch.from_numpy(D.class_weights(c)).to(dev)
    (ms, ss), (m0, s0), (mp, sp) = (_model(dev, arch, c, ignore_index=255, **kw) for kw in ({'label_smoothing': 0.1}, {'label_smoothing': 0.0}, {}))
    # Model.eval stays unsmoothed: the bits of a model built without label_smoothing, on the same parameters
    for m in (ms, m0, mp):
        m.eval(x, y8)
    assert ms.loss.flush() == mp.loss.flush() == m0.loss.flush() and len(ms.loss.intv) == 1 and not ss
    # the smoothed step is its hand composition through the _ls kernels
    loss_s = ms.train(x, y8)
    yc = ms.crop_target(y8).to(dev)
    hand = ops.multiloss(ss['logits'], yc, cw, *HALF, None, 255, None, None, label_smoothing=0.1)
    assert torch.equal(hand[0], loss_s) and torch.equal(hand[1:], _terms(ms))
    ref = soft_multiloss(ss['logits'].double().cpu(), smoothed_rows(yc.cpu(), c, 0.1, 255), None, HALF, cw.double().cpu())
    el = _loss_err(hand.cpu().tolist(), [v.item() for v in ref])
    print('ST7 %s: losses of the smoothed step against fp64 %.3g (bound %.3g)' % (arch, el, LOSS_REL))
    assert el < LOSS_REL
    # label_smoothing = 0.0 is the step as it was
    loss_0, loss_p = m0.train(x, y8), mp.train(x, y8)
    assert torch.equal(loss_0, loss_p) and torch.equal(_terms(m0), _terms(mp)) and not torch.equal(loss_0, loss_s)
    plain = ops.multiloss(sp['logits'], yc, cw, *HALF, None, 255)
    assert torch.equal(plain[0], loss_p)
    for p, q in zip(_sampled(m0), _sampled(mp)):
        assert torch.equal(p, q)
    torch.cuda.synchronize()
    for m in (ms, m0):
        assert all(torch.isfinite(p).all() for p in m.net.parameters())
        m.log()
