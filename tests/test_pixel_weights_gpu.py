"""Per-pixel loss weights and the border-weight map on the GPU (-m gpu).

  1-6  the loss head with a weight per pixel (pylc_multiloss_stats_w / _bwd_w with pylc_multiloss_finalize_ex, ops.multiloss(pixel_weights=),
       MultiLoss, the pylc_hip::multiloss_weighted operator) on the inputs of tests/test_ignore_label_gpu.py, against the fp64 statement
       tests/_pixel_weights.weighted_multiloss within the bounds the project holds this kernel to (2e-6 max(1, |x|) per loss term, 1e-5 of
       the largest gradient entry -- that entry scales with u, so the bound needs no new number).  Bit for bit: a NULL map and a map of
       1.0f == _ex; a {0, 1} map == _ex with those pixels ignored; with w_dice = 0 a map of 4.0f == a map of 1.0f (a power of two cancels
       exactly in CE and Focal: a wrong normaliser shows); uint8 == int64 targets; amax == max |dlogits|; rows of skipped pixels +0.0.
       Bad weights are skipped and counted, an all-zero map gives exact zeros, two shards with very different sum u give the single-batch
       result.
  7-8  pylc_boundary_weights and pylc_weights_from_d2 against table[distance_ref(...)] of tests/_boundary.py, bit for bit; argument errors.
  9    Model.train with Meta.border_weight and with pixel_weights=, on a U-Net (cropped target) and DeepLab/ResNet-101.

Every comparison with a bound prints its figures next to it (lines `PW1` .. `PW9` under `pytest -s`)."""
import functools

import numpy as np
import pytest
import torch

from tests import _boundary as Bd
from tests import _data as D
from tests._pixel_weights import taking_part, weighted_multiloss
from tests.test_cpu_ignore_label import ignore_blobs, masked_multiloss
from tests.test_cpu_pixel_weights import boundary_weight_refusals, from_d2_refusals
from tests.test_ignore_label_gpu import (CLASS_COUNTS, GRAD_REL, HALF, LOSS_REL, SHAPES, _as_target, _check_rows, _ex, _grad_nchw, _logits,
                                         _loss_err, _pitches, _rows, _target, r4)
from tests.test_ops_gpu import rel_err

pytestmark = pytest.mark.gpu

NO_IGNORE = -2 ** 31
MAPS = ('border', 'uniform')
COUNT_REL = 1e-6          # a class count: at most 11 fp32 roundings of sums of positive addends (1 in the thread, 6 + 3 in the block, 1 at the
#                           store; the block partials are added in fp64), each at most 2^-24 of the total: 6.6e-7


# ---- inputs and the fp64 statement, computed once and only read ------------------------------------------------------------------------------
def _profile():
    from pylc_amd import boundary
    return boundary.border_profile(3, w0=10.0, sigma=2.0)


@functools.lru_cache(maxsize=None)
def _weights(shape_id, c, kind, pattern='blobs30'):
    """float32 [B,H,W]: 'border' the profile w0 = 10, sigma = 2, R = 3 of the target (0 where it is ignored), 'uniform' a (0, 1] map,
    'ones', 'fours', 'zero_one' (about 30 % zeros in blobs)"""
    b, h, w = SHAPES[shape_id]
    if kind == 'border':
        t = _target(shape_id, c, pattern, 255)
        d2 = Bd.distance_ref(t.numpy().astype(np.uint8), 3, 255)
        return torch.from_numpy(np.where(d2 < 0, np.float32(0), _profile()[np.maximum(d2, 0)]).astype(np.float32))
    if kind == 'uniform':
        return torch.from_numpy((1.0 - np.random.RandomState(720 + c + b * h).rand(b, h, w)).astype(np.float32))
    if kind == 'zero_one':
        cell = 2 if h < 16 else 4 if h < 100 else 16
        return (~ignore_blobs(721 + c, (b, h, w), 0.3, cell=cell)).float()
    return torch.full((b, h, w), {'ones': 1.0, 'fours': 4.0}[kind])


@functools.lru_cache(maxsize=None)
def _want(shape_id, c, kind, ignore, weighted):
    """the statement in fp64: ([total, ce, dice, focal], d total / d logits)"""
    z, t, u = _logits(shape_id, c), _target(shape_id, c, 'blobs30', ignore), _weights(shape_id, c, kind)
    cw = torch.from_numpy(D.class_weights(c)).double() if weighted else None
    zr = z.double().requires_grad_(True)
    out = weighted_multiloss(zr, t, u, ignore, HALF, cw)
    out[0].backward()
    return [v.item() for v in out], zr.grad.detach()


def _w(dev, rows, pitch, target, c, ignore, cw, pw, dpitch, weights=HALF, stats_in=None):
    """pylc_multiloss_stats_w -> _finalize_ex -> _bwd_w: (stats, losses, dlogits [N, dpitch] NaN-prefilled, amax bits, n_bad)"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    n = target.numel()
    assert pw is None or (pw.dtype == torch.float32 and pw.numel() == n and pw.is_contiguous())
    stats = torch.full((3 + 3 * c,), float('nan'), device=dev)
    ws = torch.empty(lib.pylc_multiloss_workspace_floats(n, c), device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib.pylc_multiloss_stats_w(ptr(rows), pitch, ptr(target), target.element_size(), n, c, ignore, ptr(cw), ptr(pw), ptr(stats), ptr(ws),
                                     ptr(bad), stream()))
    use = stats if stats_in is None else stats_in
    losses = torch.full((4,), float('nan'), device=dev)
    check(lib.pylc_multiloss_finalize_ex(ptr(use), c, *weights, ptr(losses), stream()))
    dl = torch.full((n, dpitch), float('nan'), device=dev)
    amax = torch.full((1,), -1, dtype=torch.int32, device=dev)
    check(lib.pylc_multiloss_bwd_w(ptr(rows), pitch, ptr(target), target.element_size(), n, c, ignore, ptr(cw), ptr(pw), ptr(use), *weights, None,
                                   ptr(dl), dpitch, ptr(amax), stream()))
    return stats, losses, dl, amax, bad


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what, parts=(0, 1, 2, 3, 4)):
    """statistics, losses, dlogits, amax bits, n_bad: the same bits"""
    for i in parts:
        assert torch.equal(_bits(a[i]), _bits(b[i])), (what, ('stats', 'losses', 'dlogits', 'amax', 'n_bad')[i])


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


@pytest.mark.parametrize('shape_id,c,weighted,k', _cases())
def test_weighted_loss_head_against_the_fp64_statement(dev, shape_id, c, weighted, k):
    z = _logits(shape_id, c)
    cw = torch.from_numpy(D.class_weights(c)).to(dev) if weighted else None
    kinds = (('i64', -100), ('i64', 255), ('u8', 255), ('u8odd', 255))
    for i, kind_u in enumerate(MAPS):
        kind, ignore = kinds[(k + i) % 4]
        pitch, dpitch = _pitches(c)[(k + i) % 3], _pitches(c)[(k + i + 1) % 3]
        t, u = _target(shape_id, c, 'blobs30', ignore), _weights(shape_id, c, kind_u)
        want, g = _want(shape_id, c, kind_u, ignore, weighted)
        rows, td = _rows(dev, z, pitch), _as_target(dev, t, kind)
        stats, losses, dl, amax, bad = _w(dev, rows, pitch, td, c, ignore, cw, u.reshape(-1).to(dev), dpitch)
        torch.cuda.synchronize()
        part = taking_part(t, u, c, ignore).reshape(-1)
        el, eg = _loss_err(losses.cpu().tolist(), want), rel_err(_grad_nchw(dl, shape_id, c), g)
        sum_u = float(u.reshape(-1)[part].double().sum())
        ec = abs(float(stats[3 + 2 * c:].double().sum()) - sum_u) / sum_u
        print('PW1 %s C %2d %s %-7s %-5s ign %4d pitch %2d/%2d taking part %6d sum u %.6g: losses %.3g (bound %.3g)  grad %.3g (bound %.3g)  '
              'sum of counts %.3g (bound %.3g)' % (shape_id, c, 'w' if weighted else 'u', kind_u, kind, ignore, pitch, dpitch, int(part.sum()),
                                                   sum_u, el, LOSS_REL, eg, GRAD_REL, ec, COUNT_REL))
        if not (el < LOSS_REL and eg < GRAD_REL):        # the yardstick: the unweighted kernel on the same logits against its fp64 statement
            ref = masked_multiloss(z.double().requires_grad_(True), t, ignore, HALF, None if cw is None else cw.cpu().double())
            ex = _ex(dev, rows, pitch, td, c, ignore, cw, dpitch)
            print('PW1   _ex on the same logits: losses %.3g' % _loss_err(ex[1].cpu().tolist(), [v.item() for v in ref]))
        assert el < LOSS_REL and eg < GRAD_REL and ec < COUNT_REL
        assert int(bad) == 0 and 0 < int(part.sum()) < part.numel()
        _check_rows(dl, c, dpitch, ~part)
        assert amax.view(torch.float32).item() == dl[:, :c].abs().max().item()


# ---- 2: bit for bit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CLASS_COUNTS)
@pytest.mark.parametrize('shape_id', list(SHAPES))
def test_bit_for_bit_pins(dev, shape_id, c):
    z = _logits(shape_id, c)
    cw = torch.from_numpy(D.class_weights(c)).to(dev)
    t = _target(shape_id, c, 'blobs30', 255)
    ones, fours = (_weights(shape_id, c, kind).reshape(-1).to(dev) for kind in ('ones', 'fours'))
    zo = _weights(shape_id, c, 'zero_one')
    off = (zo == 0)
    assert 0.1 < off.float().mean() < 0.6
    t_off = torch.where(off, torch.full_like(t, 255), t)
    border = _weights(shape_id, c, 'border').reshape(-1).to(dev)
    for pitch in _pitches(c):
        rows = _rows(dev, z, pitch)
        for kind, ignore in (('i64', 255), ('i64', -100), ('u8', 255)):
            tk = _target(shape_id, c, 'blobs30', ignore)
            td = _as_target(dev, tk, kind)
            for w in (None, cw):
                ex = _ex(dev, rows, pitch, td, c, ignore, w, pitch)
                _same(_w(dev, rows, pitch, td, c, ignore, w, None, pitch), ex, ('NULL', pitch, kind, ignore))
                _same(_w(dev, rows, pitch, td, c, ignore, w, ones, pitch), ex, ('ones', pitch, kind, ignore))
        # a {0, 1} map == those pixels ignored
        td = _as_target(dev, t, 'u8')
        got = _w(dev, rows, pitch, td, c, 255, cw, zo.reshape(-1).to(dev), pitch)
        _same(got, _ex(dev, rows, pitch, _as_target(dev, t_off, 'u8'), c, 255, cw, pitch), ('zero_one', pitch))
        _check_rows(got[2], c, pitch, (off | (t == 255)).reshape(-1))
        # no ignore value at all: INT32_MIN, which no target equals
        tn = _target(shape_id, c, 'none', 255)
        _same(_w(dev, rows, pitch, _as_target(dev, tn, 'i64'), c, NO_IGNORE, cw, ones, pitch),
              _ex(dev, rows, pitch, _as_target(dev, tn, 'i64'), c, 255, cw, pitch), ('no ignore', pitch))
        # w_dice = 0: the scale of the map cancels exactly
        nodice = (0.5, 0.0, 0.5)
        one, four = (_w(dev, rows, pitch, td, c, 255, cw, m, pitch, weights=nodice) for m in (ones, fours))
        assert torch.equal(four[0][:3], 4 * one[0][:3]) and torch.equal(four[0][3 + 2 * c:], 4 * one[0][3 + 2 * c:])
        assert torch.equal(_bits(four[1][[0, 1, 3]]), _bits(one[1][[0, 1, 3]])), pitch
        _same(four, one, ('fours', pitch), parts=(2, 3, 4))
        # uint8 == int64 targets, at an odd byte address too; amax == max |dlogits|
        ref = _w(dev, rows, pitch, _as_target(dev, t, 'i64'), c, 255, cw, border, pitch)
        for kind in ('u8', 'u8odd'):
            _same(_w(dev, rows, pitch, _as_target(dev, t, kind), c, 255, cw, border, pitch), ref, (kind, pitch))
        assert ref[3].view(torch.float32).item() == ref[2][:, :c].abs().max().item() > 0


# ---- 3: bad weights ------------------------------------------------------------------------------------------------------------------------------
def test_bad_weights_are_skipped_and_counted(dev):
    c, shape_id = 9, '2880px'
    z, t = _logits(shape_id, c), _target(shape_id, c, 'blobs30', 255)
    u = _weights(shape_id, c, 'uniform').clone()
    labelled = torch.nonzero((t != 255).reshape(-1)).reshape(-1)
    pick = labelled[torch.from_numpy(np.random.RandomState(730).permutation(labelled.numel())[:120])]
    flat = u.reshape(-1)
    for j, v in enumerate((-1.0, float('nan'), float('inf'), float('-inf'), -1e-30, 0.0, -0.0)):
        flat[pick[j::7]] = v
    bad_px = ~(flat == 0) & ~((flat > 0) & torch.isfinite(flat))
    n_bad = int(bad_px[pick].sum())
    flat[torch.nonzero((t == 255).reshape(-1)).reshape(-1)[:9]] = float('nan')          # on an ignored target: the target is judged first
    assert n_bad == sum(len(pick[j::7]) for j in range(5)) and int((flat[pick] == 0).sum()) == len(pick[5::7]) + len(pick[6::7])
    cwh = torch.from_numpy(D.class_weights(c))
    zr = z.double().requires_grad_(True)
    out = weighted_multiloss(zr, t, u, 255, HALF, cwh.double())
    out[0].backward()
    part = taking_part(t, u, c, 255).reshape(-1)
    assert int((~part)[pick].sum()) == pick.numel()
    for kind in ('i64', 'u8'):
        stats, losses, dl, amax, bad = _w(dev, _rows(dev, z, 12), 12, _as_target(dev, t, kind), c, 255, cwh.to(dev), flat.to(dev), 12)
        el, eg = _loss_err(losses.cpu().tolist(), [v.item() for v in out]), rel_err(_grad_nchw(dl, shape_id, c), zr.grad)
        print('PW3 bad weights %s: n_bad %d  losses %.3g (bound %.3g)  grad %.3g (bound %.3g)' % (kind, int(bad), el, LOSS_REL, eg, GRAD_REL))
        assert int(bad) == n_bad and el < LOSS_REL and eg < GRAD_REL and torch.isfinite(stats).all()
        _check_rows(dl, c, 12, ~part)
    # a bad target and a bad weight at different pixels add up in the one counter
    t12 = t.clone()
    t12.reshape(-1)[labelled[~torch.isin(labelled, pick)][-5:]] = 12
    assert int(_w(dev, _rows(dev, z, 12), 12, _as_target(dev, t12, 'u8'), c, 255, None, flat.to(dev), 12)[4]) == n_bad + 5


# ---- 4: no participating pixel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [2, 9, 16])
def test_an_all_zero_map_gives_exact_zeros(dev, c):
    shape_id = '2880px'
    z, t = _logits(shape_id, c), _target(shape_id, c, 'blobs30', 255)
    zero = torch.zeros(t.numel(), device=dev)
    for pitch in _pitches(c):
        stats, losses, dl, amax, bad = _w(dev, _rows(dev, z, pitch), pitch, _as_target(dev, t, 'u8'), c, 255, None, zero, pitch)
        assert losses.cpu().tolist() == [0.0, 0.0, 0.0, 0.0] and int(amax) == 0 and int(bad) == 0
        assert torch.isfinite(stats).all() and torch.equal(stats.cpu(), torch.zeros(3 + 3 * c))
        _check_rows(dl, c, pitch, torch.ones(t.numel(), dtype=torch.bool))


# ---- 5: two shards -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [2, 9, 16])
def test_two_shards_with_very_different_weight_sums(dev, c):
    """MultiLossFn's wire format with a group: the statistics of two half batches, added, and each half's backward on the sum.  The second
    half's weights are a thousandth of the first's: a pixel count in place of sum u would be wrong by a factor of two."""
    shape_id = '2880px'
    b, h, w = SHAPES[shape_id]
    z, t = _logits(shape_id, c), _target(shape_id, c, 'blobs30', 255)
    u = _weights(shape_id, c, 'border').clone()
    u[1] = _weights(shape_id, c, 'uniform')[1] * 1e-3
    cwh = torch.from_numpy(D.class_weights(c))
    zr = z.double().requires_grad_(True)
    out = weighted_multiloss(zr, t, u, 255, HALF, cwh.double())
    out[0].backward()
    want = [v.item() for v in out]
    pitch = r4(c)
    rows, td, cw, ud = _rows(dev, z, pitch), _as_target(dev, t, 'u8'), cwh.to(dev), u.reshape(-1).to(dev)
    n = h * w
    half = [(rows[i * n:(i + 1) * n], td[i * n:(i + 1) * n], ud[i * n:(i + 1) * n]) for i in range(2)]
    parts = [_w(dev, r, pitch, tt, c, 255, cw, uu, pitch)[0] for r, tt, uu in half]
    sums = [float(p[3 + 2 * c:].double().sum()) for p in parts]
    assert sums[0] > 200 * sums[1] > 0
    stats = parts[0] + parts[1]
    halves = [_w(dev, r, pitch, tt, c, 255, cw, uu, pitch, stats_in=stats) for r, tt, uu in half]
    single = _w(dev, rows, pitch, td, c, 255, cw, ud, pitch)
    dl = torch.cat([halves[0][2], halves[1][2]])
    el = max(_loss_err(hv[1].cpu().tolist(), want) for hv in halves)
    eg = rel_err(_grad_nchw(dl, shape_id, c), zr.grad)
    es, egs = _loss_err(single[1].cpu().tolist(), want), rel_err(_grad_nchw(single[2], shape_id, c), zr.grad)
    print('PW5 two shards C %2d, sum u %.6g + %.6g: losses %.3g (bound %.3g)  grad %.3g (bound %.3g); one batch: losses %.3g  grad %.3g'
          % (c, sums[0], sums[1], el, LOSS_REL, eg, GRAD_REL, es, egs))
    assert el < LOSS_REL and eg < GRAD_REL and es < LOSS_REL and egs < GRAD_REL


# ---- 6: the Python layers ----------------------------------------------------------------------------------------------------------------------------
def test_python_layers_agree_with_the_c_abi(dev):
    import pylc_amd  # noqa: F401
    from pylc_amd import lib as L, ops
    from pylc_amd.loss import MultiLoss
    from torch.library import opcheck
    c, shape_id = 9, '2880px'
    z, t = _logits(shape_id, c), _target(shape_id, c, 'blobs30', 255)
    u = _weights(shape_id, c, 'border').to(dev)
    cw = torch.from_numpy(D.class_weights(c)).to(dev)
    t8 = t.to(torch.uint8).to(dev)
    abi = _w(dev, _rows(dev, z, 12), 12, t8.reshape(-1), c, 255, cw, u.reshape(-1), 12)
    g_abi = _grad_nchw(abi[2], shape_id, c)

    def leaf():
        return z.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    res = []
    zd, bad = leaf(), torch.zeros(1, dtype=torch.int64, device=dev)
    losses = ops.multiloss(zd, t8, cw, *HALF, None, 255, bad, u)
    losses[0].backward()
    res.append((losses.detach(), zd.grad))
    zd = leaf()
    strided = u.transpose(1, 2).contiguous().transpose(1, 2)          # the same values, not contiguous: made so
    assert not strided.is_contiguous()
    losses = ops.multiloss(zd, t.to(dev), cw, *HALF, None, 255, None, strided)
    losses[0].backward()
    res.append((losses.detach(), zd.grad))
    crit = MultiLoss({'weighted': True, 'weights': D.class_weights(c), 'ce': 0.5, 'dice': 0.5, 'focal': 0.5}, {'n_classes': c}, ignore_index=255).to(dev)
    zd = leaf()
    crit(zd, t8, u).backward()
    res.append((torch.stack([crit.ce * 0.5 + crit.dsc * 0.5 + crit.fl * 0.5, crit.ce, crit.dsc, crit.fl]), zd.grad))
    assert torch.equal(crit.all_losses(zd.detach(), t8, u), abi[1]) and int(crit.bad_targets) == 0
    for name, k in (('ce_loss', 1), ('dice_loss', 2), ('focal_loss', 3)):
        assert torch.equal(getattr(crit, name)(zd.detach(), t8, u), abi[1][k])
    zd = leaf()
    losses, stats, nbad = torch.ops.pylc_hip.multiloss_weighted(zd, t8, u, cw, *HALF, 255)
    losses[0].backward()
    res.append((losses.detach(), zd.grad))
    assert torch.equal(stats, abi[0]) and int(nbad) == 0
    for i, (lo, g) in enumerate(res):
        assert torch.equal(lo[1:], abi[1][1:]) and torch.equal(g, g_abi), i
    assert torch.equal(res[0][0], abi[1]) and torch.equal(res[1][0], abi[1]) and torch.equal(res[3][0], abi[1])
    # no ignore_index: INT32_MIN goes down, the bad counter is allocated as on the ignore path
    plain = MultiLoss({'weighted': False, 'weights': None, 'ce': 0.5, 'dice': 0.5, 'focal': 0.5}, {'n_classes': c}).to(dev)
    tn = _target(shape_id, c, 'none', 255).to(dev)
    neg = u.clone()
    neg[0, 0, :3] = -1.0
    assert plain.bad_targets is None and torch.equal(plain.all_losses(zd.detach(), tn), plain.all_losses(zd.detach(), tn, torch.ones_like(u)))
    plain(zd.detach(), tn, neg)
    assert int(plain.bad_targets) == 3
    want = _w(dev, _rows(dev, z, 12), 12, tn.reshape(-1), c, NO_IGNORE, None, neg.reshape(-1), 12)
    assert torch.equal(plain.all_losses(zd.detach(), tn, neg), want[1])
    lo2 = torch.ops.pylc_hip.multiloss_weighted(zd.detach(), tn, neg, None, *HALF, None)
    assert torch.equal(lo2[0], want[1]) and int(lo2[2]) == 3
    # refusals
    for bad_u in (u.double(), u[:1], u.reshape(-1), u.cpu()):
        with pytest.raises(L.PylcError, match='pixel_weights'):
            ops.multiloss(zd.detach(), t8, cw, *HALF, None, 255, None, bad_u)
    zs = _logits('35px', c).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ts = _target('35px', c, 'blobs30', 255).to(torch.uint8).to(dev)
    us = _weights('35px', c, 'uniform').to(dev)
    for ignore in (255, None):
        opcheck(torch.ops.pylc_hip.multiloss_weighted.default, (zs, ts, us, cw, 0.5, 0.5, 0.5, ignore),
                test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration'))


# ---- 7: border weights ---------------------------------------------------------------------------------------------------------------------------------
BW_SIZES = [(1, 1), (1, 9), (8, 1), (63, 127), (64, 128), (65, 129), (9, 255), (130, 66)]


def _table(radius, seed=0):
    """any positive profile will do: distinct cells, so that a wrong index shows"""
    return (0.5 + np.random.RandomState(740 + radius + seed).rand(radius * radius + 2)).astype(np.float32)


def _want_weights(d2, table):
    return np.where(d2 < 0, np.float32(0), table[np.maximum(d2, 0)]).astype(np.float32)


def _gpu_weights(dev, m, radius, table, ignore=None):
    """pylc_boundary_weights through boundary.border_weights, and the two-step form; both as numpy"""
    from pylc_amd import boundary
    md = m if torch.is_tensor(m) else torch.from_numpy(m).to(dev)
    got = boundary.border_weights(md, radius, table, ignore_index=ignore)
    assert got.dtype == torch.float32 and got.shape == md.shape
    two = boundary.weights_from_distance(boundary.boundary_distance(md, radius, ignore), radius, table)
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    return got.cpu().numpy()


@pytest.mark.parametrize('radius', [1, 3, 70])
@pytest.mark.parametrize('hw', BW_SIZES)
def test_border_weights_match_the_statement(dev, hw, radius):
    from tests.test_boundary_gpu import masks_for, want_distance
    table = _table(radius)
    for name in masks_for(*hw):
        for ignore in (None, 255):
            m, d2 = want_distance(*hw, name, radius, ignore)
            got = _gpu_weights(dev, m, radius, table, ignore)
            want = _want_weights(d2, table)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, hw, radius, ignore, int((got != want).sum()))
            assert ignore is None or (got[m == 255] == 0).all()


def test_border_weights_radius_254_profile_batch_alignment_and_full_write(dev):
    from pylc_amd import boundary
    from pylc_amd.lib import lib, check, ptr, stream
    from tests import _regions as R
    from tests.test_boundary_gpu import masks_for, want_distance
    # radius 254: a table of 64 518 cells, the window larger than the image
    table = _table(254)
    assert table.size == 64518
    for name in masks_for(9, 255):
        for ignore in (None, 255):
            m, d2 = want_distance(9, 255, name, 254, ignore)
            assert np.array_equal(_gpu_weights(dev, m, 254, table, ignore).view(np.int32), _want_weights(d2, table).view(np.int32)), (name, ignore)
    # the default profile, through w0 / sigma
    m, d2 = want_distance(65, 129, 'blobs9', 3, 255)
    got = boundary.border_weights(torch.from_numpy(m).to(dev), 3, w0=10.0, sigma=2.0, ignore_index=255).cpu().numpy()
    assert np.array_equal(got.view(np.int32), _want_weights(d2, _profile()).view(np.int32)) and got.max() == _profile()[1]          # (d2 = 1 next to a border: no labelled pixel has 0)
    # B = 3 equals three single images
    h, w = 70, 131
    imgs = np.stack([R.blobs(h, w, 9, 1, radius=3), R.noise(h, w, 4, 3), R.checkerboard(h, w)])
    for radius in (3, 70):
        tab = _table(radius, 1)
        got = _gpu_weights(dev, imgs, radius, tab)
        for i in range(3):
            assert np.array_equal(got[i].view(np.int32), _gpu_weights(dev, imgs[i], radius, tab).view(np.int32)), (radius, i)
            assert np.array_equal(got[i].view(np.int32), _want_weights(Bd.distance_ref(imgs[i], radius), tab).view(np.int32))
    # a mask at byte offsets 1..3, and an output prefilled with NaN is written everywhere
    h, w = 100, 333
    m = Bd.scatter_ignore(R.blobs(h, w, 9, 5, radius=3, noise_frac=0.02), 0.05, seed=6)
    tab = _table(5)
    want = _want_weights(Bd.distance_ref(m, 5, 255), tab)
    flat, td = torch.from_numpy(m).to(dev).reshape(-1), torch.from_numpy(tab).to(dev)
    for off in (0, 1, 2, 3):
        buf = torch.zeros(h * w + 8, device=dev, dtype=torch.uint8)
        view = buf[off:off + h * w]
        view.copy_(flat)
        assert view.data_ptr() % 4 == off
        out = torch.full((h, w), float('nan'), device=dev)
        ws = torch.empty(lib.pylc_boundary_workspace_bytes(1, h, w) // 4, device=dev, dtype=torch.int32)
        check(lib.pylc_boundary_weights(ptr(view), 1, h, w, 5, 255, ptr(td), ptr(out), ptr(ws), stream()))
        got = out.cpu().numpy()
        assert not np.isnan(got).any() and np.array_equal(got.view(np.int32), want.view(np.int32)), off
    # a map value above R*R + 1 (no map of this radius holds one) reads the saturated cell
    d2 = torch.tensor([[-1, 0, 26, 27, 10 ** 6]], dtype=torch.int32, device=dev)
    assert boundary.weights_from_distance(d2, 5, tab).cpu().tolist() == [[0.0] + [float(tab[i]) for i in (0, 26, 26, 26)]]


# ---- 8: argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_border_weight_entry_points_refuse_bad_arguments_on_the_device(dev):
    from pylc_amd.lib import lib, ptr, stream
    m = torch.zeros((8, 8), device=dev, dtype=torch.uint8)
    d2 = torch.zeros((8, 8), device=dev, dtype=torch.int32)
    tab = torch.ones(11, device=dev)
    out = torch.full((8, 8), 7.0, device=dev)
    ws = torch.zeros(64, device=dev, dtype=torch.int32)

    def bw(mask=ptr(m), b=1, h=8, w=8, radius=3, ign=-1, table=ptr(tab), out=ptr(out), ws=ptr(ws)):
        return lib.pylc_boundary_weights(mask, b, h, w, radius, ign, table, out, ws, stream())

    def fd(d2=ptr(d2), n=64, radius=3, table=ptr(tab), out=ptr(out)):
        return lib.pylc_weights_from_d2(d2, n, radius, table, out, stream())

    def at(kw):          # the refusal lists name misaligned addresses by small numbers: here they are real buffers, shifted
        base = {'table': ptr(tab), 'out': ptr(out), 'ws': ptr(ws), 'd2': ptr(d2), 'mask': ptr(m)}
        return {k: (base[k] + v % 4 if k in base and v is not None and v < 256 else v) for k, v in kw.items()}
    for kw in boundary_weight_refusals():
        assert bw(**at(kw)) == 1 and b'boundary_weights' in lib.pylc_last_error(), kw
    for kw in from_d2_refusals():
        assert fd(**at(kw)) == 1 and b'weights_from_d2' in lib.pylc_last_error(), kw
    torch.cuda.synchronize()
    assert (out == 7).all()                                           # nothing was launched
    assert bw() == 0 and fd() == 0
    torch.cuda.synchronize()
    assert (out == 1).all()


# ---- 9: the whole step -------------------------------------------------------------------------------------------------------------------------------
BORDER = {'w0': 10.0, 'sigma': 2.0, 'radius': 3}


def _model(dev, arch, c, border):
    import oracle
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    runtime.dropout_enabled = False
    backbone = 'resnet' if arch == 'deeplab' else None
    model = Model(Meta(arch=arch, backbone=backbone or 'resnet', ch=3, n_classes=c, ignore_index=255, weighted=True,
                       weights=D.class_weights(c).tolist(), border_weight=border), dev).build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec(arch, backbone, c, 3), salt=5))
    seen = {}
    inner = model.crit.forward

    def spy(pred, target, pixel_weights=None):
        seen['logits'], seen['target'], seen['u'] = pred.detach().clone(), target, pixel_weights
        return inner(pred, target, pixel_weights)
    model.crit.forward = spy
    return model, seen


def _sampled(model):
    return [p.detach().reshape(-1)[::97].clone() for p in model.net.parameters()]


@pytest.mark.parametrize('arch', ['deeplab', 'unet'])
def test_network_step_with_border_weights(dev, arch):
    from pylc_amd import boundary, ops
    c = 9
    b, hw = (2, 64) if arch == 'deeplab' else (1, 256)
    x = D.tiles(860, b, 3, hw, hw)
    y = D.blob_masks(861, b, hw, hw, c, cell=8)
    y[ignore_blobs(862, (b, hw, hw), 0.3, cell=8)] = 255
    y8 = y.to(torch.uint8)
    (mb, sb), (m0, s0), (mp, sp) = (_model(dev, arch, c, border) for border in (dict(BORDER), dict(BORDER, w0=0.0), None))
    # Model.eval stays unweighted: the same validation losses with and without border_weight, on the same parameters
    for m in (mb, m0, mp):
        m.eval(x, y8)
    assert mb.loss.flush() == mp.loss.flush() and len(mb.loss.intv) == 1 and not sb
    # the step is its hand composition: net forward, border_weights on the cropped target, ops.multiloss(pixel_weights=)
    loss_b = mb.train(x, y8)
    yc = mb.crop_target(y8).to(dev)
    u = boundary.border_weights(yc, 3, _profile(), ignore_index=255)
    lg = sb['logits']
    assert tuple(yc.shape) == (lg.shape[0], lg.shape[2], lg.shape[3]) and torch.equal(sb['u'].view(torch.int32), u.view(torch.int32))
    want_u = _want_weights(Bd.distance_ref(yc.cpu().numpy(), 3, 255), _profile())
    assert np.array_equal(u.cpu().numpy().view(np.int32), want_u.view(np.int32)) and want_u.max() == _profile()[1]
    hand = ops.multiloss(sb['logits'], yc, torch.from_numpy(D.class_weights(c)).to(dev), *HALF, None, 255, None, u)
    assert torch.equal(hand[0], loss_b) and torch.equal(hand[1:], torch.stack((mb.crit.ce, mb.crit.dsc, mb.crit.fl)))
    ref = weighted_multiloss(sb['logits'].double().cpu(), yc.cpu(), u.cpu(), 255, HALF, torch.from_numpy(D.class_weights(c)).double())
    el = _loss_err(hand.cpu().tolist(), [v.item() for v in ref])
    print('PW9 %s: losses of the step against fp64 %.3g (bound %.3g), weights %.3g .. %.3g' % (arch, el, LOSS_REL, float(u[u > 0].min()), float(u.max())))
    assert el < LOSS_REL
    # w0 = 0: a map of ones (zero where the target is ignored), the step without border_weight bit for bit -- here on an int64 target,
    # which is converted to uint8 for the distance pass only
    loss_0, loss_p = m0.train(x, y), mp.train(x, y8)
    assert s0['target'].dtype == torch.int64 and sp['target'].dtype == torch.uint8 and sp['u'] is None
    assert torch.equal(s0['u'], (s0['target'] != 255).float())
    assert torch.equal(loss_0, loss_p) and not torch.equal(loss_0, loss_b)
    for p, q in zip(_sampled(m0), _sampled(mp)):
        assert torch.equal(p, q)
    # an explicit map, a confidence say: cropped like the target, multiplied into the border map where there is one
    conf = torch.from_numpy(np.random.RandomState(863).rand(b, hw, hw).astype(np.float32)).to(dev)
    mp.train(x, y8, pixel_weights=conf)
    assert torch.equal(sp['u'], mp.crop_target(conf))
    mb.train(x, y8, pixel_weights=conf)
    assert torch.equal(sb['u'], torch.mul(u, mb.crop_target(conf)))
    torch.cuda.synchronize()
    for m in (mp, mb):
        assert all(torch.isfinite(p).all() for p in m.net.parameters())
        m.log()                                           # no bad weight was counted
