"""The ignore label on the GPU (-m gpu).

  1  the loss head with an ignore label (pylc_multiloss_stats_ex / _finalize_ex / _bwd_ex, ops.multiloss(ignore_index=), the
     pylc_hip::multiloss_ignore operator) against the fp64 statement of tests/test_cpu_ignore_label.py (masked sums; proven there against
     F.cross_entropy(ignore_index=) and the oracle), within the bounds the project already holds this kernel to: 2e-6 max(1, |x|) per loss
     term, 1e-5 of the largest gradient entry (test_multiloss_golden).  Bit for bit: nothing ignored == the entry points without _ex; uint8
     targets (at an odd byte address too) == int64 targets; rows of skipped pixels all +0.0 up to round4(C); valid rows == pylc_multiloss_bwd
     on the compacted valid pixels with the same statistics; no valid pixel -> exact zeros everywhere.  Bad targets are counted, two shards
     with very different valid counts give the single-batch result.
  2  pylc_logits_score_ex and pylc_confusion_matrix_ex against numpy counts of the valid pixels, exactly; pylc_class_encode_resize_ex.
  3  extract_photo(ignore_index=) -> TileSet.profile / oversample_rates / oversample at tile 128 against numpy counts and the augmentation
     restatement of tests/test_cpu_augment.py.
  4  a U-Net and a DeepLab/ResNet-101 step with Meta(ignore_index=255) on uint8 targets; ScoreLog rows; PhotoEvaluator.

Every comparison prints its figures next to its bound (lines `IG1` .. `IG4` under `pytest -s`)."""
import functools

import numpy as np
import pytest
import torch

from tests import _data as D
from tests.test_cpu_ignore_label import ignore_blobs, masked_multiloss, valid_pixels
from tests.test_ops_gpu import rel_err

pytestmark = pytest.mark.gpu

LOSS_REL = 2e-6           # test_multiloss_golden's bounds, as in tests/test_class_counts_gpu.py
GRAD_REL = 1e-5
HALF = (0.5, 0.5, 0.5)
SHAPES = {'35px': (1, 5, 7), '2880px': (2, 40, 36), '270336px': (2, 384, 352)}
CLASS_COUNTS = (2, 3, 9, 11, 16)
PATTERNS = ('none', 'blobs30', 'class_absent', 'all_but_one', 'all', 'index0')


def r4(c):
    return (c + 3) & ~3


def _pitches(c):
    return (c, r4(c), r4(c) + 4)


# ---- inputs and the fp64 statement, computed once and only read ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _logits(shape_id, c):
    b, h, w = SHAPES[shape_id]
    return torch.from_numpy((np.random.RandomState(700 + c + b * h).standard_normal((b, c, h, w)) * 3).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _target(shape_id, c, pattern, ignore):
    """int64 [B,H,W] class indices from tests/_data.blob_masks with `ignore` written by the pattern"""
    b, h, w = SHAPES[shape_id]
    cell = 2 if h < 16 else 4 if h < 100 else 16
    t = D.blob_masks(710 + c, b, h, w, c, cell=cell)
    if pattern == 'index0':
        assert ignore == 0                     # the index is a class: its pixels are ignored, its logit stays
    elif pattern == 'blobs30':
        t[ignore_blobs(711 + c, (b, h, w), 0.3, cell=cell)] = ignore
    elif pattern == 'class_absent':
        t[ignore_blobs(712 + c, (b, h, w), 0.3, cell=cell)] = ignore
        t[t == c - 1] = ignore                 # the last class has no valid pixel: a Dice term with zero count
    elif pattern == 'all_but_one':
        keep = int(t[-1, h // 2, w // 2])
        t[:] = ignore
        t[-1, h // 2, w // 2] = keep
    elif pattern == 'all':
        t[:] = ignore
    return t


@functools.lru_cache(maxsize=None)
def _want(shape_id, c, pattern, ignore, weighted, weights=HALF):
    """the statement in fp64: ([total, ce, dice, focal], d total / d logits)"""
    z, t = _logits(shape_id, c), _target(shape_id, c, pattern, ignore)
    cw = torch.from_numpy(D.class_weights(c)).double() if weighted else None
    zr = z.double().requires_grad_(True)
    out = masked_multiloss(zr, t, ignore, weights, cw)
    out[0].backward()
    return [v.item() for v in out], zr.grad.detach()


def _loss_err(got, want):
    return max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(got, want))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
def _rows(dev, z, pitch):
    """the [N][pitch] pixel rows of [B,C,H,W] logits, 1e9 in the unused lanes"""
    b, c, h, w = z.shape
    buf = torch.full((b * h * w, pitch), 1e9, dtype=torch.float32)
    buf[:, :c] = z.permute(0, 2, 3, 1).reshape(-1, c)
    return buf.to(dev)


def _as_target(dev, t, kind):
    """flat device target: 'i64', 'u8', or 'u8odd' (a uint8 slice that starts at an odd byte address)"""
    t = t.reshape(-1)
    if kind == 'i64':
        return t.to(dev)
    u = t.to(torch.uint8)
    assert torch.equal(u.long(), t)
    if kind == 'u8':
        return u.to(dev)
    buf = torch.zeros(t.numel() + 3, dtype=torch.uint8, device=dev)
    out = buf[3:]
    out.copy_(u)
    assert out.data_ptr() % 2 == 1
    return out


def _ex(dev, rows, pitch, target, c, ignore, cw, dpitch, weights=HALF, stats_in=None):
    """pylc_multiloss_stats_ex -> _finalize_ex -> _bwd_ex: (stats, losses, dlogits [N, dpitch] NaN-prefilled, amax bits, n_bad)"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    n = target.numel()
    stats = torch.full((3 + 3 * c,), float('nan'), device=dev)
    ws = torch.empty(lib.pylc_multiloss_workspace_floats(n, c), device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib.pylc_multiloss_stats_ex(ptr(rows), pitch, ptr(target), target.element_size(), n, c, ignore, ptr(cw), ptr(stats), ptr(ws), ptr(bad),
                                      stream()))
    use = stats if stats_in is None else stats_in
    losses = torch.full((4,), float('nan'), device=dev)
    check(lib.pylc_multiloss_finalize_ex(ptr(use), c, *weights, ptr(losses), stream()))
    dl = torch.full((n, dpitch), float('nan'), device=dev)
    amax = torch.full((1,), -1, dtype=torch.int32, device=dev)
    check(lib.pylc_multiloss_bwd_ex(ptr(rows), pitch, ptr(target), target.element_size(), n, c, ignore, ptr(cw), ptr(use), *weights, None, ptr(dl),
                                    dpitch, ptr(amax), stream()))
    return stats, losses, dl, amax, bad


def _old(dev, rows, pitch, target, c, cw, dpitch, weights=HALF, stats_in=None, n_global=None):
    """the entry points without _ex on int64 targets: (stats, losses, dlogits, amax bits)"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    n = target.numel()
    stats = torch.full((3 + 3 * c,), float('nan'), device=dev)
    ws = torch.empty(lib.pylc_multiloss_workspace_floats(n, c), device=dev)
    check(lib.pylc_multiloss_stats(ptr(rows), pitch, ptr(target), n, c, ptr(cw), ptr(stats), ptr(ws), stream()))
    use = stats if stats_in is None else stats_in
    ng = float(n if n_global is None else n_global)
    losses = torch.full((4,), float('nan'), device=dev)
    check(lib.pylc_multiloss_finalize(ptr(use), ng, c, *weights, ptr(losses), stream()))
    dl = torch.full((n, dpitch), float('nan'), device=dev)
    amax = torch.full((1,), -1, dtype=torch.int32, device=dev)
    check(lib.pylc_multiloss_bwd(ptr(rows), pitch, ptr(target), n, c, ptr(cw), ptr(use), ng, *weights, None, ptr(dl), dpitch, ptr(amax), stream()))
    return stats, losses, dl, amax


def _grad_nchw(dl, shape_id, c):
    b, h, w = SHAPES[shape_id]
    return dl[:, :c].reshape(b, h, w, c).permute(0, 3, 1, 2)


def _check_rows(dl, c, dpitch, skipped):
    """pad lanes [C, round4(C)) zero, lanes beyond untouched, skipped pixels' rows +0.0 in every stored lane"""
    cstore = r4(c) if r4(c) <= dpitch else c
    dl = dl.cpu()
    assert torch.equal(dl[:, c:cstore], torch.zeros(dl.shape[0], cstore - c))
    assert torch.isnan(dl[:, cstore:]).all()
    rows = dl[skipped][:, :cstore]
    assert torch.equal(rows, torch.zeros_like(rows)) and not torch.signbit(rows).any()
    assert torch.isfinite(dl[:, :cstore]).all()


def _cases():
    """shape x C x weighted, each with an ignore pattern list; pitches and target kinds go round so that every one meets every C"""
    out = []
    k = 0
    for shape_id in SHAPES:
        for c in CLASS_COUNTS:
            for weighted in (False, True):
                pats = PATTERNS if shape_id != '270336px' else ('blobs30', 'all_but_one')
                out.append(pytest.param(shape_id, c, weighted, pats, k, id='%s-C%d-%s' % (shape_id, c, 'w' if weighted else 'u')))
                k += 1
    return out


@pytest.mark.parametrize('shape_id,c,weighted,patterns,k', _cases())
def test_loss_head_against_the_fp64_statement(dev, shape_id, c, weighted, patterns, k):
    z = _logits(shape_id, c)
    cw = torch.from_numpy(D.class_weights(c)).to(dev) if weighted else None
    kinds = (('i64', -100), ('i64', 255), ('u8', 255), ('u8odd', 255))
    for i, pattern in enumerate(patterns):
        kind, ignore = kinds[(k + i) % 4]
        if pattern == 'index0':
            ignore = 0
        pitch, dpitch = _pitches(c)[(k + i) % 3], _pitches(c)[(k + i + 1) % 3]
        t = _target(shape_id, c, pattern, ignore)
        want, g = _want(shape_id, c, pattern, ignore, weighted)
        stats, losses, dl, amax, bad = _ex(dev, _rows(dev, z, pitch), pitch, _as_target(dev, t, kind), c, ignore, cw, dpitch)
        torch.cuda.synchronize()
        got = losses.cpu().tolist()
        valid = valid_pixels(t, c, ignore).reshape(-1)
        el, eg = _loss_err(got, want), rel_err(_grad_nchw(dl, shape_id, c), g)
        print('IG1 %s C %2d %s %-12s %-5s ign %4d pitch %2d/%2d valid %6d: losses %.3g (bound %.3g)  grad %.3g (bound %.3g)'
              % (shape_id, c, 'w' if weighted else 'u', pattern, kind, ignore, pitch, dpitch, int(valid.sum()), el, LOSS_REL, eg, GRAD_REL))
        assert el < LOSS_REL and eg < GRAD_REL
        assert int(bad) == 0 and float(stats[3 + 2 * c:].sum()) == float(valid.sum())
        _check_rows(dl, c, dpitch, ~valid)
        assert amax.view(torch.float32).item() == dl[:, :c].abs().max().item()
        if not valid.any():                          # no valid pixel: exact zeros, nothing divided by zero
            assert got == [0.0, 0.0, 0.0, 0.0] and int(amax) == 0 and torch.isfinite(stats).all()
            assert torch.equal(stats.cpu(), torch.zeros(3 + 3 * c))


@pytest.mark.parametrize('c', CLASS_COUNTS)
@pytest.mark.parametrize('shape_id', list(SHAPES))
def test_bit_for_bit_pins(dev, shape_id, c):
    z = _logits(shape_id, c)
    cw = torch.from_numpy(D.class_weights(c)).to(dev)
    for pitch in _pitches(c):
        rows = _rows(dev, z, pitch)
        # nothing ignored: the _ex path on int64 targets is the path without _ex, whatever the index
        t = _target(shape_id, c, 'none', 255)
        ti = _as_target(dev, t, 'i64')
        for w in (None, cw):
            old = _old(dev, rows, pitch, ti, c, w, pitch)
            for ignore in (255, -100):
                new = _ex(dev, rows, pitch, ti, c, ignore, w, pitch)
                for a, b in zip(old, new[:4]):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (pitch, ignore)
        # uint8 == int64 for equal values, at an odd byte address too
        t = _target(shape_id, c, 'blobs30', 255)
        ref = _ex(dev, rows, pitch, _as_target(dev, t, 'i64'), c, 255, cw, pitch)
        for kind in ('u8', 'u8odd'):
            got = _ex(dev, rows, pitch, _as_target(dev, t, kind), c, 255, cw, pitch)
            for a, b in zip(ref, got):
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), kind
        # valid rows == pylc_multiloss_bwd on the compacted valid pixels, given the same statistics and n_global = n_valid
        valid = valid_pixels(t, c, 255).reshape(-1)
        sel = valid.to(dev)
        crow, ct = rows[sel].contiguous(), _as_target(dev, t, 'i64')[sel].contiguous()
        comp = _old(dev, crow, pitch, ct, c, cw, pitch, stats_in=ref[0], n_global=int(valid.sum()))
        cstore = r4(c) if r4(c) <= pitch else c
        assert torch.equal(ref[2][sel][:, :cstore].view(torch.int32), comp[2][:, :cstore].view(torch.int32)), pitch
        assert torch.equal(ref[1].view(torch.int32), comp[1].view(torch.int32)) and int(ref[3]) == int(comp[3])
        _check_rows(ref[2], c, pitch, ~valid)


def test_no_valid_pixel_through_the_python_layers(dev):
    from pylc_amd import ops
    from pylc_amd.loss import MultiLoss
    c = 9
    z = _logits('2880px', c).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    raw = []
    z.register_hook(raw.append)
    t = torch.full(SHAPES['2880px'], 255, dtype=torch.uint8, device=dev)
    crit = MultiLoss({'weighted': True, 'weights': D.class_weights(c), 'ce': 0.5, 'dice': 0.5, 'focal': 0.5}, {'n_classes': c}, ignore_index=255).to(dev)
    loss = crit(z, t)
    loss.backward()
    assert loss.item() == 0.0 and [float(crit.ce), float(crit.dsc), float(crit.fl)] == [0.0, 0.0, 0.0]
    assert ops.pitch_of(raw[0]) == 12 and float(raw[0].abs().max()) == 0.0 and float(z.grad.abs().max()) == 0.0
    assert int(crit.bad_targets) == 0
    for name in ('ce_loss', 'dice_loss', 'focal_loss'):
        assert getattr(crit, name)(z.detach(), t).item() == 0.0
    with pytest.raises(Exception, match='int64'):          # without an index: today's path, int64 only
        ops.multiloss(z.detach(), t, None, *HALF)


def test_bad_targets_are_skipped_and_counted(dev):
    """a mask holding 12 with C = 9 and index 255, weighted: the losses are the statement's with those pixels removed, n_bad their number;
    no class weight or logit is read with them as an index (by construction: the kernel tests the range before anything else)"""
    c, shape_id = 9, '2880px'
    z = _logits(shape_id, c)
    t = _target(shape_id, c, 'blobs30', 255).clone()
    stray = ignore_blobs(900, SHAPES[shape_id], 0.1, cell=4)
    t[stray & (t != 255)] = 12
    n_bad = int((t == 12).sum())
    assert n_bad > 50 and int((t == 255).sum()) > 500
    cwh = torch.from_numpy(D.class_weights(c))
    zr = z.double().requires_grad_(True)
    out = masked_multiloss(zr, t, 255, HALF, cwh.double())
    out[0].backward()
    removed = masked_multiloss(z.double(), torch.where(t == 12, torch.full_like(t, 255), t), 255, HALF, cwh.double())
    assert [v.item() for v in out] == [v.item() for v in removed]
    for kind in ('i64', 'u8'):
        stats, losses, dl, amax, bad = _ex(dev, _rows(dev, z, 12), 12, _as_target(dev, t, kind), c, 255, cwh.to(dev), 12)
        el, eg = _loss_err(losses.cpu().tolist(), [v.item() for v in out]), rel_err(_grad_nchw(dl, shape_id, c), zr.grad)
        print('IG1 bad targets %s: n_bad %d  losses %.3g (bound %.3g)  grad %.3g (bound %.3g)' % (kind, int(bad), el, LOSS_REL, eg, GRAD_REL))
        assert int(bad) == n_bad and el < LOSS_REL and eg < GRAD_REL
        _check_rows(dl, c, 12, ~valid_pixels(t, c, 255).reshape(-1))
    neg = t.clone()
    neg[t == 12] = -7                                    # int64 only: a negative target other than the index is bad too
    neg[t == 255] = -100
    assert int(_ex(dev, _rows(dev, z, 12), 12, _as_target(dev, neg, 'i64'), c, -100, None, 12)[4]) == n_bad
    # the counter is ADDED into: MultiLoss keeps it across calls
    from pylc_amd.loss import MultiLoss
    crit = MultiLoss({'weighted': False, 'weights': None, 'ce': 0.5, 'dice': 0.5, 'focal': 0.5}, {'n_classes': c}, ignore_index=255).to(dev)
    zd = z.to(dev).contiguous(memory_format=torch.channels_last)
    crit(zd, t.to(dev))
    crit(zd, t.to(torch.uint8).to(dev))
    assert int(crit.bad_targets) == 2 * n_bad


@pytest.mark.parametrize('c', [2, 9, 16])
def test_two_shards_with_different_valid_counts(dev, c):
    """MultiLossFn's wire format with a group: the statistics of two half batches, added, and each half's backward on the sum.  The second
    half is entirely ignored and the first about a third: n * world would be wrong by a factor of three, the class counts are right."""
    shape_id = '2880px'
    b, h, w = SHAPES[shape_id]
    z = _logits(shape_id, c)
    t = _target(shape_id, c, 'blobs30', 255).clone()
    t[1] = 255
    cwh = torch.from_numpy(D.class_weights(c))
    zr = z.double().requires_grad_(True)
    out = masked_multiloss(zr, t, 255, HALF, cwh.double())
    out[0].backward()
    want = [v.item() for v in out]
    pitch = r4(c)
    rows, td, cw = _rows(dev, z, pitch), _as_target(dev, t, 'u8'), cwh.to(dev)
    n = h * w
    parts = [_ex(dev, rows[i * n:], pitch, td[i * n:(i + 1) * n], c, 255, cw, pitch)[0] for i in range(2)]
    assert float(parts[1].abs().sum()) == 0.0 and float(parts[0][3 + 2 * c:].sum()) == float((t[0] != 255).sum())
    stats = parts[0] + parts[1]
    halves = [_ex(dev, rows[i * n:], pitch, td[i * n:(i + 1) * n], c, 255, cw, pitch, stats_in=stats) for i in range(2)]
    single = _ex(dev, rows, pitch, td, c, 255, cw, pitch)
    dl = torch.cat([halves[0][2], halves[1][2]])
    for i in range(2):
        assert _loss_err(halves[i][1].cpu().tolist(), want) < LOSS_REL
    el, eg = _loss_err(halves[0][1].cpu().tolist(), want), rel_err(_grad_nchw(dl, shape_id, c), zr.grad)
    print('IG1 two shards C %2d: losses %.3g (bound %.3g)  grad %.3g (bound %.3g)' % (c, el, LOSS_REL, eg, GRAD_REL))
    assert eg < GRAD_REL and float(halves[1][2][:, :pitch].abs().max()) == 0.0 and int(halves[1][3]) == 0
    assert _loss_err(single[1].cpu().tolist(), want) < LOSS_REL and rel_err(_grad_nchw(single[2], shape_id, c), zr.grad) < GRAD_REL


def test_ops_multiloss_and_the_custom_op(dev):
    import pylc_amd  # noqa: F401
    from pylc_amd import ops
    from torch.library import opcheck
    c, shape_id = 9, '2880px'
    z, t = _logits(shape_id, c), _target(shape_id, c, 'blobs30', 255)
    want, g = _want(shape_id, c, 'blobs30', 255, True)
    cw = torch.from_numpy(D.class_weights(c)).to(dev)
    res = []
    for target in (t.to(dev), t.to(torch.uint8).to(dev)):
        zd = z.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        losses = ops.multiloss(zd, target, cw, *HALF, None, 255, bad)
        (3 * losses[0]).backward()                       # grad_scale
        el, eg = _loss_err(losses.detach().cpu().tolist(), want), rel_err(zd.grad, 3 * g)
        print('IG1 ops.multiloss %s: losses %.3g (bound %.3g)  grad x3 %.3g (bound %.3g)' % (target.dtype, el, LOSS_REL, eg, GRAD_REL))
        assert el < LOSS_REL and eg < GRAD_REL and int(bad) == 0
        res.append((losses.detach(), zd.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    zd = z.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    losses, stats, bad = torch.ops.pylc_hip.multiloss_ignore(zd, t.to(torch.uint8).to(dev), cw, *HALF, 255)
    (3 * losses[0]).backward()
    assert torch.equal(losses.detach(), res[1][0]) and torch.equal(zd.grad, res[1][1]) and int(bad) == 0 and stats.numel() == 3 + 3 * c
    zs = _logits('35px', c).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ts = _target('35px', c, 'blobs30', 255).to(torch.uint8).to(dev)
    opcheck(torch.ops.pylc_hip.multiloss_ignore.default, (zs, ts, cw, 0.5, 0.5, 0.5, 255), test_utils=('test_schema', 'test_faketensor',
                                                                                                    'test_autograd_registration'))


# ---- 2: scores and the encoder ------------------------------------------------------------------------------------------------------------------
def _score_target(c, ignore, seed):
    """[2,40,36] int64: classes in blobs, about 30 % `ignore`, a few out-of-range values"""
    shape = SHAPES['2880px']
    t = D.blob_masks(seed, *shape, c, cell=4)
    t[ignore_blobs(seed + 1, shape, 0.3)] = ignore
    rs = np.random.RandomState(seed + 2)
    stray = torch.from_numpy(rs.rand(*shape) < 0.02)
    t[stray & (t != ignore)] = c if ignore != c else c + 1
    return t


def _counts_np(t, p, c, ignore):
    """(matrix of the valid pixels, bad, ignored)"""
    t, p = t.reshape(-1), p.reshape(-1)
    ign = t == ignore
    bad = ~ign & ((t < 0) | (t >= c))
    ok = ~ign & ~bad
    cm = np.zeros((c, c), np.int64)
    np.add.at(cm, (t[ok], p[ok]), 1)
    return cm, int(bad.sum()), int(ign.sum())


@pytest.mark.parametrize('c', [2, 9, 16])
def test_logits_score_ex_counts(dev, c):
    from pylc_amd import metrics
    from tests.test_score_gpu import _nchw_view
    shape = SHAPES['2880px']
    n = 2880
    rows = np.random.RandomState(800 + c).standard_normal((n, c)).astype(np.float32)
    pred = rows.argmax(-1)
    for pitch in (r4(c), r4(c) + 1, c):                 # pitch % 4 == 0 and not
        x = _nchw_view(dev, rows, shape, pitch)
        for ignore, dtype in ((255, torch.uint8), (255, torch.int64), (-100, torch.int64), (0, torch.uint8)):
            t = _score_target(c, ignore, 810 + c)
            cm, bad, ign = _counts_np(t.numpy(), pred, c, ignore)
            counts, mask = metrics.logits_confusion(x, t.to(dtype).to(dev), return_mask=True, ignore_index=ignore)
            got = counts.cpu().numpy()
            assert got.shape == (c * c + 2,) and np.array_equal(got[:c * c].reshape(c, c), cm) and (got[c * c], got[c * c + 1]) == (bad, ign)
            assert bad > 0 and ign > 500 and cm.sum() + bad + ign == n and np.array_equal(mask.cpu().numpy().reshape(-1), pred)
            metrics.logits_confusion(x, t.to(dtype).to(dev), counts=counts, ignore_index=ignore)          # ADDS into counts
            assert np.array_equal(counts.cpu().numpy(), 2 * got)
    # without an index: today's counts, C*C + 1 cells, the ignored pixels in the out-of-range cell
    t = _score_target(c, 255, 810 + c)
    plain = metrics.logits_confusion(x, t.to(dev)).cpu().numpy()
    cm, bad, ign = _counts_np(t.numpy(), pred, c, 255)
    assert plain.shape == (c * c + 1,) and np.array_equal(plain[:-1].reshape(c, c), cm) and plain[-1] == bad + ign


@pytest.mark.parametrize('c', [2, 9, 16])
def test_confusion_matrix_ex_counts(dev, c):
    from pylc_amd import metrics
    rs = np.random.RandomState(820 + c)
    for ignore, tdt, pdt in ((255, torch.uint8, torch.uint8), (-100, torch.int64, torch.uint8), (255, torch.int64, torch.int64),
                             (0, torch.uint8, torch.int64)):
        t = _score_target(c, ignore, 830 + c)
        p = torch.from_numpy(rs.randint(0, c, t.shape))
        for cover in (False, True):
            tn, pn = t.numpy().reshape(-1).copy(), p.numpy().reshape(-1).copy()
            if cover:
                tn[:c] = pn[:c] = np.arange(c)
            cm, bad, ign = _counts_np(tn, pn, c, ignore)
            skipped = torch.zeros(2, dtype=torch.int64, device=dev)
            got = metrics.confusion_matrix(t.to(tdt).to(dev), p.to(pdt).to(dev), c, force_coverage=cover, ignore_index=ignore, skipped=skipped)
            assert np.array_equal(got.cpu().numpy(), cm) and skipped.cpu().tolist() == [bad, ign], (ignore, cover)
            assert bad > 0 and ign > 500
    want = metrics.scores(cm)
    got = metrics.evaluate(t.to(tdt).to(dev), p.to(pdt).to(dev), c, ignore_index=ignore)
    assert all(abs(got[k] - want[k]) < 1e-12 for k in ('f1', 'iou', 'mcc'))


def _stray_mask(seed, h, w, pal):
    rs = np.random.RandomState(seed)
    cls = rs.randint(0, len(pal), (h, w))
    rgb = pal[cls]
    stray = rs.rand(h, w) < 0.05
    rgb[stray] = pal[cls[stray]] ^ 1                     # a colour one bit off its class's: no palette entry (checked below)
    return rgb, cls, stray


def test_class_encode_resize_ex(dev):
    from pylc_amd import photo
    from tests.test_cpu_photo import encode_resize_np
    from tests.test_photo_gpu import PALETTE
    h, w = 37, 53
    rgb, cls, stray = _stray_mask(840, h, w, PALETTE)
    assert 0.02 < stray.mean() < 0.08
    for oh, ow in ((h, w), (23, 31)):
        ref = photo.encode_mask(rgb, PALETTE, (oh, ow), dev)
        want = encode_resize_np(rgb, PALETTE, oh, ow)
        assert np.array_equal(ref.cpu().numpy(), want)
        sy = np.minimum(np.floor(np.arange(oh) * (1 / (oh / h))).astype(int), h - 1)
        sx = np.minimum(np.floor(np.arange(ow) * (1 / (ow / w))).astype(int), w - 1)
        st = stray[sy][:, sx]
        assert st.any() and (want[st] == 1).all()
        from pylc_amd.lib import lib, check, ptr, stream
        d_rgb, pal = torch.from_numpy(rgb).to(dev), torch.from_numpy(PALETTE).to(dev)
        one = torch.empty((oh, ow), dtype=torch.uint8, device=dev)
        check(lib.pylc_class_encode_resize_ex(ptr(d_rgb), h, w, ptr(pal), 9, ptr(one), oh, ow, 1, stream()))
        assert torch.equal(one, ref)                     # value 1 is the existing entry point
        for value, kw in ((255, {'unmatched': 255}), (255, {'unmatched': 'ignore', 'ignore_index': 255}), (0, {'unmatched': 0}), (77, {'unmatched': 77})):
            got = photo.encode_mask(rgb, PALETTE, (oh, ow), dev, **kw).cpu().numpy()
            assert (got[st] == value).all() and np.array_equal(got[~st], want[~st]), (oh, ow, value)


# ---- 3: tiles, profile, oversampling ----------------------------------------------------------------------------------------------------------
def test_extract_profile_and_oversample_with_an_ignore_band(dev):
    from pylc_amd import dataset
    from tests.test_augment_gpu import _compare
    from tests.test_cpu_augment import augment_np, augment_params_np
    from tests.test_cpu_dataset import tile_sums_np
    from tests.test_photo_gpu import PALETTE, photo_np
    t, k, h, w = 128, 9, 300, 420
    image = photo_np(850, h, w)
    cls = D.blob_masks(851, 1, h, w, k, cell=16)[0].numpy()
    mask_rgb = PALETTE[cls]
    mask_rgb[100:140] = (1, 2, 3)                        # an unpainted band, and a few stray colours elsewhere
    mask_rgb[np.random.RandomState(852).rand(h, w) < 0.01] = (9, 9, 9)
    with pytest.raises(ValueError, match='ignore_index=3'):
        dataset.extract_photo(image, mask_rgb, PALETTE, tile=t, stride=96, ignore_index=3, device=dev)
    ex = dataset.extract_photo(image, mask_rgb, PALETTE, tile=t, stride=96, ignore_index=255, device=dev)
    n = ex.img.shape[0]
    assert n == 8 and ex.ignore_index == 255          # 2 x 4 tiles
    masks = ex.mask.cpu().numpy()
    assert set(np.unique(masks)) <= set(range(k)) | {255} and (masks == 255).mean() > 0.1
    sums_np, hist_np = tile_sums_np(ex.img.cpu().numpy(), masks, k)
    assert np.array_equal(ex.hist.cpu().numpy(), hist_np) and np.array_equal(hist_np[:, -1], (masks == 255).reshape(n, -1).sum(1))
    # without the index the off-palette colours are class 1, as today; a mask value 255 is refused, as today
    plain = dataset.extract_photo(image, mask_rgb, PALETTE, tile=t, stride=96, device=dev)
    assert torch.equal(plain.mask == 1, (ex.mask == 1) | (ex.mask == 255)) and not plain.hist[:, -1].any()
    with pytest.raises(ValueError, match='class index >= n_classes'):
        dataset.TileSet(3, k, t).from_arrays(ex.img, ex.mask)
    with pytest.raises(ValueError, match='other than ignore_index=255'):
        dataset.TileSet(3, k, t, ignore_index=255).from_arrays(ex.img, torch.where(ex.mask == 255, torch.full_like(ex.mask, 200), ex.mask))
    ts = dataset.TileSet(3, k, t, ignore_index=255).add(ex)
    prof = ts.profile()
    assert prof == dataset.profile_from_sums(sums_np, hist_np, t, k, ignore=True)
    assert prof['dset_px_count'] == int((masks != 255).sum()) and prof['ignored_px_count'] == int((masks == 255).sum())
    assert prof['dset_px_dist'] == [int((masks == j).sum()) for j in range(k)]
    res = dataset.oversample_rates(prof, n_samples_ratio=2.0)
    rates = np.minimum(np.maximum(np.asarray(res['rates']), [1, 0, 2, 0, 0, 1, 0, 0]), 2)          # (some copies whatever the optimum was)
    out = ts.oversample(rates.tolist(), chunk=4)
    src, copy = dataset.oversample_layout(rates)
    assert len(out) == n + int(rates.sum()) and out.ignore_index == 255
    got_img, got_mask = out.img.cpu().numpy(), out.mask.cpu().numpy()
    imgs = ex.img.cpu().numpy()
    for pos in range(len(out)):
        if copy[pos] < 0:
            assert np.array_equal(got_mask[pos], masks[src[pos]])
        else:                                            # the restatement: nearest-neighbour on the mask, so 255 only where the warped source had it
            want = augment_np(imgs[src[pos]], masks[src[pos]], *augment_params_np(int(copy[pos]), t))
            _compare(got_img[pos], got_mask[pos], want, 'IG3 entry %d' % pos)
            assert (want['mask'] == 255).any()
    o_sums, o_hist = tile_sums_np(got_img, got_mask, k)
    assert np.array_equal(out.hist, o_hist) and out.profile() == dataset.profile_from_sums(o_sums, o_hist, t, k, ignore=True)
    with pytest.raises(ValueError, match='class index >= n_classes'):          # the same copies without the index: refused as today
        dataset.TileSet(3, k, t).from_arrays(out.img, out.mask)
    x, y = next(iter(out.coshuffle(3).batches(2)))
    assert y.dtype == torch.uint8 and tuple(y.shape) == (2, t, t)


# ---- 4: the networks ------------------------------------------------------------------------------------------------------------------------------
def _model(dev, arch, c, salt, ignore=255):
    import oracle
    from pylc_amd import runtime
    from pylc_amd.metrics import ScoreLog
    from pylc_amd.model import Model, Meta
    runtime.dropout_enabled = False
    backbone = 'resnet' if arch == 'deeplab' else None
    model = Model(Meta(arch=arch, backbone=backbone or 'resnet', ch=3, n_classes=c, ignore_index=ignore, weighted=True,
                       weights=D.class_weights(c).tolist()), dev)
    model.scores = ScoreLog(c)
    model.build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec(arch, backbone, c, 3), salt=salt))
    seen = {}
    inner = model.crit.forward

    def spy(pred, target):
        seen['logits'], seen['target'] = pred.detach().clone(), target
        if pred.requires_grad:
            pred.register_hook(lambda g_: seen.__setitem__('dl', g_.detach().clone()))
        return inner(pred, target)
    model.crit.forward = spy
    return model, seen


@pytest.mark.parametrize('arch', ['deeplab', 'unet'])
def test_network_step_with_ignored_pixels(dev, arch):
    from pylc_amd import metrics
    c = 9
    b, hw = (2, 64) if arch == 'deeplab' else (1, 256)
    x = D.tiles(860, b, 3, hw, hw)
    y = D.blob_masks(861, b, hw, hw, c, cell=8)
    y[ignore_blobs(862, (b, hw, hw), 0.3, cell=8)] = 255
    y8 = y.to(torch.uint8)
    models = [_model(dev, arch, c, 5) for _ in range(2)]
    losses = []
    for (model, seen), target in zip(models, (y8, y)):
        assert model.crit.ignore_index == 255 and model.scores.ignore_index == 255
        losses.append(model.train(x, target))
        assert seen['target'].dtype == target.dtype          # uint8 targets pass through unconverted
    torch.cuda.synchronize()
    (m8, s8), (m64, s64) = models
    # the loss is the statement on the net's own logits, dlogits is zero on the ignored pixels
    yc = m8.crop_target(y)
    out = masked_multiloss(s8['logits'].double().cpu(), yc, 255, HALF, torch.from_numpy(D.class_weights(c)).double())
    got = [losses[0].item(), float(m8.crit.ce), float(m8.crit.dsc), float(m8.crit.fl)]
    el = _loss_err(got, [v.item() for v in out])
    skipped = (yc == 255)
    dl = s8['dl'].cpu()
    print('IG4 %s: losses %.3g (bound %.3g), %d of %d pixels ignored' % (arch, el, LOSS_REL, int(skipped.sum()), skipped.numel()))
    assert el < LOSS_REL and 0.15 < skipped.float().mean() < 0.45
    assert float(dl.permute(0, 2, 3, 1)[skipped].abs().max()) == 0.0 and float(dl.permute(0, 2, 3, 1)[~skipped].abs().max()) > 0
    for p in m8.net.parameters():
        assert torch.isfinite(p).all()
    # int64 targets: the same bits
    assert torch.equal(losses[0], losses[1]) and torch.equal(s8['dl'], s64['dl'])
    for p, q in zip(m8.net.parameters(), m64.net.parameters()):
        assert torch.equal(p, q)
    # validation rows: 'ignored', and the scores of the valid-pixel matrix
    logits = m8.eval(x, y8)[0]
    m8.log()
    row = m8.scores.rows[-1]
    cm, bad, ign = _counts_np(yc.numpy(), logits.argmax(1).cpu().numpy(), c, 255)
    want = metrics.scores(cm)
    assert row['ignored'] == ign == int(skipped.sum()) and bad == 0 and np.array_equal(m8.scores.last_counts.numpy(), cm)
    assert (row['iou'], row['f1'], row['mcc']) == (want['iou'], want['f1'], want['mcc'])
    # an all-ignored batch: every filter gradient exactly zero, every parameter finite
    m8.net.train()
    m8.train(x, torch.full_like(y8, 255))
    torch.cuda.synchronize()
    assert float(m8.arena.g.abs().max()) == 0.0 and float(s8['dl'].abs().max()) == 0.0
    assert torch.isfinite(m8.arena.p).all()
    # a target that is neither a class nor the index is reported at the next log
    bad_y = y8.clone()
    bad_y[:, hw // 2, hw // 2] = 12
    m8.train(x, bad_y)
    with pytest.raises(ValueError, match=r'%d targets .* ignore_index=255' % b):
        m8.log()
    m8.log()                                              # the counter was cleared


def test_photo_evaluator_scores_the_valid_pixels(dev):
    from pylc_amd import photo
    from tests.test_photo_gpu import PALETTE
    c, h, w = 9, 70, 90
    rs = np.random.RandomState(870)
    gt_cls = D.blob_masks(871, 1, h, w, c, cell=8)[0].numpy()
    gt = PALETTE[gt_cls]
    gt[20:35] = (1, 2, 3)                                 # unpainted
    pred = np.where(rs.rand(h, w) < 0.3, rs.randint(0, c, (h, w)), gt_cls).astype(np.uint8)
    geom = {'h_scaled': h, 'w_scaled': w}
    assert photo.scaled_size(h, w, 64, None) == (h, w)
    res = photo.PhotoResult(torch.from_numpy(pred).to(dev), None, geom, None, 64, None)
    ev = photo.PhotoEvaluator(c, PALETTE, ignore_index=255)
    per = ev.add(res, gt)
    yt = np.where((gt == (1, 2, 3)).all(-1), 255, gt_cls).reshape(-1)
    yp = pred.reshape(-1).astype(np.int64)
    yt[:c] = yp[:c] = np.arange(c)                        # Evaluator.validate()'s coverage overwrite, as before
    cm, bad, ign = _counts_np(yt, yp, c, 255)
    assert bad == 0 and ign == 15 * w and np.array_equal(ev.cm.cpu().numpy(), cm)
    cmf = cm.astype(np.float64)
    tp, sup, prd, n = np.diag(cmf), cmf.sum(1), cmf.sum(0), cmf.sum()
    f1 = (2 * tp / (sup + prd) * sup).sum() / n
    iou = (tp / (sup + prd - tp) * sup).sum() / n
    mcc = (tp.sum() * n - (sup * prd).sum()) / np.sqrt((n * n - (prd ** 2).sum()) * (n * n - (sup ** 2).sum()))
    print('IG4 PhotoEvaluator: f1 %.6f iou %.6f mcc %.6f over %d of %d pixels' % (f1, iou, mcc, int(n), h * w))
    assert abs(per['f1'] - f1) < 1e-12 and abs(per['iou'] - iou) < 1e-12 and abs(per['mcc'] - mcc) < 1e-12
    # without the index the band is class 1, as today
    plain = photo.PhotoEvaluator(c, PALETTE)
    plain.add(res, gt)
    assert int(plain.cm.sum()) == h * w
