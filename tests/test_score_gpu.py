"""Validation scores on the GPU (-m gpu): pylc_logits_score -- the first maximum of every pixel's NHWC logits and the confusion counts of it
against the target, in one launch -- against numpy (`p = logits.argmax(-1)`, `np.add.at(cm, (t, p), 1)`), and the plumbing above it:
metrics.logits_confusion, ScoreLog, Model.predict, Model.eval / Model.log with `scores` set, trainer(score=True).  Every result is an
integer, so every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from tests import _data as D

pytestmark = pytest.mark.gpu


def _logits_np(seed, n, c, ties=False):
    rs = np.random.RandomState(seed)
    if ties:
        return rs.randint(-1, 2, (n, c)).astype(np.float32)
    return rs.standard_normal((n, c)).astype(np.float32)


def _nchw_view(dev, rows, shape, pitch, lead=0):
    """[B,C,H,W] tensor with NHWC memory of the given pitch whose pixel rows are `rows` [N,C]; `lead` floats precede it in its buffer"""
    b, h, w = shape
    n, c = rows.shape
    buf = torch.full((lead + n * pitch,), 1e9, dtype=torch.float32)           # pad lanes hold a value that would win the argmax
    buf[lead:].view(n, pitch)[:, :c] = torch.from_numpy(rows)
    buf = buf.to(dev)
    return buf[lead:].view(b, h, w, pitch)[..., :c].permute(0, 3, 1, 2)


def _want(rows, target, c):
    p = rows.argmax(-1)
    cm = np.zeros((c, c), np.int64)
    t = np.asarray(target).reshape(-1).astype(np.int64)
    ok = (t >= 0) & (t < c)
    np.add.at(cm, (t[ok], p[ok]), 1)
    return p.astype(np.uint8), cm, int((~ok).sum())


def _check(dev, rows, shape, target, c, pitch, lead=0):
    """mask only, counts only and both, against numpy"""
    from pylc_amd import metrics
    x = _nchw_view(dev, rows, shape, pitch, lead)
    p, cm, outside = _want(rows, target, c)
    t = target.to(dev)
    _, mask = metrics.logits_confusion(x, return_mask=True)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == shape and np.array_equal(mask.cpu().numpy().reshape(-1), p)
    counts = metrics.logits_confusion(x, t)
    assert counts.dtype == torch.int64 and counts.numel() == c * c + 1
    got = counts.cpu().numpy()
    assert np.array_equal(got[:-1].reshape(c, c), cm) and got[-1] == outside
    counts2, mask2 = metrics.logits_confusion(x, t, return_mask=True)
    assert torch.equal(counts2, counts) and torch.equal(mask2, mask)
    return got


# the four cases the file began with, then every other class count at pitch round4(C) (what a head writes), then a pitch one group of four wider
# than the classes fill for every C % 4 == 0 (at pitch C those have no pad lane at all)
SCORE_CASES = [(2, 4), (9, 12), (11, 12), (16, 16)]
SCORE_CASES += [(c, (c + 3) & ~3) for c in range(2, 17) if (c, (c + 3) & ~3) not in SCORE_CASES]
SCORE_CASES += [(c, c + 4) for c in range(4, 17, 4)]


@pytest.mark.parametrize('c,pitch', SCORE_CASES)
def test_counts_and_mask_match_numpy(dev, c, pitch):
    shape = (3, 37, 53)                                  # 5883 pixels: no multiple of 4, 64 or 256
    n = shape[0] * shape[1] * shape[2]
    rows = _logits_np(100 + c, n, c)
    blobs = D.blob_masks(7 + c, *shape, c)
    rand = D.masks(8 + c, *shape, c)
    for target in (blobs, rand, blobs.to(torch.uint8), rand.to(torch.uint8)):
        got = _check(dev, rows, shape, target, c, pitch)
        assert got[:-1].sum() == n


def test_ties_take_the_first_maximum(dev):
    shape, c = (3, 37, 53), 9
    rows = _logits_np(3, 5883, c, ties=True)
    srt = np.sort(rows, -1)
    assert (srt[:, -1] == srt[:, -2]).mean() > 0.5       # most pixels tie
    _check(dev, rows, shape, D.blob_masks(4, *shape, c), c, 12)


@pytest.mark.parametrize('shape', [(2, 384, 384), (1, 1, 1), (1, 1, 3), (1, 5, 13)])
def test_grid_stride_and_tiny_inputs(dev, shape):
    """The grid is capped at 256 blocks of 256 lanes with 4 pixels each, 262144 pixels per round: 2 x 384 x 384 = 294912 pixels take a
    second round in the first 32 blocks.  1, 3 and 65 pixels: less than a lane's group, less than a wave, one pixel more than 16 lanes."""
    c = 9
    n = shape[0] * shape[1] * shape[2]
    rows = _logits_np(n % 1000, n, c)
    _check(dev, rows, shape, D.blob_masks(5, *shape, c) if n > 65 else D.masks(5, *shape, c), c, 12)
    if n > 65:
        _check(dev, rows, shape, D.masks(6, *shape, c).to(torch.uint8), c, 12)


def test_layouts(dev):
    """a pitch wider than the classes need (a channel slice of a wider buffer), a base that is not 16-byte aligned (float-by-float loads),
    and a mask that does not start on a dword"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, ptr, stream
    shape, c = (3, 37, 53), 9
    n = 5883
    rows = _logits_np(21, n, c)
    target = D.blob_masks(22, *shape, c)
    _check(dev, rows, shape, target, c, 20)
    x = _nchw_view(dev, rows, shape, 12, lead=1)
    assert x.data_ptr() % 16 == 4
    _check(dev, rows, shape, target, c, 12, lead=1)
    _check(dev, rows, shape, target, c, 11, lead=0)      # pitch % 4 != 0
    L.init()
    p, cm, _ = _want(rows, target, c)
    x = _nchw_view(dev, rows, shape, 12)
    t = target.to(dev)
    for off in (1, 2, 3):
        buf = torch.full((n + 8,), 77, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 4 == 0
        counts = torch.zeros(c * c + 1, dtype=torch.int64, device=dev)
        assert lib.pylc_logits_score(x.data_ptr(), 12, ptr(t), 8, n, c, buf.data_ptr() + off, ptr(counts), stream()) == 0
        got = buf.cpu().numpy()
        assert np.array_equal(got[off:off + n], p) and (got[:off] == 77).all() and (got[off + n:] == 77).all()
        assert np.array_equal(counts.cpu().numpy()[:-1].reshape(c, c), cm)


def test_out_of_range_targets(dev):
    from pylc_amd import metrics
    shape, c = (3, 37, 53), 9
    rows = _logits_np(31, 5883, c)
    target = D.blob_masks(32, *shape, c)
    target[0, :5, :7] = c
    target[2, 30:, 50:] = 255
    n_out = 5 * 7 + 7 * 3
    for t in (target, target.to(torch.uint8)):
        got = _check(dev, rows, shape, t, c, 12)
        assert got[-1] == n_out and got[:-1].sum() == 5883 - n_out
    neg = target.clone()
    neg[neg == 255] = -3                                  # int64 only: a negative target is outside too
    assert _check(dev, rows, shape, neg, c, 12)[-1] == n_out
    log = metrics.ScoreLog(c)
    log.add(_nchw_view(dev, rows, shape, 12), target.to(dev))
    with pytest.raises(ValueError, match=r'\b%d\b' % n_out):
        log.close(0, 0)
    assert not log.rows and int(log.counts.abs().sum()) == 0


def test_accumulation_and_close(dev):
    from pylc_amd import metrics
    shape, c = (3, 37, 53), 9
    rows = [_logits_np(41 + i, 5883, c) for i in range(2)]
    targets = [D.blob_masks(43, *shape, c), D.masks(44, *shape, c).to(torch.uint8)]
    want = sum(_want(r, t, c)[1] for r, t in zip(rows, targets))
    counts = None
    log = metrics.ScoreLog(c)
    for r, t in zip(rows, targets):
        x = _nchw_view(dev, r, shape, 12)
        counts = metrics.logits_confusion(x, t.to(dev), counts=counts)
        log.add(x, t.to(dev))
    assert np.array_equal(counts.cpu().numpy()[:-1].reshape(c, c), want) and torch.equal(log.counts, counts)
    row = log.close(7, 1)
    assert np.array_equal(log.last_counts.numpy(), want) and int(log.counts.abs().sum()) == 0
    s = metrics.scores(want)
    assert (row['iter'], row['epoch']) == (7, 1) and (row['f1'], row['iou'], row['mcc']) == (s['f1'], s['iou'], s['mcc'])
    assert row['support'] == want.sum(1).tolist() and log.is_best and log.best_iou == s['iou']
    assert log.close(8, 1) is None and len(log.rows) == 1            # nothing added since


def test_argument_errors_launch_nothing(dev):
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, ptr, stream
    L.init()
    c, n = 9, 1024
    x = torch.randn(n, 12, device=dev)
    t8 = torch.zeros(n, dtype=torch.uint8, device=dev)
    mask = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    counts = torch.full((c * c + 1,), 5, dtype=torch.int64, device=dev)
    X, T, M, K, S = ptr(x), ptr(t8), ptr(mask), ptr(counts), stream()
    for args, word in (((X, 12, T, 1, n, c, None, None, S), b'both NULL'),
                       ((X, 12, None, 0, n, c, M, K, S), b'counts without target'),
                       ((X, 12, T, 4, n, c, M, K, S), b'target_bytes=4'),
                       ((X, 12, T, 0, n, c, M, K, S), b'disagree'),
                       ((X, 12, T, 1, 0, c, M, K, S), b'N=0'),
                       ((X, 12, T, 1, -4, c, M, K, S), b'N=-4'),
                       ((X, 12, T, 1, n, 1, M, K, S), b'n_classes=1'),
                       ((X, 12, T, 1, n, 17, M, K, S), b'n_classes=17'),
                       ((X, 8, T, 1, n, c, M, K, S), b'pitch=8'),
                       ((None, 12, T, 1, n, c, M, K, S), b'logits is NULL')):
        assert lib.pylc_logits_score(*args) == 1                      # PYLC_ERR_ARG
        assert word in lib.pylc_last_error(), (word, lib.pylc_last_error())
    torch.cuda.synchronize()                                          # nothing faulted
    assert (mask == 77).all() and (counts == 5).all()                 # and nothing was written


def _model(dev, arch, salt):
    import oracle
    from pylc_amd import runtime
    from pylc_amd.model import Meta, Model
    runtime.dropout_enabled = False
    model = Model(Meta(arch=arch, backbone='resnet'), dev).build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec(arch, 'resnet', 9, 3), salt=salt))
    return model


@pytest.mark.parametrize('arch,tile,out', [('deeplab', 64, 64), ('unet', 256, 68)])
def test_eval_and_log_score_the_validation_pass(dev, arch, tile, out):
    from pylc_amd import metrics
    model = _model(dev, arch, 6)
    model.scores = metrics.ScoreLog(9)
    want = np.zeros((9, 9), np.int64)
    for i in range(2):
        x, y = D.tiles(50 + i, 2, 3, tile, tile), D.blob_masks(60 + i, 2, tile, tile, 9, cell=8)
        y_hat = model.eval(x, y)[0]
        assert tuple(y_hat.shape) == (2, 9, out, out)
        rows = np.ascontiguousarray(y_hat.cpu().permute(0, 2, 3, 1).numpy()).reshape(-1, 9)
        want += _want(rows, model.crop_target(y).numpy(), 9)[1]
    model.iter, model.epoch = 12, 3
    model.log()
    assert len(model.scores.rows) == 1 and len(model.loss.valid) == 1
    row = model.scores.rows[0]
    assert np.array_equal(model.scores.last_counts.numpy(), want) and want.sum() == 4 * out * out
    s = metrics.scores(want)
    assert (row['f1'], row['iou'], row['mcc']) == (s['f1'], s['iou'], s['mcc']) and (row['iter'], row['epoch']) == (12, 3)
    assert row['support'] == want.sum(1).tolist()
    # Model.predict: the class masks of a tile batch, at the size the net returns
    x = D.tiles(70, 2, 3, tile, tile)
    mask = model.predict(x)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (2, out, out)
    assert torch.equal(mask.cpu().long(), model.test(x)[0].cpu().argmax(1))


def _tiny_run(dev, tmp_path, watch=True, **kw):
    """one epoch of trainer on three batches (a validation before and after); with `watch`, the best-model copy is removed before every
    Model.save so that each save shows whether it wrote one"""
    from pylc_amd import train
    model = _model(dev, 'deeplab', 5)
    tr = [(D.tiles(80 + i, 2, 3, 64, 64), D.blob_masks(90 + i, 2, 64, 64, 9, cell=8)) for i in range(3)]
    va = [(D.tiles(85 + i, 2, 3, 64, 64), D.blob_masks(95 + i, 2, 64, 64, 9, cell=8)) for i in range(2)]
    d = os.path.join(str(tmp_path), model.model_id())
    best = os.path.join(d, model.model_id() + '.pth')
    seen = []
    orig = model.save

    def save(save_dir):
        if watch and os.path.exists(best):
            os.remove(best)
        orig(save_dir)
        seen.append((bool(model.loss.is_best), model.scores is not None and bool(model.scores.is_best), os.path.exists(best)))
    model.save = save
    train.trainer(model, tr, va, 1, save_dir=str(tmp_path), **kw)
    return model, d, seen


def test_trainer_with_scores(dev, tmp_path):
    import json
    from pylc_amd import checkpoint
    from pylc_amd.model import Meta, Model
    model, d, seen = _tiny_run(dev, tmp_path, score=True, best_by='iou')
    assert model.best_by == 'iou' and len(model.scores.rows) == 2 and len(seen) == 2
    with open(os.path.join(d, 'scores.json')) as f:
        data = json.load(f)
    assert len(data['rows']) == 2 and data['rows'] == model.scores.rows and data['best_iou'] == model.scores.best_iou
    assert set(data['rows'][0]) == {'iter', 'epoch', 'f1', 'iou', 'mcc', 'class_iou', 'class_f1', 'support'}
    assert [r['iter'] for r in data['rows']] == [0, 3]
    # the best-model file follows the scores, not the Dice loss
    best, running = [], 0.0
    for r in data['rows']:
        best.append(r['iou'] > running)
        running = max(running, r['iou'])
    assert [s[1] for s in seen] == best and all(s[0] == s[1] == s[2] for s in seen) and running == data['best_iou']
    assert sorted(os.listdir(d)) == sorted(['checkpoint.pth', 'losses.pth', 'scores.json'] + ([model.model_id() + '.pth'] if seen[-1][2] else []))
    fresh = Model(Meta(arch='deeplab', backbone='resnet'), dev).build()
    assert fresh.scores is None
    checkpoint.load_into(fresh, os.path.join(d, 'checkpoint.pth'), resume=True)
    assert fresh.scores.best_iou == model.scores.best_iou and fresh.scores.rows == model.scores.rows
    with pytest.raises(ValueError, match='iou'):
        Model(Meta(), dev).best_by = 'iou'


def test_trainer_without_scores_leaves_no_trace(dev, tmp_path):
    model, d, seen = _tiny_run(dev, tmp_path, watch=False)
    assert model.scores is None and model.best_by == 'dice' and len(model.loss.valid) == 2
    assert seen[0] == (True, False, True)                              # the first validation is a new best Dice, as before
    assert sorted(os.listdir(d)) == sorted(['checkpoint.pth', 'losses.pth', model.model_id() + '.pth'])
    assert sorted(torch.load(os.path.join(d, 'losses.pth'), weights_only=True)) == ['best_dice', 'lr', 'test', 'train', 'valid']
