"""The window-weighted blend on the GPU (-m gpu, csrc/blend.hip, csrc/multiscale.hip): pylc_blend_window_sums and
pylc_blend_finalize_w against the float32 models of tests/_window.py bit for bit, the windowed entry points with a table of ones against
the plain entry points bit for bit, with real windows against the float64 statement, and predict_image / predict_overlap_tile /
segment_photo with window= against window=None and against their composition by hand."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import _multiscale as M
from tests import _window as Wn
from tests.test_blend_gpu import _accumulate, _finalize, _model_test_logits, _tiles_buffer
from tests.test_cpu_overlap_tile import overlap_origins
from tests.test_cpu_window import check_entry_points_refuse
from tests.test_unet_inference_gpu import reflect_windows

pytestmark = pytest.mark.gpu

H, W, OUT = Wn.H, Wn.W, Wn.OUT


def _table(name, dev, out=OUT):
    tab = np.ones(out, np.float32) if name == 'uniform' else Wn.case_window(name, out)
    return torch.from_numpy(tab).to(dev)


def _accumulate_w(acc, buf, c, h, w, out, stride, batch, win, flip=0, beta=1.0):
    from pylc_amd.lib import lib, check, ptr, stream
    n = buf.shape[0]
    for k in range(0, n, batch):
        b = min(batch, n - k)
        check(lib.pylc_blend_accumulate_w(ptr(buf[k:k + b]), buf.shape[3], k, b, h, w, out, stride, c, flip, ptr(acc), acc.shape[2], ptr(win),
                                          beta, stream()))


def _accumulate_t(acc, buf, c, h, w, out, stride, batch, beta, flip=0):
    from pylc_amd.lib import lib, check, ptr, stream
    n = buf.shape[0]
    for k in range(0, n, batch):
        b = min(batch, n - k)
        check(lib.pylc_blend_accumulate_t(ptr(buf[k:k + b]), buf.shape[3], k, b, h, w, out, stride, c, flip, ptr(acc), acc.shape[2], stream(),
                                          beta))


def _sums(win, out, stride, n):
    from pylc_amd.lib import lib, check, ptr, stream
    sums = torch.full((n,), float('nan'), device=win.device)
    check(lib.pylc_blend_window_sums(ptr(win), out, stride, n, ptr(sums), stream()))
    return sums


def _finalize_w(acc, c, h, w, members, sy, sx):
    from pylc_amd.lib import lib, check, ptr, stream
    mask = torch.empty((h, w), device=acc.device, dtype=torch.uint8)
    probs = torch.empty((c, h, w), device=acc.device)
    conf = torch.empty((h, w), device=acc.device)
    check(lib.pylc_blend_finalize_w(ptr(acc), acc.shape[2], h, w, c, members, ptr(sy), ptr(sx), ptr(mask), ptr(probs), ptr(conf), stream()))
    only_mask = torch.empty_like(mask)                               # probs and conf are optional
    check(lib.pylc_blend_finalize_w(ptr(acc), acc.shape[2], h, w, c, members, ptr(sy), ptr(sx), ptr(only_mask), None, None, stream()))
    assert torch.equal(only_mask, mask)
    return mask, probs, conf


def _windowed(logits_members, c, h, w, out, stride, batch, win, pitch=None, beta=1.0):
    """_w accumulate (member m with flip = m) -> window sums -> finalize_w; returns (acc, (mask, probs, conf))"""
    cp = (c + 3) & ~3
    acc = torch.zeros((h, w, pitch or cp), device=win.device)
    for m, logits in enumerate(logits_members):
        _accumulate_w(acc, _tiles_buffer(logits, cp, win.device), c, h, w, out, stride, batch, win, flip=m, beta=beta)
    return acc, _finalize_w(acc, c, h, w, len(logits_members), _sums(win, out, stride, h), _sums(win, out, stride, w))


def _n_tiles(h, w, out, stride):
    return len(overlap_origins(h, out, stride)) * len(overlap_origins(w, out, stride))


# ---- 1: the axis sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [16, 8, 5, 1])
def test_window_sums_equal_the_float32_model(dev, stride):
    from pylc_amd import lib as L
    L.init()
    for name in ('uniform', 'hann', 'gauss', 'random'):
        win = _table(name, dev)
        for n in (16, 37, 53):
            got = _sums(win, OUT, stride, n).cpu().numpy()
            assert np.array_equal(got, Wn.window_sums_f32(win.cpu().numpy(), n, OUT, stride)), (name, n, stride)
            if name == 'uniform':
                assert np.array_equal(got, Wn.cover_counts(n, OUT, stride).astype(np.float32))


# ---- 2: a table of ones gives the plain entry points' bytes -------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [16, 8, 5, 1])
@pytest.mark.parametrize('c', [2, 3, 9, 16])
def test_uniform_table_equals_the_plain_path(dev, c, stride):
    from pylc_amd import lib as L
    L.init()
    n = _n_tiles(H, W, OUT, stride)
    logits = (np.random.RandomState(100 * c + stride).standard_normal((n, c, OUT, OUT)) * 3).astype(np.float32)
    cp = (c + 3) & ~3
    ones = _table('uniform', dev)
    buf = _tiles_buffer(logits, cp, dev)
    sy, sx = _sums(ones, OUT, stride, H), _sums(ones, OUT, stride, W)
    for batch in (1, 3, 7, n):
        plain = torch.zeros((H, W, cp), device=dev)
        _accumulate(plain, buf, c, H, W, OUT, stride, batch)
        acc = torch.zeros((H, W, cp), device=dev)
        _accumulate_w(acc, buf, c, H, W, OUT, stride, batch, ones)
        assert torch.equal(acc, plain), (c, stride, batch)               # the accumulation image, padding channels included (zero)
        want = _finalize(plain, c, H, W, OUT, stride, 1)
        got = _finalize_w(acc, c, H, W, 1, sy, sx)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), (c, stride, batch)
    # with a temperature, against pylc_blend_accumulate_t; two members
    plain = torch.zeros((H, W, cp), device=dev)
    acc = torch.zeros((H, W, cp), device=dev)
    for flip in (0, 1):
        _accumulate_t(plain, buf, c, H, W, OUT, stride, 7, 0.5, flip=flip)
        _accumulate_w(acc, buf, c, H, W, OUT, stride, 7, ones, flip=flip, beta=0.5)
    assert torch.equal(acc, plain)
    assert all(torch.equal(a, b) for a, b in zip(_finalize_w(acc, c, H, W, 2, sy, sx), _finalize(plain, c, H, W, OUT, stride, 2)))
    if stride == 5:                                                  # a logits pitch and an accumulator pitch beyond cp
        wide = _tiles_buffer(logits, cp + 4, dev)
        plain = torch.zeros((H, W, cp + 8), device=dev)
        _accumulate(plain, wide, c, H, W, OUT, stride, 7)
        acc = torch.zeros((H, W, cp + 8), device=dev)
        _accumulate_w(acc, wide, c, H, W, OUT, stride, 7, ones)
        assert torch.equal(acc, plain) and float(acc[..., c:].abs().max()) == 0.0
        assert all(torch.equal(a, b) for a, b in zip(_finalize_w(acc, c, H, W, 1, sy, sx), _finalize(plain, c, H, W, OUT, stride, 1)))


def test_windowed_accumulator_writes_only_the_batch_bounding_box(dev):
    """test_accumulator_writes_only_the_batch_bounding_box's construction, with a table of ones and with the Hann table"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    h, w, out, stride, c = 37, 53, 16, 8, 3
    rows, cols = len(overlap_origins(h, out, stride)), len(overlap_origins(w, out, stride))
    logits = (np.random.RandomState(4).standard_normal((rows * cols, c, out, out)) * 3).astype(np.float32)
    buf = _tiles_buffer(logits, 4, dev)
    for first, cnt in ((cols + 2, 2), (cols - 2, 4)):                # within one tile row; across a row end
        touched = np.zeros((h, w), bool)
        for k in range(first, first + cnt):
            oy, ox = overlap_origins(h, out, stride)[k // cols], overlap_origins(w, out, stride)[k % cols]
            touched[oy:oy + out, ox:ox + out] = True
        touched_d = torch.from_numpy(touched).to(dev)
        plain = torch.full((h, w, 4), -7.0, device=dev)
        check(lib.pylc_blend_accumulate(ptr(buf[first:first + cnt]), 4, first, cnt, h, w, out, stride, c, 0, ptr(plain), 4, stream()))
        for name in ('uniform', 'hann'):
            acc = torch.full((h, w, 4), -7.0, device=dev)
            check(lib.pylc_blend_accumulate_w(ptr(buf[first:first + cnt]), 4, first, cnt, h, w, out, stride, c, 0, ptr(acc), 4,
                                              ptr(_table(name, dev)), 1.0, stream()))
            assert float((acc[..., :3][~touched_d] + 7.0).abs().max()) == 0.0          # an uncovered pixel of the box is not written
            assert bool((acc[..., :3].sum(-1)[touched_d] > -21.0).all())                # a covered one gained its weight
            assert float((acc[..., 3] + 7.0).abs().max()) == 0.0                        # the padding channel is left alone
            if name == 'uniform':
                assert torch.equal(acc, plain)


# ---- 3, 4: batch partitions; a table scaled by a power of two -------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [16, 8, 5, 1])
@pytest.mark.parametrize('c', [2, 9, 16])
def test_result_does_not_depend_on_the_batch_partition(dev, c, stride):
    from pylc_amd import lib as L
    L.init()
    n = _n_tiles(H, W, OUT, stride)
    logits = (np.random.RandomState(7 + 100 * c + stride).standard_normal((n, c, OUT, OUT)) * 3).astype(np.float32)
    hann = _table('hann', dev)
    want_acc, want = _windowed([logits], c, H, W, OUT, stride, n, hann)
    for batch in (1, 3, 7):
        acc, got = _windowed([logits], c, H, W, OUT, stride, batch, hann)
        assert torch.equal(acc, want_acc) and all(torch.equal(a, b) for a, b in zip(got, want)), (c, stride, batch)
    # 4: the table times 0.25 -- every product, sum and quotient scales exactly, nothing underflows at these sizes
    quarter = hann * 0.25
    _, scaled = _windowed([logits], c, H, W, OUT, stride, 7, quarter)
    assert torch.equal(scaled[1], want[1]) and torch.equal(scaled[0], want[0]) and torch.equal(scaled[2], want[2])


# ---- 5: the finalizer against its float32 model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['hann', 'random'])
@pytest.mark.parametrize('c', [2, 3, 9, 16])
def test_finalizer_equals_the_float32_model(dev, c, name):
    from pylc_amd import lib as L
    L.init()
    for (h, w), stride, members in (((37, 53), 5, 2), ((16, 16), 16, 1), ((16, 53), 8, 1)):
        ls = Wn.case_logits(c, stride, h, w)[:members]
        win = _table(name, dev)
        acc, (mask, probs, conf) = _windowed(ls, c, h, w, OUT, stride, 7, win, pitch=((c + 3) & ~3) + 4)
        sy, sx = _sums(win, OUT, stride, h), _sums(win, OUT, stride, w)
        want_p, want_c, want_m = Wn.finalize_f32(acc.cpu().numpy()[..., :c], members, sy.cpu().numpy(), sx.cpu().numpy())
        assert np.array_equal(probs.cpu().numpy(), want_p), (c, name, h, w)
        assert np.array_equal(conf.cpu().numpy(), want_c) and np.array_equal(mask.cpu().numpy(), want_m)
        assert torch.equal(conf, probs.gather(0, mask.long()[None])[0])                  # conf is the same float as probs[mask]


# ---- 6: against the float64 statement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', Wn.WINDOWS)
@pytest.mark.parametrize('stride', Wn.STRIDES)
@pytest.mark.parametrize('c', Wn.CLASSES)
def test_two_members_match_the_float64_statement(dev, c, stride, name):
    """Bound 1e-6: the bound test_blend_gpu.py's test_two_members_match_the_float64_statement holds the unweighted form to.  The
    asymmetric 'random' table catches a window indexed before the flip mapping instead of after.  The seeds are those
    tests/test_cpu_window.py checks (decided share >= 0.999 at 1e-5).  Measured on the MI355X: see DESIGN.md 5.25."""
    from pylc_amd import lib as L
    L.init()
    l0, l1 = Wn.case_logits(c, stride)
    win = _table(name, dev)
    want_p, want_m = Wn.blend_window_np([l0, l1], H, W, OUT, stride, win.cpu().numpy())
    _, (mask, probs, conf) = _windowed([l0, l1], c, H, W, OUT, stride, 7, win)
    mask, probs = mask.cpu().numpy(), probs.cpu().numpy()
    err = np.abs(probs - want_p).max()
    decided = Wn.decided(want_p)
    print('window %s C %d stride %d: max|probs - fp64| %.3g, %.4f%% decided' % (name, c, stride, err, 100 * decided.mean()))
    assert err < 1e-6
    assert np.abs(probs.sum(0) - 1).max() < 1e-5
    assert decided.mean() >= 0.999
    assert np.array_equal(mask[decided], want_m[decided])
    assert np.array_equal(conf.cpu().numpy(), probs.max(0))
    if name == 'random' and stride < OUT:                            # the statement with the table the other way round is far away
        wrong = Wn.blend_window_np([l0, l1], H, W, OUT, stride, np.ascontiguousarray(win.cpu().numpy()[::-1]))[0]
        assert np.abs(wrong - want_p).max() > 1e-3


# ---- 7: the resampling accumulator --------------------------------------------------------------------------------------------------------------------
def _resample(acc, ens, c, stride, members, weight, add):
    from pylc_amd.lib import lib, check, ptr, stream
    check(lib.pylc_blend_resample_accumulate(ptr(acc), acc.shape[2], acc.shape[0], acc.shape[1], OUT, stride, members, weight, c, ptr(ens),
                                             ens.shape[2], ens.shape[0], ens.shape[1], add, stream()))


def _resample_w(acc, ens, c, members, weight, add, sy, sx):
    from pylc_amd.lib import lib, check, ptr, stream
    check(lib.pylc_blend_resample_accumulate_w(ptr(acc), acc.shape[2], acc.shape[0], acc.shape[1], members, weight, c, ptr(sy), ptr(sx),
                                               ptr(ens), ens.shape[2], ens.shape[0], ens.shape[1], add, stream()))


def _ensemble_finalize(ens, c, total):
    from pylc_amd.lib import lib, check, ptr, stream
    h, w = ens.shape[:2]
    mask = torch.empty((h, w), device=ens.device, dtype=torch.uint8)
    probs = torch.empty((c, h, w), device=ens.device)
    conf = torch.empty((h, w), device=ens.device)
    check(lib.pylc_ensemble_finalize(ptr(ens), ens.shape[2], h, w, c, total, ptr(mask), ptr(probs), ptr(conf), stream()))
    return mask, probs, conf


@pytest.mark.parametrize('stride', M.STRIDES)
@pytest.mark.parametrize('c', M.CLASSES)
def test_resample_with_uniform_tables_equals_the_plain_form(dev, c, stride):
    from pylc_amd import lib as L
    L.init()
    cp = (c + 3) & ~3
    ones = _table('uniform', dev)
    logits = M.case_logits(c, stride, 'near')
    for k, (hs, ws) in enumerate(M.SCALE_SETS['near']):
        acc = torch.zeros((hs, ws, cp + 4), device=dev)
        for m in range(2):
            _accumulate(acc, _tiles_buffer(logits[(hs, ws)][m], cp, dev), c, hs, ws, OUT, stride, 7, flip=m)
        acc[..., c:] = 1e30
        sy, sx = _sums(ones, OUT, stride, hs), _sums(ones, OUT, stride, ws)
        want = torch.full((H, W, cp + 8), float('nan'), device=dev)
        _resample(acc, want, c, stride, 2, 0.5, 0)
        got = torch.full((H, W, cp + 8), float('nan'), device=dev)
        _resample_w(acc, got, c, 2, 0.5, 0, sy, sx)                      # add = 0 onto NaN: the pad channels stay NaN
        assert torch.equal(got[..., :c], want[..., :c]) and not torch.isnan(got[..., :c]).any() and torch.isnan(got[..., c:]).all()
        _resample(acc, want, c, stride, 2, 2.0, 1)
        _resample_w(acc, got, c, 2, 2.0, 1, sy, sx)                      # and add = 1
        assert torch.equal(got[..., :c], want[..., :c]) and torch.isnan(got[..., c:]).all()


@pytest.mark.parametrize('stride', M.STRIDES)
@pytest.mark.parametrize('c', M.CLASSES)
def test_windowed_ensemble_matches_the_float64_statement(dev, c, stride):
    """Three scales (28 x 40, 37 x 53, 46 x 66: 0.75, 1.0, 1.25) of the 37 x 53 image with the Hann table, two members, against
    tests/_multiscale.py:ensemble_np fed with blend_window_np's per-scale probabilities.  Bound 1e-6, the bound tests/test_multiscale_gpu.py
    holds the unweighted ensemble to.  Measured on the MI355X: see DESIGN.md 5.25."""
    from pylc_amd import lib as L
    L.init()
    cp = (c + 3) & ~3
    sizes = M.SCALE_SETS['near']
    hann = _table('hann', dev)
    logits = M.case_logits(c, stride, 'near')
    weights = (2.0, 1.0, 0.5)
    ens = torch.full((H, W, cp + 4), float('nan'), device=dev)
    stated = []
    for k, ((hs, ws), wgt) in enumerate(zip(sizes, weights)):
        acc = torch.zeros((hs, ws, cp), device=dev)
        for m in range(2):
            _accumulate_w(acc, _tiles_buffer(logits[(hs, ws)][m], cp, dev), c, hs, ws, OUT, stride, 7, hann, flip=m)
        _resample_w(acc, ens, c, 2, wgt, int(k > 0), _sums(hann, OUT, stride, hs), _sums(hann, OUT, stride, ws))
        stated.append(Wn.blend_window_np(list(logits[(hs, ws)]), hs, ws, OUT, stride, hann.cpu().numpy())[0])
    mask, probs, conf = _ensemble_finalize(ens, c, float(sum(weights)))
    want_p, want_m = M.ensemble_np(stated, sizes, weights, H, W)
    err = np.abs(probs.cpu().numpy() - want_p).max()
    print('windowed ensemble C %d stride %d: max|probs - fp64| %.3g' % (c, stride, err))
    assert err <= 1e-6
    decided = Wn.decided(want_p)
    assert np.array_equal(mask.cpu().numpy()[decided], want_m[decided])
    assert torch.equal(conf, probs.max(0).values)


# ---- 8: refused arguments ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(dev):
    from pylc_amd import lib as L
    L.init()
    check_entry_points_refuse()
    torch.cuda.synchronize()                                         # nothing was launched: nothing can have faulted


# ---- the paths -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def deeplab(dev):
    """test_blend_gpu.py's recipe: tile 64, ResNet-101, 9 classes, oracle-calibrated weights, dropout off; the fitted image [3,128,192]
    and its 15 windows at stride 32"""
    import oracle
    from oracle import step as ostep
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    from tests import _data as D
    runtime.dropout_enabled = False
    tile, stride = 64, 32
    img = D.learnable_tiles(21, 1, 192, 9, cell=16)[0][0, :, :128, :]          # [3,128,192]
    tiles = torch.from_numpy(oracle.split_tiles(img.numpy(), tile, stride)[0])
    cfg = ostep.StepConfig('deeplab', 'resnet', 9, 3, dropout=False)
    w = ostep.calibrate_bn(oracle.formula_state(oracle.state_spec('deeplab', 'resnet', 9, 3), salt=2), cfg, tiles.clone())
    model = Model(Meta(), dev).build()
    model.net.load_state_dict(w)
    model.net.eval()
    return {'model': model, 'img': img, 'tiles': tiles, 'tile': tile, 'stride': stride}


def _valid(probs):
    assert bool(torch.isfinite(probs).all())
    assert float((probs.sum(0) - 1).abs().max()) < 1e-5
    assert float(probs.min()) >= 0.0 and float(probs.max()) <= 1.0


@pytest.mark.parametrize('kw', [{}, {'flip': True}, {'temperature': 1.7}, {'scales': (0.75, 1.0, 1.25)}], ids=str)
def test_uniform_window_is_window_none(dev, deeplab, kw):
    from pylc_amd import inference
    model, tile, stride = deeplab['model'], deeplab['tile'], deeplab['stride']
    for img in (deeplab['img'], deeplab['img'][:, :100, :150].contiguous()):           # fitted 128 x 192, unfitted 100 x 150
        want = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True, return_confidence=True, **kw)
        got = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True, return_confidence=True, window='uniform', **kw)
        assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want)), (kw, tuple(img.shape))
        none = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True, return_confidence=True, window=None, **kw)
        assert all(torch.equal(a, b) for a, b in zip(none, want))
    assert not model.net.training


def _hand(dev, model, windows, h, w, tile, stride, win, flip):
    """per-tile Model.test logits (batches of 8) -> pylc_blend_accumulate_w -> pylc_blend_finalize_w"""
    members = [_model_test_logits(model, windows, 8)]
    if flip:
        members.append(_model_test_logits(model, torch.flip(windows, dims=[3]).contiguous(), 8))
    c = members[0].shape[1]
    cp = (c + 3) & ~3
    acc = torch.zeros((h, w, cp), device=dev)
    for m, logits in enumerate(members):
        buf = torch.zeros((logits.shape[0], tile, tile, cp), device=dev)
        buf[..., :c] = logits.permute(0, 2, 3, 1)
        _accumulate_w(acc, buf, c, h, w, tile, stride, 8, win, flip=m)
    got = _finalize_w(acc, c, h, w, len(members), _sums(win, tile, stride, h), _sums(win, tile, stride, w))
    return got, [m.cpu().numpy() for m in members]


def test_hann_window_is_its_composition_by_hand(dev, deeplab):
    from pylc_amd import inference
    model, tile, stride = deeplab['model'], deeplab['tile'], deeplab['stride']
    hann = inference.blend_window('hann', tile, dev)
    assert hann.is_cuda and np.array_equal(hann.cpu().numpy(), Wn.window_np('hann', tile))
    for img in (deeplab['img'], deeplab['img'][:, :100, :150].contiguous()):
        h, w = img.shape[1:]
        windows = reflect_windows(img, tile, tile, stride)
        got = inference.predict_image(model, img, tile, stride, batch=8, blend='mean', return_probs=True, return_confidence=True, window='hann')
        want, members = _hand(dev, model, windows, h, w, tile, stride, hann, False)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), tuple(img.shape)       # without flip: bit for bit
        _valid(got[1])
        plain = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True)[1]
        assert not torch.equal(plain, got[1])                                            # the window is really there
        # a caller table of the same values, and the return value's shapes
        again = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True, window=Wn.window_np('hann', tile))
        assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
        assert torch.equal(inference.predict_image(model, img, tile, stride, blend='mean', window='hann'), got[0])
        # with flip: the bound of test_deeplab_flip_ensemble, against the hand composition and against the float64 statement
        gotf = inference.predict_image(model, img, tile, stride, batch=8, blend='mean', flip=True, return_probs=True, return_confidence=True,
                                       window='hann')
        wantf, members = _hand(dev, model, windows, h, w, tile, stride, hann, True)
        err = float((gotf[1] - wantf[1]).abs().max())
        stated = Wn.blend_window_np(members, h, w, tile, stride, hann.cpu().numpy())[0]
        err64 = np.abs(gotf[1].cpu().numpy() - stated).max()
        print('hann + flip %dx%d: max|path - hand composition| %.3g, max|path - fp64 statement| %.3g' % (h, w, err, err64))
        assert err <= 1e-6 and err64 <= 1e-6
        assert torch.equal(gotf[2], gotf[1].max(0).values)
        _valid(gotf[1])
        assert not torch.equal(gotf[1], got[1])


def test_windowed_path_does_not_depend_on_batch_or_a_one_rank_group(dev, deeplab):
    import torch.distributed as dist
    from pylc_amd import inference
    model, tile, stride = deeplab['model'], deeplab['tile'], deeplab['stride']
    img = deeplab['img'][:, :100, :150].contiguous()
    kw = dict(blend='mean', flip=True, return_probs=True, return_confidence=True, window='hann')
    want = inference.predict_image(model, img, tile, stride, batch=8, **kw)
    got = inference.predict_image(model, img, tile, stride, batch=3, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not dist.is_initialized()
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group('gloo', init_method='file://' + os.path.join(tmp, 'store'), rank=0, world_size=1)
        try:
            grouped = [inference.predict_image(model, img, tile, stride, group=dist.group.WORLD, **dict(kw, **extra))
                       for extra in ({}, {'scales': (0.75, 1.0)})]
        finally:
            dist.destroy_process_group()
    assert len(grouped[0]) == 3 and all(torch.equal(a, b) for a, b in zip(grouped[0], want))
    scaled = inference.predict_image(model, img, tile, stride, scales=(0.75, 1.0), **kw)
    assert all(torch.equal(a, b) for a, b in zip(grouped[1], scaled))
    _valid(scaled[1])


def test_windowed_scales_and_refine_compose(dev, deeplab):
    from pylc_amd import inference, refine
    model, tile, stride = deeplab['model'], deeplab['tile'], deeplab['stride']
    img = (deeplab['img'][:, :100, :150].clamp(0, 255)).to(torch.uint8).contiguous().to(dev)
    m, p, c = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True, return_confidence=True, window='hann')
    spec = {'radius': 4, 'eps': 1e-3}
    got = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True, return_confidence=True, window='hann', refine=spec)
    want = refine.guided_refine(p, refine.luma(img), 4, 1e-3, True, True)
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))          # refine acts on the windowed probabilities
    # scales=(1.0,) is the single-scale windowed blend resampled by the identity: the same bytes
    one = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True, return_confidence=True, window='hann', scales=(1.0,))
    assert torch.equal(one[0], m) and torch.equal(one[1], p) and torch.equal(one[2], c)
    three = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True, window='gauss', scales=(0.75, 1.0, 1.25),
                                    temperature=1.7)
    _valid(three[1])
    assert torch.equal(three[0], three[1].argmax(0).to(torch.uint8))


def test_unet_overlap_tile_window(dev):
    from pylc_amd import inference, photo, runtime
    from pylc_amd.model import Model, Meta
    from tests.test_photo_gpu import photo_np
    runtime.dropout_enabled = False
    torch.manual_seed(0)
    model = Model(Meta(arch='unet', ch=3, n_classes=9), dev).build()
    image = photo_np(23, 100, 120)
    chw = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1))).to(dev)
    out = 256 - 2 * model.meta.pad_size
    m, p, c = inference.predict_overlap_tile(model, chw, 256, stride=out // 2, return_probs=True, return_confidence=True, window='hann')
    assert tuple(m.shape) == (100, 120) and tuple(p.shape) == (9, 100, 120)
    _valid(p)
    assert torch.equal(c, p.max(0).values) and torch.equal(m, p.argmax(0).to(torch.uint8))
    m0, p0 = inference.predict_overlap_tile(model, chw, 256, stride=out // 2, return_probs=True)          # the one-launch stitch
    mu, pu = inference.predict_overlap_tile(model, chw, 256, stride=out // 2, return_probs=True, window='uniform')
    assert torch.equal(mu, m0) and torch.equal(pu, p0) and not torch.equal(p, p0)
    with pytest.raises(ValueError, match=r'\[%d\]' % out):
        inference.predict_overlap_tile(model, chw, 256, window=np.ones(256, np.float32))                 # the table has `out` entries
    res = photo.segment_photo(model, image, tile=256, stride=out // 2, return_probs=True, return_confidence=True, window='gauss')
    assert bool(torch.isfinite(res.probs).all()) and torch.equal(res.confidence, res.probs.max(0).values)
    assert model.net.training                                        # built in training mode: the network got its mode back


def test_segment_photo_window(dev, deeplab):
    from pylc_amd import inference, photo
    from tests.test_photo_gpu import photo_np
    model = deeplab['model']
    image = photo_np(31, 100, 150)
    res = photo.segment_photo(model, image, tile=64, blend='mean', return_probs=True, return_confidence=True, window='gauss')
    assert tuple(res.mask.shape) == (100, 150) and bool(torch.isfinite(res.probs).all())
    assert torch.equal(res.confidence, res.probs.max(0).values)
    _valid(res.probs)
    chw = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1))).to(dev)
    m, p = inference.predict_image(model, chw, 64, blend='mean', return_probs=True, window=('gauss', 0.125))
    assert torch.equal(res.mask, m) and torch.equal(res.probs, p)
    sieved = photo.segment_photo(model, image, tile=64, blend='mean', window='gauss', min_region=20)      # the sieve runs afterwards
    assert sieved.n_sieved is not None and tuple(sieved.mask.shape) == (100, 150)
    with pytest.raises(ValueError, match="window needs blend='mean' on a DeepLab"):
        photo.segment_photo(model, image, tile=64, window='gauss')
    with pytest.raises(ValueError, match='named window'):
        photo.segment_photo(model, image, tile=64, blend='mean', window='hamming')
    assert not model.net.training
