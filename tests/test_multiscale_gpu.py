"""The multi-scale ensemble on the GPU (-m gpu, csrc/multiscale.hip): pylc_resize_bilinear_image against the float64 statement of
tests/_multiscale.py, pylc_blend_resample_accumulate + pylc_ensemble_finalize against pylc_blend_finalize bit for bit at equal sizes and
against the statement at 0.5 .. 2 times the size, predict_image(scales=) on a DeepLab against scales=None and against its composition
by hand, and segment_photo's new keywords on a DeepLab and a U-Net."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import _multiscale as M
from tests._blend import blend_mean_np
from tests._multiscale import ensemble_np, resize_bilinear_np
from tests.test_blend_gpu import _accumulate, _finalize, _image, _tiles_buffer

pytestmark = pytest.mark.gpu

H, W = M.BASE
SIZES = [(19, 27), (28, 40), (37, 53), (46, 66), (74, 106)]          # scales 0.5, 0.75, 1, 1.25 and 2 of the base image


# ---- 1: the resize kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('u8', [False, True])
@pytest.mark.parametrize('ch', [1, 3])
def test_resize_matches_the_statement(dev, ch, u8):
    """Bound 1e-4: values of at most 255 and at most six fp32 roundings of relative 2^-24 (f, 1 - f, two products and a sum per axis)
    give 255 * 6 * 2^-24 = 9.2e-5.  Measured on the MI355X: see DESIGN.md 5.12."""
    from pylc_amd import inference
    img = _image(40 + ch, ch, H, W, u8, dev)
    if not u8:
        img = img * 0.997                                                # not only integers, still at most 255
    host = img.cpu().numpy()
    worst = 0.0
    for oh, ow in SIZES:
        got = inference.resize_image(img, oh, ow)
        assert got.dtype == torch.float32 and tuple(got.shape) == (ch, oh, ow) and got.is_cuda
        err = float(np.abs(got.cpu().numpy() - resize_bilinear_np(host, oh, ow)).max())
        worst = max(worst, err)
        assert err < 1e-4, (oh, ow, err)
        if (oh, ow) == (H, W):
            assert torch.equal(got, img.float())
    print('resize ch %d u8 %d: max|kernel - fp64| %.3g' % (ch, u8, worst))
    down = inference.resize_image(inference.resize_image(img, 74, 106), H, W)       # 2x up and back down: a source other than the base
    want = resize_bilinear_np(resize_bilinear_np(host, 74, 106), H, W)
    assert float(np.abs(down.cpu().numpy() - want).max()) < 2e-4                     # two resizes, twice the bound
    assert torch.equal(inference.resize_image(img.cpu(), 46, 66), inference.resize_image(img, 46, 66))      # a host image is uploaded


# ---- 2, 3, 4: the resampling accumulator and the ensemble finalizer -------------------------------------------------------------------------
def _sums(logits, members, c, hs, ws, stride, pitch, dev):
    """pylc_blend_accumulate's finished image [hs, ws, pitch] of one scale: member 0 unflipped, member 1 mirrored; pad channels 1e30"""
    acc = torch.zeros((hs, ws, pitch), device=dev)
    for m in range(members):
        _accumulate(acc, _tiles_buffer(logits[m], (c + 3) & ~3, dev), c, hs, ws, M.OUT, stride, 7, flip=m)
    acc[..., c:] = 1e30
    return acc


def _resample(acc, ens, c, stride, members, weight, add):
    from pylc_amd.lib import lib, check, ptr, stream
    check(lib.pylc_blend_resample_accumulate(ptr(acc), acc.shape[2], acc.shape[0], acc.shape[1], M.OUT, stride, members, weight, c, ptr(ens),
                                             ens.shape[2], ens.shape[0], ens.shape[1], add, stream()))


def _ensemble_finalize(ens, c, total):
    from pylc_amd.lib import lib, check, ptr, stream
    h, w = ens.shape[:2]
    mask = torch.empty((h, w), device=ens.device, dtype=torch.uint8)
    probs = torch.empty((c, h, w), device=ens.device)
    conf = torch.empty((h, w), device=ens.device)
    check(lib.pylc_ensemble_finalize(ptr(ens), ens.shape[2], h, w, c, total, ptr(mask), ptr(probs), ptr(conf), stream()))
    only_mask = torch.empty_like(mask)                               # probs and conf are optional
    check(lib.pylc_ensemble_finalize(ptr(ens), ens.shape[2], h, w, c, total, ptr(only_mask), None, None, stream()))
    assert torch.equal(only_mask, mask)
    return mask, probs, conf


@pytest.mark.parametrize('stride', M.STRIDES)
@pytest.mark.parametrize('c', M.CLASSES)
def test_identity_is_bit_exact(dev, c, stride):
    """Hs == H, weight 1, total 1: the interpolation runs (there is no copy branch) and returns v00, so the ensemble path gives
    pylc_blend_finalize's mask, probs and conf bit for bit, onto a NaN-filled ensemble image whose pad channels stay NaN."""
    from pylc_amd import lib as L
    L.init()
    cp = (c + 3) & ~3
    logits = M.case_logits(c, stride, 'near')[(H, W)]
    for members in (1, 2):
        for acc_pitch, ens_pitch in ((cp, cp), (cp + 4, cp + 8)):        # and a pitch beyond cp on both buffers
            acc = _sums(logits, members, c, H, W, stride, acc_pitch, dev)
            want = _finalize(acc, c, H, W, M.OUT, stride, members)
            ens = torch.full((H, W, ens_pitch), float('nan'), device=dev)
            _resample(acc, ens, c, stride, members, 1.0, 0)
            assert not torch.isnan(ens[..., :c]).any()
            assert torch.isnan(ens[..., c:]).all()
            got = _ensemble_finalize(ens, c, 1.0)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (c, stride, members, acc_pitch)


@pytest.mark.parametrize('c', M.CLASSES)
def test_add_onto_zeros_equals_overwrite_onto_nan(dev, c):
    from pylc_amd import lib as L
    L.init()
    cp = (c + 3) & ~3
    for name, stride in (('near', 8), ('far', 5)):
        logits = M.case_logits(c, stride, name)
        for (hs, ws) in M.SCALE_SETS[name]:
            acc = _sums(logits[(hs, ws)], 2, c, hs, ws, stride, cp + 4, dev)
            over = torch.full((H, W, cp + 4), float('nan'), device=dev)
            _resample(acc, over, c, stride, 2, 0.5, 0)
            added = torch.zeros((H, W, cp + 4), device=dev)
            _resample(acc, added, c, stride, 2, 0.5, 1)
            assert torch.equal(added[..., :c], over[..., :c]) and not torch.isnan(over[..., :c]).any()
            assert torch.isnan(over[..., c:]).all() and float(added[..., c:].abs().max()) == 0.0
            twice = added.clone()
            _resample(acc, twice, c, stride, 2, 0.5, 1)                   # add really adds
            assert torch.equal(twice[..., :c], added[..., :c] + over[..., :c])


@pytest.mark.parametrize('name', ['near', 'far'])
@pytest.mark.parametrize('stride', M.STRIDES)
@pytest.mark.parametrize('c', M.CLASSES)
def test_ensemble_matches_the_float64_statement(dev, c, stride, name):
    """Three scales (28 x 40, 37 x 53, 46 x 66) and two (19 x 27, 74 x 106) of the 37 x 53 image, weights (1, 1, 1) and (2, 1, 0.5), one and
    two members.  Bound 1e-6, test_two_members_match_the_float64_statement's: values of at most 1 and fewer than sixteen fp32 roundings
    of 2^-24 give 9.5e-7.  Measured on the MI355X: see DESIGN.md 5.12."""
    from pylc_amd import lib as L
    L.init()
    cp = (c + 3) & ~3
    sizes = M.SCALE_SETS[name]
    logits = M.case_logits(c, stride, name)
    worst = 0.0
    for members in (1, 2):
        accs = [_sums(logits[s], members, c, s[0], s[1], stride, cp + 4, dev) for s in sizes]
        stated = [blend_mean_np(list(logits[s][:members]), s[0], s[1], M.OUT, stride)[0] for s in sizes]
        for weights in M.WEIGHT_SETS:
            weights = weights[:len(sizes)]
            ens = torch.full((H, W, cp + 8), float('nan'), device=dev)
            for k, (acc, wgt) in enumerate(zip(accs, weights)):
                _resample(acc, ens, c, stride, members, wgt, int(k > 0))
            assert torch.isnan(ens[..., c:]).all()
            mask, probs, conf = _ensemble_finalize(ens, c, float(sum(weights)))
            want_p, want_m = ensemble_np(stated, sizes, weights, H, W)
            mask, probs_np = mask.cpu().numpy(), probs.cpu().numpy()
            err = float(np.abs(probs_np - want_p).max())
            decided = M.decided(want_p)
            worst = max(worst, err)
            print('ensemble C %d stride %d %s members %d weights %s: max|probs - fp64| %.3g, %.3f%% decided'
                  % (c, stride, name, members, weights, err, 100 * decided.mean()))
            assert err < 1e-6
            assert decided.mean() >= 0.999
            assert np.array_equal(mask[decided], want_m[decided])
            assert torch.equal(conf, probs.gather(0, torch.from_numpy(mask).to(dev).long()[None])[0])
            assert np.abs(probs_np.sum(0) - 1).max() < 1e-5
    print('ensemble C %d stride %d %s: worst %.3g' % (c, stride, name, worst))


# ---- 5: a DeepLab end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def deeplab(dev):
    """tests/test_blend_gpu.py's recipe: tile 64, ResNet-101, 9 classes, oracle-calibrated weights, dropout off; the fitted image
    [3,128,192] and stride 32 (built once, left unchanged)."""
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
    return {'model': model, 'img': img, 'tile': tile, 'stride': stride}


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('flip', [False, True])
def test_deeplab_unit_scale_is_the_single_scale_blend(dev, deeplab, flip):
    from pylc_amd import inference
    model, tile, stride = deeplab['model'], deeplab['tile'], deeplab['stride']
    for img in (deeplab['img'], deeplab['img'][:, :100, :150].contiguous()):      # fitted, and the unfitted crop (clamped last tiles)
        kw = dict(blend='mean', flip=flip, return_probs=True, return_confidence=True)
        want = inference.predict_image(model, img, tile, stride, **kw)
        got = inference.predict_image(model, img, tile, stride, scales=(1.0,), **kw)
        assert len(got) == 3 and _same(got, want)
        assert _same(inference.predict_image(model, img, tile, stride, scales=(1.0,), scale_weights=(4.0,), **kw), want)     # 4 p / 4
        assert torch.equal(inference.predict_image(model, img, tile, stride, blend='mean', flip=flip, scales=[1.0]), want[0])
        u8 = inference.predict_image(model, img.to(torch.uint8), tile, stride, scales=(1.0,), **kw)      # the image in its own dtype
        assert _same(u8, inference.predict_image(model, img.to(torch.uint8), tile, stride, **kw))
    assert not model.net.training


def test_deeplab_three_scales_match_the_hand_composition(dev, deeplab):
    """scales=(0.75, 1.0, 1.25) against resize_image, predict_image(return_probs=True) per scale and the float64 resample and average;
    the result does not depend on the batch size, and the network's mode is restored."""
    from pylc_amd import inference
    model, img, tile, stride = deeplab['model'], deeplab['img'].to(dev), deeplab['tile'], deeplab['stride']
    h, w = img.shape[1:]
    scales, weights = (0.75, 1.0, 1.25), (1.0, 2.0, 0.5)
    for flip, wts in ((False, None), (True, weights)):
        kw = dict(blend='mean', flip=flip, return_probs=True, return_confidence=True, scales=scales, scale_weights=wts)
        mask, probs, conf = inference.predict_image(model, img, tile, stride, batch=8, **kw)
        sizes = [(inference.scaled_size(h, s), inference.scaled_size(w, s)) for s in scales]
        assert sizes == [(96, 144), (128, 192), (160, 240)]
        per_scale = []
        for hs, ws in sizes:
            simg = img if (hs, ws) == (h, w) else inference.resize_image(img, hs, ws)
            per_scale.append(inference.predict_image(model, simg, tile, stride, blend='mean', flip=flip, return_probs=True)[1].double().cpu().numpy())
        want_p, want_m = ensemble_np(per_scale, sizes, wts or (1.0, 1.0, 1.0), h, w)
        err = float(np.abs(probs.cpu().numpy() - want_p).max())
        decided = M.decided(want_p)
        print('DeepLab three scales flip %d: max|probs - fp64 composition| %.3g, %.3f%% decided' % (flip, err, 100 * decided.mean()))
        assert err < 1e-6
        assert np.array_equal(mask.cpu().numpy()[decided], want_m[decided])
        assert torch.equal(conf, probs.max(0).values) and float((probs.sum(0) - 1).abs().max()) < 1e-5
        assert not torch.equal(probs, inference.predict_image(model, img, tile, stride, blend='mean', flip=flip, return_probs=True)[1])
        assert _same(inference.predict_image(model, img, tile, stride, batch=3, **kw), (mask, probs, conf))
        assert not model.net.training
    model.net.train()
    try:
        again = inference.predict_image(model, img, tile, stride, batch=8, **kw)
        assert model.net.training                                     # the mode it came with
    finally:
        model.net.eval()
    assert _same(again, (mask, probs, conf))


def test_one_rank_group_equals_no_group(dev, deeplab):
    import torch.distributed as dist
    from pylc_amd import inference
    model, img, tile, stride = deeplab['model'], deeplab['img'], deeplab['tile'], deeplab['stride']
    kw = dict(blend='mean', flip=True, return_probs=True, return_confidence=True, scales=(0.75, 1.0), scale_weights=(1.0, 2.0))
    want = inference.predict_image(model, img, tile, stride, **kw)
    assert not dist.is_initialized()                                  # (the multi-rank tests of this suite run in processes of their own)
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group('gloo', init_method='file://' + os.path.join(tmp, 'store'), rank=0, world_size=1)
        try:
            got = inference.predict_image(model, img, tile, stride, group=dist.group.WORLD, **kw)
        finally:
            dist.destroy_process_group()
    assert len(got) == 3 and _same(got, want)


# ---- 6: segment_photo and the U-Net ---------------------------------------------------------------------------------------------------------
def test_segment_photo_passes_scales_through(dev, deeplab):
    from pylc_amd import inference, photo
    from tests.test_photo_gpu import photo_np
    model = deeplab['model']
    image = photo_np(31, 100, 150)
    res = photo.segment_photo(model, image, tile=64, blend='mean', scales=(0.75, 1.0), return_confidence=True)
    chw = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1))).to(dev)
    mask, conf = inference.predict_image(model, chw, 64, blend='mean', scales=(0.75, 1.0), return_confidence=True)
    assert tuple(res.mask.shape) == (100, 150) and res.probs is None
    assert torch.equal(res.mask, mask) and torch.equal(res.confidence, conf)
    single = inference.predict_image(model, chw, 64, blend='mean', return_confidence=True)[1]
    assert not torch.equal(conf, single)                                                 # the second scale is really there
    for kw in (dict(scales=(1.0,)), dict(scales=(0.75, 1.0), scale_weights=(1.0, 1.0))):
        with pytest.raises(ValueError, match="blend='mean'"):
            photo.segment_photo(model, image, tile=64, **kw)
        with pytest.raises(ValueError, match="blend='mean'"):
            inference.predict_image(model, deeplab['img'], 64, blend='reference', **kw)
    with pytest.raises(ValueError, match=r'scale 0\.6 .* to 60x90, below the output tile 64'):
        photo.segment_photo(model, image, tile=64, blend='mean', scales=(1.0, 0.6))
    with pytest.raises(ValueError, match=r'scale 0\.6 .* to 60x90, below the output tile 64'):
        inference.predict_image(model, chw, 64, blend='mean', scales=(1.0, 0.6))
    assert not model.net.training


def test_segment_photo_unet_scales(dev):
    from pylc_amd import inference, photo, runtime
    from pylc_amd.model import Model, Meta
    from tests.test_photo_gpu import photo_np
    runtime.dropout_enabled = False
    torch.manual_seed(0)
    model = Model(Meta(arch='unet', ch=3, n_classes=9), dev).build()
    image = photo_np(23, 150, 200)
    res = photo.segment_photo(model, image, tile=256, scales=(1.0, 1.25), return_probs=True)
    assert tuple(res.mask.shape) == (150, 200) and tuple(res.probs.shape) == (9, 150, 200) and res.confidence is None
    assert float((res.probs.sum(0) - 1).abs().max()) < 1e-5
    assert torch.equal(res.mask, res.probs.argmax(0).to(torch.uint8))
    chw = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1))).to(dev)
    out = inference.overlap_tile_out(model.net, 256, model.meta.pad_size)
    mask, probs = inference.predict_blend_mean(model, chw, 256, out, scales=(1.0, 1.25), return_probs=True)
    assert torch.equal(res.mask, mask) and torch.equal(res.probs, probs)
    m1, p1 = inference.predict_overlap_tile(model, chw, 256, return_probs=True, scales=(1.0,))      # one scale: the one-launch stitch's bytes
    m0, p0 = inference.predict_overlap_tile(model, chw, 256, return_probs=True)
    assert torch.equal(m1, m0) and torch.equal(p1, p0) and not torch.equal(probs, p0)
    with pytest.raises(ValueError, match=r'scale 0\.5 .* to 34x40, below the output tile 68'):
        inference.predict_overlap_tile(model, chw[:, :68, :80].contiguous(), 256, scales=(1.0, 0.5))
