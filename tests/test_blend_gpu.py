"""The streaming mean-probability blend on the GPU (-m gpu, csrc/blend.hip): the mirrored tile cutters against the existing cutters,
pylc_blend_accumulate + pylc_blend_finalize against the one-shot pylc_stitch_overlap_argmax bit for bit at every batch partition, two
ensemble members against the float64 statement of tests/_blend.py, predict_image(blend='mean') on a DeepLab against per-tile Model.test
and the CPU oracle, and segment_photo's new keywords."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest
import torch

from tests._blend import blend_mean_np
from tests.test_cpu_overlap_tile import overlap_origins, stitch_overlap_np
from tests.test_unet_inference_gpu import reflect_windows

pytestmark = pytest.mark.gpu

MEAN, STD = (132.47, 144.47, 149.45), (24.85, 22.04, 18.77)


# ---- 1: the cutters ---------------------------------------------------------------------------------------------------------------------
def _cut(name, img, tile, out, stride, first, n, flip=None):
    """one of the four cutters on a device image [C,H,W] (float or uint8) -> [n, 4, tile, tile] (NHWC memory)"""
    from pylc_amd import ops, lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    c, h, w = img.shape
    got = ops.empty_nhwc(n, 4, tile, tile, img.device)
    m, s = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    u8 = int(img.dtype == torch.uint8)
    if name == 'reflect_ex':
        check(lib.pylc_image_pack_tiles_reflect_ex(ptr(img), u8, c, h, w, tile, out, stride, first, n, m, s, ptr(got), stream(), flip))
    elif name == 'reflect':
        check(lib.pylc_image_pack_tiles_reflect(ptr(img), u8, c, h, w, tile, out, stride, first, n, m, s, ptr(got), stream()))
    elif name == 'flip':
        check(lib.pylc_image_pack_tiles_flip(ptr(img), u8, c, h, w, tile, stride, first, n, m, s, ptr(got), stream(), flip))
    else:
        check(lib.pylc_image_pack_tiles_ex(ptr(img), u8, c, h, w, tile, stride, first, n, m, s, ptr(got), stream()))
    return got


def _image(seed, c, h, w, u8, dev):
    img = torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (c, h, w)).astype(np.uint8))
    return (img if u8 else img.float()).to(dev).contiguous()


@pytest.mark.parametrize('u8', [False, True])
@pytest.mark.parametrize('ch', [1, 3])
@pytest.mark.parametrize('tile,out,stride', [(32, 32, 20), (32, 20, 13)])
def test_mirrored_cutters(dev, tile, out, stride, ch, u8):
    h, w = 70, 93
    img = _image(11 + ch, ch, h, w, u8, dev)
    n = len(overlap_origins(h, out, stride)) * len(overlap_origins(w, out, stride))
    plain = _cut('reflect_ex', img, tile, out, stride, 0, n, 0)
    mirrored = _cut('reflect_ex', img, tile, out, stride, 0, n, 1)
    assert torch.equal(mirrored, torch.flip(plain, dims=[3]))
    assert float(plain[:, 3].abs().max()) == 0.0 and float(plain[:, :3].abs().max()) > 0
    if tile > out:                                                   # the geometry the existing entry point accepts
        assert torch.equal(plain, _cut('reflect', img, tile, out, stride, 0, n))
    else:                                                            # pad = 0: the windows themselves, against a host-side cut
        win = reflect_windows(img.cpu(), tile, out, stride)
        want = ((win - torch.tensor(MEAN[:ch] if ch == 3 else [MEAN[0]])[None, :, None, None])
                / torch.tensor(STD[:ch] if ch == 3 else [STD[0]])[None, :, None, None]) / 255
        assert (plain[:, :1 if ch == 1 else 3].cpu() - want).abs().max().item() < 1e-6
    for fl in (0, 1):                                                # a batch from the middle of the tile list
        whole = mirrored if fl else plain
        assert torch.equal(_cut('reflect_ex', img, tile, out, stride, 3, 4, fl), whole[3:7])
    # the fitted-grid cutter (the remainder right and below is dropped) with the same trailing flip
    rows, cols = (h - tile) // stride + 1, (w - tile) // stride + 1
    fitted = _cut('ex', img, tile, tile, stride, 0, rows * cols)
    assert torch.equal(_cut('flip', img, tile, tile, stride, 0, rows * cols, 0), fitted)
    assert torch.equal(_cut('flip', img, tile, tile, stride, 0, rows * cols, 1), torch.flip(fitted, dims=[3]))
    assert torch.equal(_cut('flip', img, tile, tile, stride, 3, 4, 1), torch.flip(fitted, dims=[3])[3:7])


@pytest.mark.parametrize('u8', [False, True])
def test_pad_zero_on_a_fitted_image_is_the_sliding_window_cutter(dev, u8):
    h, w, tile, stride = 64, 96, 32, 16
    img = _image(5, 3, h, w, u8, dev)
    n = ((h - tile) // stride + 1) * ((w - tile) // stride + 1)
    assert n == len(overlap_origins(h, tile, stride)) * len(overlap_origins(w, tile, stride)) == 15
    want = _cut('ex', img, tile, tile, stride, 0, n)
    assert torch.equal(_cut('reflect_ex', img, tile, tile, stride, 0, n, 0), want)
    assert torch.equal(_cut('reflect_ex', img, tile, tile, stride, 0, n, 1), torch.flip(want, dims=[3]))
    assert torch.equal(_cut('reflect_ex', img, tile, tile, stride, 3, 4, 0), want[3:7])


def test_existing_reflect_cutter_still_refuses_pad_zero(dev):
    from pylc_amd.lib import PylcError
    img = _image(5, 3, 64, 96, False, dev)
    with pytest.raises(PylcError):
        _cut('reflect', img, 32, 32, 16, 0, 15)


# ---- 2, 3: the accumulator and the finalizer ---------------------------------------------------------------------------------------------
def _tiles_buffer(logits, pitch, dev):
    """[n, C, out, out] numpy logits -> device NHWC tiles [n, out, out, pitch]; the padding channels hold a large value that must never
    reach a result"""
    n, c, out, _ = logits.shape
    buf = torch.full((n, out, out, pitch), 1e30, device=dev)
    buf[..., :c] = torch.from_numpy(logits).to(dev).permute(0, 2, 3, 1)
    return buf


def _accumulate(acc, buf, c, h, w, out, stride, batch, flip=0):
    from pylc_amd.lib import lib, check, ptr, stream
    n = buf.shape[0]
    for k in range(0, n, batch):
        b = min(batch, n - k)
        check(lib.pylc_blend_accumulate(ptr(buf[k:k + b]), buf.shape[3], k, b, h, w, out, stride, c, flip, ptr(acc), acc.shape[2], stream()))


def _finalize(acc, c, h, w, out, stride, members):
    from pylc_amd.lib import lib, check, ptr, stream
    mask = torch.empty((h, w), device=acc.device, dtype=torch.uint8)
    probs = torch.empty((c, h, w), device=acc.device)
    conf = torch.empty((h, w), device=acc.device)
    check(lib.pylc_blend_finalize(ptr(acc), acc.shape[2], h, w, out, stride, c, members, ptr(mask), ptr(probs), ptr(conf), stream()))
    only_mask = torch.empty_like(mask)                               # probs and conf are optional
    check(lib.pylc_blend_finalize(ptr(acc), acc.shape[2], h, w, out, stride, c, members, ptr(only_mask), None, None, stream()))
    assert torch.equal(only_mask, mask)
    return mask, probs, conf


@pytest.mark.parametrize('stride', [16, 8, 5, 1])
@pytest.mark.parametrize('c', [2, 3, 9, 16])
def test_accumulator_equals_the_one_shot_blend(dev, c, stride):
    from pylc_amd import inference, lib as L
    L.init()
    h, w, out = 37, 53, 16
    n = len(overlap_origins(h, out, stride)) * len(overlap_origins(w, out, stride))
    logits = (np.random.RandomState(100 * c + stride).standard_normal((n, c, out, out)) * 3).astype(np.float32)
    want_mask, want_probs = inference.stitch_overlap_logits(torch.from_numpy(logits).to(dev), h, w, out, stride, return_probs=True)
    cp = (c + 3) & ~3
    buf = _tiles_buffer(logits, cp, dev)
    for batch in (1, 3, 7, n):                                       # 3 and 7 start batches in the middle of a tile row
        acc = torch.zeros((h, w, cp), device=dev)
        _accumulate(acc, buf, c, h, w, out, stride, batch)
        mask, probs, conf = _finalize(acc, c, h, w, out, stride, 1)
        assert torch.equal(mask, want_mask) and torch.equal(probs, want_probs), (c, stride, batch)
        assert torch.equal(conf, probs.max(0).values)
        assert np.array_equal(mask.cpu().numpy(), probs.cpu().numpy().argmax(0).astype(np.uint8))      # first maximum
        assert float(acc[..., c:].abs().max()) == 0.0 if cp > c else True                            # the padding is left alone
    if stride == 5:                                                  # a logits pitch and an accumulator pitch beyond cp
        wide = _tiles_buffer(logits, cp + 4, dev)
        acc = torch.zeros((h, w, cp + 8), device=dev)
        _accumulate(acc, wide, c, h, w, out, stride, 7)
        mask, probs, conf = _finalize(acc, c, h, w, out, stride, 1)
        assert torch.equal(mask, want_mask) and torch.equal(probs, want_probs) and torch.equal(conf, probs.max(0).values)


def test_accumulator_writes_only_the_batch_bounding_box(dev):
    from pylc_amd import lib as L
    L.init()
    h, w, out, stride, c = 37, 53, 16, 8, 3
    rows, cols = len(overlap_origins(h, out, stride)), len(overlap_origins(w, out, stride))
    logits = (np.random.RandomState(4).standard_normal((rows * cols, c, out, out)) * 3).astype(np.float32)
    buf = _tiles_buffer(logits, 4, dev)
    from pylc_amd.lib import lib, check, ptr, stream
    for first, cnt in ((cols + 2, 2), (cols - 2, 4)):                # within one tile row; across a row end
        acc = torch.full((h, w, 4), -7.0, device=dev)
        check(lib.pylc_blend_accumulate(ptr(buf[first:first + cnt]), 4, first, cnt, h, w, out, stride, c, 0, ptr(acc), 4, stream()))
        touched = np.zeros((h, w), bool)
        for k in range(first, first + cnt):
            oy, ox = overlap_origins(h, out, stride)[k // cols], overlap_origins(w, out, stride)[k % cols]
            touched[oy:oy + out, ox:ox + out] = True
        got = (acc[..., :3].sum(-1) > -20.5).cpu().numpy()            # a touched pixel gained one unit of probability per covering tile
        assert np.array_equal(got, touched)
        assert float((acc[..., :3].sum(-1)[~torch.from_numpy(touched).to(dev)] + 21.0).abs().max()) == 0.0
        assert float((acc[..., 3] + 7.0).abs().max()) == 0.0


@pytest.mark.parametrize('stride', [16, 8, 5])
@pytest.mark.parametrize('c', [2, 3, 9, 16])
def test_two_members_match_the_float64_statement(dev, c, stride):
    from pylc_amd import lib as L
    L.init()
    h, w, out = 37, 53, 16
    n = len(overlap_origins(h, out, stride)) * len(overlap_origins(w, out, stride))
    rs = np.random.RandomState(3000 + 100 * c + stride)          # seeds at which the float64 statement leaves no pixel undecided
    l0 = (rs.standard_normal((n, c, out, out)) * 3).astype(np.float32)
    l1 = (rs.standard_normal((n, c, out, out)) * 3).astype(np.float32)          # the logits of the mirrored windows
    want_p, want_m = blend_mean_np([l0, l1], h, w, out, stride)
    cp = (c + 3) & ~3
    acc = torch.zeros((h, w, cp), device=dev)
    _accumulate(acc, _tiles_buffer(l0, cp, dev), c, h, w, out, stride, 7, flip=0)
    _accumulate(acc, _tiles_buffer(l1, cp, dev), c, h, w, out, stride, 7, flip=1)
    mask, probs, conf = _finalize(acc, c, h, w, out, stride, 2)
    mask, probs = mask.cpu().numpy(), probs.cpu().numpy()
    err = np.abs(probs - want_p).max()
    top2 = np.sort(want_p, axis=0)[-2:]
    decided = (top2[1] - top2[0]) > 1e-5
    print('two members C %d stride %d: max|probs - fp64| %.3g, %.4f%% decided' % (c, stride, err, 100 * decided.mean()))
    assert err < 1e-6
    assert np.abs(probs.sum(0) - 1).max() < 1e-5
    assert decided.mean() >= 0.999
    assert np.array_equal(mask[decided], want_m[decided])
    assert np.array_equal(conf.cpu().numpy(), probs.max(0))


@pytest.mark.parametrize('c', [2, 9, 16])
def test_mirrored_twin_member_reproduces_one_member_exactly(dev, c):
    """stride == out: every pixel has one tile per member; member 1 = the mirrored member-0 logits gives p + p, and / 2 is exact."""
    from pylc_amd import lib as L
    L.init()
    h, w, out = 32, 48, 16
    l0 = (np.random.RandomState(50 + c).standard_normal((6, c, out, out)) * 3).astype(np.float32)
    cp = (c + 3) & ~3
    one = torch.zeros((h, w, cp), device=dev)
    _accumulate(one, _tiles_buffer(l0, cp, dev), c, h, w, out, out, 4)
    m1, p1, c1 = _finalize(one, c, h, w, out, out, 1)
    two = torch.zeros((h, w, cp), device=dev)
    _accumulate(two, _tiles_buffer(l0, cp, dev), c, h, w, out, out, 4, flip=0)
    _accumulate(two, _tiles_buffer(np.ascontiguousarray(l0[:, :, :, ::-1]), cp, dev), c, h, w, out, out, 4, flip=1)
    m2, p2, c2 = _finalize(two, c, h, w, out, out, 2)
    assert torch.equal(p2, p1) and torch.equal(m2, m1) and torch.equal(c2, c1)


# ---- 4: a DeepLab end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def deeplab(dev):
    """test_predict_image_matches_oracle's recipe: tile 64, ResNet-101, 9 classes, oracle-calibrated weights, dropout off; the fitted
    image [3,128,192], its 15 windows at stride 32 and the oracle's logits for them (computed once, left unchanged)."""
    import oracle
    from oracle import step as ostep
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    from tests import _data as D
    runtime.dropout_enabled = False
    tile, stride = 64, 32
    img = D.learnable_tiles(21, 1, 192, 9, cell=16)[0][0, :, :128, :]          # [3,128,192]
    tiles_np, rows, cols = oracle.split_tiles(img.numpy(), tile, stride)
    tiles = torch.from_numpy(tiles_np)
    cfg = ostep.StepConfig('deeplab', 'resnet', 9, 3, dropout=False)
    w = ostep.calibrate_bn(oracle.formula_state(oracle.state_spec('deeplab', 'resnet', 9, 3), salt=2), cfg, tiles.clone())
    oracle_logits = ostep.test_step({k: v.clone() for k, v in w.items()}, cfg, tiles.clone()).numpy()
    model = Model(Meta(), dev).build()
    model.net.load_state_dict(w)
    model.net.eval()
    return {'model': model, 'img': img, 'tiles': tiles, 'oracle_logits': oracle_logits, 'tile': tile, 'stride': stride}


def _model_test_logits(model, windows, batch):
    return torch.cat([model.test(windows[k:k + batch])[0].float() for k in range(0, windows.shape[0], batch)])


def test_deeplab_mean_blend_is_the_blend_of_its_tile_logits(dev, deeplab):
    """predict_image(blend='mean') on the fitted image equals, bit for bit, stitch_overlap_logits of the per-tile Model.test logits (the
    same batches of 8 + 7 on both sides): the cutter, the network's own output pitch and the streaming accumulator add nothing."""
    from pylc_amd import inference
    model, img, tile, stride = deeplab['model'], deeplab['img'], deeplab['tile'], deeplab['stride']
    h, w = img.shape[1:]
    assert torch.equal(reflect_windows(img, tile, tile, stride), deeplab['tiles'])       # pad = 0: the fitted grid's windows
    mask, probs, conf = inference.predict_image(model, img, tile, stride, batch=8, blend='mean', return_probs=True, return_confidence=True)
    logits = _model_test_logits(model, deeplab['tiles'], 8)
    want_mask, want_probs = inference.stitch_overlap_logits(logits, h, w, tile, stride, return_probs=True)
    assert tuple(mask.shape) == (h, w) and mask.dtype == torch.uint8 and tuple(probs.shape) == (9, h, w)
    assert torch.equal(probs, want_probs) and torch.equal(mask, want_mask)
    assert torch.equal(conf, probs.max(0).values)
    assert float((probs.sum(0) - 1).abs().max()) < 1e-5
    # the return value: mask alone, or the tuple in the order (mask[, probs][, conf]); uint8 photographs give the same bytes
    assert torch.equal(inference.predict_image(model, img, tile, stride, blend='mean'), mask)
    m2, c2 = inference.predict_image(model, img.to(torch.uint8), tile, stride, blend='mean', return_confidence=True)
    assert torch.equal(m2, mask) and torch.equal(c2, conf)
    assert not model.net.training
    # the reference stitch is what it was: another mask (logits in the interiors), and no probabilities
    ref = inference.predict_image(model, img, tile, stride)
    assert ref.shape == mask.shape and ref.dtype == torch.uint8
    with pytest.raises(ValueError, match="blend='mean'"):
        inference.predict_image(model, img, tile, stride, return_probs=True)


def test_deeplab_mean_blend_matches_oracle(dev, deeplab):
    """Against the CPU oracle: test_step on the same windows, blended by the float64 numpy statement.  The conditions of
    test_predict_image_unet_matches_oracle: decided at a probability margin of 2e-3, more than 40 % decided, more than 97 % agreement,
    exact where decided."""
    from pylc_amd import inference
    model, img, tile, stride = deeplab['model'], deeplab['img'], deeplab['tile'], deeplab['stride']
    h, w = img.shape[1:]
    probs, want = stitch_overlap_np(deeplab['oracle_logits'], h, w, tile, stride)
    got = inference.predict_image(model, img, tile, stride, batch=8, blend='mean').cpu().numpy()
    assert got.shape == want.shape == (128, 192)
    top2 = np.sort(probs, axis=0)[-2:]
    decided = (top2[1] - top2[0]) > 2e-3
    agree = (got == want).mean()
    print('predict_image (DeepLab, mean blend): %.2f%% pixels agree, %.1f%% decided' % (100 * agree, 100 * decided.mean()))
    assert decided.mean() > 0.4 and agree > 0.97
    assert np.array_equal(got[decided], want[decided])


def test_deeplab_mean_blend_takes_an_unfitted_image(dev, deeplab):
    from pylc_amd import inference
    model, tile, stride = deeplab['model'], deeplab['tile'], deeplab['stride']
    img = deeplab['img'][:, :100, :150].contiguous()
    mask, probs = inference.predict_image(model, img, tile, stride, blend='mean', return_probs=True)
    assert tuple(mask.shape) == (100, 150) and mask.dtype == torch.uint8 and int(mask.max()) < 9
    assert float((probs.sum(0) - 1).abs().max()) < 1e-5
    logits = _model_test_logits(model, reflect_windows(img, tile, tile, stride), 8)       # 3 x 4 windows, the last ones moved back
    assert logits.shape[0] == 12
    want_mask, want_probs = inference.stitch_overlap_logits(logits, 100, 150, tile, stride, return_probs=True)
    assert torch.equal(mask, want_mask) and torch.equal(probs, want_probs)
    assert tuple(inference.predict_image(model, img, tile, blend='mean', stride=17).shape) == (100, 150)      # any stride in [1, tile]
    with pytest.raises(ValueError, match='not fitted'):
        inference.predict_image(model, img, tile, stride)                                  # the reference stitch, as before


def test_deeplab_flip_ensemble(dev, deeplab):
    """flip=True against its composition by hand: the network on the mirrored windows, those logits mirrored back, and the float64 mean
    over both members and the covering tiles.  The result does not depend on the batch size."""
    from pylc_amd import inference
    model, img, tile, stride = deeplab['model'], deeplab['img'], deeplab['tile'], deeplab['stride']
    h, w = img.shape[1:]
    mask, probs, conf = inference.predict_image(model, img, tile, stride, batch=8, blend='mean', flip=True, return_probs=True,
                                                return_confidence=True)
    l0 = _model_test_logits(model, deeplab['tiles'], 8).cpu().numpy()
    l1 = _model_test_logits(model, torch.flip(deeplab['tiles'], dims=[3]).contiguous(), 8).cpu().numpy()
    want_p, want_m = blend_mean_np([l0, l1], h, w, tile, stride)                         # (mirrors member 1 back)
    err = np.abs(probs.cpu().numpy() - want_p).max()
    top2 = np.sort(want_p, axis=0)[-2:]
    decided = (top2[1] - top2[0]) > 1e-5
    print('flip ensemble: max|probs - fp64 composition| %.3g, %.3f%% decided' % (err, 100 * decided.mean()))
    assert err < 1e-6
    assert np.array_equal(mask.cpu().numpy()[decided], want_m[decided])
    assert torch.equal(conf, probs.max(0).values)
    one = inference.predict_image(model, img, tile, stride, batch=8, blend='mean', return_probs=True)[1]
    assert not torch.equal(one, probs)                                                   # the second member is really there
    m3, p3, c3 = inference.predict_image(model, img, tile, stride, batch=3, blend='mean', flip=True, return_probs=True,
                                         return_confidence=True)
    assert torch.equal(m3, mask) and torch.equal(p3, probs) and torch.equal(c3, conf)


def test_one_rank_group_equals_no_group(dev, deeplab):
    import torch.distributed as dist
    from pylc_amd import inference
    model, img, tile, stride = deeplab['model'], deeplab['img'], deeplab['tile'], deeplab['stride']
    want = inference.predict_image(model, img, tile, stride, blend='mean', flip=True, return_probs=True, return_confidence=True)
    assert not dist.is_initialized()                                  # (the multi-rank tests of this suite run in processes of their own)
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group('gloo', init_method='file://' + os.path.join(tmp, 'store'), rank=0, world_size=1)
        try:
            got = inference.predict_image(model, img, tile, stride, group=dist.group.WORLD, blend='mean', flip=True, return_probs=True,
                                          return_confidence=True)
        finally:
            dist.destroy_process_group()
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and len(got) == 3


# ---- 5: segment_photo ---------------------------------------------------------------------------------------------------------------------
def test_segment_photo_deeplab_mean_blend(dev, deeplab):
    from pylc_amd import inference, photo
    from tests.test_photo_gpu import PALETTE, photo_np
    model = deeplab['model']
    image = photo_np(31, 100, 150)
    res = photo.segment_photo(model, image, tile=64, blend='mean', return_probs=True, return_confidence=True)
    g = res.geometry
    assert (g['h_scaled'], g['w_scaled'], g['h_fitted'], g['w_fitted'], g['offset']) == (100, 150, 100, 150, 0)
    assert tuple(res.mask.shape) == (100, 150) and tuple(res.probs.shape) == (9, 100, 150) and tuple(res.confidence.shape) == (100, 150)
    assert res.rgb is None
    probs = res.probs.cpu().numpy()
    assert np.abs(probs.sum(0) - 1).max() < 1e-5
    assert np.array_equal(res.mask.cpu().numpy(), probs.argmax(0).astype(np.uint8))       # first maximum
    assert torch.equal(res.confidence, res.probs.max(0).values)
    # the same call by hand: the photograph as a [C,H,W] uint8 image through predict_image
    chw = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1))).to(dev)
    m, p = inference.predict_image(model, chw, 64, blend='mean', return_probs=True)
    assert torch.equal(res.mask, m) and torch.equal(res.probs, p)
    # a scale step and a palette
    big = photo_np(32, 220, 320)
    col = photo.segment_photo(model, big, tile=64, scale=0.5, palette=PALETTE, blend='mean', flip=True, return_confidence=True)
    assert (col.geometry['h_scaled'], col.geometry['w_scaled']) == (110, 160) and tuple(col.rgb.shape) == (110, 160, 3)
    assert col.probs is None and tuple(col.confidence.shape) == (110, 160)
    assert float(col.confidence.min()) >= 1 / 9 - 1e-6 and float(col.confidence.max()) <= 1 + 1e-6
    for kw in ('flip', 'return_probs', 'return_confidence'):
        with pytest.raises(ValueError, match="blend='mean'"):
            photo.segment_photo(model, image, tile=64, **{kw: True})
    assert not model.net.training


def test_segment_photo_default_is_the_reference_round_trip(dev, deeplab):
    """The default call is what it was: predict_image on the uint8 fitted image, colourize + nearest resize back, encode."""
    from pylc_amd import inference, photo
    model = deeplab['model']
    from tests.test_photo_gpu import photo_np
    image = photo_np(33, 180, 230)
    res = photo.segment_photo(model, image, tile=64)
    fitted, g = photo.fit_image(image, 64, 32, None, dev)
    assert (g['h_fitted'], g['w_fitted']) == (128, 192)
    fm = inference.predict_image(model, fitted, 64, 32)
    ident = np.repeat(np.arange(9, dtype=np.uint8)[:, None], 3, 1)
    want = photo.encode_mask(inference.colourize(fm, ident, 180, 230), ident)
    assert torch.equal(res.mask, want) and res.probs is None and res.confidence is None and res.rgb is None
    assert torch.equal(fm, inference.predict_image(model, fitted.float(), 64, 32))


def test_segment_photo_unet_flip(dev):
    from pylc_amd import inference, photo, runtime
    from pylc_amd.model import Model, Meta
    from tests.test_photo_gpu import photo_np
    runtime.dropout_enabled = False
    torch.manual_seed(0)
    model = Model(Meta(arch='unet', ch=3, n_classes=9), dev).build()
    image = photo_np(23, 150, 200)
    res = photo.segment_photo(model, image, tile=256, flip=True, return_probs=True, return_confidence=True)
    assert tuple(res.mask.shape) == (150, 200) and tuple(res.probs.shape) == (9, 150, 200)
    assert float((res.probs.sum(0) - 1).abs().max()) < 1e-5
    assert torch.equal(res.confidence, res.probs.max(0).values)
    assert torch.equal(res.mask, res.probs.argmax(0).to(torch.uint8))
    # without the second member the streaming accumulator gives the one-shot stitch's bytes
    chw = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1))).to(dev)
    m1, p1 = inference.predict_overlap_tile(model, chw, 256, return_probs=True)
    m2, p2, c2 = inference.predict_overlap_tile(model, chw, 256, return_probs=True, return_confidence=True)
    assert torch.equal(m2, m1) and torch.equal(p2, p1) and torch.equal(c2, p1.max(0).values)
