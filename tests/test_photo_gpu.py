"""Whole photographs on the GPU (-m gpu): pylc_resize_area_u8 against the numpy INTER_AREA restatements of tests/test_cpu_photo.py,
pylc_class_encode_resize against the reference's class_encode, pylc_image_pack_tiles_ex against pylc_image_pack_tiles, segment_photo
against the hand composition of its steps and the CPU oracle, the U-Net path against predict_overlap_tile, and PhotoEvaluator against
the reference's aggregate scores."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_cpu_photo import (class_encode_np, encode_resize_np, reference_scores, resize_area_np)

pytestmark = pytest.mark.gpu


def photo_np(seed, h, w, c=3):
    """a seeded uint8 photograph with smooth structure (so resizes see gradients, not only noise) plus noise"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 60 * np.sin(x[..., None] / (7.0 + np.arange(c)) + y[..., None] / 11.0) + rs.randint(-60, 61, (h, w, c))
    img = np.clip(base, 0, 255).astype(np.uint8)
    return img if c == 3 else img[..., 0]


def gpu_resize(img_hwc, oh, ow, dev, planar=False):
    from pylc_amd import photo
    t = torch.from_numpy(np.ascontiguousarray(img_hwc.transpose(2, 0, 1) if planar else img_hwc)).to(dev)
    return photo.resize_area(t, oh, ow, planar=planar).cpu().numpy()


def check_against_exact(got, img, oh, ow):
    ex = resize_area_np(img, oh, ow, exact=True)
    frac = ex - np.floor(ex)
    decided = np.abs(frac - 0.5) > 1e-3
    assert np.array_equal(got[decided], np.rint(ex[decided]).astype(np.uint8))
    assert np.abs(got.astype(np.float64) - np.rint(ex)).max() <= 1


@pytest.mark.parametrize('c', [3, 1])
@pytest.mark.parametrize('hw,ohw', [((4940, 3453), (4096, 3072)), ((4940, 3453), (988, 690)), ((4940, 3453), (2470, 1726)),
                                    ((301, 457), (211, 333)), ((7, 5), (3, 2)), ((97, 130), (96, 129)), ((64, 66), (1, 1))])
def test_resize_area_matches_restatements(dev, c, hw, ohw):
    img = photo_np(5 + c, hw[0], hw[1], 3)[..., :c]
    got = gpu_resize(img, ohw[0], ohw[1], dev)
    assert got.shape == (c,) + ohw
    assert np.array_equal(got, resize_area_np(img, *ohw))           # OpenCV's fp32 order, bit for bit
    check_against_exact(got, img, *ohw)
    if hw[0] < 1000:
        assert np.array_equal(gpu_resize(img, ohw[0], ohw[1], dev, planar=True), got)


def test_resize_area_identity_and_factor_two(dev):
    img = photo_np(2, 203, 317)
    assert np.array_equal(gpu_resize(img, 203, 317, dev), img.transpose(2, 0, 1))
    assert np.array_equal(gpu_resize(img, 203, 317, dev, planar=True), img.transpose(2, 0, 1))
    sub = np.ascontiguousarray(img[:202, :316])
    got = gpu_resize(sub, 101, 158, dev)
    ref = torch.round(F.avg_pool2d(torch.from_numpy(sub.transpose(2, 0, 1)).float()[None], 2)[0]).to(torch.uint8).numpy()
    assert np.array_equal(got, ref)
    from pylc_amd import photo
    from pylc_amd.lib import PylcError
    with pytest.raises(PylcError):
        photo.resize_area(torch.from_numpy(img).to(dev), 204, 317)


def test_resize_area_matches_opencv(dev):
    cv2 = pytest.importorskip('cv2')
    for seed, (h, w), (oh, ow) in ((1, (4940, 3453), (4096, 3072)), (2, (301, 457), (211, 333)), (3, (400, 600), (200, 300))):
        img = photo_np(seed, h, w)
        got = gpu_resize(img, oh, ow, dev)
        want = cv2.resize(img, (ow, oh), interpolation=cv2.INTER_AREA).transpose(2, 0, 1)
        diff = np.abs(got.astype(np.int16) - want)
        assert diff.max() <= 1 and (diff == 0).mean() >= 0.999


def test_class_encode_resize(dev):
    from pylc_amd import photo
    rs = np.random.RandomState(4)
    pal = rs.randint(0, 256, (9, 3)).astype(np.uint8)
    pal[7] = pal[2]                                                   # a repeated colour: index 7 wins
    h, w = 333, 517
    rgb = pal[rs.randint(0, 9, (h, w))]
    stray = rs.rand(h, w) < 0.05
    rgb[stray] = rs.randint(0, 256, (int(stray.sum()), 3))           # colours of no class -> 1
    for oh, ow in ((h, w), (211, 400), (100, 517), (333, 17)):
        got = photo.encode_mask(rgb, pal, (oh, ow), dev).cpu().numpy()
        want = encode_resize_np(rgb, pal, oh, ow)
        assert np.array_equal(got, want), (oh, ow)
    enc = photo.encode_mask(torch.from_numpy(rgb).to(dev), pal).cpu().numpy()
    assert np.array_equal(enc, class_encode_np(rgb, pal))
    assert (enc == 7).any() and not (enc == 2).any() and (enc[stray] == 1).all()


@pytest.mark.parametrize('ch', [3, 1])
def test_pack_tiles_ex_matches_float_cutter(dev, ch):
    from pylc_amd import ops, lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    h, w, tile, stride = 96, 160, 32, 16
    img = torch.from_numpy(np.ascontiguousarray(photo_np(8, h, w).transpose(2, 0, 1)[:ch])).to(dev)
    rows, cols = (h - tile) // stride + 1, (w - tile) // stride + 1
    n = rows * cols
    m, s = (C.c_float * 3)(132.47, 144.47, 149.45), (C.c_float * 3)(24.85, 22.04, 18.77)
    want = ops.empty_nhwc(n, 4, tile, tile, dev)
    check(lib.pylc_image_pack_tiles(ptr(img.float().contiguous()), ch, h, w, tile, stride, 0, n, m, s, ptr(want), stream()))
    for u8, src in ((1, img), (0, img.float().contiguous())):
        got = ops.empty_nhwc(n - 5, 4, tile, tile, dev)
        check(lib.pylc_image_pack_tiles_ex(ptr(src), u8, ch, h, w, tile, stride, 5, n - 5, m, s, ptr(got), stream()))
        assert torch.equal(got, want[5:])


def _deeplab(dev, ch=3, salt=2, calib=None):
    import oracle
    from oracle import step as ostep
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    runtime.dropout_enabled = False
    cfg = ostep.StepConfig('deeplab', 'resnet', 9, ch, dropout=False)
    w = oracle.formula_state(oracle.state_spec('deeplab', 'resnet', 9, ch), salt=salt)
    if calib is not None:
        w = ostep.calibrate_bn(w, cfg, calib)
    model = Model(Meta(ch=ch), dev).build()
    model.net.load_state_dict(w)
    return model, w, cfg


PALETTE = np.array([[0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [128, 128, 128],
                    [255, 255, 255]], np.uint8)


def _composition(model, image, tile, stride, scale, pal, dev):
    """the steps by hand: fit, predict_image on the fitted image (as float), colourize + nearest resize, encode"""
    from pylc_amd import inference, photo
    fitted, g = photo.fit_image(image, tile, stride, scale, dev)
    m = inference.predict_image(model, fitted.float(), tile, stride)
    rgb = inference.colourize(m, pal, g['h_scaled'], g['w_scaled'])
    return photo.encode_mask(rgb, pal), rgb, fitted, m, g


def test_segment_photo_deeplab(dev):
    import oracle
    from oracle import step as ostep
    from pylc_amd import photo
    image = photo_np(21, 300, 460)
    tiles_np, rows, cols = oracle.split_tiles(resize_area_np(image, 256, 448).astype(np.float32), 64, 32)
    assert (rows, cols) == (7, 13)
    model, w, cfg = _deeplab(dev, calib=torch.from_numpy(tiles_np[::6].copy()))
    res = photo.segment_photo(model, image, tile=64, palette=PALETTE)
    g = res.geometry
    assert (g['h_fitted'], g['w_fitted'], g['h_scaled'], g['w_scaled'], g['offset']) == (256, 448, 300, 460, 0)
    want_mask, want_rgb, fitted, fmask, _ = _composition(model, image, 64, 32, None, PALETTE, dev)
    assert torch.equal(res.mask, want_mask) and torch.equal(res.rgb, want_rgb)
    assert np.array_equal(fitted.cpu().numpy(), resize_area_np(image, 256, 448))
    again = photo.segment_photo(model, image, tile=64, palette=PALETTE)            # repeated calls: the same bytes
    assert torch.equal(again.mask, res.mask) and torch.equal(again.rgb, res.rgb)
    # no palette: the identity palette gives the nearest-resized class mask
    plain = photo.segment_photo(model, image, tile=64)
    assert plain.rgb is None
    ident = np.repeat(np.arange(9, dtype=np.uint8)[:, None], 3, 1)
    assert torch.equal(plain.mask, _composition(model, image, 64, 32, None, ident, dev)[0])
    assert torch.equal(plain.mask, res.mask)                                       # a palette of distinct colours changes nothing
    # a palette with a repeated colour: the reference's round trip sends class 2 to 7
    dup = PALETTE.copy()
    dup[7] = dup[2]
    d = photo.segment_photo(model, image, tile=64, palette=dup)
    assert torch.equal(d.mask, _composition(model, image, 64, 32, None, dup, dev)[0])
    assert torch.equal(d.mask, torch.where(res.mask == 2, torch.full_like(res.mask, 7), res.mask))
    # the mask on the fitted image against the CPU oracle (split, test_step, the reference's stitch)
    logits = ostep.test_step({k: v.clone() for k, v in w.items()}, cfg, torch.from_numpy(tiles_np)).numpy()
    scores = oracle.stitch_scores(logits, rows, cols, 64, 32)
    got, want = fmask.cpu().numpy(), scores.argmax(0).astype(np.uint8)
    top2 = np.sort(scores, axis=0)[-2:]
    decided = (top2[1] - top2[0]) > 4e-3            # tests/test_inference_gpu.py: HIP and CPU logits differ by <= 1e-3
    print('segment_photo: %.2f%% of fitted pixels agree with the oracle, %.1f%% decided' % (100 * (got == want).mean(), 100 * decided.mean()))
    assert decided.mean() > 0.2 and (got == want).mean() > 0.9       # a noisy photograph: more near-ties than blob fixtures
    assert np.array_equal(got[decided], want[decided])
    with pytest.raises(ValueError):
        photo.segment_photo(model, image[..., 0], tile=64)                         # channel count
    assert model.net.training                                                      # the mode came back


def test_segment_photo_grayscale_and_scale(dev):
    from pylc_amd import photo
    image = photo_np(22, 620, 900, 1)
    model, _, _ = _deeplab(dev, ch=1, salt=3)
    model.net.eval()
    res = photo.segment_photo(model, image, tile=64, scale=0.5, palette=PALETTE)
    g = res.geometry
    assert (g['h_scaled'], g['w_scaled']) == (310, 450) and (g['h_fitted'], g['w_fitted']) == (256, 448)
    want = _composition(model, image, 64, 32, 0.5, PALETTE, dev)
    assert torch.equal(res.mask, want[0]) and torch.equal(res.rgb, want[1])
    two_step = resize_area_np(resize_area_np(image[..., None], 310, 450).transpose(1, 2, 0), 256, 448)
    assert np.array_equal(want[2].cpu().numpy(), two_step)                        # two resizes, uint8 between them
    assert not model.net.training


def test_segment_photo_unet(dev):
    from pylc_amd import inference, photo, runtime
    from pylc_amd.model import Model, Meta
    runtime.dropout_enabled = False
    torch.manual_seed(0)
    model = Model(Meta(arch='unet', ch=3, n_classes=9), dev).build()
    image = photo_np(23, 600, 700)
    res = photo.segment_photo(model, image, tile=256, scale=0.5, return_probs=True)
    g = res.geometry
    assert (g['h_scaled'], g['w_scaled'], g['h_fitted'], g['w_fitted']) == (300, 350, 300, 350)
    scaled = photo.resize_area(torch.from_numpy(image).to(dev), 300, 350)
    mask, probs = inference.predict_overlap_tile(model, scaled, 256, return_probs=True)
    assert torch.equal(res.mask, mask) and torch.equal(res.probs, probs) and res.rgb is None
    col = photo.segment_photo(model, image, tile=256, scale=0.5, palette=PALETTE)
    assert torch.equal(col.mask, mask) and torch.equal(col.rgb, inference.colourize(mask, PALETTE))


def test_photo_evaluator(dev):
    from pylc_amd import photo
    model, _, _ = _deeplab(dev, salt=4)
    rs = np.random.RandomState(9)
    ev = photo.PhotoEvaluator(9, PALETTE)
    trues, preds = [], []
    for k, (h, w, scale) in enumerate(((300, 460, None), (600, 920, 0.5), (330, 470, None))):
        res = photo.segment_photo(model, photo_np(40 + k, h, w), tile=64, scale=scale, palette=PALETTE)
        hs, ws = res.geometry['h_scaled'], res.geometry['w_scaled']
        # a ground truth at full size: the prediction nearest-upsampled with a third of its pixels changed, and a few stray colours
        pred = res.mask.cpu().numpy()
        gt_cls = pred[(np.arange(h) * hs) // h][:, (np.arange(w) * ws) // w]
        gt_cls = np.where(rs.rand(h, w) < 0.33, rs.randint(0, 9, (h, w)), gt_cls)
        gt = PALETTE[gt_cls]
        gt[rs.rand(h, w) < 0.01] = (1, 2, 3)
        per = ev.add(res, gt)
        yt = encode_resize_np(gt, PALETTE, hs, ws)
        trues.append(yt)
        preds.append(pred)
        want = reference_scores([yt], [pred], 9)
        for key in ('f1', 'iou', 'mcc'):
            assert abs(per[key] - want[key]) < 1e-12
    agg = ev.aggregate()
    want = reference_scores(trues, preds, 9)
    for key in ('f1', 'iou', 'mcc'):
        assert abs(agg[key] - want[key]) < 1e-12
    assert ev.cm.is_cuda and ev.cm.dtype == torch.int64
    with pytest.raises(ValueError, match='do not match'):
        ev.add(res, PALETTE[np.zeros((331, 470), np.int64)])
