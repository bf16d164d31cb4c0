"""Full-image U-Net inference by overlap tiles on the GPU (-m gpu): the mirrored-window cutter (pylc_image_pack_tiles_reflect)
against torch.nn.functional.pad(mode='reflect'), the blend-and-argmax stitch (pylc_stitch_overlap_argmax) against the float64 numpy
restatement of tests/test_cpu_overlap_tile.py, and predict_image on a U-Net against the CPU oracle and against per-tile Model.test."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_cpu_overlap_tile import overlap_origins, stitch_overlap_np

pytestmark = pytest.mark.gpu


def reflect_windows(img, tile, out, stride):
    """[C,H,W] host image -> [n, C, tile, tile] mirrored windows of the overlap-tile grid (row-major)."""
    pad = (tile - out) // 2
    h, w = img.shape[1:]
    p = F.pad(img[None].float(), (pad,) * 4, mode='reflect')[0]
    return torch.stack([p[:, oy:oy + tile, ox:ox + tile] for oy in overlap_origins(h, out, stride) for ox in overlap_origins(w, out, stride)])


def pack(img_dev, tile, out, stride, first, n, mean, std):
    from pylc_amd import ops
    from pylc_amd.lib import lib, check, ptr, stream
    c, h, w = img_dev.shape
    got = ops.empty_nhwc(n, 4, tile, tile, img_dev.device)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    check(lib.pylc_image_pack_tiles_reflect(ptr(img_dev), int(img_dev.dtype == torch.uint8), c, h, w, tile, out, stride, first, n, m, s,
                                            ptr(got), stream()))
    return got


@pytest.mark.parametrize('ch', [3, 1])
@pytest.mark.parametrize('stride', [68, 50])
def test_pack_reflect_matches_fpad(dev, ch, stride):
    import oracle
    from oracle import step as ostep
    from pylc_amd import lib as L
    from tests import _data as D
    L.init()
    tile, out = 256, 68
    img = D.tiles(31 + ch, 1, ch, 150, 200)[0]
    win = reflect_windows(img, tile, out, stride)
    n = win.shape[0]
    want = oracle.normalize_image(win, ostep.PX_RGB_MEAN, ostep.PX_RGB_STD)
    if ch == 1:
        want = want.expand(n, 3, tile, tile)
        mv = float(np.mean(np.asarray(ostep.PX_RGB_MEAN, np.float32)))
        sv = float(np.mean(np.asarray(ostep.PX_RGB_STD, np.float32)))
        mean, std = [mv] * 3, [sv] * 3
    else:
        mean, std = list(ostep.PX_RGB_MEAN), list(ostep.PX_RGB_STD)
    got = pack(img.to(dev), tile, out, stride, 0, n, mean, std)
    assert (got[:, :3].cpu() - want).abs().max().item() < 1e-7 and float(got[:, 3].abs().max()) == 0.0
    got_u8 = pack(img.to(torch.uint8).to(dev), tile, out, stride, 0, n, mean, std)      # a photograph's bytes: the same tiles, bit for bit
    assert torch.equal(got_u8, got)
    part = pack(img.to(dev), tile, out, stride, 3, 4, mean, std)                        # a batch from the middle of the tile list
    assert torch.equal(part, got[3:7])


STITCH = [(150, 200, 68, 68, (9, 2)), (150, 200, 68, 34, (9,)), (150, 200, 68, 25, tuple(range(2, 17))), (324, 648, 324, 324, (9,)),
          (331, 647, 324, 162, (9, 16))]


@pytest.mark.parametrize('h,w,out,stride,classes', STITCH)
def test_stitch_overlap_matches_numpy(dev, h, w, out, stride, classes):
    from pylc_amd import inference
    n = len(overlap_origins(h, out, stride)) * len(overlap_origins(w, out, stride))
    for c in classes:
        logits = (np.random.RandomState(h + w + stride + c).standard_normal((n, c, out, out)) * 3).astype(np.float32)
        mask, probs = inference.stitch_overlap_logits(torch.from_numpy(logits).to(dev), h, w, out, stride, return_probs=True)
        mask, probs = mask.cpu().numpy(), probs.cpu().numpy()
        want_p, want_m = stitch_overlap_np(logits, h, w, out, stride)
        assert mask.shape == (h, w) and probs.shape == (c, h, w)
        err = np.abs(probs - want_p).max()
        top2 = np.sort(want_p, axis=0)[-2:]
        decided = (top2[1] - top2[0]) > 1e-5            # expf vs np.exp in the last ulp at exact near-ties
        print('stitch %dx%d out %d stride %d C %d: max|probs - fp64| %.3g, %.4f%% decided' % (h, w, out, stride, c, err, 100 * decided.mean()))
        assert err < 1e-6
        assert np.abs(probs.sum(0) - 1).max() < 1e-5
        assert decided.mean() >= 0.999
        assert np.array_equal(mask[decided], want_m[decided])
        assert np.array_equal(inference.stitch_overlap_logits(torch.from_numpy(logits).to(dev), h, w, out, stride).cpu().numpy(), mask)


def test_predict_image_unet_matches_oracle(dev):
    """The U-Net path end to end: mirrored 256 px windows (out 68) -> eval forward -> overlap blend -> class mask, against the CPU
    oracle's Model.test on F.pad(reflect) windows and the numpy blend.  (predict_image raised for every U-Net before this path.)"""
    import oracle
    from oracle import step as ostep
    from pylc_amd import inference, runtime
    from pylc_amd.model import Model, Meta
    from tests import _data as D
    runtime.dropout_enabled = False
    tile, out = 256, 68
    img = D.learnable_tiles(23, 1, 200, 9, cell=16)[0][0, :, :150, :]          # [3,150,200]
    h, w = img.shape[1:]
    win = reflect_windows(img, tile, out, out)
    cfg = ostep.StepConfig('unet', 'resnet', 9, 3, dropout=False)
    wts = ostep.calibrate_bn(oracle.formula_state(oracle.state_spec('unet', 'resnet', 9, 3), salt=3), cfg, win.clone())
    logits = ostep.test_step({k: v.clone() for k, v in wts.items()}, cfg, win.clone()).numpy()
    assert logits.shape == (win.shape[0], 9, out, out)
    probs, want = stitch_overlap_np(logits, h, w, out, out)
    model = Model(Meta(arch='unet', ch=3, n_classes=9), dev).build()
    model.net.load_state_dict(wts)
    got = inference.predict_image(model, img, tile, batch=8).cpu().numpy()
    assert got.shape == want.shape == (150, 200)
    top2 = np.sort(probs, axis=0)[-2:]
    decided = (top2[1] - top2[0]) > 2e-3
    agree = (got == want).mean()
    print('predict_image (U-Net): %.2f%% pixels agree, %.1f%% decided' % (100 * agree, 100 * decided.mean()))
    assert decided.mean() > 0.4 and agree > 0.97
    assert np.array_equal(got[decided], want[decided])


@pytest.mark.parametrize('ch', [3, 1])
def test_predict_image_unet_full_size(dev, ch):
    """512 px windows (out 324) over an unfitted 700 x 900 image: 3 x 3 tiles, the last row and column clamped, batches 8 + 1.
    predict_image equals per-tile Model.test on host-cut windows in the same batches + stitch_overlap_logits, bit for bit; it is
    deterministic, takes uint8 as well as float, and its probabilities argmax to its mask."""
    import oracle
    from oracle import step as ostep
    from pylc_amd import inference
    from pylc_amd.model import Model, Meta
    h, w, tile, out = 700, 900, 512, 324
    rs = np.random.RandomState(20 + ch)
    low = torch.from_numpy(rs.uniform(0, 255, (1, ch, h // 50, w // 50)).astype(np.float32))
    img = F.interpolate(low, size=(h, w), mode='bilinear', align_corners=True)[0]
    img = (img + torch.from_numpy(rs.normal(0, 8, (ch, h, w)).astype(np.float32))).clamp(0, 255).round()
    win = reflect_windows(img, tile, out, out)
    assert win.shape[0] == 9
    # formula weights with BatchNorm statistics calibrated on these windows: O(1) eval activations, a mask of many classes
    cfg = ostep.StepConfig('unet', 'resnet', 9, ch, dropout=False)
    wts = ostep.calibrate_bn(oracle.formula_state(oracle.state_spec('unet', 'resnet', 9, ch), salt=7 + ch), cfg, win.clone())
    model = Model(Meta(arch='unet', ch=ch, n_classes=9), dev).build()
    model.net.load_state_dict(wts)
    mask = inference.predict_image(model, img, tile, batch=8)
    assert tuple(mask.shape) == (h, w) and mask.dtype == torch.uint8 and int(mask.max()) < 9
    assert torch.equal(inference.predict_image(model, img, tile, batch=8), mask)                 # deterministic
    assert torch.equal(inference.predict_image(model, img.to(torch.uint8), tile, batch=8), mask)  # uint8 photograph
    model.net.eval()
    logits = torch.cat([model.test(win[k:k + 8])[0].float() for k in range(0, win.shape[0], 8)])
    ref = inference.stitch_overlap_logits(logits, h, w, out, out)
    agree = float((ref == mask).float().mean())
    counts = torch.bincount(mask.flatten().long(), minlength=9).tolist()
    print('U-Net full size ch=%d: %.4f%% of %d pixels agree with per-tile Model.test + stitch; class counts %s' % (ch, 100 * agree, h * w, counts))
    assert sum(c > 0 for c in counts) >= 3
    assert agree >= 0.9999
    assert torch.equal(ref, mask)                   # the same batches (8 + 1) on both sides
    m2, probs = inference.predict_overlap_tile(model, img, tile, return_probs=True)
    assert torch.equal(m2, mask) and tuple(probs.shape) == (9, h, w)
    assert torch.equal(probs.argmax(0).to(torch.uint8), mask)
    assert float((probs.sum(0) - 1).abs().max()) < 1e-5
