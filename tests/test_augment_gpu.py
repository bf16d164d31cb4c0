"""The augmentation transform on the GPU (-m gpu): pylc_augment_tiles against the numpy restatement of tests/test_cpu_augment.py
(augment_np: the reference's augment_transform with OpenCV's arithmetic written out), bit for bit wherever the restatement's warp
coordinates lie farther than 1e-6 from a rounding tie -- at most 1e-4 of a tile's pixels may be left out for that reason --; the reflected
border; independence of the launch geometry; the fused statistics; TileSet.oversample against the hand composition, and into Model.train."""
import numpy as np
import pytest
import torch

from tests.test_cpu_augment import augment_np, augment_params_np, tiles_np
from tests.test_cpu_dataset import tile_sums_np

pytestmark = pytest.mark.gpu

MAX_TIE_SHARE = 1e-4


def _to_dev(dev, *arrays):
    return [torch.from_numpy(a).to(dev) for a in arrays]


def _compare(got_img, got_mask, want, what):
    """exact equality off the ties, and the share of a tile's pixels left out stays within MAX_TIE_SHARE"""
    for near in (want['near_img'], want['near_mask']):
        assert near.mean() <= MAX_TIE_SHARE, (what, near.mean())
    bad_img = (got_img != want['img']) & ~want['near_img'][None]
    bad_mask = (got_mask != want['mask']) & ~want['near_mask']
    print('%s: ties img %.2e mask %.2e, differing img %d mask %d' % (what, want['near_img'].mean(), want['near_mask'].mean(),
                                                                      int(bad_img.sum()), int(bad_mask.sum())))
    assert not bad_img.any() and not bad_mask.any(), what


@pytest.mark.parametrize('c', [3, 1])
@pytest.mark.parametrize('t', [128, 200])
def test_kernel_matches_restatement(dev, t, c):
    from pylc_amd import dataset
    img, mask = tiles_np(10 * t + c, 3, c, t)
    src = [2, 0, 1, 2, 0, 2, 1, 0]                                         # shuffled, with repeats
    copy = [0, 1, 2, 3, 3, 2, 1, 0]
    d_img, d_mask = _to_dev(dev, img, mask)
    out, mout, sums, hist = dataset.augment_tiles(d_img, d_mask, src, copy, n_classes=9)
    out, mout = out.cpu().numpy(), mout.cpu().numpy()
    assert out.shape == (8, c, t, t) and mout.shape == (8, t, t)
    seen = set()
    for k, (i, j) in enumerate(zip(src, copy)):
        minv, shift = augment_params_np(j, t)
        want = augment_np(img[i], mask[i], minv, shift)
        assert want['reflected'] == 0                                      # the reference's warps stay inside small tiles
        _compare(out[k], mout[k], want, 't %d c %d tile %d copy %d' % (t, c, i, j))
        seen |= set(np.unique(want['img']).tolist())
        assert (want['mask'] == 255).any()
        assert (want['upscaled'] - np.floor(want['upscaled']) > 0.5).any()     # np.int16 truncates where rounding would go up
    assert 255 in seen and min(seen) == 10                                 # the clip, and the smallest shift on the black band
    # the statistics: integer sums of what was written
    want_sums, want_hist = tile_sums_np(out, mout, 9)
    assert sums.dtype == torch.int64 and np.array_equal(sums.cpu().numpy(), want_sums)
    assert np.array_equal(hist.cpu().numpy(), want_hist) and want_hist[:, -1].all()          # the 255s land in the overflow bin


def _border_matrices():
    """a translation by 45 pixels with a mild perspective term, towards either corner: inverse maps, as the entry point takes them"""
    a = np.array([[1.0, 0.01, 45.0], [-0.02, 1.0, 45.0], [1e-4, 5e-5, 1.0]])
    b = np.array([[1.0, -0.01, -45.0], [0.02, 1.0, -45.0], [-5e-5, 1e-4, 1.0]])
    return np.stack([a, b])


def test_reflected_border(dev):
    """the reference's own warps never read a reflected pixel inside the crop of a small tile, so hand-made matrices drive that path"""
    from pylc_amd import dataset
    t = 128
    img, mask = tiles_np(77, 2, 3, t)
    minv = _border_matrices()
    d_img, d_mask = _to_dev(dev, img, mask)
    out, mout, sums, hist = dataset.warp_tiles(d_img, d_mask, [1, 0], minv, [0, 250], n_classes=9)
    out, mout = out.cpu().numpy(), mout.cpu().numpy()
    for k, i in enumerate((1, 0)):
        want = augment_np(img[i], mask[i], minv[k], (0, 250)[k])
        assert want['reflected'] > 0.05, want['reflected']
        _compare(out[k], mout[k], want, 'border %d (reflected share %.3f)' % (k, want['reflected']))
    assert out[1].min() >= 250                                             # the saturated shift
    want_sums, want_hist = tile_sums_np(out, mout, 9)
    assert np.array_equal(sums.cpu().numpy(), want_sums) and np.array_equal(hist.cpu().numpy(), want_hist)


def test_the_reference_warp_that_reflects(dev):
    """t = 512, j = 3: the one warp of the reference (rates are clipped to 4, so j <= 3) whose crop reads reflected pixels"""
    from pylc_amd import dataset
    t = 512
    img, mask = tiles_np(512, 1, 3, t)
    minv, shift = augment_params_np(3, t)
    want = augment_np(img[0], mask[0], minv, shift)
    assert want['reflected'] > 0.04, want['reflected']
    assert ((want['upscaled'] > 199.999) & (want['upscaled'] < 200)).mean() > 0.005       # the flat 200 band ends a hair below: 199 + shift
    d_img, d_mask = _to_dev(dev, img, mask)
    out, mout, sums, hist = dataset.augment_tiles(d_img, d_mask, [0], [3], n_classes=9)
    _compare(out[0].cpu().numpy(), mout[0].cpu().numpy(), want, 't 512 copy 3 (reflected share %.3f)' % want['reflected'])
    want_sums, want_hist = tile_sums_np(out.cpu().numpy(), mout.cpu().numpy(), 9)
    assert np.array_equal(sums.cpu().numpy(), want_sums) and np.array_equal(hist.cpu().numpy(), want_hist)


@pytest.mark.parametrize('t,c', [(128, 3), (200, 1)])
def test_result_does_not_depend_on_the_launch(dev, t, c):
    from pylc_amd import dataset
    from pylc_amd.lib import lib, check, ptr, stream
    img, mask = tiles_np(t + c, 3, c, t)
    d_img, d_mask = _to_dev(dev, img, mask)
    src, copy = [2, 0, 1, 2, 0], [0, 1, 2, 3, 0]
    base = dataset.augment_tiles(d_img, d_mask, src, copy, n_classes=9)
    for band in (1, 5, 0, t):
        again = dataset.augment_tiles(d_img, d_mask, src, copy, band_rows=band, n_classes=9)
        for a, b in zip(again, base):
            assert torch.equal(a, b), band
    # m split into two calls
    first = dataset.augment_tiles(d_img, d_mask, src[:2], copy[:2], n_classes=9)
    second = dataset.augment_tiles(d_img, d_mask, src[2:], copy[2:], band_rows=7, n_classes=9)
    for a, b, whole in zip(first, second, base):
        assert torch.equal(torch.cat([a, b]), whole)
    # without the mask (no out_mask, no hist), without statistics, and statistics without out_mask
    plain = dataset.augment_tiles(d_img, None, src, copy)
    assert torch.equal(plain[0], base[0]) and plain[1] is None and plain[3] is None and torch.equal(plain[2], base[2])
    params = [dataset.augment_params(j, t) for j in copy]
    bare = dataset.warp_tiles(d_img, d_mask, src, [p[0] for p in params], [p[1] for p in params], stats=False)
    assert torch.equal(bare[0], base[0]) and torch.equal(bare[1], base[1]) and bare[2] is None and bare[3] is None
    m = len(src)
    d_src = torch.tensor(src, dtype=torch.int32, device=dev)
    d_minv = torch.from_numpy(np.stack([p[0] for p in params])).to(dev)
    d_shift = torch.tensor([p[1] for p in params], dtype=torch.int32, device=dev)
    out = torch.empty_like(base[0])
    hist = torch.zeros_like(base[3])
    check(lib.pylc_augment_tiles(ptr(d_img), ptr(d_mask), 3, c, t, ptr(d_src), ptr(d_minv), ptr(d_shift), m, 0, ptr(out), None, 9, None,
                                 ptr(hist), stream()))
    assert torch.equal(out, base[0]) and torch.equal(hist, base[3])
    sums = torch.zeros_like(base[2])
    check(lib.pylc_augment_tiles(ptr(d_img), None, 3, c, t, ptr(d_src), ptr(d_minv), ptr(d_shift), m, 3, ptr(out), None, 0, ptr(sums), None,
                                 stream()))
    assert torch.equal(sums, base[2])


def test_oversample_on_the_device(dev):
    from pylc_amd import dataset, runtime
    from pylc_amd.model import Meta, Model
    from pylc_amd.nets import UNet
    t, k = 128, 9
    img, mask = tiles_np(6, 6, 3, t)
    mask[mask == 255] = 0                                                  # a training set: every class index is below n_classes
    rates = [0, 1, 4, 0, 2, 0]
    src, copy = dataset.oversample_layout(rates)
    wants = {int(pos): augment_np(img[src[pos]], mask[src[pos]], *augment_params_np(int(copy[pos]), t)) for pos in np.flatnonzero(copy >= 0)}
    sets = {}
    for keep in ('device', 'host'):
        ts = dataset.TileSet(3, k, t, keep=keep).from_arrays(img[:4], mask[:4]).from_arrays(img[4:], mask[4:])
        out = ts.oversample(rates, chunk=4)
        assert len(out) == 6 + 7 and out.keep == keep and len(ts) == 6
        assert out.img.is_cuda if keep == 'device' else out.img.is_pinned()
        got_img, got_mask = out.img.cpu().numpy(), out.mask.cpu().numpy()
        for pos in range(13):                                              # the hand composition: originals as they were, copies by the restatement
            if copy[pos] < 0:
                assert np.array_equal(got_img[pos], img[src[pos]]) and np.array_equal(got_mask[pos], mask[src[pos]])
            else:
                _compare(got_img[pos], got_mask[pos], wants[pos], 'oversample %s entry %d' % (keep, pos))
        want_sums, want_hist = tile_sums_np(got_img, got_mask, k)
        assert not want_hist[:, -1].any()
        assert np.array_equal(out.sums, want_sums) and np.array_equal(out.hist, want_hist[:, :k])
        assert out.profile() == dataset.profile_from_sums(want_sums, want_hist[:, :k], t, k)
        sets[keep] = out
    assert torch.equal(sets['device'].img.cpu(), sets['host'].img) and np.array_equal(sets['device'].sums, sets['host'].sums)
    one_chunk = dataset.TileSet(3, k, t).from_arrays(img, mask).oversample(rates)
    assert torch.equal(one_chunk.img, sets['device'].img) and np.array_equal(one_chunk.sums, sets['device'].sums)
    # the class-balanced set feeds training: a small valid U-Net (three levels) fits a 128 tile
    runtime.dropout_enabled = False
    balanced = sets['device'].coshuffle(5)
    x, y = next(iter(balanced.batches(2)))
    assert x.is_cuda and tuple(x.shape) == (2, 3, t, t) and tuple(y.shape) == (2, t, t)
    net = UNet(in_channels=3, n_classes=k, depth=3, wf=6, dropout=0.5)
    model = Model(Meta(arch='unet', n_classes=k, pad_size=(t - net.output_size(t)) // 2).update(balanced.profile()), dev).build()
    model.net = net.to(dev)
    model.init_optim()
    loss = model.train(x, y)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


def test_argument_errors_launch_nothing(dev):
    from pylc_amd import dataset
    from pylc_amd.lib import PylcError
    img = torch.zeros((2, 3, 128, 128), dtype=torch.uint8, device=dev)
    mask = torch.zeros((2, 128, 128), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match='src_index'):
        dataset.augment_tiles(img, mask, [0, 2], [0, 0])
    with pytest.raises(ValueError, match='src_index'):
        dataset.augment_tiles(img, mask, [-1], [0])
    with pytest.raises(ValueError, match='below 128'):
        dataset.augment_tiles(img[:, :, :64, :64], None, [0], [0])
    with pytest.raises(PylcError, match='tile=64'):
        dataset.warp_tiles(img[:, :, :64, :64].contiguous(), None, [0], np.eye(3)[None], [0])
    with pytest.raises(PylcError, match='Cimg=2'):
        dataset.warp_tiles(img[:, :2].contiguous(), None, [0], np.eye(3)[None], [0])
    with pytest.raises(PylcError, match='band_rows'):
        dataset.warp_tiles(img, None, [0], np.eye(3)[None], [0], band_rows=129)
    with pytest.raises(ValueError, match='matrices'):
        dataset.warp_tiles(img, None, [0, 1], np.eye(3)[None], [0, 0])
    from pylc_amd.lib import lib, ptr, stream
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    assert lib.pylc_augment_tiles(ptr(img), None, 2, 3, 128, ptr(idx), ptr(eye), ptr(idx), 1, 0, None, None, 0, None, None, stream()) == 1
    assert b'NULL' in lib.pylc_last_error()
    torch.cuda.synchronize()                                               # nothing faulted
