"""Training tile sets on the GPU (-m gpu): pylc_extract_tiles and pylc_tile_stats against the torch.unfold and numpy int64 restatements
of tests/test_cpu_dataset.py, extract_photo against the hand composition of its steps, TileSet.profile() against the reference's
get_profile (tests/golden/dataset_profile.json), and a TileSet feeding Model.train."""
import numpy as np
import pytest
import torch

from tests.test_cpu_dataset import CASES, check_profile, fixture, profile_case, tile_sums_np, unfold_tiles
from tests.test_cpu_photo import encode_resize_np, resize_area_np
from tests.test_photo_gpu import PALETTE, photo_np

pytestmark = pytest.mark.gpu


def _image_and_mask(seed, h, w, c, n_classes):
    """a planar uint8 image and a mask whose values run up to n_classes (one past the last class) with a few 255s"""
    rs = np.random.RandomState(seed)
    img = np.ascontiguousarray(photo_np(seed, h, w).transpose(2, 0, 1)[:c])
    mask = rs.randint(0, n_classes + 1, (h, w)).astype(np.uint8)
    mask[rs.rand(h, w) < 0.01] = 255
    return img, mask


@pytest.mark.parametrize('c', [3, 1])
@pytest.mark.parametrize('tile,stride', [(32, 32), (32, 16), (24, 8)])
@pytest.mark.parametrize('hw,n_classes', [((101, 150), 9), ((96, 160), 16), ((101, 150), 2)])
def test_cutter_and_statistics_exact(dev, c, tile, stride, hw, n_classes):
    from pylc_amd import dataset
    h, w = hw
    img, mask = _image_and_mask(h + tile + c, h, w, c, n_classes)
    want_img, want_mask = unfold_tiles(img, tile, stride), unfold_tiles(mask, tile, stride)
    want_sums, want_hist = tile_sums_np(want_img, want_mask, n_classes)
    n = want_img.shape[0]
    assert n == np.prod(dataset.tile_grid_counts(h, w, tile, stride)) and n > 1
    assert want_hist[:, n_classes - 1].all() and want_hist[:, n_classes].all()         # the last class and the overflow bin are in use
    d_img, d_mask = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    got = dataset.cut_tiles(d_img, d_mask, tile, stride, n_classes)
    assert np.array_equal(got[0].cpu().numpy(), want_img) and np.array_equal(got[1].cpu().numpy(), want_mask)
    assert got[2].dtype == torch.int64 and np.array_equal(got[2].cpu().numpy(), want_sums)
    assert np.array_equal(got[3].cpu().numpy(), want_hist)
    # two first_tile chunks, another launch geometry, a second run: the same bits
    k = n // 2 + 1
    a = dataset.cut_tiles(d_img, d_mask, tile, stride, n_classes, 0, k, band_rows=5)
    b = dataset.cut_tiles(d_img, d_mask, tile, stride, n_classes, k, n - k, band_rows=tile)
    again = dataset.cut_tiles(d_img, d_mask, tile, stride, n_classes, band_rows=1)
    for i in range(4):
        assert torch.equal(torch.cat([a[i], b[i]]), got[i]) and torch.equal(again[i], got[i])
    # the statistics entry point on the tiles just written
    for band in (0, 7):
        sums, hist = dataset.tile_stats(got[0], got[1], n_classes, band_rows=band)
        assert torch.equal(sums, got[2]) and torch.equal(hist, got[3])
    # without a mask
    plain = dataset.cut_tiles(d_img, None, tile, stride)
    assert torch.equal(plain[0], got[0]) and plain[1] is None and plain[3] is None and torch.equal(plain[2], got[2])
    assert torch.equal(dataset.tile_stats(got[0])[0], got[2])


def test_cutter_on_an_unaligned_view(dev):
    """source rows that start at every byte offset: the image is a slice of a larger buffer"""
    from pylc_amd import dataset
    img, mask = _image_and_mask(3, 70, 90, 3, 9)
    want = unfold_tiles(img, 32, 19)
    want_sums, _ = tile_sums_np(want)
    for off in (1, 2, 3, 5):
        buf = torch.zeros(img.size + off + 64, dtype=torch.uint8, device=dev)
        view = buf[off:off + img.size].view(3, 70, 90)
        view.copy_(torch.from_numpy(img))
        tiles, _, sums, _ = dataset.cut_tiles(view, None, 32, 19)
        assert np.array_equal(tiles.cpu().numpy(), want) and np.array_equal(sums.cpu().numpy(), want_sums)


@pytest.mark.parametrize('t', [264, 1024])
def test_sums_do_not_overflow(dev, t):
    """all 255: sum x^2 per channel is 4.53e9 at 264^2 (past 2^32) and 6.8e10 at 1024^2"""
    from pylc_amd import dataset
    img = torch.full((1, 3, t, t), 255, dtype=torch.uint8, device=dev)
    mask = torch.zeros((1, t, t), dtype=torch.uint8, device=dev)
    sums, hist = dataset.tile_stats(img, mask, 9)
    assert sums.cpu().tolist() == [[[t * t * 255] * 3, [t * t * 255 * 255] * 3]] and t * t * 255 * 255 > 2 ** 32
    assert hist.cpu().tolist() == [[t * t] + [0] * 9]
    cut = dataset.cut_tiles(img[0], mask[0], t, t, 9)
    assert torch.equal(cut[0], img) and torch.equal(cut[2], sums) and torch.equal(cut[3], hist)
    prof = dataset.TileSet(3, 9, t).from_arrays(img, mask).profile()
    assert prof['px_std'] == [0.0, 0.0, 0.0] and prof['px_mean'] == [255.0, 255.0, 255.0]


def test_bad_arguments_and_bad_masks(dev):
    from pylc_amd import dataset
    from pylc_amd.lib import PylcError
    img = torch.zeros((3, 64, 64), dtype=torch.uint8, device=dev)
    with pytest.raises(PylcError, match='exceeds the image'):
        dataset.cut_tiles(img, None, 65, 65)
    with pytest.raises(PylcError, match='outside the 2x2 grid'):
        dataset.cut_tiles(img, None, 32, 32, None, 3, 2)
    with pytest.raises(PylcError, match='stride'):
        dataset.cut_tiles(img, None, 32, 0, None, 0, 1)
    with pytest.raises(PylcError, match='n_classes'):
        dataset.cut_tiles(img, img[0], 32, 32, 17)
    with pytest.raises(PylcError, match='band_rows'):
        dataset.cut_tiles(img, None, 32, 32, band_rows=33)
    # a mask that holds a class index >= n_classes: the palette has 9 colours, the set 5 classes
    rs = np.random.RandomState(1)
    cls = rs.randint(0, 9, (64, 96))
    with pytest.raises(ValueError, match='%d mask pixels' % int((cls >= 5).sum())):
        dataset.extract_photo(photo_np(1, 64, 96), PALETTE[cls], PALETTE, tile=32, n_classes=5)
    ok = dataset.extract_photo(photo_np(1, 64, 96), PALETTE[cls], PALETTE, tile=32)
    assert ok.hist.shape == (6, 10) and int(ok.hist.sum()) == 6 * 32 * 32
    torch.cuda.synchronize()                                               # nothing faulted


def test_extract_photo_end_to_end(dev):
    from pylc_amd import dataset, photo
    rs = np.random.RandomState(4)
    pal = rs.randint(0, 256, (9, 3)).astype(np.uint8)
    h, w = 301, 457
    image = photo_np(31, h, w)
    rgb = pal[rs.randint(0, 9, (h, w))]
    stray = rs.rand(h, w) < 0.05
    rgb[stray] = rs.randint(0, 256, (int(stray.sum()), 3))               # colours of no class -> 1
    for scale, (hs, ws) in ((0.5, (150, 228)), (None, (h, w))):
        ex = dataset.extract_photo(image, rgb, pal, tile=32, stride=32, scale=scale)
        want_img = unfold_tiles(resize_area_np(image, hs, ws), 32, 32)
        want_mask = unfold_tiles(encode_resize_np(rgb, pal, hs, ws), 32, 32)
        assert np.array_equal(ex.img.cpu().numpy(), want_img) and np.array_equal(ex.mask.cpu().numpy(), want_mask)
        sums, hist = tile_sums_np(want_img, want_mask, 9)
        assert np.array_equal(ex.sums.cpu().numpy(), sums) and np.array_equal(ex.hist.cpu().numpy(), hist)
        g = ex.geometry
        assert (g['h_full'], g['w_full'], g['h_scaled'], g['w_scaled'], g['h_fitted'], g['w_fitted'], g['offset']) == (h, w, hs, ws, hs, ws, 0)
        assert g['n'] == want_img.shape[0] == (hs // 32) * (ws // 32)
    # grayscale, overlapping tiles
    gray = dataset.extract_photo(image[..., 0], tile=32, stride=16)
    assert np.array_equal(gray.img.cpu().numpy(), unfold_tiles(image[None, ..., 0], 32, 16)) and gray.mask is None and gray.hist is None
    # fit=True, without a mask: photo.fit_image, then the cutter
    fit = dataset.extract_photo(image, tile=32, stride=32, fit=True)
    fitted, geom = photo.fit_image(image, 32, 32, None, dev)
    assert np.array_equal(fit.img.cpu().numpy(), unfold_tiles(fitted.cpu().numpy(), 32, 32))
    assert fit.geometry == dict(geom, n=(geom['h_fitted'] // 32) * (geom['w_fitted'] // 32))
    assert (geom['h_fitted'], geom['w_fitted']) != (h, w)


@pytest.mark.parametrize('name', ['rgb', 'gray'])
def test_profile_on_the_device_path(dev, name):
    from pylc_amd import dataset
    c = CASES[name]
    img, mask = profile_case(name)
    sets = {keep: dataset.TileSet(c['ch'], c['n_classes'], c['tile'], keep=keep).from_arrays(img[:3], mask[:3]).from_arrays(img[3:], mask[3:])
            for keep in ('device', 'host')}
    profs = {keep: ts.profile() for keep, ts in sets.items()}
    check_profile(profs['device'], fixture()[name])
    assert profs['device'] == profs['host']
    want_sums, want_hist = tile_sums_np(img, mask, c['n_classes'])
    assert np.array_equal(sets['host'].sums, want_sums) and np.array_equal(sets['device'].hist, want_hist[:, :-1])
    assert sets['device'].img.is_cuda and sets['host'].img.is_pinned()
    for ts in sets.values():
        ts.coshuffle(8)
    perm = np.random.RandomState(8).permutation(c['n'])
    for drop_last in (True, False):
        d = list(sets['device'].partition(0, 0.8).batches(3, drop_last))
        hst = list(sets['host'].partition(0, 0.8).batches(3, drop_last))
        assert len(d) == len(hst) > 0
        for (dx, dy), (hx, hy) in zip(d, hst):
            assert dx.is_cuda and dx.dtype == torch.uint8 and np.array_equal(dx.cpu().numpy(), hx) and np.array_equal(dy.cpu().numpy(), hy)
        assert np.array_equal(np.concatenate([hx for hx, _ in hst]), img[perm][:sum(x.shape[0] for x, _ in hst)])
    after = sets['device'].profile()                                       # a permutation reorders px_dist and changes no count
    assert after['px_dist'] == np.asarray(profs['device']['px_dist'])[perm].tolist() and after['px_dist'] != profs['device']['px_dist']
    assert after['dset_px_dist'] == profs['device']['dset_px_dist'] and after['weights'] == profs['device']['weights']


def test_tile_set_feeds_training(dev):
    """photographs -> TileSet -> profile() -> Meta.update -> Model.train: the device-resident batch gives the same three loss terms, bit for
    bit, as the same tiles handed over from the host"""
    import oracle
    from pylc_amd import dataset, runtime
    from pylc_amd.model import Meta, Model
    from tests import _data as D
    runtime.dropout_enabled = False
    image = photo_np(41, 128, 192)
    cls = D.blob_masks(7, 1, 128, 192, 9, cell=8)[0].numpy()
    ts = dataset.TileSet(3, 9, 64).add(dataset.extract_photo(image, PALETTE[cls], PALETTE, tile=64))
    assert len(ts) == 6
    prof = ts.profile()
    batches = ts.batches(2)
    x, y = next(iter(batches))
    assert x.is_cuda and tuple(x.shape) == (2, 3, 64, 64) and tuple(y.shape) == (2, 64, 64)
    w = oracle.formula_state(oracle.state_spec('deeplab', 'resnet', 9, 3), salt=6)
    losses = []
    for feed in ((x, y), (torch.from_numpy(x.cpu().numpy()), torch.from_numpy(y.cpu().numpy()))):
        meta = Meta(arch='deeplab', backbone='resnet', weighted=True).update(prof)
        assert meta.weights == prof['weights'] and meta.px_mean == prof['px_mean'] and meta.px_std == prof['px_std']
        model = Model(meta, dev).build()
        model.net.load_state_dict(w)
        model.train(*feed)
        losses.append(torch.stack((model.crit.ce, model.crit.dsc, model.crit.fl)).cpu())
    assert torch.isfinite(losses[0]).all() and torch.equal(losses[0], losses[1])
