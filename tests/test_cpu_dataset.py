"""Training tile sets, host side (no GPU): pylc_amd.dataset's tile grid against torch.unfold, the dataset profile from exact integer sums
against the reference's own get_profile (tests/golden/dataset_profile.json, written by tests/golden/make_dataset_profile.py), the
oversampling-rate search against the reference's Augmentor.optimize, and the TileSet container's bookkeeping.  The restatements here
(unfold_tiles, tile_sums_np, profile_case) are what tests/test_dataset_gpu.py compares the kernel with."""
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

CASES = {'rgb': dict(n=40, ch=3, tile=32, n_classes=9, seed=71), 'gray': dict(n=5, ch=1, tile=48, n_classes=9, seed=72)}
PRIOR = np.array([0.34, 0.25, 0.16, 0.10, 0.06, 0.04, 0.03, 0.015, 0.005])       # a skewed class prior


# ---- restatements ------------------------------------------------------------------------------------------------------------------
def unfold_tiles(x, tile, stride):
    """Extractor.__split (utils/extract.py:296-308) on a planar array: [C,H,W] -> [n,C,t,t], [H,W] -> [n,t,t]; numpy in, numpy out"""
    t = torch.as_tensor(np.ascontiguousarray(x))
    if t.dim() == 2:
        u = t.unfold(0, tile, stride).unfold(1, tile, stride)
        return u.reshape(u.shape[0] * u.shape[1], tile, tile).contiguous().numpy()
    u = t.permute(1, 2, 0).unfold(0, tile, stride).unfold(1, tile, stride)          # [H,W,C], as the reference holds it
    return torch.reshape(u, (u.shape[0] * u.shape[1], t.shape[0], tile, tile)).contiguous().numpy()


def tile_sums_np(img_tiles, mask_tiles=None, n_classes=None):
    """per tile: int64 [n,2,C] (sum x, sum x^2) and the class histogram int64 [n, n_classes + 1], values >= n_classes in the last bin"""
    x = img_tiles.astype(np.int64)
    sums = np.stack([x.sum((2, 3)), (x * x).sum((2, 3))], 1)
    hist = None
    if mask_tiles is not None:
        m = np.minimum(mask_tiles.reshape(mask_tiles.shape[0], -1).astype(np.int64), n_classes)
        hist = np.stack([np.bincount(r, minlength=n_classes + 1) for r in m])
    return sums, hist


def profile_case(name):
    """the seeded tiles of fixture case `name`: uint8 [n,C,t,t] with a brightness of their own per tile (the first one all 255), and
    class-index masks [n,t,t] of 4 x 4 cells drawn from a per-tile perturbation of the skewed prior"""
    c = CASES[name]
    rs = np.random.RandomState(c['seed'])
    n, ch, t, k = c['n'], c['ch'], c['tile'], c['n_classes']
    level = rs.randint(40, 216, (n, ch, 1, 1))
    img = np.clip(level + rs.randint(-40, 41, (n, ch, t, t)), 0, 255).astype(np.uint8)
    img[0] = 255
    mask = np.empty((n, t, t), np.uint8)
    for i in range(n):
        p = rs.dirichlet(PRIOR * 6.0)
        cells = rs.choice(k, size=(t // 4, t // 4), p=p)
        mask[i] = np.kron(cells, np.ones((4, 4), np.int64)).astype(np.uint8)
    return img, mask


def fixture():
    with open(os.path.join(HERE, 'dataset_profile.json')) as f:
        return json.load(f)


def check_profile(prof, want):
    """the bounds of the profile against the reference's outputs: counts exact, double arithmetic on the same integers to 1e-12, and the
    pixel statistics -- which the reference sums in float32 -- within 4 x the gap the fixture's generator measured between the reference's
    float32 value and the float64 value of the exact integer sums (one sample of that summation noise, hence a small multiple)"""
    assert prof['px_dist'] == want['px_dist']
    assert prof['dset_px_dist'] == np.sum(np.asarray(want['px_dist'], np.int64), 0).tolist()
    assert prof['dset_px_count'] == want['dset_px_count'] and prof['n_samples'] == len(want['px_dist'])
    for key in ('probs', 'weights'):
        np.testing.assert_allclose(prof[key], want[key], rtol=1e-12, atol=0)
    for key in ('m2', 'jsd'):
        assert abs(prof[key] - want[key]) <= 1e-12 * abs(want[key]), key
    for key in ('px_mean', 'px_std'):
        got, ref = np.asarray(prof[key]), np.asarray(want[key])
        assert got.shape == ref.shape
        gap = want['fp32_gap_' + key[3:]]
        assert np.all(np.abs(got - ref) <= 4 * gap * np.abs(ref)), (key, got, ref, gap)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def test_tile_grid_counts_match_unfold():
    from pylc_amd import dataset
    seen = 0
    for h, w in ((101, 150), (96, 160), (32, 32), (33, 64), (64, 31), (24, 100), (100, 23)):
        for tile, stride in ((32, 32), (32, 16), (24, 8), (32, 48), (64, 64)):
            if h < tile or w < tile:
                with pytest.raises(ValueError):
                    dataset.tile_grid_counts(h, w, tile, stride)
                continue
            u = torch.zeros(h, w, dtype=torch.uint8).unfold(0, tile, stride).unfold(1, tile, stride)
            assert dataset.tile_grid_counts(h, w, tile, stride) == (u.shape[0], u.shape[1]), (h, w, tile, stride)
            seen += 1
    assert seen >= 15
    assert dataset.tile_grid_counts(32, 32, 32, 7) == (1, 1)              # a side equal to the tile
    from pylc_amd.inference import tile_grid
    assert dataset.tile_grid_counts(4096, 3072, 512, 512) == tile_grid(4096, 3072, 512, 512) == (8, 6)      # the recorded fit: 48 tiles


def test_unfold_restatement_layout():
    img = np.arange(3 * 5 * 7, dtype=np.uint8).reshape(3, 5, 7)
    tiles = unfold_tiles(img, 2, 2)
    assert tiles.shape == (6, 3, 2, 2)
    assert np.array_equal(tiles[4], img[:, 2:4, 2:4])                      # row-major: tile 4 is grid (1, 1)
    assert np.array_equal(unfold_tiles(img[0], 2, 3)[3], img[0, 3:5, 3:5])


# ---- the profile ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rgb', 'gray'])
def test_profile_matches_reference(name):
    from pylc_amd import dataset
    c = CASES[name]
    img, mask = profile_case(name)
    sums, hist = tile_sums_np(img, mask, c['n_classes'])
    assert not hist[:, -1].any()
    if name == 'rgb':
        assert sums[0].tolist() == [[32 * 32 * 255] * 3, [32 * 32 * 255 * 255] * 3]
    prof = dataset.profile_from_sums(sums, hist[:, :-1], c['tile'], c['n_classes'])
    check_profile(prof, fixture()[name])
    assert prof['tile_px_count'] == c['tile'] ** 2 and len(prof['px_mean']) == c['ch']
    # px_std is the mean of the per-tile values, not the dataset's std (the tiles differ in brightness, so the two are far apart)
    assert prof['px_std'][0] < 0.8 * img[:, 0].astype(np.float64).std()
    from pylc_amd.model import Meta
    meta = Meta(ch=c['ch'], weighted=True).update(prof)
    assert meta.px_mean == prof['px_mean'] and meta.px_std == prof['px_std'] and meta.weights == prof['weights']
    assert max(meta.weights) == 1.0 and len(meta.weights) == 9 and not hasattr(meta, 'px_dist')


def test_profile_refuses_inconsistent_counts():
    from pylc_amd import dataset
    sums = np.zeros((2, 2, 3), np.int64)
    hist = np.zeros((2, 9), np.int64)
    hist[:, 0] = 16
    dataset.profile_from_sums(sums, hist, 4, 9)
    hist[1, 0] = 15
    with pytest.raises(ValueError, match='does not match'):
        dataset.profile_from_sums(sums, hist, 4, 9)


def test_oversample_rates_match_reference():
    from pylc_amd import dataset
    want = fixture()['rgb']
    img, mask = profile_case('rgb')
    sums, hist = tile_sums_np(img, mask, 9)
    prof = dataset.profile_from_sums(sums, hist[:, :-1], 32, 9)
    got = dataset.oversample_rates(prof)
    opt = want['optimize']
    assert got['rates'].tolist() == opt['rates'] and sum(opt['rates']) > 0
    assert got['threshold'] == opt['threshold'] and got['rate_coef'] == opt['rate_coef']
    assert got['aug_n_samples'] == sum(opt['rates']) and got['n_samples'] == 40 + sum(opt['rates'])
    for key in ('jsd', 'm2'):
        assert abs(got[key] - opt[key]) <= 1e-12 * abs(opt[key]), key
    assert got['jsd'] < prof['jsd']                                        # the added tiles move the set towards balance


def test_oversample_rates_without_a_candidate():
    from pylc_amd import dataset
    img, mask = profile_case('gray')
    sums, hist = tile_sums_np(img[:1], mask[:1], 9)
    prof = dataset.profile_from_sums(sums, hist[:, :-1], 48, 9)
    with pytest.raises(ValueError, match='No augmentation optimization found'):
        dataset.oversample_rates(prof)                                     # one tile: int(0.36 * 1) = 0 extra samples allowed


# ---- the container ------------------------------------------------------------------------------------------------------------------
def _host_set(n=10, ch=3, tile=8, k=4, seed=5):
    from pylc_amd import dataset
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (n, ch, tile, tile)).astype(np.uint8)
    img[:, 0, 0, 0] = np.arange(n)                                         # every tile carries its number ...
    mask = rs.randint(0, k, (n, tile, tile)).astype(np.uint8)
    mask[:, 0, 0] = np.arange(n) % k
    sums, hist = tile_sums_np(img, mask, k)
    ts = dataset.TileSet(ch, k, tile, keep='host').from_arrays(img[:6], mask[:6], sums[:6], hist[:6])
    ts.from_arrays(img[6:], mask[6:], sums[6:], hist[6:, :k])              # with or without the overflow bin
    return ts, img, mask, sums, hist


def test_coshuffle_keeps_rows_together():
    ts, img, mask, sums, hist = _host_set()
    assert len(ts) == 10 and np.array_equal(ts.img.numpy(), img) and np.array_equal(ts.sums, sums)
    ts.coshuffle(3)
    perm = np.random.RandomState(3).permutation(10)
    assert not np.array_equal(perm, np.arange(10))
    assert np.array_equal(ts.img.numpy(), img[perm]) and np.array_equal(ts.mask.numpy(), mask[perm])
    assert np.array_equal(ts.sums, sums[perm]) and np.array_equal(ts.hist, hist[perm, :4])
    s2, h2 = tile_sums_np(ts.img.numpy(), ts.mask.numpy(), 4)
    assert np.array_equal(s2, ts.sums) and np.array_equal(h2[:, :4], ts.hist)
    assert ts.profile()['n_samples'] == 10


def test_partition_and_batches():
    ts, img, mask, _, _ = _host_set()
    train, valid = ts.partition(0, 0.75), ts.partition(0.75, 1.0)
    assert (train.start, train.end, valid.start, valid.end) == (0, 8, 8, 10)          # ceil, as db/database.py:89-90
    assert len(train) == 8 and len(valid) == 2
    b = train.batches(3)
    assert len(b) == 2 and [x.shape[0] for x, _ in b] == [3, 3]
    again = [(x.copy(), y.copy()) for x, y in b]                           # re-iterable
    assert np.array_equal(np.concatenate([x for x, _ in again]), img[:6]) and np.array_equal(np.concatenate([y for _, y in again]), mask[:6])
    full = train.batches(3, drop_last=False)
    assert len(full) == 3 and [x.shape[0] for x, _ in full] == [3, 3, 2]
    assert np.array_equal(np.concatenate([x for x, _ in full]), img[:8])
    assert np.array_equal(np.concatenate([y for _, y in valid.batches(4, drop_last=False)]), mask[8:])
    assert len(valid.batches(4)) == 0 and list(valid.batches(4)) == []
    assert valid.profile()['n_samples'] == 2 and train.profile()['dset_px_count'] == 8 * 64
    for x, y in train.batches(2):
        assert x.dtype == np.uint8 and x.shape == (2, 3, 8, 8) and y.dtype == np.uint8 and y.shape == (2, 8, 8)
    with pytest.raises(ValueError):
        train.coshuffle(1)                                                 # a view
    ts.coshuffle(1)
    assert np.array_equal(valid.img.numpy(), img[np.random.RandomState(1).permutation(10)][8:])      # views follow their set


def test_tile_set_refuses_what_does_not_fit():
    from pylc_amd import dataset
    ts, img, mask, sums, hist = _host_set()
    with pytest.raises(ValueError):
        ts.from_arrays(img[:, :, :4, :4], mask[:, :4, :4], sums, hist)     # another tile size
    with pytest.raises(ValueError):
        ts.from_arrays(img, None, sums, None)                              # masks for all or for none
    bad = hist.copy()
    bad[2, -1] = 1
    with pytest.raises(ValueError, match='class index'):
        ts.from_arrays(img, mask, sums, bad)
    with pytest.raises(ValueError):
        dataset.TileSet(3, 17, 8)
    with pytest.raises(ValueError):
        dataset.TileSet(3, 9, 8, keep='disk')


def test_extract_photo_argument_errors():
    from pylc_amd import dataset
    image = np.zeros((64, 96, 3), np.uint8)
    rgb = np.zeros((64, 96, 3), np.uint8)
    pal = np.zeros((9, 3), np.uint8)
    with pytest.raises(ValueError, match='fit'):
        dataset.extract_photo(image, rgb, pal, tile=32, stride=16, fit=True)
    for k in (0, 17):
        with pytest.raises(ValueError, match='n_classes'):
            dataset.extract_photo(image, rgb, pal, tile=32, n_classes=k)
    with pytest.raises(ValueError, match='n_classes'):
        dataset.extract_photo(image, rgb, np.zeros((17, 3), np.uint8), tile=32)
    with pytest.raises(ValueError, match='palette'):
        dataset.extract_photo(image, rgb, None, tile=32)
    with pytest.raises(ValueError, match='smaller than the tile'):
        dataset.extract_photo(image, tile=80)
    with pytest.raises(ValueError, match='upscale'):
        dataset.extract_photo(image, tile=80, scale=0.5)                   # short side below the tile: get_image raises the scale
    with pytest.raises(ValueError, match='do not match'):
        dataset.extract_photo(np.zeros((128, 192, 3), np.uint8), np.zeros((128, 190, 3), np.uint8), pal, tile=32, scale=0.5)


def test_dataset_entry_points_declared():
    import re
    from pylc_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'pylc_hip.h')).read(), flags=re.S)
    for name in ('pylc_extract_tiles', 'pylc_tile_stats'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in L.SIGNATURES and hasattr(L.lib, name)
    # argument checks happen on the host before any launch: no GPU needed, never a fault
    assert L.lib.pylc_extract_tiles(16, 3, 20, 40, None, 0, 32, 32, 0, 1, 0, 16, None, 16, None, None) != 0
    assert b'exceeds the image' in L.lib.pylc_last_error()
    assert L.lib.pylc_extract_tiles(16, 3, 64, 64, None, 0, 32, 0, 0, 1, 0, 16, None, 16, None, None) != 0
    assert L.lib.pylc_extract_tiles(16, 3, 64, 64, None, 0, 32, 32, 3, 2, 0, 16, None, 16, None, None) != 0
    assert b'outside the 2x2 grid' in L.lib.pylc_last_error()
    assert L.lib.pylc_extract_tiles(16, 3, 64, 64, 16, 17, 32, 32, 0, 1, 0, 16, 16, 16, 16, None) != 0
    assert L.lib.pylc_tile_stats(16, 2, 3, 32, 16, 0, 0, 16, 16, None) != 0
    assert L.lib.pylc_tile_stats(16, 2, 3, 512, None, 0, 256, 16, None, None) != 0          # 256 rows x 512: past 65536 pixels per block
