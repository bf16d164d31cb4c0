"""The per-step augmenter, host side (no GPU): the integer statement of tests/_batch_augment.py on the cases where the answer is known
exactly (identity, mirrors, quarter turns, integer translations under both borders, np.pad's reflection), its distance from
F.grid_sample in double within the derived bound, the nearest sampling shared by mask and weights; dataset.tone_lut, affine_q24 and
batch_augment_params against plain re-computations; TileSet.batches(augment=None) as it was; and every argument the entry point and the
Python layer refuse, none of which needs a device.  tests/test_batch_augment_gpu.py compares the kernel with the statement."""
import math
import os

import numpy as np
import pytest
import torch

from tests import _batch_augment as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, MASK_FILL = [7, 80, 200], 255


def _one(img, mask, weights, mat, out_hw, border, s=1):
    o = S.batch_augment_np(img, mask, weights, [s], [mat], None, out_hw, border, FILL[:img.shape[1]], MASK_FILL)
    return o[0][0], o[1][0], o[2][0]


# ---- the statement where the answer is known ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('border', ['constant', 'reflect'])
@pytest.mark.parametrize('hw,c', [((33, 47), 3), ((8, 8), 1), ((64, 64), 3)])
def test_exact_cases(hw, c, border):
    from pylc_amd.dataset import affine_q24
    img, mask, w = S.sources(2, c, hw[0], hw[1], 5)
    turned = (hw[1], hw[0])
    cases = [(affine_q24(hw, hw), hw, lambda a: a),
             (affine_q24(hw, hw, flip_x=True), hw, lambda a: a[..., ::-1]),
             (affine_q24(hw, hw, flip_y=True), hw, lambda a: a[..., ::-1, :]),
             (affine_q24(hw, turned, rotate_deg=90), turned, lambda a: np.rot90(a, 3, axes=(-2, -1))),
             (affine_q24(hw, hw, rotate_deg=180), hw, lambda a: np.rot90(a, 2, axes=(-2, -1))),
             (affine_q24(hw, turned, rotate_deg=270), turned, lambda a: np.rot90(a, 1, axes=(-2, -1)))]
    for mat, out_hw, f in cases:
        gi, gm, gw = _one(img, mask, w, mat, out_hw, border)
        assert np.array_equal(gi, f(img[1])) and np.array_equal(gm, f(mask[1])) and np.array_equal(gw, f(w[1]))


@pytest.mark.parametrize('dx,dy', [(3, -2), (-4, 5), (0, 1)])
def test_integer_translation_under_both_borders(dx, dy):
    """the window moved by (dx, dy): the slice where it overlaps; fill / mask_fill / 0 in the uncovered rows and columns (constant),
    np.pad's mirror image (reflect)"""
    from pylc_amd.dataset import affine_q24
    hw, p = (33, 47), 6
    img, mask, w = S.sources(2, 3, hw[0], hw[1], 9)
    mat = affine_q24(hw, hw, centre_xy=((hw[1] - 1) / 2.0 + dx, (hw[0] - 1) / 2.0 + dy))
    assert list(mat) == [S.ONE, 0, dx * S.ONE, 0, S.ONE, dy * S.ONE]
    gi, gm, gw = _one(img, mask, w, mat, hw, 'constant')
    pi = np.stack([np.pad(img[1][c], p, constant_values=FILL[c]) for c in range(3)])
    pm, pw = np.pad(mask[1], p, constant_values=MASK_FILL), np.pad(w[1], p, constant_values=0)
    win = (slice(p + dy, p + dy + hw[0]), slice(p + dx, p + dx + hw[1]))
    assert np.array_equal(gi, pi[(slice(None),) + win]) and np.array_equal(gm, pm[win]) and np.array_equal(gw, pw[win])
    assert (gm == MASK_FILL).sum() == hw[0] * hw[1] - (hw[0] - abs(dy)) * (hw[1] - abs(dx))
    gi, gm, gw = _one(img, mask, w, mat, hw, 'reflect')
    pi = np.stack([np.pad(img[1][c], p, mode='reflect') for c in range(3)])
    pm, pw = np.pad(mask[1], p, mode='reflect'), np.pad(w[1], p, mode='reflect')
    assert np.array_equal(gi, pi[(slice(None),) + win]) and np.array_equal(gm, pm[win]) and np.array_equal(gw, pw[win])


def test_reflection_of_any_integer():
    for n in (2, 3, 8, 47):
        ref = np.pad(np.arange(n), (n - 1, n - 1), mode='reflect')          # one period to either side
        p = np.arange(-(n - 1), 2 * n - 1)
        assert np.array_equal(S.reflect101(p, n), ref)
        period = 2 * (n - 1)
        far = np.array([-(1 << 40) - 3, (1 << 40) + 5, -(1 << 20), 1 << 23], dtype=np.int64)
        assert np.array_equal(S.reflect101(far, n), S.reflect101(far % period, n))
    # a window 2^20 pixels to the left of a source of 9 columns (period 16 divides 2^20): the source itself
    from pylc_amd.dataset import affine_q24
    img, mask, w = S.sources(1, 1, 9, 9, 2)
    mat = affine_q24((9, 9), (5, 5), centre_xy=(4.0 - 2.0 ** 20, 4.0))
    gi, gm, gw = _one(img, mask, w, mat, (5, 5), 'reflect', s=0)
    assert np.array_equal(gi[0], img[0, 0, 2:7, 2:7]) and np.array_equal(gm, mask[0, 2:7, 2:7]) and np.array_equal(gw, w[0, 2:7, 2:7])


def test_zero_weight_taps_and_fractions():
    """fractions of 31/32 weigh the far taps 31 : 1; at the last row and column the taps beyond read the border"""
    img = np.zeros((1, 1, 2, 2), np.uint8)
    img[0, 0] = [[0, 64], [128, 255]]
    mat = np.array([S.ONE, 0, 31 << 19, 0, S.ONE, 31 << 19], np.int64)
    got = S.batch_augment_np(img, None, None, [0], [mat], None, (2, 2), 'constant', [10])[0][0, 0]
    t = lambda a, b, c, d: ((a * 1 + b * 31) * 1 + (c * 1 + d * 31) * 31 + 512) >> 10
    assert got.tolist() == [[t(0, 64, 128, 255), t(64, 10, 255, 10)], [t(128, 255, 10, 10), t(255, 10, 10, 10)]]
    got = S.batch_augment_np(img, None, None, [0], [mat], None, (2, 2), 'reflect')[0][0, 0]
    assert got.tolist() == [[t(0, 64, 128, 255), t(64, 0, 255, 128)], [t(128, 255, 0, 64), t(255, 128, 64, 0)]]


def test_against_grid_sample_in_double():
    """Where the sample lies inside the source the statement stays within 0.5 + (gx + gy) / 32 grey levels of bilinear interpolation in
    double (F.grid_sample, align_corners=True), gx and gy the image's largest horizontal and vertical neighbour differences: the final
    rounding, plus a coordinate floored to 1/32 pixel per axis on a surface that is piecewise linear with those slopes at the most."""
    import torch.nn.functional as F
    from pylc_amd.dataset import affine_q24
    hs, ws, oh, ow = 96, 130, 64, 80
    img = S.smooth_image(1, 3, hs, ws, 3)
    gx = int(np.abs(np.diff(img.astype(np.int64), axis=3)).max())
    gy = int(np.abs(np.diff(img.astype(np.int64), axis=2)).max())
    bound = 0.5 + (gx + gy) / 32.0
    worst, compared = 0.0, 0
    for scale, deg in ((0.5, 0.0), (2.0, 45.0), (1.37, 17.0), (0.8, -100.0), (1.0, 3.0)):
        mat = affine_q24((hs, ws), (oh, ow), scale, deg)
        got = S.batch_augment_np(img, None, None, [0], [mat], None, (oh, ow), 'constant', [0, 0, 0])[0][0].astype(np.float64)
        a = mat.astype(np.float64) / S.ONE
        x, y = np.meshgrid(np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64))
        sx, sy = a[0] * x + a[1] * y + a[2], a[3] * x + a[4] * y + a[5]
        grid = torch.from_numpy(np.stack([2 * sx / (ws - 1) - 1, 2 * sy / (hs - 1) - 1], -1))[None]
        want = F.grid_sample(torch.from_numpy(img.astype(np.float64)), grid, mode='bilinear', padding_mode='zeros', align_corners=True)[0].numpy()
        inside = (sx >= 0) & (sx <= ws - 1) & (sy >= 0) & (sy <= hs - 1)
        assert inside.mean() > 0.2
        err = np.abs(got - want)[:, inside].max()
        worst, compared = max(worst, err), compared + int(inside.sum())
        assert err <= bound + 1e-9, (scale, deg, err, bound)
    print('grid_sample: worst %.3f grey levels against the bound %.3f (gx %d gy %d) over %d pixels' % (worst, bound, gx, gy, compared))


def test_mask_and_weights_pick_the_same_pixel():
    from pylc_amd.dataset import affine_q24
    hs, ws = 33, 47
    img, _, _ = S.sources(2, 1, hs, ws, 1)
    ids = np.arange(hs * ws).reshape(hs, ws)
    mask = np.stack([(ids % 251).astype(np.uint8)] * 2)
    w = np.stack([ids.astype(np.float32) + 1] * 2)
    for border in ('constant', 'reflect'):
        mat = affine_q24((hs, ws), (40, 40), 0.7, 33.0)
        _, gm, gw = S.batch_augment_np(img, mask, w, [1], [mat], None, (40, 40), border, [0], 255)
        inside = gw[0] > 0
        assert (((gw[0][inside] - 1).astype(np.int64) % 251) == gm[0][inside]).all()
        assert (gm[0][~inside] == 255).all() and (inside.all() if border == 'reflect' else not inside.all())


# ---- the host functions -------------------------------------------------------------------------------------------------------------------
def test_tone_lut():
    from pylc_amd.dataset import tone_lut
    ident = tone_lut()
    assert ident.dtype == np.uint8 and ident.shape == (3, 256) and (ident == np.arange(256)).all()
    assert tone_lut(ch=1).shape == (1, 256)
    b = tone_lut(brightness=10)
    assert b[0, 0] == 10 and b[1, 100] == 110 and b[2, 250] == 255
    c = tone_lut(contrast=2.0)
    assert c[0, 100] == 72 and c[0, 64] == 0 and c[0, 192] == 255 and c[0, 128] == 128
    g = tone_lut(gamma=2.0)
    assert g[0, 128] == 64 and g[0, 255] == 255 and g[0, 0] == 0 and g[0, 16] == 1           # 64.25, 255, 0, 1.004
    h = tone_lut(gamma=0.5)
    assert h[0, 64] == int(np.rint(255 * math.sqrt(64 / 255.0))) == 128
    per = tone_lut(brightness=[0, 10, -10], contrast=[1, 1, 2], gamma=[1, 2, 1])
    assert (per[0] == np.arange(256)).all() and per[1, 118] == 64 and per[2, 100] == 62
    with pytest.raises(ValueError):
        tone_lut(brightness=[1, 2])
    with pytest.raises(ValueError):
        tone_lut(gamma=0)


def test_affine_q24_entries():
    from pylc_amd.dataset import affine_q24
    a = affine_q24((33, 47), (16, 20))
    assert a.dtype == np.int64 and list(a) == [S.ONE, 0, int((23 - 9.5) * S.ONE), 0, S.ONE, int((16 - 7.5) * S.ONE)]
    a = affine_q24((64, 64), (64, 64), scale=2.0, rotate_deg=30.0, centre_xy=(10.0, 20.0))
    cs, sn = math.cos(math.radians(30.0)) / 2, math.sin(math.radians(30.0)) / 2
    want = [cs, sn, 10.0 - (cs * 31.5 + sn * 31.5), -sn, cs, 20.0 - (-sn * 31.5 + cs * 31.5)]
    assert list(a) == [int(np.rint(v * S.ONE)) for v in want]
    a = affine_q24((64, 64), (64, 64), flip_x=True, flip_y=True)
    assert list(a) == [-S.ONE, 0, 63 * S.ONE, 0, -S.ONE, 63 * S.ONE]
    with pytest.raises(ValueError):
        affine_q24((8, 8), (8, 8), scale=0.0)


def test_batch_augment_params_draws():
    from pylc_amd import dataset
    kw = dict(scale=(0.5, 2.0), rotate=10.0, flip=0.5, vflip=0.25, brightness=(-20, 20), contrast=(0.8, 1.25), gamma=(0.7, 1.4))
    src_hw, out_hw, m = (96, 130), (64, 48), 9
    mats, luts = dataset.batch_augment_params(np.random.RandomState(42), m, src_hw, out_hw, **kw)
    assert mats.dtype == np.int64 and mats.shape == (m, 6) and luts.dtype == np.uint8 and luts.shape == (m, 3, 256)
    rs = np.random.RandomState(42)
    (hs, ws), (oh, ow) = src_hw, out_hw
    v = np.arange(256.0)
    for k in range(m):                                                     # the nine draws of a sample, in their order
        sc, deg = rs.uniform(0.5, 2.0), rs.uniform(-10.0, 10.0)
        fx, fy = rs.uniform() < 0.5, rs.uniform() < 0.25
        ux, uy = rs.uniform(-1, 1), rs.uniform(-1, 1)
        br, co, ga = rs.uniform(-20, 20), rs.uniform(0.8, 1.25), rs.uniform(0.7, 1.4)
        cx, cy = (ws - 1) / 2.0 + ux * (ws - ow / sc) / 2.0, (hs - 1) / 2.0 + uy * (hs - oh / sc) / 2.0
        cs, sn = math.cos(math.radians(deg)) / sc, math.sin(math.radians(deg)) / sc
        l00, l01, l10, l11 = cs * (-1 if fx else 1), sn * (-1 if fy else 1), -sn * (-1 if fx else 1), cs * (-1 if fy else 1)
        hx, hy = (ow - 1) / 2.0, (oh - 1) / 2.0
        want = [l00, l01, cx - (l00 * hx + l01 * hy), l10, l11, cy - (l10 * hx + l11 * hy)]
        assert list(mats[k]) == [int(np.rint(t * S.ONE)) for t in want], k
        lut = np.rint(255.0 * (np.clip(co * (v - 128.0) + 128.0 + br, 0.0, 255.0) / 255.0) ** ga).astype(np.uint8)
        assert (luts[k] == lut).all()
    assert rs.uniform() == np.random.RandomState(42).uniform(size=9 * m + 1)[-1]              # nine draws per sample, no more
    # trivial tone ranges: no tables, the same matrices (the draws are made whatever the ranges); one channel; a scalar range
    geo = {k_: v_ for k_, v_ in kw.items() if k_ in ('scale', 'rotate', 'flip', 'vflip')}
    mats2, none = dataset.batch_augment_params(np.random.RandomState(42), m, src_hw, out_hw, **geo)
    assert none is None and np.array_equal(mats2, mats)
    _, l1 = dataset.batch_augment_params(np.random.RandomState(42), 2, src_hw, out_hw, brightness=5, ch=1)
    assert l1.shape == (2, 1, 256) and (l1 == dataset.tone_lut(5, ch=1)).all()
    # the centre formula keeps a crop that fits inside the source, at every draw
    mats3, _ = dataset.batch_augment_params(np.random.RandomState(1), 200, (64, 64), (32, 32), scale=(1.0, 2.0), flip=0.0)
    x0, y0 = mats3[:, 2] / S.ONE, mats3[:, 5] / S.ONE
    x1, y1 = x0 + 31 * mats3[:, 0] / S.ONE, y0 + 31 * mats3[:, 4] / S.ONE
    assert min(x0.min(), y0.min()) >= -0.5 - 1e-6 and max(x1.max(), y1.max()) <= 63.5 + 1e-6
    for bad in (dict(scale=(0.0, 1.0)), dict(scale=(2.0, 1.0)), dict(rotate=-1.0), dict(flip=1.5), dict(gamma=(1.2, 0.8))):
        with pytest.raises(ValueError):
            dataset.batch_augment_params(np.random.RandomState(0), 1, (8, 8), (8, 8), **bad)
    with pytest.raises(TypeError):
        dataset.batch_augment_params(np.random.RandomState(0), 1, (8, 8), (8, 8), hue=0.1)


def _host_set(ignore_index=None):
    from pylc_amd import dataset
    img, mask, _ = S.sources(5, 3, 16, 16, 8, n_classes=4)
    sums = np.stack([img.astype(np.int64).sum((2, 3)), (img.astype(np.int64) ** 2).sum((2, 3))], 1)
    bins = 4 + (ignore_index is not None)
    hist = np.stack([np.bincount(m_.ravel(), minlength=bins)[:bins] for m_ in mask])
    ts = dataset.TileSet(3, 4, 16, keep='host', ignore_index=ignore_index).from_arrays(img, mask, sums=sums, hist=hist)
    return ts, img, mask


def test_batches_without_augment_are_as_before():
    from pylc_amd import dataset
    ts, img, mask = _host_set()
    it = ts.batches(2)
    assert type(it) is dataset._Batches and len(it) == 2 and len(ts.batches(2, drop_last=False)) == 3
    for _ in range(2):
        got = list(it)
        assert len(got) == 2
        for k, (x, y) in enumerate(got):
            assert isinstance(x, np.ndarray) and np.array_equal(x, img[2 * k:2 * k + 2]) and np.array_equal(y, mask[2 * k:2 * k + 2])
    assert type(ts.batches(2, True, None, 3, None)) is dataset._Batches
    # with augment: the keywords are checked when the iterable is made, nothing is launched
    aug = ts.batches(2, augment={'rotate': 5.0}, seed=1, out=8)
    assert len(aug) == 2 and aug.out_hw == (8, 8)
    with pytest.raises(TypeError):
        ts.batches(2, augment={'hue': 1})
    with pytest.raises(ValueError):
        ts.batches(2, augment={'scale': (0, 1)})


# ---- what is refused, without a device ------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_bound():
    from pylc_amd import lib as L
    hdr = open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read()
    assert 'int pylc_batch_augment(' in hdr and 'pylc_batch_augment' in L.SIGNATURES
    assert len(L.SIGNATURES['pylc_batch_augment'][1]) == 21 and L.lib.pylc_batch_augment.restype is not None
    assert L.lib.pylc_abi_version() == 15 == L.ABI_VERSION
    assert 'batch_augment.hip' in open(os.path.join(ROOT, 'pylc_amd', 'csrc', 'Makefile')).read()


def _call(**over):
    """pylc_batch_augment with valid host-side arguments (pointers that are never followed: every refusal comes before a launch)"""
    from pylc_amd.lib import lib
    from pylc_amd.dataset import affine_q24
    keep = {'src': np.array([0, 1], np.int32), 'mats': np.stack([affine_q24((8, 8), (8, 8))] * 2), 'fill': np.zeros(3, np.uint8)}
    a = dict(img=0x1000, mask=0x2000, weights=0x3000, n_src=2, C=3, Hs=8, Ws=8, src=keep['src'].ctypes.data, mats=keep['mats'].ctypes.data,
             lut=None, m=2, oh=8, ow=8, border=0, fill=keep['fill'].ctypes.data, mask_fill=255, band_rows=0, out=0x4000, out_mask=0x5000,
             out_w=0x6000)
    for k, v in over.items():
        if isinstance(v, np.ndarray):
            keep[k] = v
            v = v.ctypes.data
        a[k] = v
    rc = lib.pylc_batch_augment(a['img'], a['mask'], a['weights'], a['n_src'], a['C'], a['Hs'], a['Ws'], a['src'], a['mats'], a['lut'], a['m'],
                                a['oh'], a['ow'], a['border'], a['fill'], a['mask_fill'], a['band_rows'], a['out'], a['out_mask'], a['out_w'], None)
    return rc, lib.pylc_last_error().decode()


def _mat(k, v):
    a = np.array([[S.ONE, 0, 0, 0, S.ONE, 0]] * 2, np.int64)
    a[1, k] = v
    return a


@pytest.mark.parametrize('over,word', [
    (dict(C=2), 'Cimg'), (dict(C=4), 'Cimg'), (dict(Hs=1), 'source'), (dict(Ws=1), 'source'), (dict(oh=0), 'output'), (dict(ow=16385), 'output'),
    (dict(n_src=0), 'n_src'), (dict(m=-1), 'm='), (dict(border=2), 'border'), (dict(border=-1), 'border'),
    (dict(mask_fill=256), 'mask_fill'), (dict(mask_fill=-1), 'mask_fill'), (dict(fill=None), 'fill'),
    (dict(mask=None), 'masks'), (dict(out_mask=None), 'masks'), (dict(weights=None), 'weights'), (dict(out_w=None), 'weights'),
    (dict(out_w=0x6002), 'misaligned'),
    (dict(img=None), 'NULL'), (dict(out=None), 'NULL'), (dict(src=None), 'NULL'), (dict(mats=None), 'NULL'),
    (dict(src=np.array([0, 2], np.int32)), 'src_index[1]=2'), (dict(src=np.array([-1, 0], np.int32)), 'src_index[0]=-1'),
    (dict(mats=_mat(0, (1 << 32) + 1)), 'matrix 1'), (dict(mats=_mat(1, -(1 << 32) - 1)), 'matrix 1'), (dict(mats=_mat(3, 1 << 40)), 'matrix 1'),
    (dict(mats=_mat(4, -(1 << 62))), 'matrix 1'), (dict(mats=_mat(2, 1 << 44)), 'matrix 1'), (dict(mats=_mat(5, -(1 << 44))), 'matrix 1'),
    (dict(mats=_mat(5, -(1 << 63))), 'matrix 1'),
])
def test_entry_point_refusals(over, word):
    rc, msg = _call(**over)
    assert rc != 0 and 'batch_augment' in msg and word in msg, (rc, msg)


def test_m_zero_launches_nothing():
    assert _call(m=0)[0] == 0
    assert _call(m=0, border=1, fill=None)[0] == 0                          # reflect needs no fill


def test_python_layer_refusals():
    """augment_batch refuses what the entry point refuses, before it touches the device: host tensors get this far"""
    from pylc_amd import dataset
    img, mask, w = (torch.from_numpy(a) for a in S.sources(2, 3, 8, 8, 1))
    ok = np.array([[S.ONE, 0, 0, 0, S.ONE, 0]] * 2, np.int64)
    good = dict(img=img, mask=mask, src_index=[0, 1], mats=ok, mask_fill=255, weights=w)

    def refused(match, **over):
        with pytest.raises(ValueError, match=match):
            dataset.augment_batch(**dict(good, **over))
    refused('uint8', img=img.float())
    refused('uint8', img=img[0])
    refused('not 1 or 3', img=img[:, :2])
    refused('2x2', img=img[:, :, :1])
    refused('output', out_hw=(0, 8))
    refused('output', out_hw=(8, 16385))
    refused('border', border='wrap')
    refused('masks', mask=mask[:1])
    refused('masks', mask=mask.long())
    refused('weights', weights=w.double())
    refused('weights', weights=w[:, :4])
    refused('mask_fill', mask_fill=None)
    refused('mask_fill', mask_fill=256)
    refused('fill', fill=[1, 2])
    refused('fill', fill=[1, 2, 300])
    refused('fill', fill=[0.5, 1, 2])
    refused('src_index', src_index=[0, 2])
    refused('src_index', src_index=[-1, 0])
    refused('integers', src_index=[0.0, 1.0])
    refused('matrices', src_index=[0])
    refused('int64', mats=ok.astype(np.float64))
    refused('int64', mats=ok[:, :5])
    refused('tone tables', luts=np.zeros((2, 1, 256), np.uint8))
    refused('tone tables', luts=np.zeros((2, 3, 256), np.int32))
    for k, v in ((0, (1 << 32) + 1), (1, -(1 << 32) - 1), (3, 1 << 40), (4, -(1 << 62))):
        refused('2\\^32', mats=_mat(k, v))
    for k, v in ((2, 1 << 44), (5, -(1 << 44)), (5, -(1 << 63))):
        refused('2\\^44', mats=_mat(k, v))
    # the bounds themselves pass the matrix check
    edge = np.array([[1 << 32, -(1 << 32), (1 << 44) - 1, -(1 << 32), 1 << 32, -(1 << 44) + 1]], np.int64)
    assert dataset.check_affine_q24(edge) is not None
    # reflect needs neither fill nor mask_fill: with host tensors the call then stops at the device, not at an argument
    from pylc_amd.lib import PylcError
    if not torch.cuda.is_available():
        with pytest.raises(PylcError):
            dataset.augment_batch(img, mask, [0, 1], ok, border='reflect')
