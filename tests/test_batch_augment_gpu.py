"""The per-step augmenter on the GPU (-m gpu): pylc_batch_augment against the integer statement of tests/_batch_augment.py, BIT FOR BIT and
with no pixel left out -- image, mask and weights; every output lies inside a larger buffer pre-filled with a sentinel, at byte offsets
0..3, so a byte that is not written or a byte written outside shows.  Then the Python layers: augment_batch against the C ABI,
TileSet.batches(augment=) against its hand composition, epochs that differ, seeds that repeat, host-kept against device-kept sets, and
one DeepLab / ResNet step on an augmented batch whose samples are partly (and wholly) out of frame."""
import numpy as np
import pytest
import torch

from tests import _batch_augment as S

pytestmark = pytest.mark.gpu

SOURCES = [(8, 8), (33, 47), (64, 64), (130, 96)]
OUTPUTS = [(4, 4), (16, 16), (37, 53), (64, 64), (96, 128)]
N_SRC = 3
SENTINEL, W_SENTINEL, GUARD = 0xA5, -1234.5, 64


def matrices(src_hw, out_hw):
    """[(name, int64 [6])]: the exact cases, scales, rotations, maps that leave most or all of the output outside, fractions of 31/32,
    and a window 2^20 pixels to the left (where |a02| stays below 2^44: an output narrower than the source)"""
    from pylc_amd.dataset import affine_q24
    (hs, ws), (oh, ow) = src_hw, out_hw
    cx, cy = (ws - 1) / 2.0, (hs - 1) / 2.0
    out = [('identity', affine_q24(src_hw, out_hw)),
           ('mirror x', affine_q24(src_hw, out_hw, flip_x=True)),
           ('mirror y', affine_q24(src_hw, out_hw, flip_y=True)),
           ('turn 90', affine_q24(src_hw, out_hw, rotate_deg=90)),
           ('turn 180', affine_q24(src_hw, out_hw, rotate_deg=180)),
           ('turn 270', affine_q24(src_hw, out_hw, rotate_deg=270)),
           ('shift (3,-2)', affine_q24(src_hw, out_hw, centre_xy=(cx + 3, cy - 2))),
           ('scale 0.5', affine_q24(src_hw, out_hw, scale=0.5)),
           ('scale 2', affine_q24(src_hw, out_hw, scale=2.0)),
           ('scale 1.37', affine_q24(src_hw, out_hw, scale=1.37, flip_x=True)),
           ('rotate 17', affine_q24(src_hw, out_hw, rotate_deg=17.0)),
           ('mostly outside', affine_q24(src_hw, out_hw, scale=0.2, rotate_deg=-40.0, centre_xy=(cx + 0.8 * ws, cy + 0.3 * hs))),
           ('all outside', affine_q24(src_hw, out_hw, scale=1.3, rotate_deg=5.0, centre_xy=(cx + 4 * ws + 2 * ow, cy - 3 * hs - 2 * oh)))]
    frac = affine_q24(src_hw, out_hw)
    frac[[2, 5]] += 31 << 19
    out.append(('fractions 31/32', frac))
    if ow < ws:
        out.append(('window at -2^20', affine_q24(src_hw, out_hw, centre_xy=(cx - 2.0 ** 20, cy + (0 if oh >= hs else -2.0 ** 20 + 1)))))
    return out


def _luts(mode, m, c, seed):
    if mode == 'none':
        return None
    if mode == 'identity':
        return np.broadcast_to(np.arange(256, dtype=np.uint8), (m, c, 256)).copy()
    return np.random.RandomState(seed).randint(0, 256, (m, c, 256)).astype(np.uint8)


def _guarded(dev, nbytes, offset, dtype=torch.uint8):
    """a device buffer of `nbytes` elements at element offset GUARD + offset inside a sentinel-filled one"""
    buf = torch.full((2 * GUARD + nbytes + 4,), W_SENTINEL if dtype == torch.float32 else SENTINEL, device=dev, dtype=dtype)
    lo = GUARD + offset
    return buf, lo, buf.data_ptr() + lo * buf.element_size()


def _take(buf, lo, shape, what):
    """the result out of a guarded buffer; everything around it must still hold the sentinel"""
    host = buf.cpu().numpy()
    n = int(np.prod(shape))
    sentinel = np.float32(W_SENTINEL) if host.dtype == np.float32 else SENTINEL
    assert (host[:lo] == sentinel).all() and (host[lo + n:] == sentinel).all(), '%s: a write outside the output' % what
    return host[lo:lo + n].reshape(shape)


def run_abi(dev, img, mask, weights, src, mats, luts, out_hw, border, fill, mask_fill, band_rows=0, offset=0, device_params=False):
    """pylc_batch_augment on numpy inputs -> numpy outputs, through guarded buffers at byte (float: element) offset `offset`"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    n, c, hs, ws = img.shape
    (oh, ow), m = out_hw, len(src)
    d_img = torch.from_numpy(img).to(dev)
    d_mask = torch.from_numpy(mask).to(dev) if mask is not None else None
    d_w = torch.from_numpy(weights).to(dev) if weights is not None else None
    d_lut = torch.from_numpy(luts).to(dev) if luts is not None else None
    src = np.ascontiguousarray(src, dtype=np.int32)
    mats = np.ascontiguousarray(mats, dtype=np.int64)
    keep = [torch.from_numpy(src).to(dev), torch.from_numpy(mats).to(dev)]
    p_src, p_mats = (keep[0].data_ptr(), keep[1].data_ptr()) if device_params else (src.ctypes.data, mats.ctypes.data)
    fill = np.ascontiguousarray(fill, dtype=np.uint8)
    o_buf, o_lo, o_ptr = _guarded(dev, m * c * oh * ow, offset)
    m_buf, m_lo, m_ptr = _guarded(dev, m * oh * ow, offset) if mask is not None else (None, 0, None)
    w_buf, w_lo, w_ptr = _guarded(dev, m * oh * ow, offset, torch.float32) if weights is not None else (None, 0, None)
    check(lib.pylc_batch_augment(ptr(d_img), ptr(d_mask), ptr(d_w), n, c, hs, ws, p_src, p_mats, ptr(d_lut), m, oh, ow, S.BORDERS[border],
                                 fill.ctypes.data, mask_fill, band_rows, o_ptr, m_ptr, w_ptr, stream()))
    torch.cuda.synchronize()
    return (_take(o_buf, o_lo, (m, c, oh, ow), 'image'), _take(m_buf, m_lo, (m, oh, ow), 'mask') if mask is not None else None,
            _take(w_buf, w_lo, (m, oh, ow), 'weights') if weights is not None else None)


def _same(got, want, what):
    for g, w, name in zip(got, want, ('image', 'mask', 'weights')):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape
            bad = g.view(np.uint8) != w.view(np.uint8)
            assert not bad.any(), '%s: %d %s bytes differ' % (what, int(bad.sum()), name)


CASES = [(si, oi, c) for si in range(len(SOURCES)) for oi in range(len(OUTPUTS)) for c in (1, 3)]


@pytest.mark.parametrize('si,oi,c', CASES)
def test_kernel_matches_the_statement(dev, si, oi, c):
    src_hw, out_hw = SOURCES[si], OUTPUTS[oi]
    idx = CASES.index((si, oi, c))
    img, mask, weights = S.sources(N_SRC, c, src_hw[0], src_hw[1], 100 + idx)
    named = matrices(src_hw, out_hw)
    mats = np.stack([a for _, a in named])
    m = len(named)
    src = (np.arange(m) * 2 + idx) % N_SRC                                  # every source, repeated
    fill = [17, 130, 250][:c]
    for bi, border in enumerate(('constant', 'reflect')):
        v = idx * 2 + bi                                                   # walks through every option below, each with each other
        lut_mode = ('none', 'identity', 'random')[v % 3]
        with_mask, with_w = (v // 3) % 2 == 0, (v // 6) % 2 == 0
        band_rows, offset, device_params = (0, 1, 7)[(v // 2) % 3], (idx + bi) % 4, (v // 4) % 2 == 1
        luts = _luts(lut_mode, m, c, v)
        mk, wt = (mask if with_mask else None), (weights if with_w else None)
        want = S.batch_augment_np(img, mk, wt, src, mats, luts, out_hw, border, fill, 255)
        got = run_abi(dev, img, mk, wt, src, mats, luts, out_hw, border, fill, 255, band_rows, offset, device_params)
        _same(got, want, '%s -> %s C %d %s lut %s band %d offset %d' % (src_hw, out_hw, c, border, lut_mode, band_rows, offset))
        if border == 'constant':                                           # the cases do what their names say
            k = [name for name, _ in named].index('all outside')
            flat = np.array([fill[ch] if luts is None else luts[k, ch, fill[ch]] for ch in range(c)], np.uint8)
            assert (want[0][k] == flat[:, None, None]).all()
            if with_mask:
                assert (want[1][k] == 255).all()
            if with_w:
                assert (want[2][k] == 0).all()
            k = [name for name, _ in named].index('mostly outside')
            if with_mask and min(out_hw) >= 16:
                assert 0.5 < (want[1][k] == 255).mean() < 1.0


@pytest.mark.parametrize('m', [1, 5, 70])
@pytest.mark.parametrize('border', ['constant', 'reflect'])
def test_sample_counts_launches_and_offsets(dev, m, border):
    """m = 1, 5 and 70 (host parameters: three launches of 32, 32 and 6 samples; device parameters: one), three band_rows values and the
    output offsets 0..3 all give the same bytes: the statement's"""
    src_hw, out_hw, c = (33, 47), (37, 53), 3
    img, mask, weights = S.sources(N_SRC, c, 33, 47, 7 + m)
    named = matrices(src_hw, out_hw)
    mats = np.stack([named[(3 * k + 7) % len(named)][1] for k in range(m)])
    src = np.array([(k * k) % N_SRC for k in range(m)])                     # repeats
    luts = _luts('random', m, c, m)
    fill = [9, 99, 199]
    want = S.batch_augment_np(img, mask, weights, src, mats, luts, out_hw, border, fill, 254)
    for band_rows, offset, device_params in ((0, 0, False), (1, 1, True), (5, 2, False), (37, 3, True), (1000, 0, False)):
        got = run_abi(dev, img, mask, weights, src, mats, luts, out_hw, border, fill, 254, band_rows, offset, device_params)
        _same(got, want, 'm %d %s band %d offset %d' % (m, border, band_rows, offset))


def test_device_parameters_out_of_range_leave_the_sample_unwritten(dev):
    """a DEVICE src_index or matrix the entry point cannot see: that sample stays as it was, its neighbours are made"""
    img, mask, weights = S.sources(2, 1, 8, 8, 3)
    from pylc_amd.dataset import affine_q24
    mats = np.stack([affine_q24((8, 8), (8, 8))] * 3)
    mats[1, 0] = (1 << 32) + 1
    src = np.array([0, 1, 2])
    got = run_abi(dev, img, mask, weights, src, mats, None, (8, 8), 'reflect', [0], 0, device_params=True)
    assert np.array_equal(got[0][0], img[0]) and (got[0][1:] == SENTINEL).all()
    assert np.array_equal(got[1][0], mask[0]) and np.array_equal(got[2][0], weights[0]) and (got[2][1:] == np.float32(W_SENTINEL)).all()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
def test_augment_batch_is_the_entry_point(dev):
    from pylc_amd import dataset
    src_hw, out_hw, c = (64, 64), (37, 53), 3
    img, mask, weights = S.sources(N_SRC, c, 64, 64, 21)
    m = 6
    mats, luts = dataset.batch_augment_params(np.random.RandomState(4), m, src_hw, out_hw, rotate=25.0, vflip=0.5, brightness=(-20, 20),
                                              contrast=(0.7, 1.3), gamma=(0.8, 1.25))
    src = [2, 0, 1, 1, 2, 0]
    d = [torch.from_numpy(a).to(dev) for a in (img, mask, weights)]
    for border, fill, mf in (('constant', [3, 4, 5], 255), ('reflect', None, None)):
        want = run_abi(dev, img, mask, weights, src, mats, luts, out_hw, border, fill or [0, 0, 0], mf or 0)
        got = dataset.augment_batch(d[0], d[1], src, mats, luts, out_hw, border=border, fill=fill, mask_fill=mf, weights=d[2], band_rows=3)
        _same([t.cpu().numpy() for t in got], want, 'augment_batch ' + border)
        _same(want, S.batch_augment_np(img, mask, weights, src, mats, luts, out_hw, border, fill, mf), 'statement ' + border)
        # device tensors for the parameters, no mask, no weights, the source's own size
        got = dataset.augment_batch(d[0], None, torch.tensor(src, dtype=torch.int32, device=dev), torch.from_numpy(mats).to(dev), None, None,
                                    border=border, fill=fill)
        assert got[1] is None and got[2] is None
        _same([got[0].cpu().numpy()], S.batch_augment_np(img, None, None, src, mats, None, src_hw, border, fill)[:1], 'device parameters')
    # random crops out of ONE resident photograph
    photo, pmask, _ = S.sources(1, 3, 130, 96, 5)
    mats, _ = dataset.batch_augment_params(np.random.RandomState(1), 4, (130, 96), (32, 32), scale=(1.0, 1.0))
    got = dataset.augment_batch(torch.from_numpy(photo).to(dev), torch.from_numpy(pmask).to(dev), [0] * 4, mats, out_hw=(32, 32), mask_fill=255)
    _same([got[0].cpu().numpy(), got[1].cpu().numpy()], S.batch_augment_np(photo, pmask, None, [0] * 4, mats, None, (32, 32), 'constant',
                                                                            [0, 0, 0], 255)[:2], 'photo crops')
    assert not (got[1] == 255).any().item()                                # scale 1: the crop stays inside (up to the rounded centre)


def _tile_set(dev, keep, ignore_index, t=64, n=7, c=3, k=5):
    from pylc_amd import dataset
    img, mask, _ = S.sources(n, c, t, t, 77, n_classes=k)
    if ignore_index is not None:
        mask[:, :5] = ignore_index
    ts = dataset.TileSet(c, k, t, keep=keep, ignore_index=ignore_index).from_arrays(img, mask)
    return ts, img, mask


AUG = dict(scale=(0.5, 2.0), rotate=10.0, flip=0.5, brightness=(-15, 15), contrast=(0.8, 1.2), gamma=(0.9, 1.1))


@pytest.mark.parametrize('ignore_index', [255, None])
def test_tileset_batches_against_the_hand_composition(dev, ignore_index):
    from pylc_amd import dataset
    ts, img, mask = _tile_set(dev, 'device', ignore_index)
    t, bs = ts.tile, 3
    it = ts.batches(bs, augment=AUG, seed=11)
    assert len(it) == 2
    first, second = [[(x.cpu().numpy(), y.cpu().numpy()) for x, y in it] for _ in range(2)]
    rs = np.random.RandomState(11)
    fill = np.rint(img.astype(np.float64).mean(axis=(0, 2, 3)))
    for epoch in (first, second):                                          # ONE stream of draws runs through the epochs
        for b, (x, y) in enumerate(epoch):
            assert x.shape == (bs, 3, t, t) and y.shape == (bs, t, t)
            mats, luts = dataset.batch_augment_params(rs, bs, (t, t), (t, t), **AUG)
            src = np.arange(b * bs, b * bs + bs)
            if ignore_index is None:
                want = S.batch_augment_np(img, mask, None, src, mats, luts, (t, t), 'reflect')
            else:
                want = S.batch_augment_np(img, mask, None, src, mats, luts, (t, t), 'constant', fill, ignore_index)
            _same([x, y], want[:2], 'batches(augment=) batch %d' % b)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(first, second))           # two iterations differ
    again = [(x.cpu().numpy(), y.cpu().numpy()) for x, y in ts.batches(bs, augment=AUG, seed=11)]
    _same([again[1][0], again[1][1]], first[1], 'the same seed')                          # the same seed repeats
    other = [(x.cpu().numpy(), y.cpu().numpy()) for x, y in ts.batches(bs, augment=AUG, seed=12)]
    assert not np.array_equal(other[0][0], first[0][0])
    if ignore_index is not None:
        assert any((y == 255).any() for _, y in first)
    # a host-kept set, a partition of it and another output size: the same bytes as the device-kept one
    hs, _, _ = _tile_set(dev, 'host', ignore_index)
    for a, b in ((ts, hs), (ts.partition(0.3, 1.0), hs.partition(0.3, 1.0))):
        ga = [(x.cpu().numpy(), y.cpu().numpy()) for x, y in a.batches(2, drop_last=False, augment=AUG, seed=5, out=(48, 40))]
        gb = [(x.cpu().numpy(), y.cpu().numpy()) for x, y in b.batches(2, drop_last=False, augment=AUG, seed=5, out=(48, 40))]
        assert len(ga) == len(gb) and ga[0][0].shape[-2:] == (48, 40)
        for p, q in zip(ga, gb):
            _same(list(p), list(q), 'host-kept against device-kept')
    # augment=None: the stored tiles, as before
    x, y = next(iter(ts.batches(bs)))
    assert np.array_equal(x.cpu().numpy(), img[:bs]) and np.array_equal(y.cpu().numpy(), mask[:bs])


def _deeplab(dev, c, salt):
    import oracle
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    runtime.dropout_enabled = False
    model = Model(Meta(arch='deeplab', backbone='resnet', ch=3, n_classes=c, ignore_index=255), dev)
    model.build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec('deeplab', 'resnet', c, 3), salt=salt))
    return model


def test_network_step_on_an_augmented_batch(dev):
    """one DeepLab / ResNet step at 128^2 on the augmented batch (scale 0.5: part of every sample is out of frame and carries the ignore
    label) == the step on the batch made by hand; then a batch mapped wholly outside: every gradient exactly zero"""
    from pylc_amd import dataset
    c, t, bs = 5, 128, 2
    ts, img, mask = _tile_set(dev, 'device', 255, t=t, n=2, k=c)
    aug = dict(scale=(0.5, 0.5), rotate=10.0)
    x, y = next(iter(ts.batches(bs, augment=aug, seed=3)))
    mats, luts = dataset.batch_augment_params(np.random.RandomState(3), bs, (t, t), (t, t), **aug)
    fill = np.rint(img.astype(np.float64).mean(axis=(0, 2, 3)))
    hx, hy, _ = S.batch_augment_np(img, mask, None, [0, 1], mats, luts, (t, t), 'constant', fill, 255)
    assert np.array_equal(x.cpu().numpy(), hx) and np.array_equal(y.cpu().numpy(), hy)
    share = (hy == 255).reshape(bs, -1).mean(1)
    assert (share > 0.3).all() and (share < 0.95).all()                    # out of frame in part, every sample
    m1, m2 = _deeplab(dev, c, 5), _deeplab(dev, c, 5)
    l1 = m1.train(x, y)
    l2 = m2.train(torch.from_numpy(hx).to(dev), torch.from_numpy(hy).to(dev))
    torch.cuda.synchronize()
    assert torch.isfinite(l1).all() and torch.equal(l1, l2)
    for p, q in zip(m1.net.parameters(), m2.net.parameters()):
        assert torch.equal(p, q) and torch.isfinite(p).all()
    # wholly outside: an all-ignored batch
    far = np.stack([dataset.affine_q24((t, t), (t, t), centre_xy=(5.0 * t, -3.0 * t))] * bs)
    x0, y0, _ = dataset.augment_batch(ts.img, ts.mask, [0, 1], far, mask_fill=255, fill=fill)
    assert (y0 == 255).all().item()
    m1.train(x0, y0)
    torch.cuda.synchronize()
    assert float(m1.arena.g.abs().max()) == 0.0 and torch.isfinite(m1.arena.p).all()
