"""pylc_amd.regions on the GPU (-m gpu): labels, sizes, the sieve and the region table against the numpy statement of tests/_regions.py,
bit for bit (integers only: no tolerance anywhere), the entry points' argument errors, and segment_photo's min_region."""
import functools

import numpy as np
import pytest
import torch

from tests import _regions as R
from tests.test_cpu_regions import hand_cases

pytestmark = pytest.mark.gpu

# one below, at and one above the 128 x 16 tile's edges, single-row and single-column images, several tiles each way
SIZES = [(1, 1), (1, 5), (7, 1), (2, 2), (16, 128), (17, 129), (33, 257), (100, 333), (256, 384), (300, 400)]


@functools.lru_cache(maxsize=None)
def masks_for(h, w):
    """every pattern that fits the size (computed once, shared by the tests, never written to)"""
    return R.patterns(h, w)


@functools.lru_cache(maxsize=None)
def blob_map(h, w, seed=5, noise_frac=0.02):
    return R.blobs(h, w, 9, seed, radius=5, noise_frac=noise_frac)


def gpu_labels(m, dev, connectivity=4, ignore_index=None):
    from pylc_amd import regions
    return regions.label_regions(torch.from_numpy(m).to(dev), connectivity, ignore_index)


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('hw', SIZES)
def test_labels_match_statement(dev, hw, connectivity):
    for name, m in masks_for(*hw).items():
        got = gpu_labels(m, dev, connectivity)
        assert got.dtype == torch.int32 and tuple(got.shape) == hw
        assert np.array_equal(got.cpu().numpy(), R.label_ref(m, connectivity)), (name, hw, connectivity)


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('hw', [(1, 5), (17, 129), (100, 333), (300, 400)])
def test_labels_with_ignore(dev, hw, connectivity):
    rng = np.random.default_rng(11)
    for name, m in masks_for(*hw).items():
        scattered = np.where(rng.random(hw) < 0.1, 255, m).astype(np.uint8)
        for mm, ign in ((scattered, 255), (m, 0)):                   # 255 scattered at 10 %, and 0 inside the class range
            got = gpu_labels(mm, dev, connectivity, ign).cpu().numpy()
            assert np.array_equal(got == -1, mm == ign), (name, ign)
            assert np.array_equal(got, R.label_ref(mm, connectivity, ign)), (name, hw, connectivity, ign)


def test_labels_alignment_and_determinism(dev):
    from pylc_amd import regions
    h, w = 100, 333
    m = blob_map(h, w)
    want = R.label_ref(m, 8)
    flat = torch.from_numpy(m).to(dev).reshape(-1)
    first = regions.label_regions(flat.reshape(h, w), 8)
    assert np.array_equal(first.cpu().numpy(), want)
    assert torch.equal(regions.label_regions(flat.reshape(h, w), 8), first)           # two runs: the same bytes
    for off in (1, 2, 3):
        buf = torch.zeros(h * w + 8, device=dev, dtype=torch.uint8)
        view = buf[off:off + h * w]
        view.copy_(flat)
        assert view.data_ptr() % 4 == off
        assert torch.equal(regions.label_regions(view.reshape(h, w), 8), first), off
        out = regions.sieve(view.reshape(h, w), 16)
        assert torch.equal(out, regions.sieve(flat.reshape(h, w), 16)), off


@pytest.mark.parametrize('hw', [(1, 5), (17, 129), (300, 400)])
def test_region_sizes(dev, hw):
    from pylc_amd import regions
    rng = np.random.default_rng(12)
    for name, m in masks_for(*hw).items():
        for ign in (None, 255):
            mm = m if ign is None else np.where(rng.random(hw) < 0.1, 255, m).astype(np.uint8)
            lab = gpu_labels(mm, dev, 4, ign)
            sizes = regions.region_sizes(lab)
            assert sizes.dtype == torch.int32 and tuple(sizes.shape) == (hw[0] * hw[1],)
            got, lab_np = sizes.cpu().numpy(), lab.cpu().numpy().reshape(-1)
            assert np.array_equal(got, np.bincount(lab_np[lab_np >= 0], minlength=lab_np.size)), name
            roots = np.flatnonzero(lab_np == np.arange(lab_np.size))
            assert (got[np.setdiff1d(np.arange(lab_np.size), roots)] == 0).all()
            assert got.sum() == (mm.size if ign is None else (mm != ign).sum())


@functools.lru_cache(maxsize=None)
def crossing_mask(name):
    if name == 'serpentine':
        return R.serpentine(511, 513)          # one region threading every tile, one background region per gap
    if name == 'spiral':
        return R.spiral(512, 512)
    return R.blobs(1024, 1536, 9, 5, radius=6, noise_frac=0.01)       # (label_ref takes about half a second here)


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('name', ['serpentine', 'spiral', 'blobs'])
def test_mask_that_crosses_every_tile(dev, name, connectivity):
    from pylc_amd import regions
    m_np = crossing_mask(name)
    h, w = m_np.shape
    m = torch.from_numpy(m_np).to(dev)
    lab = regions.label_regions(m, connectivity)
    flat, mflat = lab.reshape(-1).long(), m.reshape(-1)
    assert bool((flat <= torch.arange(h * w, device=dev)).all()) and bool((flat >= 0).all())
    assert torch.equal(flat[flat], flat)                             # a label is a root
    assert torch.equal(mflat[flat], mflat)                           # of the pixel's own value
    assert bool((lab[:, 1:] == lab[:, :-1])[m[:, 1:] == m[:, :-1]].all())
    assert bool((lab[1:] == lab[:-1])[m[1:] == m[:-1]].all())
    n_roots = int((flat == torch.arange(h * w, device=dev)).sum())
    want = R.label_ref(m_np, connectivity)
    assert n_roots == len(np.unique(want))
    assert np.array_equal(lab.cpu().numpy(), want)
    if name == 'serpentine':
        assert n_roots == 256 and bool((lab[m == 1] == 0).all())
    sizes = regions.region_sizes(lab)
    assert np.array_equal(sizes.cpu().numpy(), R.sizes_ref(want))


def gpu_sieve(m, dev, **kw):
    from pylc_amd import regions
    out, n = regions.sieve(torch.from_numpy(m).to(dev), return_changed=True, **kw)
    assert out.dtype == torch.uint8 and n.dtype == torch.int64 and n.is_cuda
    return out.cpu().numpy(), int(n)


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('hw', [(100, 333), (300, 400)])
def test_sieve_matches_statement(dev, hw, connectivity):
    m = blob_map(*hw)
    rng = np.random.default_rng(13)
    holes = np.where(rng.random(hw) < 0.1, 255, m).astype(np.uint8)
    for min_size in (2, 16, 64, hw[0] * hw[1] + 1):
        for fill in ('neighbour', 0, 255):
            for mm, ign in ((m, None), (holes, 255), (m, 0)):
                want, n_want = R.sieve_ref(mm, min_size, connectivity, fill, ign)
                got, n = gpu_sieve(mm, dev, min_size=min_size, connectivity=connectivity, fill=fill, ignore_index=ign)
                assert np.array_equal(got, want), (min_size, fill, ign)
                assert n == n_want == int((got != mm).sum())
                if ign is not None:
                    assert np.array_equal(got[mm == ign], mm[mm == ign])
    got, n = gpu_sieve(holes, dev, min_size=16, connectivity=connectivity, fill='ignore', ignore_index=255)
    want, n_want = R.sieve_ref(holes, 16, connectivity, 255, 255)
    assert np.array_equal(got, want) and n == n_want


@pytest.mark.parametrize('name', sorted(hand_cases()))
def test_sieve_hand_cases(dev, name):
    m, kw, want, n_want = hand_cases()[name]
    got, n = gpu_sieve(m, dev, **kw)
    assert np.array_equal(got, want) and n == n_want


def test_sieve_off_and_iterations(dev):
    from pylc_amd import regions
    m = torch.from_numpy(blob_map(100, 333)).to(dev)
    for k in (1, 0):
        out, n = regions.sieve(m, k, return_changed=True)
        assert torch.equal(out, m) and out.data_ptr() != m.data_ptr() and int(n) == 0
    once, n1 = regions.sieve(m, 12, 8, return_changed=True)
    twice, n2 = regions.sieve(once, 12, 8, return_changed=True)
    both, n12 = regions.sieve(m, 12, 8, iterations=2, return_changed=True)
    assert torch.equal(both, twice) and int(n12) == int(n1) + int(n2) and int(n1) > 0
    want = R.sieve_ref(R.sieve_ref(blob_map(100, 333), 12, 8)[0], 12, 8)[0]
    assert np.array_equal(both.cpu().numpy(), want)
    assert torch.equal(regions.sieve(m, 12, 8), once)                # without the counter: the same mask


@pytest.mark.parametrize('ign', [None, 255])
def test_region_table(dev, ign):
    from pylc_amd import regions
    m = blob_map(100, 333)
    if ign is not None:
        m = np.where(np.random.default_rng(14).random(m.shape) < 0.1, 255, m).astype(np.uint8)
    for connectivity in (4, 8):
        t = regions.region_table(torch.from_numpy(m).to(dev), connectivity, ign)
        want = R.region_table_ref(m, connectivity, ign)
        for k in ('root', 'cls', 'size'):
            assert isinstance(t[k], np.ndarray) and np.array_equal(t[k], want[k]), k
        pc = t['per_class']
        counts = np.bincount(m.reshape(-1), minlength=256)
        if ign is not None:
            counts[ign] = 0
        assert np.array_equal(pc['value'], np.flatnonzero(counts))
        assert np.array_equal(pc['pixels'], counts[pc['value']])
        assert np.array_equal(pc['n_regions'], np.bincount(want['cls'], minlength=256)[pc['value']])
        assert np.array_equal(pc['largest'], [want['size'][want['cls'] == v].max() for v in pc['value']])


def test_entry_point_argument_errors(dev):
    """every refused call returns PYLC_ERR_ARG, and a correct call right after it still gives the right labels: nothing was launched or
    left behind"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, ptr, stream
    L.init()
    m_np = blob_map(100, 333)
    h, w = m_np.shape
    want = torch.from_numpy(R.label_ref(m_np)).to(dev)
    m = torch.from_numpy(m_np).to(dev)
    lab = torch.empty((h, w), device=dev, dtype=torch.int32)
    sizes = torch.empty((h * w,), device=dev, dtype=torch.int32)
    best = torch.empty((h * w,), device=dev, dtype=torch.int64)
    out = torch.empty_like(m)
    n = torch.zeros((), device=dev, dtype=torch.int64)
    st = stream()

    def good():
        lab.fill_(-7)
        assert lib.pylc_label_regions(ptr(m), h, w, 4, -1, ptr(lab), st) == 0
        assert torch.equal(lab, want)

    good()
    assert lib.pylc_region_sizes(ptr(lab), h * w, ptr(sizes), st) == 0
    bad_label = [(None, h, w, 4, -1, ptr(lab)), (ptr(m), h, w, 4, -1, None), (ptr(m), h, w, 6, -1, ptr(lab)), (ptr(m), h, w, 0, -1, ptr(lab)),
                 (ptr(m), 0, w, 4, -1, ptr(lab)), (ptr(m), h, -1, 4, -1, ptr(lab)), (ptr(m), 1 << 16, 1 << 15, 4, -1, ptr(lab)),
                 (ptr(m), h, w, 4, 256, ptr(lab)), (ptr(m), h, w, 4, -2, ptr(lab))]
    for args in bad_label:
        assert lib.pylc_label_regions(*args, st) == 1, args
        good()
    for args in ((None, h * w, ptr(sizes)), (ptr(lab), h * w, None), (ptr(lab), 0, ptr(sizes)), (ptr(lab), 1 << 31, ptr(sizes))):
        assert lib.pylc_region_sizes(*args, st) == 1, args
        good()
    ok = dict(mask=ptr(m), labels=ptr(lab), sizes=ptr(sizes), H=h, W=w, min_size=8, ignore_index=-1, fill=-1, best=ptr(best), out=ptr(out),
              n=ptr(n))
    bad_sieve = [dict(mask=None), dict(labels=None), dict(sizes=None), dict(out=None), dict(best=None), dict(H=0), dict(H=1 << 16, W=1 << 15),
                 dict(min_size=0), dict(fill=256), dict(fill=-2), dict(ignore_index=256), dict(ignore_index=-2), dict(out=ptr(m))]
    for change in bad_sieve:
        a = dict(ok, **change)
        assert lib.pylc_sieve_regions(a['mask'], a['labels'], a['sizes'], a['H'], a['W'], a['min_size'], a['ignore_index'], a['fill'], a['best'],
                                      a['out'], a['n'], st) == 1, change
        good()
    assert int(n) == 0
    a = ok
    assert lib.pylc_sieve_regions(a['mask'], a['labels'], a['sizes'], a['H'], a['W'], a['min_size'], a['ignore_index'], a['fill'], a['best'],
                                  a['out'], a['n'], st) == 0
    w_out, w_n = R.sieve_ref(m_np, 8)
    assert np.array_equal(out.cpu().numpy(), w_out) and int(n) == w_n
    assert lib.pylc_sieve_regions(a['mask'], a['labels'], a['sizes'], a['H'], a['W'], a['min_size'], a['ignore_index'], a['fill'], a['best'],
                                  a['out'], a['n'], st) == 0
    assert int(n) == 2 * w_n                                         # n_changed is ADDED into


# ---- segment_photo ------------------------------------------------------------------------------------------------------------------------
def _check_sieved(photo, regions, plain, res, palette, min_region):
    want = regions.sieve(plain.mask, min_region)
    assert torch.equal(res.mask, want)
    assert int(res.n_sieved) == int((res.mask != plain.mask).sum()) > 0
    if palette is not None:
        pal = torch.from_numpy(palette).to(want.device)
        assert torch.equal(res.rgb, photo._colourize(want, pal, want.shape[0], want.shape[1]))
    else:
        assert res.rgb is None


def test_segment_photo_deeplab_min_region(dev):
    from pylc_amd import photo, regions
    from tests.test_photo_gpu import PALETTE, _deeplab, photo_np
    image = photo_np(21, 300, 460)
    model, _, _ = _deeplab(dev)
    for blend in ('reference', 'mean'):
        kw = dict(tile=64, palette=PALETTE, blend=blend, return_confidence=blend == 'mean')
        plain = photo.segment_photo(model, image, **kw)
        assert plain.n_sieved is None
        off = photo.segment_photo(model, image, min_region=0, **kw)
        assert torch.equal(off.mask, plain.mask) and torch.equal(off.rgb, plain.rgb) and off.n_sieved is None
        res = photo.segment_photo(model, image, min_region=24, **kw)
        _check_sieved(photo, regions, plain, res, PALETTE, 24)
        if blend == 'mean':
            assert torch.equal(res.confidence, plain.confidence)
        # the small regions unlabelled: 255 exactly where the mask changed
        ign = photo.segment_photo(model, image, min_region=24, region_fill='ignore', ignore_index=255, **kw)
        changed = ign.mask != plain.mask
        assert bool((ign.mask[changed] == 255).all()) and bool(((ign.mask == 255) == changed).all())
        assert int(ign.n_sieved) == int(changed.sum()) > 0
        assert bool((ign.rgb[changed] == 0).all()) and torch.equal(ign.rgb[~changed], plain.rgb[~changed])
        c8 = photo.segment_photo(model, image, min_region=24, region_connectivity=8, **kw)
        assert torch.equal(c8.mask, regions.sieve(plain.mask, 24, 8))
    with pytest.raises(ValueError):
        photo.segment_photo(model, image, tile=64, min_region=24, region_connectivity=5)
    with pytest.raises(ValueError):
        photo.segment_photo(model, image, tile=64, min_region=24, region_fill='ignore')


def test_segment_photo_unet_min_region(dev):
    import oracle
    from oracle import step as ostep
    from pylc_amd import photo, regions, runtime
    from pylc_amd.model import Model, Meta
    from tests.test_photo_gpu import PALETTE, photo_np
    from tests.test_unet_inference_gpu import reflect_windows
    runtime.dropout_enabled = False
    image = photo_np(23, 600, 700)
    # formula weights with BatchNorm statistics calibrated on a few windows of the scaled photograph: a mask of several classes
    scaled = photo.resize_area(torch.from_numpy(image).to(dev), 300, 350).cpu().float()
    win = reflect_windows(scaled, 256, 68, 68)[::8]
    cfg = ostep.StepConfig('unet', 'resnet', 9, 3, dropout=False)
    wts = ostep.calibrate_bn(oracle.formula_state(oracle.state_spec('unet', 'resnet', 9, 3), salt=5), cfg, win.clone())
    model = Model(Meta(arch='unet', ch=3, n_classes=9), dev).build()
    model.net.load_state_dict(wts)
    for palette in (None, PALETTE):
        kw = dict(tile=256, scale=0.5, palette=palette, return_confidence=True)
        plain = photo.segment_photo(model, image, **kw)
        off = photo.segment_photo(model, image, min_region=0, **kw)
        assert torch.equal(off.mask, plain.mask) and off.n_sieved is None
        assert (off.rgb is None and plain.rgb is None) or torch.equal(off.rgb, plain.rgb)
        res = photo.segment_photo(model, image, min_region=24, **kw)
        _check_sieved(photo, regions, plain, res, palette, 24)
        assert torch.equal(res.confidence, plain.confidence)
