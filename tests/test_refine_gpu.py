"""The guided-filter refinement on the GPU (-m gpu, csrc/refine.hip): the luma bit for bit, the coefficients and q of
every case of tests/_refine.py (sizes x radii x class counts x eps) within 4 x the float32 model's measured distance from the fp64
statement, the mask where the statement decides, the exact relations between the outputs, the synthetic border scene, and the `refine`
keyword of predict_image / predict_overlap_tile / segment_photo against its composition by hand."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import _refine as R

pytestmark = pytest.mark.gpu

SPEC = {'radius': 8, 'eps': 1e-3}


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ---- 1: luma ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', R.SIZES)
def test_luma_bit_for_bit(dev, h, w):
    from pylc_amd import refine
    rng = np.random.default_rng(h * 1000 + w)
    for ch in (1, 3):
        img = rng.integers(0, 256, (ch, h, w)).astype(np.uint8)
        want = R.luma_np(img)
        assert np.array_equal(refine.luma(_dev(img, dev)).cpu().numpy(), want)
        for off in (1, 2, 3):                                           # the image at byte offsets 1..3 of an allocation
            buf = torch.zeros(img.size + 8, dtype=torch.uint8, device=dev)
            view = buf[off:off + img.size].view(ch, h, w)
            view.copy_(_dev(img, dev))
            assert view.data_ptr() % 4 == (buf.data_ptr() + off) % 4
            assert np.array_equal(refine.luma(view).cpu().numpy(), want)
    for v in (0, 255):
        assert (refine.luma(torch.full((3, h, w), v, dtype=torch.uint8, device=dev)) == v).all()


# ---- 2: the kernel cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.CLASSES)
@pytest.mark.parametrize('r', R.RADII)
@pytest.mark.parametrize('h,w', R.SIZES)
def test_kernels_against_the_statement(dev, h, w, r, c):
    from pylc_amd import refine
    tol_q, tol_a, tol_b = R.tolerances()
    g, p, refs = R.case_reference(h, w, c, r)
    gd, pd = _dev(g, dev), _dev(p, dev)
    for eps in R.EPSS:
        ref = refs[eps]
        a, b = refine.guided_coeffs(pd, gd, r, eps)
        mask, q, conf = refine.guided_refine(pd, gd, r, eps, return_probs=True, return_confidence=True, clip=False)
        assert a.dtype == b.dtype == q.dtype == conf.dtype == torch.float32 and mask.dtype == torch.uint8
        assert tuple(a.shape) == tuple(b.shape) == tuple(q.shape) == (c, h, w) and tuple(mask.shape) == tuple(conf.shape) == (h, w)
        an, bn, qn, mn, cn = (t.cpu().numpy() for t in (a, b, q, mask, conf))
        scale = ref['var'] + eps
        err_a = float((np.abs(an - ref['a']) * scale).max())
        err_b = float((np.abs(bn - ref['b']) * scale).max())
        err_q = float(np.abs(qn - ref['q']).max())
        print('%dx%d r=%d C=%d eps=%g: scaled |a - ref| %.3g (tol %.3g)  scaled |b - ref| %.3g (tol %.3g)  |q - ref| %.3g (tol %.3g)'
              % (h, w, r, c, eps, err_a, tol_a, err_b, tol_b, err_q, tol_q))
        assert err_a <= tol_a and err_b <= tol_b and err_q <= tol_q
        flat = R.guide_sums(g, r)[3] == 0
        assert (an[:, flat] == 0).all()                                 # a flat window: a = 0 exactly
        # the mask where the statement decides
        decided = R.top2_margin(ref['q']) > 8 * tol_q
        assert (~decided).mean() <= 2e-3
        assert np.array_equal(mn[decided], ref['mask'][decided])
        # exact relations between the kernel's own outputs
        assert np.array_equal(mn, qn.argmax(0).astype(np.uint8))        # the first maximum of its own q
        assert np.array_equal(cn, np.clip(qn.max(0), np.float32(0), np.float32(1)))
        assert float(np.abs(qn.astype(np.float64).sum(0) - 1).max()) <= c * tol_q
        m2, c2 = refine.guided_refine(pd, gd, r, eps, return_confidence=True)
        assert torch.equal(m2, mask) and torch.equal(c2, conf)           # the same bytes without the volume
        assert torch.equal(refine.guided_refine(pd, gd, r, eps), mask)
        m3, q3 = refine.guided_refine(pd, gd, r, eps, return_probs=True)
        assert torch.equal(m3, mask) and torch.equal(q3, q.clamp(0, 1))      # clip = 1 is the clamp of clip = 0
        a2, b2 = refine.guided_coeffs(pd, gd, r, eps)
        m4, q4, c4 = refine.guided_refine(pd, gd, r, eps, return_probs=True, return_confidence=True, clip=False)
        assert all(torch.equal(x, y) for x, y in ((a2, a), (b2, b), (m4, mask), (q4, q), (c4, conf)))      # two runs, the same bytes


@pytest.mark.parametrize('r', [2, 16, 64])
@pytest.mark.parametrize('h,w,c', [(5, 7, 3), (65, 63, 9), (96, 131, 2), (257, 2, 16), (150, 140, 16)])
def test_strided_view_and_constant_guide(dev, h, w, c, r):
    from pylc_amd import refine
    g, p = R.case_guide(h, w), R.case_probs(h, w, c)
    gd, pd = _dev(g, dev), _dev(p, dev)
    # a window of a larger volume: row pitch > W, plane stride > H * pitch, read in place
    big = torch.full((c, h + 3, w + 5), float('nan'), device=dev)
    view = big[:, 1:1 + h, 2:2 + w]
    view.copy_(pd)
    assert view.stride() == ((h + 3) * (w + 5), w + 5, 1) and not view.is_contiguous()
    assert refine._strided(view)[0] is view
    for x, y in zip(refine.guided_coeffs(view, gd, r, 1e-4), refine.guided_coeffs(pd, gd, r, 1e-4)):
        assert torch.equal(x, y)
    for x, y in zip(refine.guided_refine(view, gd, r, 1e-4, True, True), refine.guided_refine(pd, gd, r, 1e-4, True, True)):
        assert torch.equal(x, y)
    # any other layout goes through one contiguous copy
    perm = pd.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert torch.equal(refine.guided_refine(perm, gd, r, 1e-4), refine.guided_refine(pd, gd, r, 1e-4))
    # a constant guide: every window is flat, a = 0 exactly and eps is not looked at
    flat = torch.full((h, w), 117, dtype=torch.uint8, device=dev)
    lo, hi = refine.guided_coeffs(pd, flat, r, 1e-6), refine.guided_coeffs(pd, flat, r, 1.0)
    assert torch.equal(lo[0], hi[0]) and torch.equal(lo[1], hi[1]) and int((lo[0] != 0).sum()) == 0
    for x, y in zip(refine.guided_refine(pd, flat, r, 1e-6, True, True, clip=False), refine.guided_refine(pd, flat, r, 1.0, True, True, clip=False)):
        assert torch.equal(x, y)
    want = R.statement(p, np.full((h, w), 117, np.uint8), r, 1e-3)['q']      # the box mean of the box mean
    got = refine.guided_refine(pd, flat, r, 1e-3, return_probs=True, clip=False)[1].cpu().numpy()
    assert np.abs(got - want).max() <= R.tolerances()[0]


def test_image_guide_is_its_luma(dev):
    from pylc_amd import refine
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (3, 65, 63)).astype(np.uint8)
    p = _dev(R.case_probs(65, 63, 9), dev)
    for image in (img, img[:1]):
        want = refine.guided_refine(p, _dev(R.luma_np(image), dev), 4, 1e-3, True, True)
        got = refine.guided_refine(p, _dev(image, dev), 4, 1e-3, True, True)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        ca, cb = refine.guided_coeffs(p, _dev(image, dev), 4, 1e-3)
        wa, wb = refine.guided_coeffs(p, refine.luma(_dev(image, dev)), 4, 1e-3)
        assert torch.equal(ca, wa) and torch.equal(cb, wb)


def test_non_finite_values_stay_in_their_windows(dev):
    """p is used as given: a NaN reaches the windows that contain it (q within 2r of it) and nothing else"""
    from pylc_amd import refine
    h, w, r = 40, 70, 3
    g, p = R.case_guide(h, w), R.case_probs(h, w, 3)
    clean = refine.guided_refine(_dev(p, dev), _dev(g, dev), r, 1e-3, return_probs=True, clip=False)[1].cpu().numpy()
    p[1, 20, 30] = np.nan
    q = refine.guided_refine(_dev(p, dev), _dev(g, dev), r, 1e-3, return_probs=True, clip=False)[1].cpu().numpy()
    bad = np.isnan(q[1])
    yy, xx = np.mgrid[0:h, 0:w]
    assert np.array_equal(bad, (np.abs(yy - 20) <= 2 * r) & (np.abs(xx - 30) <= 2 * r))
    assert not np.isnan(q[[0, 2]]).any() and np.array_equal(q[1][~bad], clean[1][~bad]) and np.array_equal(q[0], clean[0])


def test_border_scene_on_the_gpu(dev):
    from pylc_amd import boundary, refine
    g, truth, p = R.border_scene()
    td = _dev(truth, dev)
    unrefined = _dev(p.argmax(0).astype(np.uint8), dev)
    before = int((unrefined != td).sum())
    mask = refine.guided_refine(_dev(p, dev), _dev(g, dev), 8, 1e-3)
    after = int((mask != td).sum())
    radius = boundary.default_radius(*truth.shape)
    biou = [boundary.boundary_scores(boundary.boundary_counts(td, m, 3, radius), 3)['boundary_iou'] for m in (unrefined, mask)]
    print('border scene on the GPU: %d -> %d wrong pixels, boundary IoU (radius %d) %.4f -> %.4f' % (before, after, radius, biou[0], biou[1]))
    assert 4 * after <= before and biou[1] > biou[0]


# ---- 3: the pipeline ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def deeplab(dev):
    """test_blend_gpu's sizes: ResNet-101, 9 classes, tile 64, a [3,100,150] uint8 image (not fitted)"""
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    from tests.test_photo_gpu import photo_np
    runtime.dropout_enabled = False
    torch.manual_seed(0)
    model = Model(Meta(), dev).build()
    model.net.eval()
    photo_img = photo_np(31, 100, 150)
    img = torch.from_numpy(np.ascontiguousarray(photo_img.transpose(2, 0, 1))).to(dev)
    return {'model': model, 'img': img, 'photo': photo_img}


def _by_hand(dev, model, img, spec, **kw):
    """guided_refine of the call's own return_probs volume, with the luma of the image"""
    from pylc_amd import inference, refine
    probs = inference.predict_image(model, img, 64, blend='mean', return_probs=True, **kw)[1]
    guide = refine.luma(img.to(dev))
    return refine.guided_refine(probs, guide, spec['radius'], spec['eps'], True, True, spec.get('clip', True))


@pytest.mark.parametrize('kw', [{}, {'flip': True}, {'scales': (0.75, 1.0)}, {'temperature': 2.0, 'flip': True}], ids=str)
def test_predict_image_refine_is_the_composition(dev, deeplab, kw):
    from pylc_amd import inference
    model, img = deeplab['model'], deeplab['img']
    want = _by_hand(dev, model, img, SPEC, **kw)
    got = inference.predict_image(model, img, 64, blend='mean', return_probs=True, return_confidence=True, refine=SPEC, **kw)
    assert len(got) == 3 and all(torch.equal(x, y) for x, y in zip(got, want))
    assert torch.equal(inference.predict_image(model, img, 64, blend='mean', refine=SPEC, **kw), want[0])
    m, c = inference.predict_image(model, img, 64, blend='mean', return_confidence=True, refine=SPEC, **kw)
    assert torch.equal(m, want[0]) and torch.equal(c, want[2])
    assert not model.net.training
    plain = inference.predict_image(model, img, 64, blend='mean', return_probs=True, **kw)[1]
    assert not torch.equal(plain, want[1])                                # the filter is really there
    assert float(want[1].min()) >= 0 and float(want[1].max()) <= 1        # clip defaults to True
    raw = inference.predict_image(model, img, 64, blend='mean', return_probs=True, refine=dict(SPEC, clip=False), **kw)[1]
    assert torch.equal(raw.clamp(0, 1), want[1]) and float((raw.sum(0) - 1).abs().max()) < 1e-4
    # independent of the batch size, and a host image gives the same bytes
    b3 = inference.predict_image(model, img.cpu(), 64, batch=3, blend='mean', return_probs=True, return_confidence=True, refine=SPEC, **kw)
    assert all(torch.equal(x, y) for x, y in zip(b3, want))


def test_refine_none_is_the_current_output(dev, deeplab):
    from pylc_amd import inference
    model, img = deeplab['model'], deeplab['img']
    for kw in ({}, {'flip': True, 'return_confidence': True}):
        want = inference.predict_image(model, img, 64, blend='mean', return_probs=True, **kw)
        got = inference.predict_image(model, img, 64, blend='mean', return_probs=True, refine=None, **kw)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    fitted = img[:, :64, :128].contiguous()
    assert torch.equal(inference.predict_image(model, fitted, 64, refine=None), inference.predict_image(model, fitted, 64))


def test_refine_one_rank_group_equals_no_group(dev, deeplab):
    import torch.distributed as dist
    from pylc_amd import inference
    model, img = deeplab['model'], deeplab['img']
    want = inference.predict_image(model, img, 64, blend='mean', flip=True, return_probs=True, return_confidence=True, refine=SPEC)
    assert not dist.is_initialized()
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group('gloo', init_method='file://' + os.path.join(tmp, 'store'), rank=0, world_size=1)
        try:
            got = inference.predict_image(model, img, 64, group=dist.group.WORLD, blend='mean', flip=True, return_probs=True,
                                          return_confidence=True, refine=SPEC)
        finally:
            dist.destroy_process_group()
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))


def test_pipeline_value_errors(dev, deeplab):
    from pylc_amd import inference, photo
    model, img = deeplab['model'], deeplab['img']
    with pytest.raises(ValueError, match='uint8'):
        inference.predict_image(model, img.float(), 64, blend='mean', refine=SPEC)
    with pytest.raises(ValueError, match="refine needs blend='mean'"):
        inference.predict_image(model, img[:, :64, :128].contiguous(), 64, refine=SPEC)
    with pytest.raises(ValueError, match="refine needs blend='mean' on a DeepLab"):
        photo.segment_photo(model, deeplab['photo'], tile=64, refine=SPEC)
    for bad, word in (({'radius': 0, 'eps': 1e-3}, 'radius'), ({'radius': 8, 'eps': 2.0}, '2.0'), ({'radius': 8}, 'eps'),
                      ({'radius': 8, 'eps': 1e-3, 'clip': 'yes'}, 'yes'), ([8, 1e-3], 'dict')):
        with pytest.raises(ValueError, match=word):
            inference.predict_image(model, img, 64, blend='mean', refine=bad)
        with pytest.raises(ValueError, match=word):
            photo.segment_photo(model, deeplab['photo'], tile=64, blend='mean', refine=bad)
    assert not model.net.training


def test_segment_photo_refine_then_colour_then_sieve(dev, deeplab):
    from pylc_amd import inference, photo, regions
    from tests.test_photo_gpu import PALETTE
    model, img, image = deeplab['model'], deeplab['img'], deeplab['photo']
    res = photo.segment_photo(model, image, tile=64, blend='mean', palette=PALETTE, return_probs=True, return_confidence=True, min_region=20,
                              refine=SPEC)
    m, p, c = inference.predict_image(model, img, 64, blend='mean', return_probs=True, return_confidence=True, refine=SPEC)
    assert torch.equal(res.probs, p) and torch.equal(res.confidence, c)
    encoded = photo.encode_mask(inference.colourize(m, PALETTE), PALETTE)
    want, n = regions.sieve(encoded, 20, return_changed=True)
    assert torch.equal(res.mask, want) and int(res.n_sieved) == int(n)            # the sieve saw the refined mask
    assert torch.equal(res.rgb, inference.colourize(want, PALETTE))
    plain = photo.segment_photo(model, image, tile=64, blend='mean', palette=PALETTE, min_region=20)
    assert not torch.equal(plain.mask, res.mask)
    # without the sieve and the palette: predict_image's outputs as they are
    res = photo.segment_photo(model, image, tile=64, blend='mean', refine=SPEC)
    assert torch.equal(res.mask, m) and res.probs is None and res.confidence is None and res.n_sieved is None
    # a scale step: the guide is the scaled-size image the blend ran on
    from tests.test_photo_gpu import photo_np
    big = photo_np(32, 220, 320)
    res = photo.segment_photo(model, big, tile=64, scale=0.5, blend='mean', return_probs=True, refine=SPEC)
    scaled = photo.resize_area(photo._upload_photo(big, dev), 110, 160)
    m2, p2 = inference.predict_image(model, scaled, 64, blend='mean', return_probs=True, refine=SPEC)
    assert tuple(res.mask.shape) == (110, 160) and torch.equal(res.mask, m2) and torch.equal(res.probs, p2)


def test_unet_overlap_tile_refine(dev):
    from pylc_amd import inference, refine, runtime
    from pylc_amd.model import Model, Meta
    from tests.test_photo_gpu import photo_np
    runtime.dropout_enabled = False
    torch.manual_seed(0)
    model = Model(Meta(arch='unet', ch=3, n_classes=9), dev).build()
    chw = torch.from_numpy(np.ascontiguousarray(photo_np(23, 150, 200).transpose(2, 0, 1))).to(dev)
    probs = inference.predict_overlap_tile(model, chw, 256, return_probs=True)[1]
    want = refine.guided_refine(probs, refine.luma(chw), SPEC['radius'], SPEC['eps'], True, True)
    got = inference.predict_overlap_tile(model, chw, 256, return_probs=True, return_confidence=True, refine=SPEC)
    assert len(got) == 3 and all(torch.equal(x, y) for x, y in zip(got, want))
    assert torch.equal(inference.predict_image(model, chw, 256, refine=SPEC), want[0])         # `blend` is ignored on a U-Net
    flipped = inference.predict_overlap_tile(model, chw, 256, flip=True, return_probs=True)[1]
    got = inference.predict_overlap_tile(model, chw, 256, flip=True, refine=SPEC)
    assert torch.equal(got, refine.guided_refine(flipped, refine.luma(chw), SPEC['radius'], SPEC['eps']))


def test_one_channel_xception_is_its_own_guide(dev):
    from pylc_amd import inference, refine
    from pylc_amd.model import Model, Meta
    from tests.test_photo_gpu import photo_np
    torch.manual_seed(5)
    model = Model(Meta(backbone='xception', ch=1, n_classes=11), dev).build()
    model.net.eval()
    img = torch.from_numpy(photo_np(7, 100, 150, c=1)[None].copy()).to(dev)
    probs = inference.predict_image(model, img, 64, blend='mean', return_probs=True)[1]
    assert tuple(probs.shape) == (11, 100, 150)
    want = refine.guided_refine(probs, img[0], 4, 1e-2, True, True)
    got = inference.predict_image(model, img, 64, blend='mean', return_probs=True, return_confidence=True, refine={'radius': 4, 'eps': 1e-2})
    assert all(torch.equal(x, y) for x, y in zip(got, want))
