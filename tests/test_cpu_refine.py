"""CPU suite (-m "not gpu") for the guided-filter refinement (pylc_amd.refine, csrc/refine.hip).  The reference has no
such filter, so the fp64 statement of tests/_refine.py -- what the GPU tests compare the kernels with -- is pinned here: against He et
al.'s equations written with F.avg_pool2d, against a per-pixel window loop, on hand-worked cases and on the synthetic border scene.
Then the float32 model's distance from the statement (the GPU tolerances are 4 x it), the near-tie rule of the case generator, the
bindings and every argument error that needs no device."""
import ctypes
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _refine as R


def _inputs(h, w, c, seed, flat=False):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    if flat:
        g[:h // 2, :w // 2] = 255
        g[h // 2:, w // 2:] = 0
    z = rng.normal(0, 2, (c, h, w))
    e = np.exp(z - z.max(0))
    return g, (e / e.sum(0)).astype(np.float32)


def _avg_pool_form(p, g, r, eps, flat_rule):
    """He et al., Algorithm 1, with mean = boxfilter / N written as avg_pool2d(count_include_pad=False), in float64"""
    def mean(t):
        return F.avg_pool2d(t[None], 2 * r + 1, 1, r, count_include_pad=False)[0]
    i = torch.from_numpy(g.astype(np.float64) / 255.0)[None]
    pt = torch.from_numpy(p.astype(np.float64))
    mean_i, mean_p = mean(i), mean(pt)
    var = mean(i * i) - mean_i * mean_i
    cov = mean(i * pt) - mean_i * mean_p
    a = cov / (var + eps)
    if flat_rule is not None:
        a = torch.where(torch.from_numpy(flat_rule)[None], torch.zeros_like(a), a)
    b = mean_p - a * mean_i
    return (mean(a) * i + mean(b)).numpy(), a.numpy(), b.numpy()


@pytest.mark.parametrize('h,w,c,r', [(23, 31, 3, 1), (23, 31, 3, 4), (40, 37, 9, 8), (12, 50, 2, 5)])
@pytest.mark.parametrize('eps', [1e-6, 1e-3, 1.0])
def test_statement_is_he_et_al_with_avg_pool(h, w, c, r, eps):
    """2r + 1 <= the image here: avg_pool2d wants its padding within half the window, and its windows are the clipped ones"""
    g, p = _inputs(h, w, c, 11)                                         # random bytes: no flat window
    ref = R.statement(p, g, r, eps)
    assert (R.guide_sums(g, r)[3] != 0).all()
    q, a, b = _avg_pool_form(p, g, r, eps, None)
    scale = ref['var'] + eps                                            # a itself grows as 1 / eps; its numerator is what is compared
    assert np.abs(ref['q'] - q).max() < 1e-12
    assert (np.abs(ref['a'] - a) * scale).max() < 1e-12 and (np.abs(ref['b'] - b) * scale).max() < 1e-12
    # with flat windows: the flat rule on both sides (in exact arithmetic it changes nothing: cov is 0 there)
    g, p = _inputs(h, w, c, 12, flat=True)
    ref = R.statement(p, g, r, eps)
    flat = R.guide_sums(g, r)[3] == 0
    assert flat.any() or 2 * r + 1 > min(h, w) // 2
    q, a, b = _avg_pool_form(p, g, r, eps, flat)
    assert np.abs(ref['q'] - q).max() < 1e-12
    assert (ref['a'][:, flat] == 0).all()


def test_statement_is_the_window_loop():
    """every pixel's windows written out, r below and above the image size"""
    h, w, c = 7, 9, 3
    g, p = _inputs(h, w, c, 3, flat=True)
    gf = g.astype(np.float64) / 255.0
    for r in (1, 2, 5, 12):
        for eps in (1e-6, 1e-2):
            a, b = np.zeros((c, h, w)), np.zeros((c, h, w))
            for y in range(h):
                for x in range(w):
                    ys, xs = slice(max(y - r, 0), min(y + r, h - 1) + 1), slice(max(x - r, 0), min(x + r, w - 1) + 1)
                    gw, gi = gf[ys, xs], g[ys, xs].astype(np.int64)
                    flat = gi.size * (gi * gi).sum() - gi.sum() ** 2 == 0
                    for k in range(c):
                        pw = p[k, ys, xs].astype(np.float64)
                        cov = (gw * pw).mean() - gw.mean() * pw.mean()
                        a[k, y, x] = 0.0 if flat else cov / (gw.var() + eps)
                        b[k, y, x] = pw.mean() - a[k, y, x] * gw.mean()
            q = np.zeros((c, h, w))
            for y in range(h):
                for x in range(w):
                    ys, xs = slice(max(y - r, 0), min(y + r, h - 1) + 1), slice(max(x - r, 0), min(x + r, w - 1) + 1)
                    q[:, y, x] = a[:, ys, xs].mean(axis=(1, 2)) * gf[y, x] + b[:, ys, xs].mean(axis=(1, 2))
            ref = R.statement(p, g, r, eps)
            assert np.abs(ref['q'] - q).max() < 1e-12 and (np.abs(ref['a'] - a) * (ref['var'] + eps)).max() < 1e-12
            assert np.array_equal(ref['n'], R.window_count(h, w, r)) and ref['n'].max() == min(2 * r + 1, h) * min(2 * r + 1, w)
            for prefix in (False, True):                                # the prefix-sum form of the big cases is the same statement
                assert np.abs(R.statement(p, g, r, eps, prefix=prefix)['q'] - q).max() < 1e-12


def test_hand_worked_cases():
    # 1 x 1: the window is the pixel, flat: a = 0, b = p, q = p
    p = np.array([0.25, 0.75], np.float32).reshape(2, 1, 1)
    g = np.array([[93]], np.uint8)
    for r in (1, 64):
        ref = R.statement(p, g, r, 1e-3)
        assert np.array_equal(ref['a'], np.zeros((2, 1, 1))) and np.array_equal(ref['q'], p.astype(np.float64))
        assert ref['mask'][0, 0] == 1 and ref['conf'][0, 0] == 0.75
        m = R.model32(p, g, r, 1e-3)
        assert np.array_equal(m['q'], p) and np.array_equal(m['a'], np.zeros((2, 1, 1), np.float32))
    # a constant guide: q is the box mean of the box mean of p, whatever eps
    _, p = _inputs(14, 11, 3, 5)
    g = np.full((14, 11), 200, np.uint8)
    n = R.window_count(14, 11, 2)
    want = R.box_sum(R.box_sum(p.astype(np.float64), 2) / n, 2) / n
    for eps in (1e-6, 1.0):
        ref = R.statement(p, g, 2, eps)
        assert np.array_equal(ref['a'], np.zeros_like(ref['a'])) and np.abs(ref['q'] - want).max() < 1e-15
        assert np.array_equal(R.model32(p, g, 2, eps)['q'], R.model32(p, g, 2, 1e-3)['q'])
    # a constant p_c gives that constant back; the rows of q sum to 1 where those of p do
    g, p = _inputs(14, 11, 3, 6, flat=True)
    p[0] = 0.125
    ref = R.statement(p, g, 3, 1e-4)
    assert np.abs(ref['q'][0] - 0.125).max() < 1e-14
    g, p = _inputs(20, 17, 9, 7, flat=True)
    p64 = p.astype(np.float64) / p.astype(np.float64).sum(0)           # rows that sum to 1 in fp64 (the float32 rows do to 1e-7)
    for r in (1, 6, 30):
        assert np.abs(R.statement(p64, g, r, 1e-4)['q'].sum(0) - 1).max() < 1e-12
        assert np.abs(R.statement(p, g, r, 1e-4)['q'].sum(0) - 1).max() < 1e-6
    # r at least the image size: every window is the image, so a and b are one number per class
    ref = R.statement(p, g, 20, 1e-4)
    assert (ref['n'] == 20 * 17).all()
    assert np.ptp(ref['a'], axis=(1, 2)).max() < 1e-15 and np.ptp(ref['b'], axis=(1, 2)).max() < 1e-15
    big = R.statement(p, g, 64, 1e-4)
    assert np.abs(big['q'] - ref['q']).max() < 1e-15
    # the first maximum
    assert R.statement(np.full((3, 2, 2), 1 / 3, np.float32), np.zeros((2, 2), np.uint8), 1, 1e-3)['mask'].max() == 0


def test_luma():
    for v in (0, 255):
        assert (R.luma_np(np.full((3, 2, 5), v, np.uint8)) == v).all()
    img = np.random.default_rng(2).integers(0, 256, (3, 31, 17)).astype(np.uint8)
    want = np.array([[(77 * int(img[0, y, x]) + 150 * int(img[1, y, x]) + 29 * int(img[2, y, x]) + 128) >> 8 for x in range(17)]
                     for y in range(31)])
    got = R.luma_np(img)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.abs(got - (0.299 * img[0] + 0.587 * img[1] + 0.114 * img[2])).max() < 1.2          # it is the Rec. 601 luma
    assert np.array_equal(R.luma_np(img[:1]), img[0])
    assert 77 + 150 + 29 == 256


def test_border_scene_is_repaired():
    """the issue's scene: truth borders on image edges, the prediction displaced 3 px and blurred with sigma 3"""
    g, truth, p = R.border_scene()
    assert g.shape == (96, 128) and p.shape == (3, 96, 128) and set(np.unique(truth)) == {0, 1, 2}
    before = int((p.argmax(0) != truth).sum())
    after = int((R.statement(p, g, 8, 1e-3)['mask'] != truth).sum())
    wider = int((R.statement(p, g, 16, 1e-3)['mask'] != truth).sum())
    print('border scene: %d wrong pixels, %d after r = 8, %d after r = 16' % (before, after, wider))
    assert before > 500 and 4 * after <= before and 4 * wider <= before


def test_gap32_constants():
    """The float32 model's distance from the statement, re-measured on the cases up to 65 x 63 (the recorded constants are the maxima
    over all of them: `python -c "from tests import _refine as R; print(R.measure_gap32())"`, a few minutes); the worst case of q is
    among these.  The near-tie margin of the generator covers the mask comparison's 8 x tol_q."""
    small = [s for s in R.SIZES if s[0] * s[1] <= 65 * 63]
    gq, ga, gb = R.measure_gap32(small)
    print('gap32 on %d sizes: q %.4g  a (scaled) %.4g  b (scaled) %.4g' % (len(small), gq, ga, gb))
    assert gq <= R.GAP32_Q and ga <= R.GAP32_A and gb <= R.GAP32_B
    assert gq > 0.9 * R.GAP32_Q                                         # the recorded maximum is this subset's
    tol_q, tol_a, tol_b = R.tolerances()
    assert (tol_q, tol_a, tol_b) == (4 * R.GAP32_Q, 4 * R.GAP32_A, 4 * R.GAP32_B)
    assert 8 * tol_q <= R.NEAR_TIE_MARGIN and R.NEAR_TIE_SHARE <= 1e-3


def test_generated_cases():
    """the generator: slabs and texture in the guide, softmax-like p, near ties within the share at every eps"""
    tol_q = R.tolerances()[0]
    for h, w in [s for s in R.SIZES if s[0] * s[1] <= 2200]:
        g = R.case_guide(h, w)
        assert g.dtype == np.uint8 and g.shape == (h, w)
        if h >= 17 and w >= 16:
            assert (g == 255).sum() >= (h // 3) * (w // 2) and (g == 0).sum() >= (h // 3) * (w - w // 2)
            assert (R.guide_sums(g, 1)[3] == 0).any() and (R.guide_sums(g, 1)[3] != 0).any()
        for c in R.CLASSES:
            for r in R.RADII:
                g2, p, refs = R.case_reference(h, w, c, r)
                assert np.array_equal(g2, g) and p.dtype == np.float32 and np.abs(p.sum(0) - 1).max() < 1e-6 and p.min() > 0
                assert sorted(refs) == R.EPSS
                for ref in refs.values():
                    assert (R.top2_margin(ref['q']) < 8 * tol_q).mean() <= 1e-3
    g3, p3, _ = R.case_reference(17, 16, 9, 4)
    assert np.array_equal(p3, R.case_reference(17, 16, 9, 4)[1])          # the same case gives the same draw


# ---- the package side that needs no device -------------------------------------------------------------------------------------------------
def test_bindings_exist():
    from pylc_amd import lib as L
    dll = ctypes.CDLL(L.LIB_PATH)
    for name, nargs in (('pylc_luma_u8', 6), ('pylc_guided_coeffs', 12), ('pylc_guided_apply', 12)):
        assert hasattr(dll, name)
        assert len(L.SIGNATURES[name][1]) == nargs and L.SIGNATURES[name][0] is ctypes.c_int
    assert L.ABI_VERSION == 15 and L.lib.pylc_abi_version() == 15


def test_entry_point_errors_without_gpu():
    """argument validation happens on the host before any launch"""
    from pylc_amd.lib import lib
    one = 1 << 12                                     # any non-NULL, aligned address: nothing is dereferenced

    def refused(rc, word):
        assert rc == 1 and word in lib.pylc_last_error(), lib.pylc_last_error()

    refused(lib.pylc_luma_u8(None, 3, 4, 4, one, None), b'NULL')
    refused(lib.pylc_luma_u8(one, 3, 4, 4, None, None), b'NULL')
    refused(lib.pylc_luma_u8(one, 2, 4, 4, one, None), b'channels')
    refused(lib.pylc_luma_u8(one, 4, 4, 4, one, None), b'channels')
    refused(lib.pylc_luma_u8(one, 3, 0, 4, one, None), b'image')
    refused(lib.pylc_luma_u8(one, 3, 4, -1, one, None), b'image')
    refused(lib.pylc_luma_u8(one, 3, 1 << 16, 1 << 15, one, None), b'2^31')

    def coeffs(p=one, plane=16, pitch=4, g=one, c=3, h=4, w=4, r=2, eps=1e-3, a=one, b=one):
        return lib.pylc_guided_coeffs(p, plane, pitch, g, c, h, w, r, eps, a, b, None)
    for kw in ({'p': None}, {'g': None}, {'a': None}, {'b': None}):
        refused(coeffs(**kw), b'NULL')
    for c in (1, 17, 0):
        refused(coeffs(c=c), b'n_classes')
    for r in (0, 65, -1):
        refused(coeffs(r=r), b'radius')
    for eps in (0.0, 9e-7, 1.0001, -1e-3, float('nan'), float('inf')):
        refused(coeffs(eps=eps), b'eps')
    refused(coeffs(h=0), b'image')
    refused(coeffs(w=0), b'image')
    refused(coeffs(h=1 << 16, w=1 << 15, plane=1 << 40, pitch=1 << 15), b'2^31')
    refused(coeffs(pitch=3), b'pitch')
    refused(coeffs(plane=15), b'plane stride')
    refused(coeffs(pitch=6, plane=21), b'plane stride')          # (4 - 1) * 6 + 4 = 22
    for kw in ({'p': one + 2}, {'a': one + 1}, {'b': one + 3}):
        refused(coeffs(**kw), b'aligned')

    def apply(a=one, b=one, g=one, c=3, h=4, w=4, r=2, clip=1, mask=one, probs=None, conf=None):
        return lib.pylc_guided_apply(a, b, g, c, h, w, r, clip, mask, probs, conf, None)
    for kw in ({'a': None}, {'b': None}, {'g': None}, {'mask': None}):
        refused(apply(**kw), b'NULL')
    for c in (1, 17):
        refused(apply(c=c), b'n_classes')
    for r in (0, 65):
        refused(apply(r=r), b'radius')
    refused(apply(clip=2), b'clip')
    refused(apply(clip=-1), b'clip')
    refused(apply(h=0), b'image')
    refused(apply(h=1 << 16, w=1 << 15), b'2^31')
    for kw in ({'a': one + 2}, {'b': one + 1}, {'probs': one + 2}, {'conf': one + 3}):
        refused(apply(**kw), b'aligned')


def test_spec_validation():
    from pylc_amd import refine
    assert refine.check_spec({'radius': 8, 'eps': 1e-3}) == (8, 1e-3, True)
    assert refine.check_spec({'radius': 64, 'eps': 1, 'clip': False}) == (64, 1.0, False)
    assert refine.check_spec({'radius': 1, 'eps': 1e-6}) == (1, 1e-6, True)
    for bad, word in (({'radius': 0, 'eps': 1e-3}, '0'), ({'radius': 65, 'eps': 1e-3}, '65'), ({'radius': 8.0, 'eps': 1e-3}, '8.0'),
                      ({'radius': True, 'eps': 1e-3}, 'True'), ({'radius': 8, 'eps': 0}, '0'), ({'radius': 8, 'eps': 2.5}, '2.5'),
                      ({'radius': 8, 'eps': float('nan')}, 'nan'), ({'radius': 8, 'eps': '1e-3'}, "'1e-3'"), ({'radius': 8}, 'eps'),
                      ({'eps': 1e-3}, 'radius'), ({'radius': 8, 'eps': 1e-3, 'clip': 1}, '1'),
                      ({'radius': 8, 'eps': 1e-3, 'sigma': 2}, 'sigma'), ((8, 1e-3), '(8, 0.001)'), ('guided', 'guided')):
        with pytest.raises(ValueError, match=word.replace('(', r'\(').replace(')', r'\)')):
            refine.check_spec(bad)


def test_python_argument_errors():
    from pylc_amd import refine
    p = torch.full((3, 4, 5), 1 / 3)
    g = torch.zeros((4, 5), dtype=torch.uint8)
    img = torch.zeros((3, 4, 5), dtype=torch.uint8)
    for call in (lambda: refine.luma(img.float()), lambda: refine.luma(img[0]), lambda: refine.luma(torch.zeros((2, 4, 5), dtype=torch.uint8)),
                 lambda: refine.luma(img[:, :0]), lambda: refine.luma(img.numpy()),
                 lambda: refine.guided_refine(p, g, radius=0), lambda: refine.guided_refine(p, g, radius=65),
                 lambda: refine.guided_refine(p, g, eps=1e-7), lambda: refine.guided_refine(p, g, eps=1.5),
                 lambda: refine.guided_refine(p, g, clip=1), lambda: refine.guided_refine(p.double(), g),
                 lambda: refine.guided_refine(p[0], g), lambda: refine.guided_refine(p[:1], g),
                 lambda: refine.guided_refine(torch.zeros((17, 4, 5)), g), lambda: refine.guided_refine(p, g.float()),
                 lambda: refine.guided_refine(p, g[:3]), lambda: refine.guided_refine(p, img[:, :, :4]),
                 lambda: refine.guided_refine(p, torch.zeros((2, 4, 5), dtype=torch.uint8)), lambda: refine.guided_refine(p, None),
                 lambda: refine.guided_coeffs(p, g, 0, 1e-3), lambda: refine.guided_coeffs(p, g, 8, 2.0),
                 lambda: refine.guided_coeffs(p, g[:, :4], 8, 1e-3)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: refine.luma(img), lambda: refine.guided_refine(p, g), lambda: refine.guided_refine(p, img),
                 lambda: refine.guided_coeffs(p, g, 8, 1e-3)):
        with pytest.raises(ValueError, match='device'):               # a host tensor: there is no CPU path
            call()


def test_pipeline_argument_errors():
    """the spec and the image are checked before the model or the device are touched"""
    from pylc_amd import inference, photo
    deeplab = types.SimpleNamespace(meta=types.SimpleNamespace(arch='deeplab', ch=3))
    img = torch.zeros((3, 64, 64), dtype=torch.uint8)
    good = {'radius': 8, 'eps': 1e-3}
    with pytest.raises(ValueError, match='65'):
        inference.predict_blend_mean(deeplab, img, 64, 64, refine={'radius': 65, 'eps': 1e-3})
    with pytest.raises(ValueError, match='uint8'):
        inference.predict_blend_mean(deeplab, img.float(), 64, 64, refine=good)
    with pytest.raises(ValueError, match='uint8'):
        inference.predict_image(deeplab, img.float(), 64, blend='mean', refine=good)
    with pytest.raises(ValueError, match='eps'):
        inference.predict_image(deeplab, img, 64, blend='mean', refine={'radius': 8})
    with pytest.raises(ValueError, match="refine needs blend='mean'"):
        inference.predict_image(deeplab, img, 64, refine=good)
    with pytest.raises(ValueError, match="flip, refine needs blend='mean'"):
        inference.predict_image(deeplab, img, 64, flip=True, refine=good)
    photo_img = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="refine needs blend='mean' on a DeepLab"):
        photo.segment_photo(deeplab, photo_img, tile=64, refine=good)
    with pytest.raises(ValueError, match='sigma'):
        photo.segment_photo(deeplab, photo_img, tile=64, blend='mean', refine={'radius': 8, 'eps': 1e-3, 'sigma': 1})


def test_refine_none_imports_nothing_new():
    """the package, the inference and the photograph paths load without the refine module: it is imported where a spec is given"""
    code = ('import sys, pylc_amd, pylc_amd.inference, pylc_amd.photo, pylc_amd.model\n'
            'assert "pylc_amd.refine" not in sys.modules\n'
            'from pylc_amd import refine\n'
            'assert refine.check_spec({"radius": 8, "eps": 1e-3}) == (8, 1e-3, True)\n')
    subprocess.run([sys.executable, '-c', code], check=True, cwd=R.__file__.rsplit('/tests/', 1)[0])
    import inspect
    from pylc_amd import inference, photo
    for fn in (inference.predict_image, inference.predict_overlap_tile, inference.predict_blend_mean, photo.segment_photo):
        assert inspect.signature(fn).parameters['refine'].default is None
