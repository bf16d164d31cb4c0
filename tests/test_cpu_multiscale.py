"""CPU suite (-m "not gpu") for the multi-scale ensemble: the float64 statement of tests/_multiscale.py against torch's bilinear
interpolation, scaled_size, the host-side argument checks of the three entry points of csrc/multiscale.hip through their bindings, and
the ValueErrors of the Python layer on a stub model (no device)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._multiscale import ensemble_np, resize_bilinear_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'pylc_resize_bilinear_image': 9, 'pylc_blend_resample_accumulate': 15, 'pylc_ensemble_finalize': 10}


@pytest.mark.parametrize('hw,ohw', [((37, 53), (19, 27)), ((37, 53), (28, 40)), ((37, 53), (37, 53)), ((37, 53), (46, 66)),
                                    ((37, 53), (74, 106)), ((19, 27), (37, 53)), ((74, 106), (37, 53)), ((5, 7), (13, 3)), ((1, 1), (4, 5)),
                                    ((6, 9), (1, 1)), ((64, 48), (33, 95))])
def test_statement_is_torch_bilinear(hw, ohw):
    x = np.random.RandomState(hw[0] + 7 * ohw[1]).standard_normal((3,) + hw)
    want = torch.nn.functional.interpolate(torch.from_numpy(x)[None], size=ohw, mode='bilinear', align_corners=False)[0].numpy()
    got = resize_bilinear_np(x, *ohw)
    assert got.dtype == np.float64 and got.shape == (3,) + ohw
    assert np.abs(got - want).max() < 1e-12
    if hw == ohw:
        assert np.array_equal(got, x)                                    # equal sizes: f == 0, the identity is exact


def test_statement_takes_uint8_and_averages_with_weights():
    img = np.random.RandomState(1).randint(0, 256, (3, 9, 11)).astype(np.uint8)
    assert np.array_equal(resize_bilinear_np(img, 9, 11), img.astype(np.float64))
    p = np.random.RandomState(2).random_sample((4, 9, 11))
    q = np.random.RandomState(3).random_sample((4, 5, 6))
    ens, mask = ensemble_np([p, q], [(9, 11), (5, 6)], [2.0, 0.5], 9, 11)
    want = (2.0 * p + 0.5 * resize_bilinear_np(q, 9, 11)) / 2.5
    assert np.abs(ens - want).max() < 1e-15 and np.array_equal(mask, want.argmax(0).astype(np.uint8))
    one, _ = ensemble_np([p], [(9, 11)], [3.0], 9, 11)
    assert np.abs(one - p).max() < 1e-15


def test_scaled_size():
    from pylc_amd.inference import scaled_size
    assert scaled_size(37, 0.5) == 19 and scaled_size(53, 0.5) == 27            # 18.5 and 26.5: the .5 case rounds up
    assert (scaled_size(37, 0.75), scaled_size(53, 0.75)) == (28, 40)
    assert (scaled_size(37, 1.0), scaled_size(53, 1.0)) == (37, 53)
    assert (scaled_size(37, 1.25), scaled_size(53, 1.25)) == (46, 66)
    assert (scaled_size(37, 2.0), scaled_size(53, 2.0)) == (74, 106)
    assert (scaled_size(3072, 1.25), scaled_size(4096, 0.75)) == (3840, 3072)
    assert scaled_size(10, 0.54) == 5 and scaled_size(10, 0.55) == 6


def test_new_entry_points_are_declared_and_bound():
    import ctypes
    from pylc_amd import lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read(), flags=re.S)
    dll = ctypes.CDLL(L.LIB_PATH)
    for name, nargs in NEW.items():
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert hasattr(dll, name) and len(L.SIGNATURES[name][1]) == nargs and L.SIGNATURES[name][0] is ctypes.c_int, name
    assert 'multiscale.hip' in open(os.path.join(ROOT, 'pylc_amd', 'csrc', 'Makefile')).read()


def test_entry_point_errors_without_gpu():
    """argument validation happens on the host before any launch: every call below returns PYLC_ERR_ARG"""
    from pylc_amd.lib import lib
    a, b, c = 1 << 12, 1 << 13, 1 << 14                # non-NULL, 16-byte aligned addresses: nothing is dereferenced

    def resize(src=a, is_u8=1, cimg=3, h=8, w=8, dst=b, oh=4, ow=4):
        return lib.pylc_resize_bilinear_image(src, is_u8, cimg, h, w, dst, oh, ow, None)
    assert resize(src=None) == 1
    assert b'NULL' in lib.pylc_last_error()
    assert resize(dst=None) == 1
    for cimg in (0, 2, 4):
        assert resize(cimg=cimg) == 1
    assert b'Cimg' in lib.pylc_last_error()
    assert resize(is_u8=2) == 1
    assert resize(oh=0) == 1 and resize(ow=0) == 1 and resize(h=0) == 1 and resize(w=-1) == 1
    assert resize(dst=a) == 1

    def resample(acc=a, sp=12, hs=20, ws=24, out=16, stride=8, members=1, weight=1.0, ncls=9, ens=b, ep=12, h=37, w=53, add=0):
        return lib.pylc_blend_resample_accumulate(acc, sp, hs, ws, out, stride, members, weight, ncls, ens, ep, h, w, add, None)
    assert resample(acc=None) == 1
    assert b'NULL' in lib.pylc_last_error()
    assert resample(ens=None) == 1
    assert resample(sp=10) == 1 and resample(ep=10) == 1                       # a pitch that is no multiple of 4
    assert resample(sp=8) == 1 and resample(ep=8) == 1                         # a pitch below C
    assert resample(acc=a + 4) == 1 and resample(ens=b + 8) == 1               # not 16-byte aligned
    assert resample(ncls=1, sp=4, ep=4) == 1 and resample(ncls=17, sp=20, ep=20) == 1
    assert b'n_classes' in lib.pylc_last_error()
    assert resample(hs=15) == 1
    assert b'smaller than the output tile' in lib.pylc_last_error()
    assert resample(ws=15) == 1
    assert resample(stride=0) == 1 and resample(stride=17) == 1
    assert b'stride' in lib.pylc_last_error()
    assert resample(weight=0.0) == 1 and resample(weight=-1.0) == 1 and resample(weight=float('nan')) == 1
    assert resample(weight=float('inf')) == 1
    assert b'weight' in lib.pylc_last_error()
    assert resample(members=0) == 1
    assert resample(h=0) == 1 and resample(w=0) == 1 and resample(add=2) == 1
    assert resample(ens=a) == 1
    assert b'alias' in lib.pylc_last_error()

    def finalize(ens=a, pitch=12, h=37, w=53, ncls=9, total=1.0, mask=b, probs=c, conf=None):
        return lib.pylc_ensemble_finalize(ens, pitch, h, w, ncls, total, mask, probs, conf, None)
    assert finalize(ens=None) == 1 and finalize(mask=None) == 1
    assert b'NULL' in lib.pylc_last_error()
    assert finalize(pitch=10) == 1 and finalize(pitch=8) == 1 and finalize(ens=a + 4) == 1 and finalize(mask=b + 2) == 1
    assert finalize(ncls=1, pitch=4) == 1 and finalize(ncls=17, pitch=20) == 1
    assert finalize(total=0.0) == 1 and finalize(total=-2.0) == 1 and finalize(total=float('nan')) == 1
    assert b'total_weight' in lib.pylc_last_error()
    assert finalize(h=0) == 1 and finalize(w=0) == 1


def test_ensemble_plan_and_its_errors():
    from pylc_amd.inference import ensemble_plan
    assert ensemble_plan((0.75, 1.0, 1.25), None, 128, 192, 64) == [(0.75, 96, 144, 1.0), (1.0, 128, 192, 1.0), (1.25, 160, 240, 1.0)]
    assert ensemble_plan([2, 0.5], (3, 0.25), 128, 192, 64) == [(2.0, 256, 384, 3.0), (0.5, 64, 96, 0.25)]      # the order given
    with pytest.raises(ValueError, match='empty'):
        ensemble_plan((), None, 128, 192, 64)
    for bad in (0.49, 2.01, 0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='outside'):
            ensemble_plan((1.0, bad), None, 128, 192, 64)
    with pytest.raises(ValueError, match='2 entries for 3 scales'):
        ensemble_plan((0.75, 1.0, 1.25), (1, 1), 128, 192, 64)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='not a positive number'):
            ensemble_plan((0.75, 1.0), (1.0, bad), 128, 192, 64)
    with pytest.raises(ValueError, match=r'scale 0\.75 takes the 80x192 image to 60x144, below the output tile 64'):
        ensemble_plan((1.0, 0.75), None, 80, 192, 64)


def test_python_errors_need_no_device():
    """Raised from the arguments alone, before the library is initialised: a stub model, no GPU."""
    from pylc_amd import inference, photo
    model = SimpleNamespace(meta=SimpleNamespace(arch='deeplab', ch=3, n_classes=9))
    img = torch.zeros(3, 80, 192)
    rgb = np.zeros((80, 192, 3), np.uint8)
    for kw in (dict(scales=(1.0,)), dict(scale_weights=(1.0,)), dict(scales=(0.75, 1.0), scale_weights=(1, 2))):
        with pytest.raises(ValueError, match="blend='mean'"):                      # the reference stitch: flip's error
            inference.predict_image(model, img, 64, **kw)
        with pytest.raises(ValueError, match="blend='mean'"):
            photo.segment_photo(model, rgb, tile=64, **kw)
    with pytest.raises(ValueError, match='scale'):
        inference.predict_image(model, img, 64, blend='mean', scales=(1.0, 2.5))
    with pytest.raises(ValueError, match='empty'):
        inference.predict_image(model, img, 64, blend='mean', scales=())
    with pytest.raises(ValueError, match='1 entries for 2 scales'):
        inference.predict_image(model, img, 64, blend='mean', scales=(1.0, 1.25), scale_weights=(1.0,))
    with pytest.raises(ValueError, match='not a positive number'):
        inference.predict_image(model, img, 64, blend='mean', scales=(1.0, 1.25), scale_weights=(1.0, 0.0))
    with pytest.raises(ValueError, match='needs scales'):
        inference.predict_image(model, img, 64, blend='mean', scale_weights=(1.0,))
    with pytest.raises(ValueError, match=r'scale 0\.75 .* to 60x144, below the output tile 64'):
        inference.predict_image(model, img, 64, blend='mean', scales=(1.0, 0.75))
    with pytest.raises(ValueError, match=r'scale 0\.75 .* to 60x144, below the output tile 64'):
        inference.predict_blend_mean(model, img, 64, 64, scales=(0.75,))


def test_statement_decides_the_gpu_cases():
    """The kernel cases of tests/test_multiscale_gpu.py, on the statement alone: at the seeds used no case leaves more than 0.1 % of
    the pixels within MARGIN of a tie, and every case's probabilities sum to 1."""
    from tests import _multiscale as M
    from tests._blend import blend_mean_np
    for c in M.CLASSES:
        for stride in M.STRIDES:
            for name, sizes in M.SCALE_SETS.items():
                logits = M.case_logits(c, stride, name)
                for members in (1, 2):
                    probs = [blend_mean_np(list(logits[s][:members]), s[0], s[1], M.OUT, stride)[0] for s in sizes]
                    for weights in M.WEIGHT_SETS:
                        p, mask = ensemble_np(probs, sizes, weights[:len(sizes)], *M.BASE)
                        assert M.decided(p).mean() >= 0.999, (c, stride, name, members, weights)
                        assert np.abs(p.sum(0) - 1).max() < 1e-12 and mask.shape == M.BASE
