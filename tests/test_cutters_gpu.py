"""The tile cutter and the tile-batch driver of full-image inference on the GPU (-m gpu, csrc/pack_tiles.hip, pylc_amd/inference.py).

One kernel stands behind the five pylc_image_pack_tiles* entry points, so a test that compares one entry point with another compares
the kernel with itself: here every entry point is checked against a cut made on the host.  Then the two things every driver owes its
caller whichever blend it runs: the network's mode comes back after an exception, and the weight ranges are refreshed before the
first forward."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.test_cpu_overlap_tile import overlap_origins
from tests.test_unet_inference_gpu import reflect_windows

pytestmark = pytest.mark.gpu

MEAN, STD = (132.47, 144.47, 149.45), (24.85, 22.04, 18.77)
H, W = 70, 93                           # not fitted to anything below: the fitted entry points must drop the remainder
FITTED, MIRRORED = (32, 32, 20), (32, 20, 13)      # (tile, out, stride); MIRRORED: pad 6, the clamped last tile on both axes, all four edges

# entry point -> (takes uint8, has a flip argument, any-size grid, its geometries)
ENTRY = {'pack_tiles': (False, False, False, (FITTED,)),
         'pack_tiles_ex': (True, False, False, (FITTED,)),
         'pack_tiles_flip': (True, True, False, (FITTED,)),
         'pack_tiles_reflect': (True, False, True, (MIRRORED,)),
         'pack_tiles_reflect_ex': (True, True, True, (FITTED, MIRRORED))}
CASES = [(name, geom, u8, ch, flip) for name, (takes_u8, flips, _, geoms) in ENTRY.items() for geom in geoms
         for u8 in ((False, True) if takes_u8 else (False,)) for ch in (1, 3) for flip in ((0, 1) if flips else (0,))]


@functools.lru_cache(maxsize=None)
def _host_image(ch):
    return torch.from_numpy(np.random.RandomState(40 + ch).randint(0, 256, (ch, H, W)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _host_tiles(ch, geom, any_size):
    """the expected tiles [n, 3, tile, tile] in float32 torch, computed once per case and left unchanged"""
    tile, out, stride = geom
    img = _host_image(ch).float()
    if any_size:
        win = reflect_windows(img, tile, out, stride)
    else:                                                            # slices at i * stride, the remainder right and below dropped
        win = torch.stack([img[:, i * stride:i * stride + tile, j * stride:j * stride + tile]
                           for i in range((H - tile) // stride + 1) for j in range((W - tile) // stride + 1)])
    win = win.expand(-1, 3, -1, -1)                                  # one channel is copied into three
    m, s = torch.tensor(MEAN)[None, :, None, None], torch.tensor(STD)[None, :, None, None]
    return ((win - m) / s) / 255


def _cut(name, img, geom, first, n, flip):
    from pylc_amd import ops, lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    tile, out, stride = geom
    c, h, w = img.shape
    got = ops.empty_nhwc(n, 4, tile, tile, img.device)
    m, s = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    u8 = int(img.dtype == torch.uint8)
    if name == 'pack_tiles':
        check(lib.pylc_image_pack_tiles(ptr(img), c, h, w, tile, stride, first, n, m, s, ptr(got), stream()))
    elif name == 'pack_tiles_ex':
        check(lib.pylc_image_pack_tiles_ex(ptr(img), u8, c, h, w, tile, stride, first, n, m, s, ptr(got), stream()))
    elif name == 'pack_tiles_flip':
        check(lib.pylc_image_pack_tiles_flip(ptr(img), u8, c, h, w, tile, stride, first, n, m, s, ptr(got), stream(), flip))
    elif name == 'pack_tiles_reflect':
        check(lib.pylc_image_pack_tiles_reflect(ptr(img), u8, c, h, w, tile, out, stride, first, n, m, s, ptr(got), stream()))
    else:
        check(lib.pylc_image_pack_tiles_reflect_ex(ptr(img), u8, c, h, w, tile, out, stride, first, n, m, s, ptr(got), stream(), flip))
    return got


@pytest.mark.parametrize('name,geom,u8,ch,flip', CASES)
def test_every_cutter_entry_point_against_a_host_cut(dev, name, geom, u8, ch, flip):
    from pylc_amd.lib import PylcError
    any_size = ENTRY[name][2]
    tile, out, stride = geom
    if any_size:
        n = len(overlap_origins(H, out, stride)) * len(overlap_origins(W, out, stride))
    else:
        n = ((H - tile) // stride + 1) * ((W - tile) // stride + 1)
    want = _host_tiles(ch, geom, any_size)
    assert want.shape[0] == n >= 7
    want = torch.flip(want, dims=[3]) if flip else want
    img = (_host_image(ch) if u8 else _host_image(ch).float()).to(dev).contiguous()
    got = _cut(name, img, geom, 0, n, flip)
    err = (got[:, :3].cpu() - want).abs().max().item()
    print('%s %s u8 %d ch %d flip %d: %d tiles, max|tiles - host| %.3g' % (name, geom, u8, ch, flip, n, err))
    assert err < 1e-7
    assert float(got[:, 3].abs().max()) == 0.0
    assert torch.equal(_cut(name, img, geom, 3, 4, flip), got[3:7])                 # a batch from the middle of the tile list
    with pytest.raises(PylcError):                                                   # one tile past the grid: refused on the host
        _cut(name, img, geom, n - 3, 4, flip)


# ---- the driver --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def deeplab(dev):
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    runtime.dropout_enabled = False
    torch.manual_seed(0)
    return Model(Meta(ch=3), dev).build()


@pytest.mark.parametrize('blend', ['reference', 'mean'])
def test_an_exception_in_the_network_leaves_its_mode_as_it_was(dev, deeplab, blend, monkeypatch):
    from pylc_amd import inference

    def boom(*a, **k):
        raise RuntimeError('boom')
    deeplab.net.train()
    monkeypatch.setattr(deeplab.net, 'forward', boom)
    try:
        with pytest.raises(RuntimeError, match='boom'):
            inference.predict_image(deeplab, torch.zeros(3, 64, 96), tile=32, blend=blend)
        assert deeplab.net.training is True
    finally:
        deeplab.net.eval()


def _count_refreshes(model, monkeypatch):
    calls = []
    refresh = model._refresh_for_inference
    monkeypatch.setattr(model, '_refresh_for_inference', lambda: (calls.append(1), refresh())[1])
    return calls


def test_every_deeplab_path_refreshes_the_weight_ranges(dev, deeplab, monkeypatch):
    from pylc_amd import inference, photo
    from tests.test_photo_gpu import photo_np
    calls = _count_refreshes(deeplab, monkeypatch)
    img = torch.from_numpy(np.ascontiguousarray(photo_np(34, 64, 128).transpose(2, 0, 1)))
    for blend in ('reference', 'mean'):
        del calls[:]
        mask = inference.predict_image(deeplab, img, tile=64, blend=blend)
        assert tuple(mask.shape) == (64, 128) and len(calls) >= 1, blend
    del calls[:]
    res = photo.segment_photo(deeplab, photo_np(33, 180, 230), tile=64)
    assert tuple(res.mask.shape) == (180, 230) and len(calls) >= 1


def test_the_unet_path_refreshes_the_weight_ranges(dev, monkeypatch):
    from pylc_amd import inference, runtime
    from pylc_amd.model import Model, Meta
    from tests.test_photo_gpu import photo_np
    runtime.dropout_enabled = False
    torch.manual_seed(0)
    model = Model(Meta(arch='unet', ch=3, n_classes=9), dev).build()
    calls = _count_refreshes(model, monkeypatch)
    img = torch.from_numpy(np.ascontiguousarray(photo_np(23, 150, 200).transpose(2, 0, 1)))
    mask = inference.predict_overlap_tile(model, img, 256)
    assert tuple(mask.shape) == (150, 200) and len(calls) >= 1
