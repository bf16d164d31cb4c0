"""SHA-256 of what full-image inference produces for seeded inputs at the test sizes, one line each: run it at two commits and diff the
lines to show that a change to the tile cutter or to the tile-batch driver moved no byte.

    the five cutters     pylc_image_pack_tiles, _ex, _flip, _reflect, _reflect_ex on a seeded 70 x 93 image, uint8 and float, 1 and 3
                         channels, flip 0 and 1 where there is one: (32, 32, 20) on the fitted grid, (32, 20, 13) mirrored
    DeepLab (R101)       predict_image(blend='mean', flip=True, return_probs=True, return_confidence=True) on a 128 x 192 image, tile 64
    U-Net                predict_overlap_tile(return_probs=True) on a 150 x 200 image, tile 256
    segment_photo        the default call on a 180 x 230 photograph, tile 64

    python tools/cutter_hashes.py > hashes.txt
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN, STD = (132.47, 144.47, 149.45), (24.85, 22.04, 18.77)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def photo_np(seed, h, w):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 60 * np.sin(x[..., None] / (7.0 + np.arange(3)) + y[..., None] / 11.0) + rs.randint(-60, 61, (h, w, 3))
    return np.clip(base, 0, 255).astype(np.uint8)


def cutters(dev):
    from pylc_amd import ops
    from pylc_amd.lib import lib, check, ptr, stream
    h, w = 70, 93
    m, s = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    for ch in (1, 3):
        host = torch.from_numpy(np.random.RandomState(40 + ch).randint(0, 256, (ch, h, w)).astype(np.uint8))
        for u8 in (0, 1):
            img = (host if u8 else host.float()).to(dev).contiguous()
            for name, (tile, out, stride), flips in (('pack_tiles', (32, 32, 20), (None,)), ('pack_tiles_ex', (32, 32, 20), (None,)),
                                                     ('pack_tiles_flip', (32, 32, 20), (0, 1)), ('pack_tiles_reflect', (32, 20, 13), (None,)),
                                                     ('pack_tiles_reflect_ex', (32, 32, 20), (0, 1)),
                                                     ('pack_tiles_reflect_ex', (32, 20, 13), (0, 1))):
                if name == 'pack_tiles' and u8:
                    continue
                if name.startswith('pack_tiles_reflect'):
                    n = (-(-(h - out) // stride) + 1) * (-(-(w - out) // stride) + 1)
                else:
                    n = ((h - tile) // stride + 1) * ((w - tile) // stride + 1)
                for flip in flips:
                    got = ops.empty_nhwc(n, 4, tile, tile, dev)
                    if name == 'pack_tiles':
                        check(lib.pylc_image_pack_tiles(ptr(img), ch, h, w, tile, stride, 0, n, m, s, ptr(got), stream()))
                    elif name == 'pack_tiles_ex':
                        check(lib.pylc_image_pack_tiles_ex(ptr(img), u8, ch, h, w, tile, stride, 0, n, m, s, ptr(got), stream()))
                    elif name == 'pack_tiles_flip':
                        check(lib.pylc_image_pack_tiles_flip(ptr(img), u8, ch, h, w, tile, stride, 0, n, m, s, ptr(got), stream(), flip))
                    elif name == 'pack_tiles_reflect':
                        check(lib.pylc_image_pack_tiles_reflect(ptr(img), u8, ch, h, w, tile, out, stride, 0, n, m, s, ptr(got), stream()))
                    else:
                        check(lib.pylc_image_pack_tiles_reflect_ex(ptr(img), u8, ch, h, w, tile, out, stride, 0, n, m, s, ptr(got), stream(),
                                                                   flip))
                    print('%-22s tile %d out %d stride %d ch %d u8 %d flip %s  %3d tiles  %s'
                          % (name, tile, out, stride, ch, u8, flip, n, sha(got)))


def model_for(arch, salt, dev):
    import oracle
    from pylc_amd.model import Model, Meta
    model = Model(Meta(arch=arch, ch=3, n_classes=9), dev).build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec(arch, 'resnet', 9, 3), salt=salt))
    return model


def main():
    from pylc_amd import inference, photo, runtime, lib as L
    L.init()
    runtime.dropout_enabled = False
    dev = torch.device('cuda:0')
    cutters(dev)
    chw = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
    deeplab = model_for('deeplab', 2, dev)
    mask, probs, conf = inference.predict_image(deeplab, chw(photo_np(21, 128, 192)), 64, 32, blend='mean', flip=True, return_probs=True,
                                                return_confidence=True)
    print('deeplab mean+flip  mask %s  probs %s  conf %s  (%d classes in the mask)' % (sha(mask), sha(probs), sha(conf), len(mask.unique())))
    res = photo.segment_photo(deeplab, photo_np(33, 180, 230), tile=64)
    print('segment_photo default  mask %s  (%d classes in the mask)' % (sha(res.mask), len(res.mask.unique())))
    unet = model_for('unet', 3, dev)
    mask, probs = inference.predict_overlap_tile(unet, chw(photo_np(23, 150, 200)), 256, return_probs=True)
    print('unet overlap tiles  mask %s  probs %s  (%d classes in the mask)' % (sha(mask), sha(probs), len(mask.unique())))


if __name__ == '__main__':
    main()
