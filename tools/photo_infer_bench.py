"""Whole-photograph inference throughput (pylc_amd.photo.segment_photo) on one MI355X: a seeded uint8 photograph the size of the reference's
recorded test image (W x H 3453 x 4940, pylc_gpu.ipynb), fitted on the device to 3072 x 4096, run through DeepLab, stitched,
resized back to 3453 x 4940 and class-encoded.  Two legs:

    r101      DeepLabV3+/ResNet101, RGB, 9 classes, tile 512, stride 256 (11 x 15 = 165 tiles)
    xception  DeepLabV3+/Xception, grayscale, 11 classes, tile 1024, stride 512 (5 x 7 = 35 tiles; the configs[4] inference leg)

Warm-up calls, then N timed calls, each ending in a device synchronise; prints one JSON line with images/s per leg and the algorithmic
bytes of the photograph kernels (for their share of the copy rate, with the kernel times of a trace).

    python tools/photo_infer_bench.py [--calls N] [--warmup W] [--legs r101,xception]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/photo_infer_bench.py --once     # one call per leg, for the kernel trace
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

H, W = 4940, 3453
LEGS = {
    'r101': dict(backbone='resnet', ch=3, classes=9, tile=512),
    'xception': dict(backbone='xception', ch=1, classes=11, tile=1024),
}


def kernel_bytes(geom, ch):
    """Bytes each photograph kernel must move for one image: the fit resize reads the photograph once and writes the fitted image
    (1 B per sample each way); the class encode reads one RGB pixel and writes one byte per scaled-size pixel; the colourize (the
    existing pylc_colourize_resize) reads one mask byte and writes three per scaled-size pixel; the upload is one byte per sample."""
    full = geom['h_full'] * geom['w_full']
    scaled = geom['h_scaled'] * geom['w_scaled']
    fitted = geom['h_fitted'] * geom['w_fitted']
    return {'upload_bytes': full * ch, 'resize_bytes': (full + fitted) * ch, 'encode_bytes': scaled * 4, 'colourize_bytes': scaled * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--legs', default='r101,xception')
    ap.add_argument('--once', action='store_true', help='one call per leg and nothing else (under rocprofv3 --kernel-trace --stats)')
    a = ap.parse_args()
    from pylc_amd import photo
    from pylc_amd.model import Model, Meta
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(1)
    rgb = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    out = {'image_hw': [H, W], 'dtype': 'uint8', 'batch': a.batch}
    for name in a.legs.split(','):
        leg = LEGS[name]
        torch.manual_seed(0)
        model = Model(Meta(backbone=leg['backbone'], ch=leg['ch'], n_classes=leg['classes']), dev).build()
        model.net.eval()
        img = rgb if leg['ch'] == 3 else np.ascontiguousarray(rgb[..., 0])
        pal = rs.randint(0, 256, (leg['classes'], 3)).astype(np.uint8)
        tile = leg['tile']

        def run():
            return photo.segment_photo(model, img, tile=tile, palette=pal, batch=a.batch)
        if a.once:
            res = run()
            torch.cuda.synchronize()
            out[name] = {'once': True, 'mask': list(res.mask.shape), 'geometry': res.geometry}
            continue
        for _ in range(a.warmup):
            res = run()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            res = run()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        g = res.geometry
        rows, cols = (g['h_fitted'] - tile) // (tile // 2) + 1, (g['w_fitted'] - tile) // (tile // 2) + 1
        mean = sum(times) / len(times)
        out[name] = dict({'backbone': leg['backbone'], 'ch': leg['ch'], 'classes': leg['classes'], 'tile': tile, 'stride': tile // 2,
                          'tiles': rows * cols, 'fitted_hw': [g['h_fitted'], g['w_fitted']], 'calls': a.calls, 'seconds_mean': mean,
                          'seconds_min': min(times), 'seconds_max': max(times), 'images_per_s': 1.0 / mean}, **kernel_bytes(g, leg['ch']))
        del model
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
