"""Full-image U-Net inference throughput (pylc_amd.inference.predict_image -> predict_overlap_tile) on one MI355X: a seeded 3072 x 4096
uint8 RGB image, 512 px windows (324 px output tiles, stride 324: 10 x 13 = 130 tiles), batches of 8.  Warm-up calls, then N timed
calls, each ending in a device synchronise; prints one JSON line with images/s, megapixels/s and tiles/s, and the algorithmic bytes of
the two overlap-tile kernels (for their share of the copy rate, with the kernel times of a trace).

    python tools/unet_infer_bench.py [--calls N] [--warmup W] [--classes C] [--stride S]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/unet_infer_bench.py --once      # one call, for the kernel trace
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def kernel_bytes(h, w, cimg, tile, out, stride, ncls):
    """Bytes each kernel must move for one image: the cutter reads one uint8 per channel and writes one 16-B pixel per window pixel; the
    stitch reads every logit tile once (its ceil(C/4) 16-B vectors per pixel) and writes one mask byte per image pixel."""
    rows = -(-(h - out) // stride) + 1
    cols = -(-(w - out) // stride) + 1
    n = rows * cols
    pack = n * tile * tile * (cimg + 16)
    stitch = n * out * out * 16 * ((ncls + 3) // 4) + h * w
    return n, pack, stitch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--classes', type=int, default=9)
    ap.add_argument('--stride', type=int, default=None, help='output-tile stride (default: the output tile, 324)')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--once', action='store_true', help='one call and nothing else (under rocprofv3 --kernel-trace --stats)')
    a = ap.parse_args()
    from pylc_amd import inference
    from pylc_amd.model import Model, Meta
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = Model(Meta(arch='unet', ch=3, n_classes=a.classes), dev).build()
    h, w, tile = 3072, 4096, 512
    img = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (3, h, w)).astype(np.uint8)).to(dev)
    out = tile - 2 * model.meta.pad_size
    stride = a.stride or out
    if a.once:
        mask = inference.predict_image(model, img, tile, stride, batch=a.batch)
        torch.cuda.synchronize()
        print(json.dumps({'once': True, 'mask': list(mask.shape)}))
        return
    for _ in range(a.warmup):
        inference.predict_image(model, img, tile, stride, batch=a.batch)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        inference.predict_image(model, img, tile, stride, batch=a.batch)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    n, pack, stitch = kernel_bytes(h, w, 3, tile, out, stride, a.classes)
    mean = sum(times) / len(times)
    print(json.dumps({'image': [3, h, w], 'dtype': 'uint8', 'tile': tile, 'out': out, 'stride': stride, 'batch': a.batch, 'classes': a.classes,
                      'tiles': n, 'calls': a.calls, 'seconds_mean': mean, 'seconds_min': min(times), 'seconds_max': max(times),
                      'images_per_s': 1.0 / mean, 'megapixels_per_s': h * w / mean / 1e6, 'tiles_per_s': n / mean,
                      'pack_bytes_per_image': pack, 'stitch_bytes_per_image': stitch}))


if __name__ == '__main__':
    main()
