"""The multi-scale ensemble's two launches at the recorded photograph's grid: a 3072 x 4096 image, 9 classes
(pitch 12), tile 512, stride 256, scales 0.75 / 1.0 / 1.25 -> accumulation images of 2304 x 3072, 3072 x 4096 and 3840 x 5120 pixels, each
filled by pylc_blend_accumulate from random logits (3 * randn, drawn batch by batch: no network is needed and none is timed).

    resample    pylc_blend_resample_accumulate, one launch per scale into the ensemble image (add = 0 for the first)
    finalize    pylc_ensemble_finalize (mask only)
    aten        the same by ATen, per scale: the probability volume [1, C, hs, ws] = sums / counts (the counts of the geometry, a
                device image prepared outside the timed region), F.interpolate(mode='bilinear', align_corners=False) to 3072 x 4096,
                a weighted add into the sum; at the end argmax

The results are compared first: the kernels' probabilities against the ATen route's (whose coordinates are fp32 and may be off by up
to about 2.4e-4 px at x = 4096, so the comparison is to 1e-3; the maximum is reported) and the fraction of equal mask pixels.
Everything is timed in ONE process between device events after warm-up, the two routes taking turns within a round (--rounds, the
median is reported).  Bytes are the algorithm's: a resample launch reads its accumulation image once (hs * ws * pitch * 4 B) and writes
the ensemble image (H * W * pitch * 4 B), which every launch but the first also reads; the finalizer reads the ensemble image and
writes 1 B of mask per pixel.  The ATen route is charged the same bytes (it moves more): the ratio compares times.

    python tools/multiscale_bench.py [--batch B] [--rounds R] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, C, PITCH, TILE, STRIDE = 3072, 4096, 9, 12, 512, 256
SCALES = (0.75, 1.0, 1.25)


def cover_counts(n, out, origins):
    cnt = np.zeros(n, np.float32)
    for o in origins:
        cnt[o:o + out] += 1
    return cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch.nn.functional as F
    from pylc_amd import lib as L
    from pylc_amd.inference import overlap_tile_grid, scaled_size
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    dev = torch.device('cuda:0')
    st = stream()
    torch.manual_seed(0)
    sizes = [(scaled_size(H, s), scaled_size(W, s)) for s in SCALES]
    accs, counts = [], []
    for hs, ws in sizes:                                   # the finished sums of every scale, and the geometry's counts for the ATen route
        row_o, col_o = overlap_tile_grid(hs, ws, TILE, STRIDE)
        n = len(row_o) * len(col_o)
        acc = torch.zeros((hs, ws, PITCH), device=dev)
        for k in range(0, n, a.batch):
            b = min(a.batch, n - k)
            logits = torch.randn((b, TILE, TILE, PITCH), device=dev) * 3
            check(lib.pylc_blend_accumulate(ptr(logits), PITCH, k, b, hs, ws, TILE, STRIDE, C, 0, ptr(acc), PITCH, st))
        torch.cuda.synchronize()
        accs.append(acc)
        cnt = np.outer(cover_counts(hs, TILE, row_o), cover_counts(ws, TILE, col_o))
        counts.append(torch.from_numpy(cnt).to(dev)[:, :, None])
    ens = torch.full((H, W, PITCH), float('nan'), device=dev)
    mask = torch.empty((H, W), device=dev, dtype=torch.uint8)
    aten = {}

    def resample(k):
        hs, ws = sizes[k]
        return lambda: check(lib.pylc_blend_resample_accumulate(ptr(accs[k]), PITCH, hs, ws, TILE, STRIDE, 1, 1.0, C, ptr(ens), PITCH, H, W,
                                                                int(k > 0), st))

    def finalize(probs=None):
        check(lib.pylc_ensemble_finalize(ptr(ens), PITCH, H, W, C, float(len(SCALES)), ptr(mask), ptr(probs), None, st))

    def aten_scale(k):
        def run():
            vol = (accs[k][:, :, :C] / counts[k]).permute(2, 0, 1)[None].contiguous()         # the probability volume [1, C, hs, ws]
            up = F.interpolate(vol, size=(H, W), mode='bilinear', align_corners=False)
            aten['sum'] = up if k == 0 else aten['sum'] + up
        return run

    def aten_argmax():
        aten['mask'] = aten['sum'].argmax(1)

    # the same result first
    probs = torch.empty((C, H, W), device=dev)
    for k in range(len(SCALES)):
        resample(k)()
        aten_scale(k)()
    finalize(probs)
    aten_argmax()
    torch.cuda.synchronize()
    diff = float((probs - aten['sum'][0] / len(SCALES)).abs().max())
    same = float((mask.long() == aten['mask'][0]).float().mean())
    if not diff < 1e-3 or bool(torch.isnan(ens[:, :, :C]).any()):
        raise SystemExit('the ensemble kernels differ from the ATen route: max|probs difference| %g' % diff)
    del probs

    def span(fns):
        """device-event times (s) of the consecutive phases fns"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
        ev[0].record()
        for f, e in zip(fns, ev[1:]):
            f()
            e.record()
        torch.cuda.synchronize()
        return [p.elapsed_time(q) * 1e-3 for p, q in zip(ev, ev[1:])]

    forms = {'kernels': [resample(k) for k in range(len(SCALES))] + [finalize],
             'aten': [aten_scale(k) for k in range(len(SCALES))] + [aten_argmax]}
    times = {k: [] for k in forms}
    for r in range(a.warmup + a.rounds):
        for k, fns in forms.items():
            t = span(fns)
            if r >= a.warmup:
                times[k].append(t)
    med = {k: np.median(np.asarray(v), axis=0) for k, v in times.items()}

    px = H * W
    names = ['resample_%g' % s for s in SCALES] + ['finalize']
    bytes_ = {names[k]: (hs * ws + (2 if k else 1) * px) * PITCH * 4 for k, (hs, ws) in enumerate(sizes)}
    bytes_['finalize'] = px * PITCH * 4 + px
    us = {n: float(med['kernels'][i]) * 1e6 for i, n in enumerate(names)}
    us_aten = {n: float(med['aten'][i]) * 1e6 for i, n in enumerate(names)}
    us['total'], us_aten['total'], bytes_['total'] = sum(us.values()), sum(us_aten.values()), sum(bytes_.values())
    out = {'image': [H, W], 'n_classes': C, 'pitch': PITCH, 'tile': TILE, 'stride': STRIDE, 'scales': list(SCALES), 'sizes': sizes,
           'rounds': a.rounds, 'warmup': a.warmup,
           'lib': os.path.relpath(L.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
           'device': torch.cuda.get_device_name(0),
           'max_abs_probs_difference_to_aten': diff, 'mask_pixels_equal_to_aten': same,
           'us': us, 'us_aten': us_aten,
           'us_total_min_max': {k: [float(np.asarray(v).sum(1).min()) * 1e6, float(np.asarray(v).sum(1).max()) * 1e6] for k, v in times.items()},
           'bytes': bytes_, 'gb_per_s': {k: bytes_[k] / us[k] * 1e-3 for k in us},
           'aten_over_kernels': {k: us_aten[k] / us[k] for k in us},
           'resident_bytes': {'ensemble': px * PITCH * 4, 'largest_scaled_sums': max(hs * ws for hs, ws in sizes) * PITCH * 4}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
