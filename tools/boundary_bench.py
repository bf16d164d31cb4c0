"""The boundary scores on one 3072 x 4096 pair of nine-class blob masks, against the whole-mask scoring pass the
project had before.

Inputs, generated on the device from a seed: the truth is the argmax of 9 box-smoothed noise fields; the prediction is the truth moved by
(2, 3) pixels with 1 % of its pixels replaced by random classes (every border off by a few pixels, plus speckle).  Two pairs:
    fine     a 17-wide box twice (regions some tens of pixels across: at R >= 32 every pixel lies in the band and every scan ends early)
    coarse   a 129-wide box twice (regions some hundreds of pixels across, as on a landscape photograph: most pixels lie deep inside a region
             and scan the full radius, the worst case of the kernels)

Timed per radius R in {8, 32, default_radius(3072, 4096) = 102}, between device events after --warmup rounds, the forms taking turns within
a round (--rounds, the median and the spread are reported):
    fused       pylc_boundary_counts: a column pass per mask, then ONE row pass of both masks that counts          3 launches
    two_map     pylc_boundary_distance of the truth and of the prediction, then pylc_boundary_counts_maps         5 launches
    distance    pylc_boundary_distance of the truth alone (the public map)                                        2 launches
    confusion   metrics.confusion_matrix of the same pair: the yardstick, the project's whole-mask scoring pass   (zero fill + 1 launch)
The two forms' counts are compared first, bit for bit.

Bytes are what each form must move per pixel, halo re-reads (served by the caches) left out:
    fused       8 B   column passes: 1 B mask in + 1 B g out, twice; row pass: 2 masks + 2 g in
    two_map    26 B   column passes 4 B; row passes: (1 B mask + 1 B g in, 4 B d2 out) twice; counts: 2 masks + 2 d2 in
    distance    7 B   1 B in + 1 B out; 1 B + 1 B in, 4 B out
    confusion   2 B   2 masks in
The bandwidth floor of a form is its bytes over the HBM rate a copy achieves on this GPU (--hbm-tbps, 6.29 TB/s measured).

    python tools/boundary_bench.py [--rounds R] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, C = 3072, 4096, 9
BYTES_PER_PIXEL = {'fused': 8, 'two_map': 26, 'distance': 7, 'confusion': 2}


def make_pair(dev, box, seed=0):
    import torch.nn.functional as F
    g = torch.Generator(device=dev).manual_seed(seed)
    f = torch.randn((C, 1, H, W), device=dev, generator=g)
    for _ in range(2):                               # a box twice: close to a Gaussian
        f = F.avg_pool2d(f, box, 1, box // 2, count_include_pad=False)
    truth = f[:, 0].argmax(0).to(torch.uint8).contiguous()
    del f
    pred = torch.roll(truth, (2, 3), (0, 1))
    hit = torch.rand((H, W), device=dev, generator=g) < 0.01
    rnd = torch.randint(0, C, (H, W), device=dev, generator=g, dtype=torch.uint8)
    return truth, torch.where(hit, rnd, pred).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--hbm-tbps', type=float, default=6.29)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import boundary, lib as L, metrics
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    dev = torch.device('cuda:0')
    pairs = {'fine': make_pair(dev, 17), 'coarse': make_pair(dev, 129)}
    truth, pred = pairs['fine']
    n = H * W
    st = stream()
    radii = [8, 32, boundary.default_radius(H, W)]
    ws = torch.empty((lib.pylc_boundary_workspace_bytes(1, H, W) // 4,), device=dev, dtype=torch.int32)
    d2t = torch.empty((H, W), device=dev, dtype=torch.int32)
    d2p = torch.empty((H, W), device=dev, dtype=torch.int32)
    counts = {k: torch.zeros(boundary.n_cells(C), device=dev, dtype=torch.int64) for k in ('fused', 'two_map')}

    def fused(r):
        check(lib.pylc_boundary_counts(ptr(truth), ptr(pred), 1, H, W, C, r, -1, ptr(counts['fused']), ptr(ws), st))

    def two_map(r):
        check(lib.pylc_boundary_distance(ptr(truth), 1, H, W, r, -1, None, ptr(d2t), ptr(ws), st))
        check(lib.pylc_boundary_distance(ptr(pred), 1, H, W, r, -1, None, ptr(d2p), ptr(ws), st))
        check(lib.pylc_boundary_counts_maps(ptr(truth), ptr(pred), ptr(d2t), ptr(d2p), n, C, r, -1, ptr(counts['two_map']), st))

    def distance(r):
        check(lib.pylc_boundary_distance(ptr(truth), 1, H, W, r, -1, None, ptr(d2t), ptr(ws), st))

    def confusion(r):
        metrics.confusion_matrix(truth, pred, C, force_coverage=False)

    forms = {'fused': fused, 'two_map': two_map, 'distance': distance, 'confusion': confusion}

    def span(r):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(forms) + 1)]
        ev[0].record()
        for f, e in zip(forms.values(), ev[1:]):
            f(r)
            e.record()
        torch.cuda.synchronize()
        return [p.elapsed_time(q) * 1e3 for p, q in zip(ev, ev[1:])]

    res = {}
    for name, r in [(name, r) for name in pairs for r in radii]:
        truth, pred = pairs[name]                    # (the closures above read these names)
        for c in counts.values():
            c.zero_()
        fused(r)
        two_map(r)
        torch.cuda.synchronize()
        if not torch.equal(counts['fused'], counts['two_map']):
            raise SystemExit('the fused and the two-map counts differ at radius %d (%s)' % (r, name))
        if not torch.equal(counts['fused'], boundary.boundary_counts(truth, pred, C, r)):
            raise SystemExit('boundary.boundary_counts differs from the entry point at radius %d (%s)' % (r, name))
        s = boundary.boundary_scores(counts['fused'], C)
        times = np.asarray([span(r) for _ in range(a.warmup + a.rounds)][a.warmup:])
        med = np.median(times, axis=0)
        us = {k: float(v) for k, v in zip(forms, med)}
        whole = metrics.scores(metrics.confusion_matrix(truth, pred, C, force_coverage=False))
        res.setdefault(name, {})[str(r)] = {'us': us, 'us_min_max': {k: [float(times[:, i].min()), float(times[:, i].max())] for i, k in enumerate(forms)},
                       'floor_us': {k: BYTES_PER_PIXEL[k] * n / (a.hbm_tbps * 1e12) * 1e6 for k in forms},
                       'times_bandwidth_floor': {k: us[k] / (BYTES_PER_PIXEL[k] * n / (a.hbm_tbps * 1e12) * 1e6) for k in forms},
                       'times_confusion_pass': {k: us[k] / us['confusion'] for k in forms},
                       'fused_over_two_map': us['fused'] / us['two_map'],
                       'boundary_iou': s['boundary_iou'], 'trimap_iou': s['trimap_iou'], 'band_px': s['band_px'],
                       'whole_mask_iou': whole['iou']}
    out = {'image': [H, W], 'n_classes': C, 'radii': radii, 'rounds': a.rounds, 'warmup': a.warmup, 'hbm_tbps': a.hbm_tbps,
           'lib': os.path.relpath(L.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
           'device': torch.cuda.get_device_name(0), 'bytes_per_pixel': BYTES_PER_PIXEL,
           'inputs': res}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
