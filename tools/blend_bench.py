"""The streaming mean-probability blend against the one-shot stitchers at the recorded photograph's grid: a
3072 x 4096 image, 9 classes (pitch 12), tile 512, stride 256 -> 11 x 15 = 165 logit tiles of random logits (3 * randn), 2.08 GB.

    reference   pylc_stitch_argmax, one launch over all tiles (the reference's reconstruct())
    one_shot    pylc_stitch_overlap_argmax, one launch over all tiles (the mean blend from resident tiles)
    streaming   torch's zero fill of the accumulation image, pylc_blend_accumulate per batch of --batch tiles (ceil(165 / batch)
                launches, each reading its slice of the same tile buffer), pylc_blend_finalize (mask only)

The streaming result is compared with one_shot's first (bit for bit).  Everything is timed in ONE process between device events after
warm-up, the forms taking turns within a round (--rounds, the median is reported).  The tile buffer (2.08 GB) and the accumulation image
(0.60 GB) are both larger than the 256 MB last-level cache.  Bytes are the algorithm's: every form reads each logit tile once (pitch *
4 B per tile pixel) and writes 1 B of mask per image pixel; the accumulator additionally reads and writes pitch * 4 B for every pixel
its batch covers (counted on the host from the geometry), the finalizer reads the accumulation image once.  `resident` is what each
form needs in HBM at its peak besides the image: all tiles, or one batch of tiles plus the accumulation image.

--window adds the window-weighted legs after the rows above, which are measured and printed as before: in a
second loop of the same warm-up and round counts the plain streaming form (zero, pylc_blend_accumulate, pylc_blend_finalize) and the
windowed one (zero, pylc_blend_accumulate_w with the Hann table of 512 floats, pylc_blend_finalize_w with the two axis tables, built
once outside the timing) take turns.  Its JSON line holds, per phase, the median and the min / max over the rounds of both forms, and
`slower_than_spread`: whether the windowed median exceeds the plain median by more than the plain form's own min-max spread.

    python tools/blend_bench.py [--batch B] [--rounds R] [--warmup W] [--out FILE] [--window [--window-out FILE]]
"""
import argparse
import json
import os
import platform
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, C, PITCH, TILE, STRIDE = 3072, 4096, 9, 12, 512, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--window', action='store_true')
    ap.add_argument('--window-out', default=None)
    a = ap.parse_args()
    from pylc_amd import lib as L
    from pylc_amd.inference import overlap_tile_grid, tile_grid
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    dev = torch.device('cuda:0')
    rows, cols = tile_grid(H, W, TILE, STRIDE)
    row_o, col_o = overlap_tile_grid(H, W, TILE, STRIDE)
    n = rows * cols
    assert (len(row_o), len(col_o)) == (rows, cols)
    torch.manual_seed(0)
    logits = torch.randn((n, TILE, TILE, PITCH), device=dev) * 3
    acc = torch.empty((H, W, PITCH), device=dev)
    masks = {k: torch.empty((H, W), device=dev, dtype=torch.uint8) for k in ('reference', 'one_shot', 'streaming')}
    probs = {k: torch.empty((C, H, W), device=dev) for k in ('one_shot', 'streaming')}
    batches = [(k, min(a.batch, n - k)) for k in range(0, n, a.batch)]
    st = stream()

    def reference():
        check(lib.pylc_stitch_argmax(ptr(logits), PITCH, rows, cols, TILE, STRIDE, C, ptr(masks['reference']), st))

    def one_shot(p=None):
        check(lib.pylc_stitch_overlap_argmax(ptr(logits), PITCH, n, H, W, TILE, STRIDE, C, ptr(masks['one_shot']), ptr(p), st))

    def accumulate():
        for k, b in batches:
            check(lib.pylc_blend_accumulate(ptr(logits[k:k + b]), PITCH, k, b, H, W, TILE, STRIDE, C, 0, ptr(acc), PITCH, st))

    def finalize(p=None):
        check(lib.pylc_blend_finalize(ptr(acc), PITCH, H, W, TILE, STRIDE, C, 1, ptr(masks['streaming']), ptr(p), None, st))

    # the same result first
    one_shot(probs['one_shot'])
    acc.zero_()
    accumulate()
    finalize(probs['streaming'])
    torch.cuda.synchronize()
    if not (torch.equal(masks['streaming'], masks['one_shot']) and torch.equal(probs['streaming'], probs['one_shot'])):
        raise SystemExit('the streaming blend differs from pylc_stitch_overlap_argmax')
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

    forms = {'reference': [reference], 'one_shot': [one_shot], 'streaming': [acc.zero_, accumulate, finalize]}
    times = {k: [] for k in forms}
    for r in range(a.warmup + a.rounds):
        for k, fns in forms.items():
            t = span(fns)
            if r >= a.warmup:
                times[k].append(t)
    med = {k: np.median(np.asarray(v), axis=0) for k, v in times.items()}

    # the algorithm's bytes
    tile_bytes = n * TILE * TILE * PITCH * 4
    px = H * W
    band_px = 0
    for k, b in batches:
        cover = np.zeros((H, W), bool)
        for t in range(k, k + b):
            cover[row_o[t // cols]:row_o[t // cols] + TILE, col_o[t % cols]:col_o[t % cols] + TILE] = True
        band_px += int(cover.sum())
    bytes_ = {'reference': tile_bytes + px, 'one_shot': tile_bytes + px, 'zero': px * PITCH * 4,
              'accumulate': tile_bytes + 2 * band_px * PITCH * 4, 'finalize': px * PITCH * 4 + px}
    us = {'reference': med['reference'][0], 'one_shot': med['one_shot'][0], 'zero': med['streaming'][0], 'accumulate': med['streaming'][1],
          'finalize': med['streaming'][2]}
    us = {k: float(v) * 1e6 for k, v in us.items()}
    us['streaming'] = us['zero'] + us['accumulate'] + us['finalize']
    bytes_['streaming'] = bytes_['zero'] + bytes_['accumulate'] + bytes_['finalize']
    out = {'image': [H, W], 'n_classes': C, 'pitch': PITCH, 'tile': TILE, 'stride': STRIDE, 'tiles': n, 'batch': a.batch,
           'accumulate_launches': len(batches), 'rounds': a.rounds, 'warmup': a.warmup,
           'lib': os.path.relpath(L.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
           'device': torch.cuda.get_device_name(0), 'host': platform.node(),
           'us': us, 'us_total_min_max': {k: [float(np.asarray(v).sum(1).min()) * 1e6, float(np.asarray(v).sum(1).max()) * 1e6]
                                          for k, v in times.items()},
           'bytes': bytes_, 'gb_per_s': {k: bytes_[k] / us[k] * 1e-3 for k in us},
           'streaming_over_one_shot': us['streaming'] / us['one_shot'],
           'resident_bytes': {'one_shot': tile_bytes + px, 'streaming': a.batch * TILE * TILE * PITCH * 4 + px * PITCH * 4 + px}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    if not a.window:
        return

    # ---- the window-weighted legs: the plain and the windowed streaming form take turns ------------------------------------------------
    from pylc_amd.inference import blend_window, _window_sums
    win = blend_window('hann', TILE, dev)
    sum_y, sum_x = _window_sums(win, TILE, STRIDE, H), _window_sums(win, TILE, STRIDE, W)

    def accumulate_w():
        for k, b in batches:
            check(lib.pylc_blend_accumulate_w(ptr(logits[k:k + b]), PITCH, k, b, H, W, TILE, STRIDE, C, 0, ptr(acc), PITCH, ptr(win), 1.0, st))

    def finalize_w():
        check(lib.pylc_blend_finalize_w(ptr(acc), PITCH, H, W, C, 1, ptr(sum_y), ptr(sum_x), ptr(masks['streaming']), None, None, st))

    # a table of ones gives the plain form's bytes, first
    ones = blend_window('uniform', TILE, dev)
    acc.zero_()
    accumulate()
    want = acc.clone()
    acc.zero_()
    for k, b in batches:
        check(lib.pylc_blend_accumulate_w(ptr(logits[k:k + b]), PITCH, k, b, H, W, TILE, STRIDE, C, 0, ptr(acc), PITCH, ptr(ones), 1.0, st))
    torch.cuda.synchronize()
    if not torch.equal(acc, want):
        raise SystemExit('pylc_blend_accumulate_w with a table of ones differs from pylc_blend_accumulate')
    del want

    wforms = {'plain': [acc.zero_, accumulate, finalize], 'windowed': [acc.zero_, accumulate_w, finalize_w]}
    wtimes = {k: [] for k in wforms}
    for r in range(a.warmup + a.rounds):
        for k, fns in wforms.items():
            t = span(fns)
            if r >= a.warmup:
                wtimes[k].append(t)
    phases = {}
    for j, name in ((1, 'accumulate'), (2, 'finalize')):
        col = {k: np.asarray(v)[:, j] * 1e6 for k, v in wtimes.items()}
        spread = float(col['plain'].max() - col['plain'].min())
        phases[name] = {'plain_us': float(np.median(col['plain'])), 'plain_min_max_us': [float(col['plain'].min()), float(col['plain'].max())],
                        'windowed_us': float(np.median(col['windowed'])),
                        'windowed_min_max_us': [float(col['windowed'].min()), float(col['windowed'].max())],
                        'plain_spread_us': spread,
                        'slower_than_spread': bool(np.median(col['windowed']) - np.median(col['plain']) > spread)}
    wout = {'image': [H, W], 'n_classes': C, 'pitch': PITCH, 'tile': TILE, 'stride': STRIDE, 'tiles': n, 'batch': a.batch, 'window': 'hann',
            'rounds': a.rounds, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'host': platform.node(),
            'table_bytes': {'window': TILE * 4, 'axis_sums': (H + W) * 4}, 'phases': phases}
    wline = json.dumps(wout)
    print(wline)
    if a.window_out:
        with open(a.window_out, 'w') as f:
            f.write(wline + '\n')


if __name__ == '__main__':
    main()
