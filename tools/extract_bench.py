"""The tile cutter (pylc_extract_tiles, csrc/dataset.hip) at the size of the reference's recorded photograph: a seeded uint8 RGB image of
H x W 4940 x 3453 with a class-index mask, no scale, tile 512, stride 512 (9 x 6 = 54 tiles), on one MI355X.

Warm-up launches, then N timed launches back to back between two device events, twice: on ONE set of buffers (113 MB read + written per
launch: it stays in the 256 MiB Infinity Cache) and rotating over SETS sets of inputs and outputs (about 1 GB: every launch reads and
writes HBM).  Reports bytes read + written / time next to the achievable HBM rate (MI355X: 6.3 TB/s), the same for pylc_tile_stats on
the tiles (reads only), one dataset.extract_photo call end to end (upload, relayout, mask encode, cut; host clock around a synchronise),
and for comparison the numpy / torch restatement of tests/test_cpu_dataset.py (unfold_tiles + tile_sums_np) on this host's CPU share.

    python tools/extract_bench.py [--launches N] [--warmup W] [--sets K] [--cpu-runs R] [--band-rows 4,8,16,32] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

H, W, C, TILE, STRIDE, NCLS = 4940, 3453, 3, 512, 512, 9
HBM_ACHIEVABLE = 6.3e12


def timed(fn, launches, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--sets', type=int, default=8)
    ap.add_argument('--cpu-runs', type=int, default=3)
    ap.add_argument('--band-rows', default='', help='comma-separated band_rows values to time the cutter with as well (the default band is 0)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import dataset, lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    from tests.test_cpu_dataset import tile_sums_np, unfold_tiles
    assert torch.cuda.is_available(), 'needs the MI355X'
    L.init()
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(1)
    image = rs.randint(0, 256, (H, W, C)).astype(np.uint8)
    cls = rs.randint(0, NCLS, (H // 8 + 1, W // 8 + 1)).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:H, :W]       # 8 x 8 blobs
    planar = np.ascontiguousarray(image.transpose(2, 0, 1))
    rows, cols = dataset.tile_grid_counts(H, W, TILE, STRIDE)
    n = rows * cols
    moved = n * TILE * TILE * (C + 1)
    out = {'image_hw': [H, W], 'ch': C, 'tile': TILE, 'stride': STRIDE, 'n_classes': NCLS, 'tiles': n, 'launches': a.launches,
           'warmup': a.warmup, 'bytes_read': moved, 'bytes_written': moved, 'hbm_achievable_TBps': HBM_ACHIEVABLE / 1e12}

    sets = []
    for _ in range(a.sets):
        sets.append(dict(img=torch.from_numpy(planar).to(dev), mask=torch.from_numpy(np.ascontiguousarray(cls)).to(dev),
                         tiles=torch.empty((n, C, TILE, TILE), device=dev, dtype=torch.uint8),
                         mtiles=torch.empty((n, TILE, TILE), device=dev, dtype=torch.uint8),
                         sums=torch.zeros((n, 2, C), device=dev, dtype=torch.int64), hist=torch.zeros((n, NCLS + 1), device=dev, dtype=torch.int64)))

    def cut(s, band_rows=0):
        check(lib.pylc_extract_tiles(ptr(s['img']), C, H, W, ptr(s['mask']), NCLS, TILE, STRIDE, 0, n, band_rows, ptr(s['tiles']),
                                     ptr(s['mtiles']), ptr(s['sums']), ptr(s['hist']), stream()))

    def stats(s):
        check(lib.pylc_tile_stats(ptr(s['tiles']), n, C, TILE, ptr(s['mtiles']), NCLS, 0, ptr(s['sums']), ptr(s['hist']), stream()))

    # the result first: against the restatement, once
    cut(sets[0])
    want_img, want_mask = unfold_tiles(planar, TILE, STRIDE), unfold_tiles(cls, TILE, STRIDE)
    want_sums, want_hist = tile_sums_np(want_img, want_mask, NCLS)
    assert np.array_equal(sets[0]['tiles'].cpu().numpy(), want_img) and np.array_equal(sets[0]['mtiles'].cpu().numpy(), want_mask)
    assert np.array_equal(sets[0]['sums'].cpu().numpy(), want_sums) and np.array_equal(sets[0]['hist'].cpu().numpy(), want_hist)
    out['matches_restatement'] = True

    for name, fn, nbytes in (('extract', cut, 2 * moved), ('tile_stats', stats, moved)):
        one = timed(lambda i: fn(sets[0]), a.launches, a.warmup)
        rot = timed(lambda i: fn(sets[i % a.sets]), a.launches, a.warmup)
        out[name] = {'bytes': nbytes, 'one_set_us': one * 1e6, 'one_set_TBps': nbytes / one / 1e12, 'rotating_sets': a.sets,
                     'rotating_us': rot * 1e6, 'rotating_TBps': nbytes / rot / 1e12, 'rotating_share_of_achievable_hbm': nbytes / rot / HBM_ACHIEVABLE}

    if a.band_rows:
        out['extract_by_band_rows'] = {}
        for band in [int(b) for b in a.band_rows.split(',')]:
            rot = timed(lambda i: cut(sets[i % a.sets], band), a.launches, a.warmup)
            out['extract_by_band_rows'][str(band)] = {'rotating_us': rot * 1e6, 'rotating_TBps': 2 * moved / rot / 1e12}

    pal = rs.randint(0, 256, (NCLS, 3)).astype(np.uint8)
    rgb_mask = pal[cls]
    times = []
    for k in range(4):
        t0 = time.perf_counter()
        ex = dataset.extract_photo(image, rgb_mask, pal, tile=TILE)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert ex.geometry['n'] == n
    out['extract_photo_end_to_end_ms'] = {'first_call': times[0] * 1e3, 'best_of_next_3': min(times[1:]) * 1e3}

    torch.set_num_threads(min(16, torch.get_num_threads()))
    cpu = []
    for _ in range(a.cpu_runs):
        t0 = time.perf_counter()
        ti, tm = unfold_tiles(planar, TILE, STRIDE), unfold_tiles(cls, TILE, STRIDE)
        tile_sums_np(ti, tm, NCLS)
        cpu.append(time.perf_counter() - t0)
    out['cpu_restatement'] = {'threads': torch.get_num_threads(), 'runs': a.cpu_runs, 'seconds_min': min(cpu), 'seconds_max': max(cpu),
                              'what': 'tests/test_cpu_dataset.py unfold_tiles (torch.unfold + reshape) of image and mask, then tile_sums_np '
                                      '(numpy int64 sums and bincount)'}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
