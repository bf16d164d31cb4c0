"""The augmentation transform (pylc_augment_tiles, csrc/augment.hip) at the size of the reference's recorded photograph: 54 seeded uint8 RGB
tiles of 512^2 with class-index masks, 4 augmented copies of each (the largest rate Augmentor.optimize gives), m = 216 copies per launch,
on one MI355X.

Warm-up launches, then N timed launches back to back between two device events, on ONE set of buffers and rotating over SETS sets of
sources and outputs (one set's outputs alone are 226 MB: with several sets every launch reads and writes HBM).  Reports us per launch and
useful bytes / time -- m * t^2 * (C + 1) written plus the same read -- next to the achievable HBM rate (MI355X: 6.3 TB/s), and
  * the statistics fused into the launch against the launch without them followed by pylc_tile_stats on its output, alternating A / B;
  * a band_rows sweep;
  * the yardstick: pylc_extract_tiles cutting 54 tiles (the recorded photograph) and 216 tiles (the same tile count) out of an image;
  * the numpy restatement of tests/test_cpu_augment.py for the same 216 copies on 16 host threads.
The result is first compared with the restatement, one copy per copy index.

    python tools/augment_bench.py [--launches N] [--warmup W] [--sets K] [--rounds R] [--band-rows 4,8,16,32,64] [--cpu-copies M] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

N_SRC, COPIES, C, TILE, NCLS = 54, 4, 3, 512, 9
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
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--sets', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=3, help='A / B alternations of fused against separate statistics')
    ap.add_argument('--band-rows', default='4,8,16,32,64,128')
    ap.add_argument('--cpu-copies', type=int, default=N_SRC * COPIES, help='copies the numpy restatement is timed on (scaled to 216)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import dataset, lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    from tests.test_cpu_augment import augment_np, augment_params_np, tiles_np
    assert torch.cuda.is_available(), 'needs the MI355X'
    L.init()
    dev = torch.device('cuda:0')
    img, mask = tiles_np(1, N_SRC, C, TILE, NCLS)
    mask[mask == 255] = 0
    src, copy = dataset.oversample_layout(np.full(N_SRC, COPIES))
    src, copy = src[copy >= 0], copy[copy >= 0]
    m = src.size
    params = [dataset.augment_params(j, TILE) for j in range(COPIES)]
    moved = m * TILE * TILE * (C + 1)
    out = {'src_tiles': N_SRC, 'copies_per_tile': COPIES, 'm': m, 'ch': C, 'tile': TILE, 'n_classes': NCLS, 'launches': a.launches,
           'warmup': a.warmup, 'bytes_written': moved, 'bytes_read_counted': moved, 'hbm_achievable_TBps': HBM_ACHIEVABLE / 1e12}

    d_src = torch.from_numpy(src.astype(np.int32)).to(dev)
    d_minv = torch.from_numpy(np.stack([params[j][0] for j in copy])).to(dev)
    d_shift = torch.from_numpy(np.array([params[j][1] for j in copy], np.int32)).to(dev)
    sets = []
    for _ in range(a.sets):
        sets.append(dict(img=torch.from_numpy(img).to(dev), mask=torch.from_numpy(mask).to(dev),
                         out=torch.empty((m, C, TILE, TILE), device=dev, dtype=torch.uint8),
                         mout=torch.empty((m, TILE, TILE), device=dev, dtype=torch.uint8),
                         sums=torch.zeros((m, 2, C), device=dev, dtype=torch.int64), hist=torch.zeros((m, NCLS + 1), device=dev, dtype=torch.int64)))

    def aug(s, band_rows=0, stats=True):
        check(lib.pylc_augment_tiles(ptr(s['img']), ptr(s['mask']), N_SRC, C, TILE, ptr(d_src), ptr(d_minv), ptr(d_shift), m, band_rows,
                                     ptr(s['out']), ptr(s['mout']), NCLS, ptr(s['sums']) if stats else None, ptr(s['hist']) if stats else None,
                                     stream()))

    def aug_then_stats(s):
        aug(s, 0, False)
        check(lib.pylc_tile_stats(ptr(s['out']), m, C, TILE, ptr(s['mout']), NCLS, 0, ptr(s['sums']), ptr(s['hist']), stream()))

    # the result first: against the restatement, one copy per copy index
    aug(sets[0])
    got_img, got_mask = sets[0]['out'].cpu().numpy(), sets[0]['mout'].cpu().numpy()
    for k in (0, 1 + COPIES, 2 + 2 * COPIES, m - 1):
        want = augment_np(img[src[k]], mask[src[k]], *augment_params_np(int(copy[k]), TILE))
        assert not ((got_img[k] != want['img']) & ~want['near_img'][None]).any() and not ((got_mask[k] != want['mask']) & ~want['near_mask']).any(), k
    x = got_img.astype(np.int64)
    assert np.array_equal(sets[0]['sums'].cpu().numpy(), np.stack([x.sum((2, 3)), (x * x).sum((2, 3))], 1))
    out['matches_restatement'] = True

    def rates(sec):
        return {'us': sec * 1e6, 'TBps': 2 * moved / sec / 1e12, 'share_of_achievable_hbm': 2 * moved / sec / HBM_ACHIEVABLE}

    out['augment_fused_stats'] = {'one_set': rates(timed(lambda i: aug(sets[0]), a.launches, a.warmup)), 'rotating_sets': a.sets,
                                  'rotating': rates(timed(lambda i: aug(sets[i % a.sets]), a.launches, a.warmup))}
    ab = {'fused_us': [], 'separate_us': [], 'no_stats_us': []}
    for _ in range(a.rounds):
        ab['fused_us'].append(timed(lambda i: aug(sets[i % a.sets]), a.launches, a.warmup) * 1e6)
        ab['separate_us'].append(timed(lambda i: aug_then_stats(sets[i % a.sets]), a.launches, a.warmup) * 1e6)
        ab['no_stats_us'].append(timed(lambda i: aug(sets[i % a.sets], 0, False), a.launches, a.warmup) * 1e6)
    out['statistics_ab_rotating'] = ab
    out['augment_by_band_rows'] = {}
    for band in [int(b) for b in a.band_rows.split(',') if b]:
        out['augment_by_band_rows'][str(band)] = rates(timed(lambda i: aug(sets[i % a.sets], band), a.launches, a.warmup))
    del sets[1:]

    # the yardstick: the tile cutter on 54 and on 216 tiles
    out['extract_tiles'] = {}
    for rows, cols in ((9, 6), (18, 12)):
        n = rows * cols
        h, w = rows * TILE + 332, cols * TILE + 381
        cut_sets = []
        for _ in range(a.sets if n == 54 else 2):
            cut_sets.append(dict(img=torch.randint(0, 256, (C, h, w), device=dev, dtype=torch.uint8),
                                 mask=torch.randint(0, NCLS, (h, w), device=dev, dtype=torch.uint8),
                                 tiles=torch.empty((n, C, TILE, TILE), device=dev, dtype=torch.uint8),
                                 mtiles=torch.empty((n, TILE, TILE), device=dev, dtype=torch.uint8),
                                 sums=torch.zeros((n, 2, C), device=dev, dtype=torch.int64),
                                 hist=torch.zeros((n, NCLS + 1), device=dev, dtype=torch.int64)))

        def cut(i):
            s = cut_sets[i % len(cut_sets)]
            check(lib.pylc_extract_tiles(ptr(s['img']), C, h, w, ptr(s['mask']), NCLS, TILE, TILE, 0, n, 0, ptr(s['tiles']), ptr(s['mtiles']),
                                         ptr(s['sums']), ptr(s['hist']), stream()))
        sec = timed(cut, a.launches * 4, a.warmup)
        nbytes = 2 * n * TILE * TILE * (C + 1)
        out['extract_tiles'][str(n)] = {'image_hw': [h, w], 'rotating_sets': len(cut_sets), 'us': sec * 1e6, 'TBps': nbytes / sec / 1e12}
        del cut_sets
    out['augment_over_extract_same_tile_count'] = out['augment_fused_stats']['rotating']['us'] / out['extract_tiles'][str(m)]['us']

    # the numpy restatement of the same copies on 16 host threads
    torch.set_num_threads(1)
    k = min(a.cpu_copies, m)
    if k > 0:
        cpu_params = [augment_params_np(j, TILE) for j in range(COPIES)]
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            list(pool.map(lambda q: augment_np(img[src[q]], mask[src[q]], *cpu_params[int(copy[q])])['img'][0, 0, 0], range(k)))
        sec = time.perf_counter() - t0
        out['cpu_restatement'] = {'threads': 16, 'copies_timed': k, 'seconds': sec, 'seconds_for_216': sec * m / k,
                                  'what': 'tests/test_cpu_augment.py augment_np (numpy) per copy, a pool of 16 threads'}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
