"""The per-step augmenter (pylc_batch_augment, csrc/batch_augment.hip) at the size of a training batch: 32 samples
of 512^2 RGB with masks out of 54 resident source tiles, scale 0.5-2, rotation +-10 degrees, mirror 0.5, tone tables on, on one MI355X.

The result is first compared with the integer statement (tests/_batch_augment.py), every byte.  Then warm-up launches and N timed
launches back to back between two device events, rotating over SETS sets of sources and outputs, for
  * the launch as TileSet.batches(augment=) makes it (host indices and matrices as kernel arguments, constant border, masks);
  * the same with device indices and matrices, with the reflected border, with a weight map as well, without tone tables;
  * a band_rows sweep;
  * the yardsticks on the SAME tile count in the same run: pylc_extract_tiles cutting 32 tiles (and the 54 of the recorded
    photograph), and pylc_augment_tiles (the reference's offline transform) making 32 copies.
Reports us per launch, useful bytes (m * oh * ow * (C + 1) written plus the same read) / time, and the ratios.

    python tools/batch_augment_bench.py [--launches N] [--warmup W] [--sets K] [--band-rows 4,8,16,32,64] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

N_SRC, M, C, TILE, NCLS = 54, 32, 3, 512, 9
AUG = dict(scale=(0.5, 2.0), rotate=10.0, flip=0.5, brightness=(-20, 20), contrast=(0.8, 1.25), gamma=(0.8, 1.25))
FILL, IGNORE = [124, 116, 104], 255


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
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--sets', type=int, default=6)
    ap.add_argument('--band-rows', default='4,8,16,32,64,128')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import dataset, lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    from tests import _batch_augment as S
    assert torch.cuda.is_available(), 'needs the MI355X'
    L.init()
    dev = torch.device('cuda:0')
    img, mask, weights = S.sources(N_SRC, C, TILE, TILE, 1, n_classes=NCLS)
    rs = np.random.RandomState(2)
    src = rs.randint(0, N_SRC, M).astype(np.int32)
    mats, luts = dataset.batch_augment_params(rs, M, (TILE, TILE), (TILE, TILE), **AUG)
    fill = np.array(FILL, np.uint8)
    moved = M * TILE * TILE * (C + 1)
    out = {'src_tiles': N_SRC, 'm': M, 'ch': C, 'tile': TILE, 'augment': {k: list(v) if isinstance(v, tuple) else v for k, v in AUG.items()},
           'launches': a.launches, 'warmup': a.warmup, 'rotating_sets': a.sets, 'bytes_written': moved, 'bytes_read_counted': moved}

    d_src, d_mats, d_luts = torch.from_numpy(src).to(dev), torch.from_numpy(mats).to(dev), torch.from_numpy(luts).to(dev)
    sets = []
    for _ in range(a.sets):
        sets.append(dict(img=torch.from_numpy(img).to(dev), mask=torch.from_numpy(mask).to(dev), w=torch.from_numpy(weights).to(dev),
                         out=torch.empty((M, C, TILE, TILE), device=dev, dtype=torch.uint8),
                         mout=torch.empty((M, TILE, TILE), device=dev, dtype=torch.uint8),
                         wout=torch.empty((M, TILE, TILE), device=dev, dtype=torch.float32)))

    def aug(s, border=0, device_params=False, with_w=False, lut=True, band_rows=0):
        check(lib.pylc_batch_augment(ptr(s['img']), ptr(s['mask']), ptr(s['w']) if with_w else None, N_SRC, C, TILE, TILE,
                                     ptr(d_src) if device_params else src.ctypes.data, ptr(d_mats) if device_params else mats.ctypes.data,
                                     ptr(d_luts) if lut else None, M, TILE, TILE, border, fill.ctypes.data, IGNORE, band_rows, ptr(s['out']),
                                     ptr(s['mout']), ptr(s['wout']) if with_w else None, stream()))

    # the result first: against the statement, every byte
    aug(sets[0], with_w=True)
    want = S.batch_augment_np(img, mask, weights, src, mats, luts, (TILE, TILE), 'constant', FILL, IGNORE)
    got = [sets[0][k].cpu().numpy() for k in ('out', 'mout', 'wout')]
    assert all(np.array_equal(g, w_) for g, w_ in zip(got, want))
    out['matches_statement'] = True
    out['share_of_output_out_of_frame'] = float((want[1] == IGNORE).mean())

    def rates(sec, nbytes=2 * moved):
        return {'us': sec * 1e6, 'TBps': nbytes / sec / 1e12}

    rot = lambda **kw: rates(timed(lambda i: aug(sets[i % a.sets], **kw), a.launches, a.warmup))
    out['batch_augment'] = rot()
    out['batch_augment_one_set'] = rates(timed(lambda i: aug(sets[0]), a.launches, a.warmup))
    out['batch_augment_device_params'] = rot(device_params=True)
    out['batch_augment_reflect'] = rot(border=1)
    out['batch_augment_with_weights'] = rot(with_w=True)
    out['batch_augment_no_lut'] = rot(lut=False)
    out['batch_augment_again'] = rot()
    out['batch_augment_by_band_rows'] = {str(b): rot(band_rows=b) for b in [int(b) for b in a.band_rows.split(',') if b]}

    # the yardsticks: the reference's offline transform on the same tile count ...
    params = [dataset.augment_params(j, TILE) for j in range(4)]
    d_minv = torch.from_numpy(np.stack([params[k % 4][0] for k in range(M)])).to(dev)
    d_shift = torch.from_numpy(np.array([params[k % 4][1] for k in range(M)], np.int32)).to(dev)

    def offline(i):
        s = sets[i % a.sets]
        check(lib.pylc_augment_tiles(ptr(s['img']), ptr(s['mask']), N_SRC, C, TILE, ptr(d_src), ptr(d_minv), ptr(d_shift), M, 0, ptr(s['out']),
                                     ptr(s['mout']), NCLS, None, None, stream()))
    out['augment_tiles_same_tile_count'] = rates(timed(offline, a.launches, a.warmup))
    del sets

    # ... and the tile cutter on 32 tiles and on the 54 of the recorded photograph
    out['extract_tiles'] = {}
    for rows, cols in ((4, 8), (9, 6)):
        n = rows * cols
        h, w = rows * TILE + 332, cols * TILE + 381
        cut_sets = []
        for _ in range(a.sets):
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
        sec = timed(cut, a.launches, a.warmup)
        out['extract_tiles'][str(n)] = dict(rates(sec, 2 * n * TILE * TILE * (C + 1)), image_hw=[h, w])
        del cut_sets
    us = out['batch_augment']['us']
    out['batch_augment_over_extract_same_tile_count'] = us / out['extract_tiles'][str(M)]['us']
    out['batch_augment_over_augment_tiles'] = us / out['augment_tiles_same_tile_count']['us']
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
