"""The loss head with and without an ignore label: kernel time of statistics + backward at the benchmark's loss
shape (32 x 512^2 pixels, 9 classes, pitch 12, weighted) for

    old        pylc_multiloss_stats + pylc_multiloss_bwd on int64 targets (what Model.train runs without Meta.ignore_index)
    ex_i64_0   the _ex entry points, int64 targets, nothing ignored
    ex_u8_0    the _ex entry points, uint8 targets, nothing ignored
    ex_u8_30   uint8 targets, about 30 % of the pixels ignored in 64 x 64 blobs
    ex_u8_100  uint8 targets, every pixel ignored

Results are compared first (old == ex_i64_0 == ex_u8_0 bit for bit).  Then everything is timed in ONE process between device events after
warm-up launches, the variants taking turns within a round (--rounds of them, the median is reported), each launch on the next of --sets
buffer sets (a set is 403 MB of logits plus as much gradient: nothing stays in the 256 MB last-level cache either way).  A library without the
_ex entry points (an older build, PYLC_LIB=) runs `old` alone.

    python tools/loss_ignore_bench.py [--batch B] [--launches N] [--warmup W] [--rounds R] [--sets K] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, PITCH, TILE = 9, 12, 512


def timed(fn, launches, warmup):
    for i in range(warmup):
        fn(i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sets', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    dev = torch.device('cuda:0')
    has_ex = hasattr(lib, 'pylc_multiloss_stats_ex')
    n = a.batch * TILE * TILE
    rs = np.random.RandomState(0)
    cells = TILE // 64
    cls = torch.from_numpy(rs.randint(0, C, (a.batch, cells, cells))).repeat_interleave(64, 1).repeat_interleave(64, 2).reshape(-1)
    blobs = torch.from_numpy(rs.rand(a.batch, cells, cells) < 0.3).repeat_interleave(64, 1).repeat_interleave(64, 2).reshape(-1)
    t30 = torch.where(blobs, torch.full_like(cls, 255), cls)
    targets = {'i64': cls.to(dev), 'u8_0': cls.to(torch.uint8).to(dev), 'u8_30': t30.to(torch.uint8).to(dev),
               'u8_100': torch.full((n,), 255, dtype=torch.uint8, device=dev)}
    cw = torch.rand(C, device=dev) + 0.5
    sets = [(torch.randn(n, PITCH, device=dev) * 3, torch.empty(n, PITCH, device=dev)) for _ in range(a.sets)]
    stats = torch.empty(3 + 3 * C, device=dev)
    ws = torch.empty(lib.pylc_multiloss_workspace_floats(n, C), device=dev)
    amax = torch.zeros(1, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    st = stream()

    def old(i):
        z, dl = sets[i % len(sets)]
        check(lib.pylc_multiloss_stats(ptr(z), PITCH, ptr(targets['i64']), n, C, ptr(cw), ptr(stats), ptr(ws), st))
        check(lib.pylc_multiloss_bwd(ptr(z), PITCH, ptr(targets['i64']), n, C, ptr(cw), ptr(stats), float(n), 0.5, 0.5, 0.5, None, ptr(dl), PITCH,
                                     ptr(amax), st))

    def ex(key):
        t = targets[key]

        def run(i):
            z, dl = sets[i % len(sets)]
            check(lib.pylc_multiloss_stats_ex(ptr(z), PITCH, ptr(t), t.element_size(), n, C, 255, ptr(cw), ptr(stats), ptr(ws), ptr(bad), st))
            check(lib.pylc_multiloss_bwd_ex(ptr(z), PITCH, ptr(t), t.element_size(), n, C, 255, ptr(cw), ptr(stats), 0.5, 0.5, 0.5, None, ptr(dl),
                                            PITCH, ptr(amax), st))
        return run
    variants = {'old': old}
    if has_ex:
        variants.update({'ex_i64_0': ex('i64'), 'ex_u8_0': ex('u8_0'), 'ex_u8_30': ex('u8_30'), 'ex_u8_100': ex('u8_100')})
        ref = None
        for name in ('old', 'ex_i64_0', 'ex_u8_0'):
            variants[name](0)
            got = (stats.clone(), sets[0][1].clone(), amax.clone())
            if ref is not None and not all(torch.equal(p, q) for p, q in zip(ref, got)):
                raise SystemExit('%s differs from the entry points without _ex' % name)
            ref = got
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, a.launches, a.warmup))
    out = {'n_classes': C, 'pitch': PITCH, 'pixels': n, 'launches': a.launches, 'warmup': a.warmup, 'rounds': a.rounds, 'sets': a.sets,
           'ignored_share_30': float(blobs.float().mean()), 'lib': L.LIB_PATH,
           'us': {k: float(np.median(v)) * 1e6 for k, v in times.items()},
           'us_min_max': {k: [min(v) * 1e6, max(v) * 1e6] for k, v in times.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
