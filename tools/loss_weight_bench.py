"""The loss head with a weight per pixel, and the border-weight map: kernel time of statistics + backward at the
benchmark's loss shape (32 x 512^2 pixels, 9 classes, pitch 12, weighted, uint8 targets, nothing ignored) for

    parent_ex   pylc_multiloss_stats_ex + _bwd_ex of another build of the library (--parent-lib: the parent commit's), loaded next to this one
    ex          the same entry points of this library: the same instantiations, so the pair must agree within its round-to-round spread
    w_null      the _w entry points with pixel_weights = NULL (they dispatch to the kernels of _ex)
    w_border    _w with a border map (boundary.border_weights of the target, radius 10, the default profile)
    w_zero30    _w with a {0, 1} map, about 30 % zeros in 64 x 64 blobs

and of the map itself at radius 3 and 10

    map_fused_R   pylc_boundary_weights (column pass + row pass with the lookup epilogue)
    map_two_R     pylc_boundary_distance + pylc_weights_from_d2 (the int32 map written and read back)

Results are compared first (parent_ex == ex == w_null == _w with a map of ones, bit for bit; the fused map == the two-step map).  Then
everything is timed in ONE process between device events after warm-up launches, the variants taking turns within a round (--rounds of
them, the median is reported), each launch on the next of --sets buffer sets, as tools/loss_ignore_bench.py does.

    python tools/loss_weight_bench.py [--parent-lib FILE] [--batch B] [--launches N] [--warmup W] [--rounds R] [--sets K] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from loss_ignore_bench import C, PITCH, TILE, timed      # noqa: E402  (the same shape and the same clock)


def other_build(path, signatures):
    """another build of the library with the _ex entry points bound as this one binds them"""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ('pylc_init', 'pylc_multiloss_stats_ex', 'pylc_multiloss_bwd_ex'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = signatures[name]
    if lib.pylc_init() != 0:
        raise SystemExit('pylc_init of %s failed' % path)
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sets', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import boundary, lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    dev = torch.device('cuda:0')
    parent = other_build(a.parent_lib, L.SIGNATURES) if a.parent_lib else None
    n = a.batch * TILE * TILE
    rs = np.random.RandomState(0)
    cells = TILE // 64
    cls = torch.from_numpy(rs.randint(0, C, (a.batch, cells, cells))).repeat_interleave(64, 1).repeat_interleave(64, 2)
    blobs = torch.from_numpy(rs.rand(a.batch, cells, cells) < 0.3).repeat_interleave(64, 1).repeat_interleave(64, 2)
    t = cls.to(torch.uint8).to(dev)
    maps = {'ones': torch.ones(n, device=dev), 'border': boundary.border_weights(t, 10).reshape(-1), 'zero30': (~blobs).float().reshape(-1).to(dev)}
    cw = torch.rand(C, device=dev) + 0.5
    sets = [(torch.randn(n, PITCH, device=dev) * 3, torch.empty(n, PITCH, device=dev)) for _ in range(a.sets)]
    stats = torch.empty(3 + 3 * C, device=dev)
    ws = torch.empty(lib.pylc_multiloss_workspace_floats(n, C), device=dev)
    amax = torch.zeros(1, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    st = stream()

    def ex(which):
        def run(i):
            z, dl = sets[i % len(sets)]
            check(which.pylc_multiloss_stats_ex(ptr(z), PITCH, ptr(t), 1, n, C, 255, ptr(cw), ptr(stats), ptr(ws), ptr(bad), st))
            check(which.pylc_multiloss_bwd_ex(ptr(z), PITCH, ptr(t), 1, n, C, 255, ptr(cw), ptr(stats), 0.5, 0.5, 0.5, None, ptr(dl), PITCH, ptr(amax),
                                              st))
        return run

    def weighted(u):
        def run(i):
            z, dl = sets[i % len(sets)]
            check(lib.pylc_multiloss_stats_w(ptr(z), PITCH, ptr(t), 1, n, C, 255, ptr(cw), ptr(u), ptr(stats), ptr(ws), ptr(bad), st))
            check(lib.pylc_multiloss_bwd_w(ptr(z), PITCH, ptr(t), 1, n, C, 255, ptr(cw), ptr(u), ptr(stats), 0.5, 0.5, 0.5, None, ptr(dl), PITCH,
                                           ptr(amax), st))
        return run
    variants = {'ex': ex(lib), 'w_null': weighted(None), 'w_border': weighted(maps['border']), 'w_zero30': weighted(maps['zero30'])}
    if parent is not None:
        variants = dict({'parent_ex': ex(parent)}, **variants)
    ref = None
    for name, fn in list(variants.items())[:-2] + [('w_ones', weighted(maps['ones']))]:
        fn(0)
        got = (stats.clone(), sets[0][1].clone(), amax.clone())
        if ref is not None and not all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(ref, got)):
            raise SystemExit('%s differs from the _ex entry points' % name)
        ref = got
    # the map itself
    b, h, w = t.shape
    bws = torch.empty(lib.pylc_boundary_workspace_bytes(b, h, w) // 4, device=dev, dtype=torch.int32)
    d2 = torch.empty((b, h, w), device=dev, dtype=torch.int32)
    out_f, out_t = torch.empty((b, h, w), device=dev), torch.empty((b, h, w), device=dev)
    for radius in (3, 10):
        table = torch.from_numpy(boundary.border_profile(radius)).to(dev)

        def fused(i, radius=radius, table=table):
            check(lib.pylc_boundary_weights(ptr(t), b, h, w, radius, -1, ptr(table), ptr(out_f), ptr(bws), st))

        def two(i, radius=radius, table=table):
            check(lib.pylc_boundary_distance(ptr(t), b, h, w, radius, -1, None, ptr(d2), ptr(bws), st))
            check(lib.pylc_weights_from_d2(ptr(d2), n, radius, ptr(table), ptr(out_t), st))
        fused(0)
        two(0)
        if not torch.equal(out_f.view(torch.int32), out_t.view(torch.int32)):
            raise SystemExit('pylc_boundary_weights differs from distance + lookup at radius %d' % radius)
        variants['map_fused_%d' % radius], variants['map_two_%d' % radius] = fused, two
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, a.launches, a.warmup))
    us = {k: float(np.median(v)) * 1e6 for k, v in times.items()}
    out = {'n_classes': C, 'pitch': PITCH, 'pixels': n, 'launches': a.launches, 'warmup': a.warmup, 'rounds': a.rounds, 'sets': a.sets,
           'zero_share_30': float(blobs.float().mean()), 'border_map_mean': float(maps['border'].mean()), 'lib': L.LIB_PATH,
           'parent_lib': a.parent_lib, 'us': us, 'us_min_max': {k: [min(v) * 1e6, max(v) * 1e6] for k, v in times.items()},
           'w_border_over_ex': us['w_border'] / us['ex']}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
