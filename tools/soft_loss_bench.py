"""The loss head against soft targets: kernel time of the statistics pass, of the backward pass and of the pair at the
benchmark's loss shape (32 x 512^2 pixels, 9 classes, pitch 12, class weights, a weight per pixel) for

    w             pylc_multiloss_stats_w + _bwd_w on a uint8 target: the yardstick
    ls            pylc_multiloss_stats_ls + _bwd_ls on the same target, smoothing 0.1
    soft_planar   pylc_multiloss_stats_soft + _bwd_soft on a planar float32 [B,C,H,W] probability volume
    soft_nhwc     the same volume channels-last
    soft_logits   teacher logits in a planar volume, softened in the kernel at T = 1.7

all on the same logits.  Results are compared first (_ls with smoothing 0 and a one-hot volume give the statistics of _w bit for bit; the
channels-last volume gives the bits of the planar one).  Then everything is timed in ONE process between device events after warm-up launches,
the variants taking turns within a round (--rounds of them, the median is reported), each launch on the next of --sets buffer sets, as
tools/loss_ignore_bench.py does.  Next to every time stands the byte model of the path -- per pixel the logits row (pitch floats), the target
(1 byte, or the 4C-byte soft row) and the weight, in the backward also the gradient row (pitch floats) -- and the rate it gives.

    python tools/soft_loss_bench.py [--batch B] [--launches N] [--warmup W] [--rounds R] [--sets K] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from loss_ignore_bench import C, PITCH, TILE, timed      # noqa: E402  (the same shape and the same clock)


def byte_model(soft):
    """bytes per pixel of (statistics, backward): logits row + target or soft row + weight, and in the backward + the gradient row"""
    target = 4 * C if soft else 1
    fwd = 4 * PITCH + target + 4
    return fwd, fwd + 4 * PITCH


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
    b, h, w = a.batch, TILE, TILE
    n = b * h * w
    rs = np.random.RandomState(0)
    cells = TILE // 64
    cls = torch.from_numpy(rs.randint(0, C, (b, cells, cells))).repeat_interleave(64, 1).repeat_interleave(64, 2)
    t = cls.to(torch.uint8).to(dev)
    u = (torch.rand(n, device=dev) * 0.9 + 0.1)
    cw = torch.rand(C, device=dev) + 0.5
    probs = torch.softmax(torch.randn(b, C, h, w, device=dev) * 2, 1)
    probs_nhwc = probs.contiguous(memory_format=torch.channels_last)
    teacher = torch.randn(b, C, h, w, device=dev) * 2
    onehot = torch.nn.functional.one_hot(cls, C).permute(0, 3, 1, 2).float().contiguous().to(dev)
    sets = [(torch.randn(n, PITCH, device=dev) * 3, torch.empty(n, PITCH, device=dev)) for _ in range(a.sets)]
    stats = torch.empty(3 + 3 * C, device=dev)
    ws = torch.empty(lib.pylc_multiloss_workspace_floats(n, C), device=dev)
    amax = torch.zeros(1, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    st = stream()

    def hard(eps):
        def fwd(i):
            z, dl = sets[i % len(sets)]
            if eps is None:
                check(lib.pylc_multiloss_stats_w(ptr(z), PITCH, ptr(t), 1, n, C, 255, ptr(cw), ptr(u), ptr(stats), ptr(ws), ptr(bad), st))
            else:
                check(lib.pylc_multiloss_stats_ls(ptr(z), PITCH, ptr(t), 1, n, C, 255, ptr(cw), ptr(u), eps, ptr(stats), ptr(ws), ptr(bad), st))

        def bwd(i):
            z, dl = sets[i % len(sets)]
            if eps is None:
                check(lib.pylc_multiloss_bwd_w(ptr(z), PITCH, ptr(t), 1, n, C, 255, ptr(cw), ptr(u), ptr(stats), 0.5, 0.5, 0.5, None, ptr(dl), PITCH,
                                               ptr(amax), st))
            else:
                check(lib.pylc_multiloss_bwd_ls(ptr(z), PITCH, ptr(t), 1, n, C, 255, ptr(cw), ptr(u), eps, ptr(stats), 0.5, 0.5, 0.5, None, ptr(dl),
                                                PITCH, ptr(amax), st))
        return fwd, bwd

    def soft(vol, kind, inv_t):
        strides = [int(v) for v in vol.stride()]

        def fwd(i):
            z, dl = sets[i % len(sets)]
            check(lib.pylc_multiloss_stats_soft(ptr(z), PITCH, n, h, w, C, ptr(vol), *strides, kind, inv_t, ptr(cw), ptr(u), ptr(stats), ptr(ws),
                                                ptr(bad), st))

        def bwd(i):
            z, dl = sets[i % len(sets)]
            check(lib.pylc_multiloss_bwd_soft(ptr(z), PITCH, n, h, w, C, ptr(vol), *strides, kind, inv_t, ptr(cw), ptr(u), ptr(stats), 0.5, 0.5, 0.5,
                                              None, ptr(dl), PITCH, ptr(amax), st))
        return fwd, bwd
    variants = {'w': hard(None), 'ls': hard(0.1), 'soft_planar': soft(probs, 0, 1.0), 'soft_nhwc': soft(probs_nhwc, 0, 1.0),
                'soft_logits': soft(teacher, 1, 1.0 / 1.7)}
    is_soft = {'w': False, 'ls': False, 'soft_planar': True, 'soft_nhwc': True, 'soft_logits': True}

    def result(pair):
        pair[0](0)
        pair[1](0)
        return stats.clone(), sets[0][1].clone(), amax.clone()

    def same(p, q, parts):
        return all(torch.equal(p[i].view(torch.int32), q[i].view(torch.int32)) for i in parts)
    ref = result(variants['w'])
    if not same(result(hard(0.0)), ref, (0,)) or not same(result(soft(onehot, 0, 1.0)), ref, (0,)):
        raise SystemExit('smoothing 0 or a one-hot volume differs from the statistics of the _w entry points')
    if not same(result(variants['soft_nhwc']), result(variants['soft_planar']), (0, 1, 2)):
        raise SystemExit('the channels-last volume differs from the planar one')
    if int(bad) != 0:
        raise SystemExit('%d pixels were counted as bad' % int(bad))
    passes = {}
    for k, (fwd, bwd) in variants.items():
        passes[k + '.stats'], passes[k + '.bwd'] = fwd, bwd
        passes[k + '.both'] = lambda i, fwd=fwd, bwd=bwd: (fwd(i), bwd(i))
    times = {k: [] for k in passes}
    for _ in range(a.rounds):
        for k, fn in passes.items():
            times[k].append(timed(fn, a.launches, a.warmup))
    us = {k: float(np.median(v)) * 1e6 for k, v in times.items()}
    table = {}
    for k in variants:
        f, bw = byte_model(is_soft[k])
        for part, nbytes in (('stats', f), ('bwd', bw), ('both', f + bw)):
            key = '%s.%s' % (k, part)
            table[key] = {'us': us[key], 'bytes': nbytes * n, 'GB_per_s': nbytes * n / us[key] * 1e-3, 'over_w': us[key] / us['w.' + part],
                          'bytes_over_w': nbytes / dict(zip(('stats', 'bwd'), byte_model(False)), both=sum(byte_model(False)))[part]}
    out = {'n_classes': C, 'pitch': PITCH, 'pixels': n, 'launches': a.launches, 'warmup': a.warmup, 'rounds': a.rounds, 'sets': a.sets,
           'lib': os.path.relpath(L.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'paths': table, 'us_min_max': {k: [min(v) * 1e6, max(v) * 1e6] for k, v in times.items()}}
    lines = [json.dumps(out), '%-20s %10s %14s %10s %10s %12s' % ('path', 'us', 'model bytes', 'GB/s', 'time / w', 'bytes / w')]
    for k, r in table.items():
        lines.append('%-20s %10.1f %14d %10.1f %10.3f %12.3f' % (k, r['us'], r['bytes'], r['GB_per_s'], r['over_w'], r['bytes_over_w']))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
