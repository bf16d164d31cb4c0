"""Connected-region labelling and the small-region sieve on one 3072 x 4096 mask of 9 classes, against the host
route they replace.

Inputs, generated on the device from a seed:
    blobs      argmax of 9 box-smoothed noise fields, then 1 % of the pixels replaced by random classes (a land-cover mask with speckle)
    constant   one value everywhere (one region of 12.6 million pixels: the worst case for anything that counts per region)
    random     uniformly random classes (millions of regions of a few pixels: the worst case for the union-find)

Entry points (connectivity 4, min_size 16, the neighbour rule): pylc_label_regions, pylc_region_sizes, pylc_sieve_regions, and their sum
`device_route`.  Timed in ONE process between device events after --warmup rounds, the inputs and entry points taking turns within a round
(--rounds, the median is reported).  Bytes are the passes' streaming bytes per pixel, data-dependent gathers and atomics left out:
    label   9 B   tile pass: 1 B mask in, 4 B labels out; flatten pass: 4 B labels in (it writes only where a label changes)
    sizes   8 B   4 B zero fill, 4 B labels in
    sieve  18 B   8 B zero fill of the workspace; bids: 4 B labels in; apply: 1 B mask + 4 B labels in, 1 B out

The host route of the same run, once per input: mask.cpu(), scipy.ndimage.label per class plus the numpy bookkeeping of the same sieve
rule, and the copy back -- what a user had to write before.  Its result is compared with the device's bit for bit.  Without scipy that
part is skipped with a note.

    python tools/regions_bench.py [--rounds R] [--warmup W] [--min-size M] [--no-host] [--out FILE]
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, C = 3072, 4096, 9


def make_inputs(dev, seed=0):
    import torch.nn.functional as F
    g = torch.Generator(device=dev).manual_seed(seed)
    f = torch.randn((C, 1, H, W), device=dev, generator=g)
    for _ in range(2):                               # a 17-wide box twice: close to a Gaussian of sigma 7
        f = F.avg_pool2d(f, 17, 1, 8, count_include_pad=False)
    blobs = f[:, 0].argmax(0).to(torch.uint8)
    del f
    hit = torch.rand((H, W), device=dev, generator=g) < 0.01
    rnd = torch.randint(0, C, (H, W), device=dev, generator=g, dtype=torch.uint8)
    blobs = torch.where(hit, rnd, blobs)
    rnd2 = torch.randint(0, C, (H, W), device=dev, generator=g, dtype=torch.uint8)
    return {'blobs': blobs.contiguous(), 'constant': torch.full((H, W), 3, device=dev, dtype=torch.uint8), 'random': rnd2}


def host_route(m, min_size):
    """numpy uint8 [H,W] -> sieved mask: scipy.ndimage.label per class, then the neighbour rule in numpy"""
    from scipy import ndimage as ndi
    h, w = m.shape
    lab = np.zeros((h, w), np.int64)                 # region ids 1..n over all classes
    n = 0
    for v in np.unique(m):
        comp, k = ndi.label(m == v)
        sel = comp > 0
        lab[sel] = comp[sel] + n
        n += k
    size = np.bincount(lab.reshape(-1), minlength=n + 1)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    root = np.concatenate([[0], np.asarray(ndi.minimum(idx, lab, np.arange(1, n + 1))).astype(np.int64)])
    small = size[lab] < min_size
    best = np.zeros(n + 1, np.uint64)
    for a, b in (((slice(0, h), slice(0, w - 1)), (slice(0, h), slice(1, w))), ((slice(0, h - 1), slice(0, w)), (slice(1, h), slice(0, w)))):
        for p, q in ((a, b), (b, a)):
            cond = small[p] & (lab[q] != lab[p]) & (size[lab[q]] >= min_size)
            lq = lab[q][cond]
            key = (size[lq].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - root[lq].astype(np.uint64))
            np.maximum.at(best, lab[p][cond], key)
    win = best[lab]
    take = small & (win > 0)
    out = m.copy()
    out[take] = m.reshape(-1)[(np.uint64(0xFFFFFFFF) - (win[take] & np.uint64(0xFFFFFFFF))).astype(np.int64)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--min-size', type=int, default=16)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import lib as L, regions
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    dev = torch.device('cuda:0')
    inputs = make_inputs(dev)
    n = H * W
    st = stream()
    labels = {k: torch.empty((H, W), device=dev, dtype=torch.int32) for k in inputs}
    sizes = {k: torch.empty((n,), device=dev, dtype=torch.int32) for k in inputs}
    outs = {k: torch.empty((H, W), device=dev, dtype=torch.uint8) for k in inputs}
    best = torch.empty((n,), device=dev, dtype=torch.int64)

    def label(k):
        check(lib.pylc_label_regions(ptr(inputs[k]), H, W, 4, -1, ptr(labels[k]), st))

    def size(k):
        check(lib.pylc_region_sizes(ptr(labels[k]), n, ptr(sizes[k]), st))

    def sieve(k):
        check(lib.pylc_sieve_regions(ptr(inputs[k]), ptr(labels[k]), ptr(sizes[k]), H, W, a.min_size, -1, -1, ptr(best), ptr(outs[k]), None, st))

    def span(fns, k):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
        ev[0].record()
        for f, e in zip(fns, ev[1:]):
            f(k)
            e.record()
        torch.cuda.synchronize()
        return [p.elapsed_time(q) * 1e-3 for p, q in zip(ev, ev[1:])]

    times = {k: [] for k in inputs}
    for r in range(a.warmup + a.rounds):
        for k in inputs:
            t = span([label, size, sieve], k)
            if r >= a.warmup:
                times[k].append(t)
    for k in inputs:                                 # the public route gives the same bytes
        if not torch.equal(regions.sieve(inputs[k], a.min_size), outs[k]):
            raise SystemExit('regions.sieve differs from the entry points on %s' % k)
    bytes_ = {'label': 9 * n, 'sizes': 8 * n, 'sieve': 18 * n}
    bytes_['device_route'] = sum(bytes_.values())
    res = {}
    for k in inputs:
        med = np.median(np.asarray(times[k]), axis=0)
        us = {'label': float(med[0]) * 1e6, 'sizes': float(med[1]) * 1e6, 'sieve': float(med[2]) * 1e6}
        us['device_route'] = sum(us.values())
        tot = np.asarray(times[k]).sum(1)
        res[k] = {'regions': int((sizes[k] > 0).sum()), 'largest_region': int(sizes[k].max()), 'pixels_changed': int((outs[k] != inputs[k]).sum()),
                  'us': us, 'us_total_min_max': [float(tot.min()) * 1e6, float(tot.max()) * 1e6],
                  'gb_per_s': {p: bytes_[p] / us[p] * 1e-3 for p in us}}
    host = None
    try:
        import scipy  # noqa: F401
    except ImportError:
        host = 'skipped: scipy is not installed on this box'
    if a.no_host:
        host = 'skipped: --no-host'
    if host is None:
        host = {}
        for k in inputs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = inputs[k].cpu().numpy()
            t1 = time.perf_counter()
            o = host_route(m, a.min_size)
            t2 = time.perf_counter()
            back = torch.from_numpy(o).to(dev)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            host[k] = {'s': t3 - t0, 's_to_host': t1 - t0, 's_label_and_sieve': t2 - t1, 's_to_device': t3 - t2,
                       'same_bytes_as_device': bool(torch.equal(back, outs[k])),
                       'host_over_device': (t3 - t0) * 1e6 / res[k]['us']['device_route']}
    out = {'image': [H, W], 'n_classes': C, 'connectivity': 4, 'min_size': a.min_size, 'fill': 'neighbour', 'rounds': a.rounds, 'warmup': a.warmup,
           'lib': os.path.relpath(L.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
           'device': torch.cuda.get_device_name(0), 'host': platform.node(), 'host_threads': torch.get_num_threads(),
           'bytes': bytes_, 'inputs': res, 'host_route': host}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
