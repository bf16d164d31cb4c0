"""The validation-score launch (pylc_logits_score, csrc/score.hip) at validation size: seeded NHWC logits of 9
classes at pitch 12, 512^2 tiles, batches of 8 and 32, with blob targets (tests/_data.blob_masks) and with uniformly random targets, int64
as Model.eval hands them over, on one MI355X.

  (A) the new launch, counts only;
  (B) what the library offered before for the same matrix: torch.argmax(dim=1) on the same logits (an int64 mask written and read back),
      then pylc_confusion_matrix on that mask and the target.

Both results are compared for equality first.  Then everything is timed in ONE process between device events, after warm-up launches,
alternating A and B for --rounds rounds; the median round is reported.  The yardstick is B: `a_over_b` must not exceed 1 in any case.
Also reported: A's algorithmic bytes, N x (4 x pitch + target bytes), over its time, as a share of the achievable HBM rate (MI355X:
6.3 TB/s).  With --sets K > 1 the launches rotate over K sets of logits and targets (a batch of 8 is 101 MB: one set stays in the
256 MB last-level cache, several do not).

    python tools/score_bench.py [--launches N] [--warmup W] [--rounds R] [--sets K] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

C, PITCH, TILE = 9, 12, 512
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
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='A / B alternations; the median is reported')
    ap.add_argument('--sets', type=int, default=4, help='sets of logits and targets the launches rotate over')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import lib as L, metrics
    from pylc_amd.lib import lib, check, ptr, stream
    from tests import _data as D
    assert torch.cuda.is_available(), 'needs the MI355X'
    L.init()
    dev = torch.device('cuda:0')
    out = {'n_classes': C, 'pitch': PITCH, 'tile': TILE, 'launches': a.launches, 'warmup': a.warmup, 'rounds': a.rounds, 'sets': a.sets,
           'hbm_achievable_TBps': HBM_ACHIEVABLE / 1e12, 'cases': {}}
    for batch in (8, 32):
        n = batch * TILE * TILE
        g = torch.Generator(device=dev).manual_seed(1234 + batch)
        sets = []
        for k in range(a.sets if batch == 8 else max(1, min(a.sets, 2))):
            buf = torch.randn((batch, TILE, TILE, PITCH), device=dev, generator=g)
            sets.append({'x': buf[..., :C].permute(0, 3, 1, 2),                       # [B,C,H,W] with NHWC memory, as a net returns it
                         'blob': D.blob_masks(7 + k, batch, TILE, TILE, C).to(dev), 'random': D.masks(8 + k, batch, TILE, TILE, C).to(dev)})
        counts = torch.zeros(C * C + 1, device=dev, dtype=torch.int64)
        cm = torch.zeros(C * C, device=dev, dtype=torch.int64)
        for kind in ('blob', 'random'):
            def run_a(i):
                s = sets[i % len(sets)]
                check(lib.pylc_logits_score(ptr(s['x']), PITCH, ptr(s[kind]), 8, n, C, None, ptr(counts), stream()))

            def run_b(i):
                s = sets[i % len(sets)]
                pred = torch.argmax(s['x'], dim=1)
                check(lib.pylc_confusion_matrix(ptr(s[kind]), 8, ptr(pred), 8, n, C, 0, ptr(cm), stream()))

            counts.zero_(); cm.zero_()
            run_a(0); run_b(0)
            assert torch.equal(counts[:-1], cm) and int(counts[-1]) == 0 and int(cm.sum()) == n, 'A and B disagree'
            want = np.zeros((C, C), np.int64)                                        # and against numpy, on the first tile
            p0 = sets[0]['x'][0].permute(1, 2, 0).cpu().numpy().argmax(-1)
            np.add.at(want, (sets[0][kind][0].cpu().numpy(), p0), 1)
            first = metrics.logits_confusion(sets[0]['x'][:1], sets[0][kind][:1])
            assert np.array_equal(first.cpu().numpy()[:-1].reshape(C, C), want)
            ta, tb = [], []
            for _ in range(a.rounds):
                ta.append(timed(run_a, a.launches, a.warmup))
                tb.append(timed(run_b, a.launches, a.warmup))
            sa, sb = float(np.median(ta)), float(np.median(tb))
            nbytes = n * (4 * PITCH + 8)
            out['cases']['b%d_%s' % (batch, kind)] = {
                'pixels': n, 'rotating_sets': len(sets), 'a_us': sa * 1e6, 'b_us': sb * 1e6, 'a_over_b': sa / sb,
                'a_us_rounds': [t * 1e6 for t in ta], 'b_us_rounds': [t * 1e6 for t in tb], 'a_slower_in_rounds': sum(x > y for x, y in zip(ta, tb)),
                'a_algorithmic_bytes': nbytes, 'a_TBps': nbytes / sa / 1e12, 'a_share_of_achievable_hbm': nbytes / sa / HBM_ACHIEVABLE,
                'results_equal': True}
        del sets
    out['a_not_slower_in_any_case'] = all(v['a_over_b'] <= 1.0 for v in out['cases'].values())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
