"""The calibration launches (csrc/calibration.hip) at the sizes they are used at, on one MI355X:

  logits_reliability and nll_grid (K = 33: two launches of 17 and 16) on 8 x 9 x 512^2 seeded NHWC logits at pitch 12 with int64 blob
  targets, as Model.eval hands them over; reliability_counts on a 3072 x 4096 confidence map with uint8 masks.

Each is timed against the same quantity composed from torch ops on the same device in the same process (B):
  logits_reliability:  softmax(dim=1) -> max -> bucketize -> three bincounts (pixels, hits, and the float64-weighted confidence sum)
  nll_grid:            for every beta: logsumexp(beta * z) - beta * z[target], summed in float64
  reliability_counts:  bucketize + the same three bincounts
B's results are compared with A's first (counts: pixels and hits equal wherever no confidence lies within 1e-6 of a bin edge, ECE to 1e-5;
NLL to 1e-6 relative).  Everything is timed between device events after warm-up launches, A and B alternating for --rounds rounds, the
median round reported; the launches rotate over --sets sets of inputs (a set of logits is 101 MB: one stays in the last-level cache,
several do not).  Also reported: A's algorithmic bytes over its time as a share of the achievable HBM rate (6.3 TB/s), and for nll_grid
its exponentials per second -- K * C per pixel.

The third part times a validation pass (Model.eval on two batches + Model.log) of a DeepLab with and without calibration_bins.

    python tools/calibration_bench.py [--launches N] [--warmup W] [--rounds R] [--sets K] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

C, PITCH, TILE, BATCH, BINS = 9, 12, 512, 8, 15
PHOTO = (3072, 4096)
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


def alternate(run_a, run_b, args, b_launches=None):
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(timed(run_a, args.launches, args.warmup))
        tb.append(timed(run_b, b_launches or args.launches, min(args.warmup, b_launches or args.warmup)))
    return float(np.median(ta)), float(np.median(tb)), ta, tb


def torch_counts(conf, pred, truth, edges):
    """pixels, hits and confidence sum per (class, bin) from torch ops; targets are all classes here"""
    b = torch.bucketize(conf, edges, right=True).clamp_(max=BINS - 1)
    cell = pred.long() * BINS + b
    n = torch.bincount(cell, minlength=C * BINS)
    hits = torch.bincount(cell[pred.long() == truth.long()], minlength=C * BINS)
    s = torch.bincount(cell, weights=conf.double(), minlength=C * BINS)
    return n, hits, s


def ece_of(n, hits, s):
    n, hits, s = (t.view(C, BINS).sum(0).double().cpu().numpy() for t in (n, hits, s))
    full = n > 0
    return float((np.abs(hits[full] - s[full]) / n.sum()).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5, help='A / B alternations; the median is reported')
    ap.add_argument('--sets', type=int, default=4, help='sets of inputs the launches rotate over')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import calibration as cal, lib as L
    from tests import _data as D
    assert torch.cuda.is_available(), 'needs the MI355X'
    L.init()
    dev = torch.device('cuda:0')
    out = {'n_classes': C, 'pitch': PITCH, 'tile': TILE, 'batch': BATCH, 'bins': BINS, 'launches': a.launches, 'warmup': a.warmup,
           'rounds': a.rounds, 'sets': a.sets, 'hbm_achievable_TBps': HBM_ACHIEVABLE / 1e12, 'cases': {}}
    edges = torch.arange(1, BINS, device=dev, dtype=torch.float32) / BINS
    n = BATCH * TILE * TILE
    g = torch.Generator(device=dev).manual_seed(4321)
    sets = []
    for k in range(a.sets):
        buf = torch.randn((BATCH, TILE, TILE, PITCH), device=dev, generator=g) * 3
        t = D.blob_masks(7 + k, BATCH, TILE, TILE, C).to(dev)
        # 'blob': logits that mostly follow a blob mask (the target moved by (3, 5) pixels), as a trained network's do: the predicted
        # classes come in regions and the confidences cluster at the top; 'x' is plain noise, the case in which nothing clusters
        blob = (torch.randn((BATCH, TILE, TILE, PITCH), device=dev, generator=g) * 1.5)
        blob[..., :C] += 7.0 * torch.nn.functional.one_hot(torch.roll(t, (3, 5), (1, 2)), C)
        sets.append({'x': buf[..., :C].permute(0, 3, 1, 2), 'blob': blob[..., :C].permute(0, 3, 1, 2), 't': t})
    counts = torch.zeros(cal.n_cells(C, BINS), device=dev, dtype=torch.int64)

    # ---- logits_reliability -----------------------------------------------------------------------------------------------------------
    nbytes = n * (4 * PITCH + 8)
    for kind in ('blob', 'x'):
        def lr_a(i):
            s = sets[i % len(sets)]
            cal.logits_reliability(s[kind], s['t'], BINS, counts=counts)

        def lr_b(i):
            s = sets[i % len(sets)]
            conf, pred = torch.softmax(s[kind], dim=1).max(dim=1)
            return torch_counts(conf.reshape(-1), pred.reshape(-1), s['t'].reshape(-1), edges)
        counts.zero_()
        lr_a(0)
        bn, bh, bs = lr_b(0)
        mine = counts[:-3].view(C * BINS, 3)
        ece_a, ece_b = cal.reliability_scores(counts, C, BINS)['ece'], ece_of(bn, bh, bs)
        assert int(mine[:, 0].sum()) == n == int(bn.sum()) and int((mine[:, 0] - bn).abs().sum()) <= 256 and abs(ece_a - ece_b) < 1e-5, (ece_a, ece_b)
        sa, sb, ta, tb = alternate(lr_a, lr_b, a)
        out['cases']['logits_reliability_' + ('blob' if kind == 'blob' else 'noise')] = {'pixels': n, 'a_us': sa * 1e6, 'b_us': sb * 1e6, 'a_over_b': sa / sb, 'a_us_rounds': [t * 1e6 for t in ta],
            'b_us_rounds': [t * 1e6 for t in tb], 'a_algorithmic_bytes': nbytes, 'a_TBps': nbytes / sa / 1e12,
            'a_share_of_achievable_hbm': nbytes / sa / HBM_ACHIEVABLE, 'ece_a': ece_a, 'ece_b': ece_b}

    # ---- nll_grid, K = 33 -------------------------------------------------------------------------------------------------------------
    betas = cal.default_betas()
    sums, tail = torch.zeros(len(betas), device=dev, dtype=torch.float64), torch.zeros(3, device=dev, dtype=torch.int64)

    def nll_a(i):
        s = sets[i % len(sets)]
        cal.nll_grid(s['blob'], s['t'], betas, sums=sums, tail=tail)

    def nll_b(i):
        s = sets[i % len(sets)]
        idx = s['t'].unsqueeze(1)
        res = []
        for beta in betas:
            z = s['blob'] * float(beta)
            res.append((torch.logsumexp(z, dim=1) - z.gather(1, idx).squeeze(1)).sum(dtype=torch.float64))
        return torch.stack(res)
    nll_a(0)
    want = nll_b(0)
    assert float(((sums - want).abs() / want).max()) < 1e-6 and int(tail[0]) == n
    sa, sb, ta, tb = alternate(nll_a, nll_b, a, b_launches=max(2, a.launches // 10))
    nbytes2 = 2 * n * (4 * PITCH + 8)                        # the logits are read once per launch, and 33 betas are two launches
    out['cases']['nll_grid_k33'] = {'pixels': n, 'betas': len(betas), 'launches_per_call': 2, 'a_us': sa * 1e6, 'b_us': sb * 1e6, 'a_over_b': sa / sb,
                                    'a_us_rounds': [t * 1e6 for t in ta], 'b_us_rounds': [t * 1e6 for t in tb], 'a_algorithmic_bytes': nbytes2,
                                    'a_TBps': nbytes2 / sa / 1e12, 'a_share_of_achievable_hbm': nbytes2 / sa / HBM_ACHIEVABLE,
                                    'a_exp_per_s': n * len(betas) * C / sa}
    # the same grid at K = 8 and K = 16 (one launch each): how the time scales with the number of exponentials
    for k in (8, 16, 32):
        bk = cal.default_betas(k + 1)[:k]
        sk = torch.zeros(k, device=dev, dtype=torch.float64)

        def nll_k(i):
            s = sets[i % len(sets)]
            cal.nll_grid(s['blob'], s['t'], bk, sums=sk, tail=tail)
        t = float(np.median([timed(nll_k, a.launches, a.warmup) for _ in range(a.rounds)]))
        out['cases']['nll_grid_k%d' % k] = {'a_us': t * 1e6, 'a_exp_per_s': n * k * C / t, 'a_TBps': nbytes / t / 1e12}
    del sets

    # ---- reliability_counts on a photograph's maps --------------------------------------------------------------------------------------
    h, w = PHOTO
    psets = []
    for k in range(a.sets):
        truth = D.blob_masks(20 + k, 1, h, w, C).to(dev).to(torch.uint8)[0]
        flip = D.blob_masks(40 + k, 1, h, w, 7, cell=48).to(dev)[0] == 0              # wrong in regions (1 / 7 of the area), as a network is
        pred = torch.where(flip, D.blob_masks(30 + k, 1, h, w, C).to(dev).to(torch.uint8)[0], truth)
        conf = 1 - torch.rand((h, w), device=dev, generator=g) ** 3 * 0.9                # 42 % in the top bin, the rest spread per pixel
        psets.append({'conf': conf, 'pred': pred, 'truth': truth})
    pcounts = torch.zeros(cal.n_cells(C, BINS), device=dev, dtype=torch.int64)

    def rc_a(i):
        s = psets[i % len(psets)]
        cal.reliability_counts(s['conf'], s['pred'], s['truth'], C, BINS, counts=pcounts)

    def rc_b(i):
        s = psets[i % len(psets)]
        return torch_counts(s['conf'].reshape(-1), s['pred'].reshape(-1), s['truth'].reshape(-1), edges)
    rc_a(0)
    bn, bh, bs = rc_b(0)
    mine = pcounts[:-3].view(C * BINS, 3)
    ece_a, ece_b = cal.reliability_scores(pcounts, C, BINS)['ece'], ece_of(bn, bh, bs)
    assert int(mine[:, 0].sum()) == h * w and int((mine[:, 0] - bn).abs().sum()) <= 256 and abs(ece_a - ece_b) < 1e-5, (ece_a, ece_b)
    sa, sb, ta, tb = alternate(rc_a, rc_b, a)
    nbytes = h * w * 6
    out['cases']['reliability_counts_photo'] = {'pixels': h * w, 'a_us': sa * 1e6, 'b_us': sb * 1e6, 'a_over_b': sa / sb,
                                                'a_us_rounds': [t * 1e6 for t in ta], 'b_us_rounds': [t * 1e6 for t in tb],
                                                'a_algorithmic_bytes': nbytes, 'a_TBps': nbytes / sa / 1e12,
                                                'a_share_of_achievable_hbm': nbytes / sa / HBM_ACHIEVABLE}
    del psets

    # ---- a validation pass with and without calibration_bins ----------------------------------------------------------------------------
    import oracle
    from pylc_amd import metrics, runtime
    from pylc_amd.model import Meta, Model
    runtime.dropout_enabled = False
    model = Model(Meta(arch='deeplab', backbone='resnet'), dev).build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec('deeplab', 'resnet', 9, 3), salt=6))
    va = [(D.tiles(50 + i, 8, 3, TILE, TILE), D.blob_masks(60 + i, 8, TILE, TILE, 9, cell=8)) for i in range(2)]

    def pass_time(bins):
        model.scores = metrics.ScoreLog(9, calibration_bins=bins)
        times = []
        for r in range(a.rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for x, y in va:
                model.eval(x, y)
            model.log()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return float(np.median(times[1:])), model.scores.rows[-1]
    plain, _ = pass_time(None)
    with_bins, row = pass_time(BINS)
    plain2, _ = pass_time(None)
    out['cases']['validation_pass_2x8x512'] = {'plain_ms': plain * 1e3, 'plain_again_ms': plain2 * 1e3, 'calibration_bins_ms': with_bins * 1e3,
                                               'extra_ms': (with_bins - 0.5 * (plain + plain2)) * 1e3, 'ece': row['ece'], 'temperature': row['temperature']}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
