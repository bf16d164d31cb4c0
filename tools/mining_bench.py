"""Hard-pixel mining (csrc/mining.hip) at the benchmark's loss shape on one MI355X: 32 x 512^2 pixels, 9 classes at
pitch 12, uint8 targets, keep = 0.25, on three sets of logits --

  random    standard normal logits times 3: the losses spread over many histogram bins;
  peaked    the target's logit 12 above the rest on 97 % of the pixels, as a trained model gives: most nll near 0;
  constant  every logit 0: every key is the same, log 9.

For each set: the median over --rounds rounds of --launches launches between device events of pylc_hard_pixel_weights (the fused path: one
memset and four kernels), of pylc_pixel_nll (the nll kernel without the histogram) and of pylc_hard_select on the stored map (one memset
and four kernels), the entry points taking turns within a round; the GB/s of the byte model below; and, from the same process, the time of
pylc_multiloss_stats_w + pylc_multiloss_finalize_ex + pylc_multiloss_bwd_w on the same inputs with the mined map, and the ratio of the fused
path to it.  Results are checked first: the fused path against pixel_nll + hard_select bit for bit, k and the kept count against the
rule.  Per-kernel times come from a kernel trace: --once SET makes --launches fused launches and exits (run it under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR/SET -- python tools/mining_bench.py --once SET`), and --stats DIR folds the traces' per-kernel
averages into the report.

Byte model (N pixels, C classes at pitch P, float32; uint8 targets): nll + first histogram reads N (4 P + 1) and writes 4 N; each of the
two histogram passes reads 4 N; apply reads 4 N and writes 4 N (+ 4 N with weights).  Fused, without weights: N (4 P + 21).

    python tools/mining_bench.py [--launches 20] [--rounds 5] [--warmup 3] [--stats DIR] [--out profiles/mining_bench.txt]
"""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

B, C, PITCH, TILE, KEEP = 32, 9, 12, 512, 0.25
SETS = ('random', 'peaked', 'constant')
KERNELS = ('mine_nll_kernel', 'mine_hist_kernel<2>', 'mine_hist_kernel<3>', 'mine_apply_kernel')


def make_logits(kind, dev):
    g = torch.Generator(device='cpu').manual_seed(4242)
    n = B * TILE * TILE
    t = torch.randint(0, C, (n,), generator=g, dtype=torch.int64)
    if kind == 'random':
        z = torch.randn((n, C), generator=g) * 3.0
    elif kind == 'peaked':
        z = torch.randn((n, C), generator=g) * 0.5
        sure = torch.rand((n,), generator=g) < 0.97
        z[torch.arange(n)[sure], t[sure]] += 12.0
    else:
        z = torch.zeros((n, C))
    buf = torch.zeros((B, TILE, TILE, PITCH), device=dev)
    buf[..., :C] = z.view(B, TILE, TILE, C).to(dev)
    return buf.permute(0, 3, 1, 2)[:, :C], t.to(torch.uint8).view(B, TILE, TILE).to(dev)


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches


def kernel_stats(root, kind):
    """{kernel: average seconds} from the kernel-trace statistics under root/kind"""
    out = {}
    for path in glob.glob(os.path.join(root, kind, '**', '*kernel_stats.csv'), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get('Name', '')
            for k in KERNELS:
                base, _, arg = k.partition('<')
                if base in name and (not arg or ('<%s' % arg[:-1]) in name.replace('(int)', '').replace(' ', '')):
                    out[k] = out.get(k, 0.0) + float(row['AverageNs']) * 1e-9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--once', choices=SETS, default=None)
    ap.add_argument('--stats', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import lib as L, mining
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    dev = torch.device('cuda:0')
    n = B * TILE * TILE
    lines = ['mining_bench: %d x %d^2 pixels, C = %d, pitch %d, uint8 targets, keep = %.2f; median of %d rounds of %d launches between device events'
             % (B, TILE, C, PITCH, KEEP, a.rounds, a.launches)]
    for kind in (a.once,) if a.once else SETS:
        z, t = make_logits(kind, dev)
        out, nll, info = (torch.empty((B, TILE, TILE), device=dev), torch.empty((B, TILE, TILE), device=dev),
                          torch.empty(4, device=dev, dtype=torch.int64))
        ws = torch.empty(lib.pylc_mining_workspace_bytes(n), device=dev, dtype=torch.uint8)
        inf = float('inf')

        def fused():
            check(lib.pylc_hard_pixel_weights(ptr(z), PITCH, ptr(t), 1, n, C, mining.NO_IGNORE, None, KEEP, 0, inf, None, ptr(out), ptr(info), ptr(ws),
                                              stream()))

        def nll_only():
            check(lib.pylc_pixel_nll(ptr(z), PITCH, ptr(t), 1, n, C, mining.NO_IGNORE, None, ptr(nll), stream()))

        def select_only():
            check(lib.pylc_hard_select(ptr(nll), n, None, KEEP, 0, inf, ptr(out), ptr(info), ptr(ws), stream()))

        if a.once:
            for _ in range(a.warmup + a.launches):
                fused()
            torch.cuda.synchronize()
            return
        # results first
        fused()
        w1, i1 = out.clone(), info.clone()
        nll_only()
        select_only()
        assert torch.equal(w1.view(torch.int32), out.view(torch.int32)) and torch.equal(i1, info), 'fused path differs from pixel_nll + hard_select'
        n_valid, k, kept, _ = i1.cpu().tolist()
        assert n_valid == n and k == mining.expected_k(n, KEEP) and kept >= k and int((w1 > 0).sum()) == kept
        # the loss head on the same inputs, with the mined map
        stats, lws = torch.empty(3 + 3 * C, device=dev), torch.empty(lib.pylc_multiloss_workspace_floats(n, C), device=dev)
        losses, dl, gs = torch.empty(4, device=dev), torch.empty((B, TILE, TILE, PITCH), device=dev), torch.ones(1, device=dev)

        def loss_head():
            check(lib.pylc_multiloss_stats_w(ptr(z), PITCH, ptr(t), 1, n, C, mining.NO_IGNORE, None, ptr(w1), ptr(stats), ptr(lws), None, stream()))
            check(lib.pylc_multiloss_finalize_ex(ptr(stats), C, 0.5, 0.5, 0.5, ptr(losses), stream()))
            check(lib.pylc_multiloss_bwd_w(ptr(z), PITCH, ptr(t), 1, n, C, mining.NO_IGNORE, None, ptr(w1), ptr(stats), 0.5, 0.5, 0.5, ptr(gs),
                                           ptr(dl), PITCH, None, stream()))

        runs = {'hard_pixel_weights (fused)': fused, 'pixel_nll': nll_only, 'hard_select': select_only, 'loss head stats_w + bwd_w': loss_head}
        times = {name: [] for name in runs}
        for _ in range(a.rounds):
            for name, fn in runs.items():
                times[name].append(timed(fn, a.launches, a.warmup))
        med = {name: float(np.median(v)) for name, v in times.items()}
        model = {'hard_pixel_weights (fused)': n * (4 * PITCH + 21), 'pixel_nll': n * (4 * PITCH + 5), 'hard_select': n * 20}
        lines.append('%s logits: %d of %d pixels kept (k = %d)' % (kind, kept, n_valid, k))
        for name in runs:
            gbs = '  %7.0f GB/s of the byte model (%.0f MB)' % (model[name] / med[name] * 1e-9, model[name] * 1e-6) if name in model else ''
            lines.append('  %-30s %8.1f us  (rounds: %s)%s' % (name, med[name] * 1e6, ' '.join('%.1f' % (v * 1e6) for v in times[name]), gbs))
        lines.append('  fused path / loss head = %.3f' % (med['hard_pixel_weights (fused)'] / med['loss head stats_w + bwd_w']))
        if a.stats:
            ks = kernel_stats(a.stats, kind)
            if ks:
                kb = {'mine_nll_kernel': n * (4 * PITCH + 5), 'mine_hist_kernel<2>': n * 4, 'mine_hist_kernel<3>': n * 4, 'mine_apply_kernel': n * 8}
                lines.append('  per kernel (kernel trace of the fused path, average): ' + '; '.join(
                    '%s %.1f us (%.0f GB/s)' % (k_, ks[k_] * 1e6, kb[k_] / ks[k_] * 1e-9) for k_ in KERNELS if k_ in ks))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
