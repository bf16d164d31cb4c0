"""The guided-filter refinement (csrc/refine.hip) at a photograph's size on one MI355X: 3072 x 4096 pixels, 9
classes, radius 4 / 8 / 16 / 64, eps 1e-3, plus one line for 1024 x 1536.  For each radius: the median over --rounds rounds of --launches
launches between device events of pylc_luma_u8, of pylc_guided_coeffs (stage 1), of pylc_guided_apply without and with the probability
volume written (stage 2), the entry points taking turns within a round; the GB/s of the byte model below; the streaming rate of a plain
device copy of the volume in the same process for comparison (profiles/blend_bench.txt has the blend's accumulate pass at 4.4 TB/s); and
the same filter composed from torch operators on the same GPU -- He et al.'s equations with F.avg_pool2d(2r+1, 1, r,
count_include_pad=False) in float32, 4 C + 2 box-filter planes plus the elementwise glue, argmax at the end -- with the ratio to it.
The torch composition computes every window directly ((2r+1)^2 terms per pixel); it is timed at the radii of --torch-radii only
(default 4 8 16).  Results are checked first: the fused mask against the composition's at the small size.

Byte model (N pixels, C classes, float32 volume, uint8 guide): luma reads 3 N and writes N; stage 1 reads N (4 C + 1) and writes 8 C N;
stage 2 reads N (8 C + 1) and writes N (1 + 4) without the volume, N (1 + 4 + 4 C) with it.

    python tools/refine_bench.py [--launches 5] [--rounds 5] [--warmup 2] [--torch-radii 4 8 16] [--out profiles/refine_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

C, EPS = 9, 1e-3
RADII = (4, 8, 16, 64)
BIG, SMALL = (3072, 4096), (1024, 1536)


def make_inputs(h, w, dev):
    """a photograph-like uint8 image (smooth field, edges, noise) and a softmax volume whose borders sit a few pixels off its edges"""
    g = torch.Generator(device='cpu').manual_seed(77)
    low = torch.rand((1, 3, h // 64 + 2, w // 64 + 2), generator=g) * 255
    img = F.interpolate(low, size=(h, w), mode='bilinear', align_corners=True)[0]
    img = (torch.round(img / 48) * 48 + torch.randn((3, h, w), generator=g) * 6).clamp(0, 255).to(torch.uint8)
    z = F.interpolate(torch.randn((1, C, h // 16 + 1, w // 16 + 1), generator=g) * 3, size=(h, w), mode='bilinear', align_corners=False)[0]
    return img.to(dev).contiguous(), torch.softmax(z.to(dev), 0).contiguous()


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


def torch_composition(p, g, r, eps):
    """the filter a user would write: float32, avg_pool2d box means, the argmax of q"""
    k = 2 * r + 1

    def mean(t):
        return F.avg_pool2d(t[None], k, 1, r, count_include_pad=False)[0]
    i = (g.float() / 255.0)[None]
    mean_i, mean_p = mean(i), mean(p)
    var = mean(i * i) - mean_i * mean_i
    cov = mean(i * p) - mean_i * mean_p
    a = cov / (var + eps)
    b = mean_p - a * mean_i
    q = mean(a) * i + mean(b)
    return q.argmax(0).to(torch.uint8), q.max(0).values.clamp(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--torch-radii', type=int, nargs='*', default=[4, 8, 16])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pylc_amd import lib as L, refine
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    dev = torch.device('cuda:0')
    lines = ['refine_bench: C = %d, eps = %g, float32 volume, uint8 guide; median of %d rounds of %d launches between device events'
             % (C, EPS, a.rounds, a.launches)]

    # results first, at the small size: the fused mask against the torch composition's (float32 on both sides: near ties may differ)
    img, p = make_inputs(*SMALL, dev)
    want = torch_composition(p, refine.luma(img), 8, EPS)[0]
    got = refine.guided_refine(p, img, 8, EPS)
    agree = float((got == want).float().mean())
    lines.append('check at %d x %d, r = 8: %.4f%% of the fused mask equals the torch composition\'s' % (SMALL + (100 * agree,)))
    assert agree > 0.999, agree

    for (h, w), radii in ((BIG, RADII), (SMALL, (8,))):
        n = h * w
        img, p = make_inputs(h, w, dev)
        g = refine.luma(img)
        ca, cb = torch.empty_like(p), torch.empty_like(p)
        mask, conf, vol = torch.empty((h, w), device=dev, dtype=torch.uint8), torch.empty((h, w), device=dev), torch.empty_like(p)
        copy_t = float(np.median([timed(lambda: vol.copy_(p), a.launches, a.warmup) for _ in range(a.rounds)]))
        lines.append('%d x %d (%.1f M pixels): a device copy of the volume streams at %.0f GB/s (%.0f MB read + written)'
                     % (h, w, n * 1e-6, 2 * 4 * C * n / copy_t * 1e-9, 2 * 4 * C * n * 1e-6))
        for r in radii:
            def luma():
                check(lib.pylc_luma_u8(ptr(img), 3, h, w, ptr(g), stream()))

            def stage1():
                check(lib.pylc_guided_coeffs(ptr(p), n, w, ptr(g), C, h, w, r, EPS, ptr(ca), ptr(cb), stream()))

            def stage2():
                check(lib.pylc_guided_apply(ptr(ca), ptr(cb), ptr(g), C, h, w, r, 1, ptr(mask), None, ptr(conf), stream()))

            def stage2_vol():
                check(lib.pylc_guided_apply(ptr(ca), ptr(cb), ptr(g), C, h, w, r, 1, ptr(mask), ptr(vol), ptr(conf), stream()))

            runs = {'luma': luma, 'stage 1 (coeffs)': stage1, 'stage 2 (apply)': stage2, 'stage 2 + volume': stage2_vol}
            model = {'luma': 4 * n, 'stage 1 (coeffs)': n * (12 * C + 1), 'stage 2 (apply)': n * (8 * C + 6), 'stage 2 + volume': n * (12 * C + 6)}
            times = {name: [] for name in runs}
            for _ in range(a.rounds):
                for name, fn in runs.items():
                    times[name].append(timed(fn, a.launches, a.warmup))
            med = {name: float(np.median(v)) for name, v in times.items()}
            fused = med['luma'] + med['stage 1 (coeffs)'] + med['stage 2 (apply)']
            lines.append('  r = %d' % r)
            for name in runs:
                lines.append('    %-20s %9.3f ms  (rounds: %s)  %6.0f GB/s of the byte model (%.0f MB)'
                             % (name, med[name] * 1e3, ' '.join('%.3f' % (v * 1e3) for v in times[name]), model[name] / med[name] * 1e-9,
                                model[name] * 1e-6))
            lines.append('    fused route (luma + stage 1 + stage 2): %.3f ms without the volume, %.3f ms with it; stage 1 at %.2f of the copy\'s rate'
                         % (fused * 1e3, (fused - med['stage 2 (apply)'] + med['stage 2 + volume']) * 1e3,
                            model['stage 1 (coeffs)'] / med['stage 1 (coeffs)'] / (2 * 4 * C * n / copy_t)))
            if r in a.torch_radii:
                t = float(np.median([timed(lambda: torch_composition(p, g, r, EPS), 1, 1) for _ in range(3)]))
                lines.append('    torch composition (avg_pool2d, float32, mask + conf): %.3f ms; fused route / torch = %.4f (%.1f x faster)'
                             % (t * 1e3, fused / t, t / fused))
                if r == 8:
                    assert fused < t, 'the fused route must beat the torch composition at r = 8'
            else:
                lines.append('    torch composition: not timed at this radius')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
