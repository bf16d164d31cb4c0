"""SHA-256 of what the loss head and the hard-pixel mining produce for seeded inputs at the smallest sizes their kernels can still go wrong
at, one line each: run it at two commits and diff the lines to show that a change to the host side of loss.hip / mining.hip or to the Python
driver moved no byte.

    pixels        (1, 5, 7) = 35, one partial block; (2, 40, 36) = 2880, 12 blocks (the column sum sees several rows)
    classes       2, 9, 16
    class weights none, given                                                                    (the loss head only)
    logits        dense; a channel slice of a wider NHWC buffer (pitch > C, not 16-byte aligned)
    loss head     plain int64; ignore 255 with a few out-of-range targets (uint8, int64); pixel weights with zero, negative and NaN entries,
                  with and without an index; soft 'probs' contiguous and as a channels-last view; soft 'logits' at T = 2; smoothing 0.1
                  (uint8, int64) -- losses, stats, bad and dlogits of multiloss_forward / multiloss_backward
    mining        pixel_nll; hard_pixel_weights with keep=0.25 and with thresh=0.7; each with and without incoming weights, uint8 and int64

    python tools/loss_hashes.py > hashes.txt
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WEIGHTS = (0.5, 0.3, 0.2)
SHAPES = ((1, 5, 7), (2, 40, 36))
CLASSES = (2, 9, 16)


def sha(t):
    return 'none' if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def inputs(seed, shape, c, sliced, dev):
    """logits (NHWC memory), uint8 / int64 targets with ignored (255) and out-of-range entries, pixel weights with 0, -1 and NaN, a soft
    volume (planar) and class weights"""
    rs = np.random.RandomState(seed)
    b, h, w = shape
    pitch, off = (c + 7, 3) if sliced else (c, 0)
    buf = torch.from_numpy(rs.standard_normal((b, h, w, pitch)).astype(np.float32) * 3).to(dev)
    logits = buf.permute(0, 3, 1, 2)[:, off:off + c]
    n = b * h * w
    tgt = rs.randint(0, c, n)
    pick = rs.permutation(n)
    tgt[pick[:4]] = 255
    u8 = tgt.copy()
    u8[pick[4:6]] = 200
    i64 = tgt.astype(np.int64)
    i64[pick[4:6]] = (-3, 1000)
    pw = rs.uniform(0.1, 2.0, n).astype(np.float32)
    pw[pick[6:9]] = 0.0
    pw[pick[9]] = -1.0
    pw[pick[10]] = np.nan
    soft = rs.uniform(0.0, 1.0, (b, c, h, w)).astype(np.float32)
    soft /= soft.sum(1, keepdims=True)
    return {'logits': logits,
            'u8': torch.from_numpy(u8.astype(np.uint8).reshape(b, h, w)).to(dev),
            'i64': torch.from_numpy(i64.reshape(b, h, w)).to(dev),
            'plain': torch.from_numpy(rs.randint(0, c, (b, h, w)).astype(np.int64)).to(dev),
            'pw': torch.from_numpy(pw.reshape(b, h, w)).to(dev),
            'soft': torch.from_numpy(soft).to(dev),
            'cw': torch.from_numpy(rs.uniform(0.5, 1.5, c).astype(np.float32)).to(dev)}


def loss_cases(t):
    """(name, target, keywords of multiloss_forward)"""
    soft_cl = t['soft'].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    teacher = (t['soft'] * 8 - 4).contiguous()
    return (('plain_i64', t['plain'], {}),
            ('ignore255_u8', t['u8'], {'ignore_index': 255}),
            ('ignore255_i64', t['i64'], {'ignore_index': 255}),
            ('weights_index255_u8', t['u8'], {'ignore_index': 255, 'pixel_weights': t['pw']}),
            ('weights_noindex_i64', t['i64'], {'pixel_weights': t['pw']}),
            ('soft_probs', None, {'soft_target': t['soft']}),
            ('soft_probs_channels_last', None, {'soft_target': soft_cl}),
            ('soft_logits_T2', None, {'soft_target': teacher, 'soft_kind': 'logits', 'temperature': 2.0}),
            ('smooth0.1_u8', t['u8'], {'label_smoothing': 0.1, 'ignore_index': 255}),
            ('smooth0.1_i64', t['i64'], {'label_smoothing': 0.1, 'ignore_index': 255}))


def main():
    from pylc_amd import lib as L, mining, ops
    L.init()
    dev = torch.device('cuda:0')
    dlosses = torch.tensor([1.5, 0.0, 0.0, 0.0], device=dev)
    seed = 0
    for shape in SHAPES:
        for c in CLASSES:
            for sliced in (0, 1):
                seed += 1
                t = inputs(seed, shape, c, sliced, dev)
                where = 'px %s C %2d slice %d' % ('x'.join(map(str, shape)), c, sliced)
                for with_cw in (0, 1):
                    for name, target, kw in loss_cases(t):
                        bad = None if name == 'plain_i64' else torch.zeros(1, dtype=torch.int64, device=dev)
                        losses, saved, state, _ = ops.multiloss_forward(None, t['logits'], target, t['cw'] if with_cw else None, *WEIGHTS, None,
                                                                        bad=bad, **kw)
                        (dl,) = ops.multiloss_backward(state, saved, None, dlosses)
                        amax = getattr(dl, '_pylc_amax', (None,))[0]
                        print('loss %-26s %s cw %d  losses %s stats %s bad %s dlogits %s amax %s'
                              % (name, where, with_cw, sha(losses), sha(saved[2]), sha(bad), sha(dl), sha(amax)))
                for tname in ('u8', 'i64'):
                    for pw in (None, t['pw']):
                        tail = '%s target %s weights %d' % (where, tname, pw is not None)
                        nll = mining.pixel_nll(t['logits'], t[tname], ignore_index=255, pixel_weights=pw)
                        print('mining pixel_nll                   %s  nll %s' % (tail, sha(nll)))
                        for rule in ({'keep': 0.25}, {'thresh': 0.7}):
                            out, info = mining.hard_pixel_weights(t['logits'], t[tname], ignore_index=255, pixel_weights=pw, **rule)
                            print('mining hard_pixel_weights %-8s %s  weights %s info %s'
                                  % ('%s=%s' % next(iter(rule.items())), tail, sha(out), sha(info)))
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
