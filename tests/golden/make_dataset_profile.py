#!/usr/bin/env python3
"""Generate tests/golden/dataset_profile.json from the REAL reference: its get_profile (utils/profile.py:21-150) and its
Augmentor.optimize (utils/augment.py:92-182) on the seeded tiles of tests/test_cpu_dataset.py::profile_case.

Runs only in the build container (needs the reference checkout; make_golden.enter_reference() sets up the scratch cwd and the stub
modules).  get_profile is fed a duck-typed dataset (get_meta(), loader() yielding (float32 [1,C,t,t], int64 [1,t,t]), size);
Augmentor.optimize an object.__new__(Augmentor) holding the profiled meta.  The fixture holds the reference's OUTPUTS only, plus, per case,
fp32_gap_mean / fp32_gap_std: the largest relative distance over channels between the reference's float32 px_mean / px_std and the
float64 value of the exact integer sums -- the measured size of the reference's own summation noise, which bounds the tests' comparison.

    python tests/golden/make_dataset_profile.py        ->  tests/golden/dataset_profile.json
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402


class Tiles:
    """what get_profile asks of an MLPDataset"""

    def __init__(self, meta, img, mask):
        self.meta, self.img, self.mask, self.size = meta, img, mask, img.shape[0]

    def get_meta(self):
        return self.meta

    def loader(self, batch_size=1, n_workers=0, drop_last=False):
        assert batch_size == 1
        pairs = [(torch.from_numpy(self.img[i:i + 1].astype(np.float32)), torch.from_numpy(self.mask[i:i + 1].astype(np.int64)))
                 for i in range(self.size)]
        return pairs, self.size


def exact_stats(img):
    """float64 px_mean / px_std from exact integer sums (python integers), the reference's definition: means over tiles"""
    n, c, t, _ = img.shape
    N = t * t
    x = img.astype(np.int64)
    s, ss = x.sum((2, 3)), (x * x).sum((2, 3))
    mean = np.array([[int(s[i, k]) / N for k in range(c)] for i in range(n)])
    std = np.array([[((N * int(ss[i, k]) - int(s[i, k]) ** 2) / (N * (N - 1))) ** 0.5 for k in range(c)] for i in range(n)])
    return mean.mean(0), std.mean(0)


def run():
    from make_golden import enter_reference
    from tests.test_cpu_dataset import CASES, profile_case
    enter_reference()
    from config import Parameters
    from utils.profile import get_profile
    from utils.augment import Augmentor
    out = {}
    for name, c in CASES.items():
        img, mask = profile_case(name)
        meta = Parameters()
        meta.ch, meta.n_classes, meta.tile_size = c['ch'], c['n_classes'], c['tile']
        meta.tile_px_count = c['tile'] * c['tile']
        meta = get_profile(Tiles(meta, img, mask))
        mean64, std64 = exact_stats(img)
        ref_mean, ref_std = np.asarray(meta.px_mean, np.float64), np.asarray(meta.px_std, np.float64)
        case = {'px_mean': meta.px_mean, 'px_std': meta.px_std, 'px_dist': np.asarray(meta.px_dist).astype(np.int64).tolist(),
                'probs': meta.probs, 'weights': meta.weights, 'm2': float(meta.m2), 'jsd': float(meta.jsd),
                'dset_px_count': int(meta.dset_px_count),
                'fp32_gap_mean': float(np.max(np.abs(ref_mean - mean64) / np.abs(mean64))),
                'fp32_gap_std': float(np.max(np.abs(ref_std - std64) / np.abs(std64)))}
        assert ref_mean.shape == (c['ch'],) and case['dset_px_count'] == c['n'] * c['tile'] ** 2
        print(name, 'px_mean', meta.px_mean, 'px_std', meta.px_std, 'gaps', case['fp32_gap_mean'], case['fp32_gap_std'])
        if name == 'rgb':
            aug = object.__new__(Augmentor)
            aug.input_meta, aug.input_size = meta, c['n']
            aug.optimize()
            o = aug.optim_meta
            case['optimize'] = {'rates': [int(r) for r in o['rates']], 'threshold': float(o['threshold']), 'rate_coef': float(o['rate_coef']),
                                'jsd': float(o['jsd']), 'm2': float(o['m2'])}
            assert sum(case['optimize']['rates']) > 0, 'the optimiser chose no oversampling: the fixture would test nothing'
            print('optimize', case['optimize'])
        out[name] = case
    with open(os.path.join(HERE, 'dataset_profile.json'), 'w') as f:
        json.dump(out, f)


if __name__ == '__main__':
    run()
