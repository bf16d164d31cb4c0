"""CPU suite (-m "not gpu") of the validation scores: the per-class closed forms against sklearn, ScoreLog's bookkeeping and file, its
group sum on two gloo ranks, and the C entry point's declaration and host-side argument checks."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(rs, c, empty, n=3000):
    """a random count matrix whose classes `empty` are neither present nor predicted"""
    live = np.array([k for k in range(c) if k not in empty])
    yt = live[rs.randint(0, live.size, n)]
    yp = np.where(rs.rand(n) < 0.6, yt, live[rs.randint(0, live.size, n)])
    cm = np.zeros((c, c), np.int64)
    np.add.at(cm, (yt, yp), 1)
    return cm, yt, yp


def test_per_class_and_scores_equal_sklearn():
    from sklearn.metrics import f1_score, jaccard_score, matthews_corrcoef
    from pylc_amd import metrics
    rs = np.random.RandomState(5)
    for c, empty in ((9, ()), (9, (0, 4)), (11, (10,)), (2, ()), (16, (1, 2, 3, 15))):
        cm, yt, yp = _counts(rs, c, empty)
        if c == 9 and empty:
            cm[:, 7] = 0                                   # a class that is present but never predicted
            yp = yp.copy()
            keep = yp != 7
            yt, yp = yt[keep], yp[keep]
        labels = list(range(c))
        pc, s = metrics.per_class(cm), metrics.scores(cm)
        assert np.array_equal(pc['support'], cm.sum(1)) and all(pc['support'][k] == 0 for k in empty)
        assert np.abs(pc['f1'] - f1_score(yt, yp, labels=labels, average=None, zero_division=0)).max() < 1e-12
        assert np.abs(pc['iou'] - jaccard_score(yt, yp, labels=labels, average=None, zero_division=0)).max() < 1e-12
        assert abs(s['f1'] - f1_score(yt, yp, average='weighted', zero_division=0)) < 1e-12
        assert abs(s['iou'] - jaccard_score(yt, yp, average='weighted', zero_division=0)) < 1e-12
        assert abs(s['mcc'] - matthews_corrcoef(yt, yp)) < 1e-12
        w = pc['support'] / pc['support'].sum()
        assert abs(s['iou'] - (pc['iou'] * w).sum()) < 1e-12 and abs(s['f1'] - (pc['f1'] * w).sum()) < 1e-12


def _inject(log, cm, outside=0):
    c = log.n_classes
    log.counts = torch.cat([torch.as_tensor(cm, dtype=torch.int64).reshape(-1), torch.tensor([outside], dtype=torch.int64)])


def _diag(c, hit, miss):
    """every class: `hit` right, `miss` taken for the next class"""
    cm = np.zeros((c, c), np.int64)
    for k in range(c):
        cm[k, k], cm[k, (k + 1) % c] = hit, miss
    return cm


def test_score_log_rows_best_and_file(tmp_path):
    from pylc_amd import metrics
    log = metrics.ScoreLog(3)
    assert log.close(0, 0) is None and not log.rows and not log.is_best          # nothing added: no row
    seq = [(50, 50), (80, 20), (70, 30), (80, 20), (90, 10)]
    best, flags = 0.0, []
    for i, (hit, miss) in enumerate(seq):
        _inject(log, _diag(3, hit, miss))
        row = log.close(10 * i, i)
        want = metrics.scores(_diag(3, hit, miss))
        assert set(row) == {'iter', 'epoch', 'f1', 'iou', 'mcc', 'class_iou', 'class_f1', 'support'}
        assert (row['iter'], row['epoch'], row['iou'], row['f1'], row['mcc']) == (10 * i, i, want['iou'], want['f1'], want['mcc'])
        assert row['support'] == [hit + miss] * 3 and row['class_iou'] == [hit / (hit + 2 * miss)] * 3
        assert int(log.counts.abs().sum()) == 0 and np.array_equal(log.last_counts.numpy(), _diag(3, hit, miss))
        flags.append(log.is_best)
        best = max(best, want['iou'])
        assert log.best_iou == best
    assert flags == [True, True, False, False, True]                              # an equal score is not a new best
    path = str(tmp_path / 'scores.json')
    log.save(path)
    assert os.listdir(str(tmp_path)) == ['scores.json']                           # written under a temporary name, renamed into place
    with open(path) as f:
        data = json.load(f)
    assert data['rows'] == log.rows and data['best_iou'] == log.best_iou and data['n_classes'] == 3
    back = metrics.ScoreLog(3)
    assert back.load(path) and back.rows == log.rows and back.best_iou == log.best_iou and not back.is_best
    assert not back.load(str(tmp_path / 'none.json'))
    with pytest.raises(ValueError, match='3 classes'):
        metrics.ScoreLog(9).load(path)
    # targets outside the classes: close() names their number, keeps no row, and the log goes on
    _inject(log, _diag(3, 5, 5), outside=17)
    with pytest.raises(ValueError, match=r'\b17\b'):
        log.close(60, 6)
    assert len(log.rows) == 5 and int(log.counts.abs().sum()) == 0


WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import json, numpy as np, torch, torch.distributed as dist
from pylc_amd import parallel, metrics
from pylc_amd.runtime import runtime

rank, world = parallel.init_from_env('gloo')
assert world == 2 and runtime.sync_group is not None
c = 4
mine = np.random.RandomState(10 + rank).randint(0, 50, (c, c)).astype(np.int64)
both = sum(np.random.RandomState(10 + r).randint(0, 50, (c, c)).astype(np.int64) for r in range(world))
log = metrics.ScoreLog(c)
log.counts = torch.cat([torch.from_numpy(mine).reshape(-1), torch.zeros(1, dtype=torch.int64)])
n0 = runtime.collectives
row = log.close(5, 1, runtime.sync_group)
assert runtime.collectives - n0 == 1
assert np.array_equal(log.last_counts.numpy(), both) and int(log.counts.abs().sum()) == 0
want = metrics.scores(both)
assert (row['iou'], row['f1'], row['mcc']) == (want['iou'], want['f1'], want['mcc']) and row['support'] == both.sum(1).tolist()
rows = [None] * world
dist.all_gather_object(rows, json.dumps(row, sort_keys=True))
assert rows[0] == rows[1]
# a rank that saw no batch still takes part; an out-of-range target on ONE rank raises on both
log2 = metrics.ScoreLog(c)
if rank == 0:
    log2.counts = torch.cat([torch.from_numpy(mine).reshape(-1), torch.tensor([3])])
try:
    log2.close(6, 1, runtime.sync_group)
    raise SystemExit('out-of-range targets were accepted')
except ValueError as e:
    assert '3 validation targets' in str(e)
parallel.barrier()
if rank == 0:
    print('SCORE_DIST_OK')
'''


def test_close_sums_over_two_gloo_ranks():
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='2')
    script = WORKER % {'root': ROOT}
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', '29547', '--no-python', sys.executable, '-c', script]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'SCORE_DIST_OK' in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_entry_point_is_declared_exported_and_checks_its_arguments():
    from pylc_amd import lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read(), flags=re.S)
    assert re.search(r'\bpylc_logits_score\s*\(', hdr) and 'pylc_logits_score' in L.SIGNATURES and hasattr(L.lib, 'pylc_logits_score')
    assert L.ABI_VERSION == 15 and L.lib.pylc_abi_version() == 15
    # the argument checks happen on the host before any launch: no GPU needed, never a fault
    P = 64

    def call(logits=P, pitch=12, target=P, tbytes=1, n=100, c=9, mask=P, counts=P):
        return L.lib.pylc_logits_score(logits, pitch, target, tbytes, n, c, mask, counts, None)
    assert call(mask=None, counts=None) == 1 and b'both NULL' in L.lib.pylc_last_error()
    assert call(target=None, tbytes=0) == 1 and b'counts without target' in L.lib.pylc_last_error()
    assert call(tbytes=2) == 1 and b'target_bytes=2' in L.lib.pylc_last_error()
    assert call(n=0) == 1 and call(n=-1) == 1 and call(n=(1 << 39) + 1) == 1 and b'2^39' in L.lib.pylc_last_error()
    assert call(c=1) == 1 and call(c=17) == 1 and b'n_classes=17' in L.lib.pylc_last_error()
    assert call(pitch=8) == 1 and b'pitch=8' in L.lib.pylc_last_error()
    assert call(logits=None) == 1
    assert call(target=60, tbytes=8) == 1 and b'aligned' in L.lib.pylc_last_error()


def test_model_rules_without_gpu():
    """best_by is 'dice' or 'iou', and 'iou' needs a ScoreLog; a model without scores logs and saves as before"""
    from pylc_amd import metrics
    from pylc_amd.model import Model
    m = Model(device='cpu')
    assert m.scores is None and m.best_by == 'dice'
    with pytest.raises(ValueError, match='ScoreLog'):
        m.best_by = 'iou'
    with pytest.raises(ValueError, match="'dice' or 'iou'"):
        m.best_by = 'f1'
    m.scores = metrics.ScoreLog(9)
    m.best_by = 'iou'
    assert m.best_by == 'iou'
