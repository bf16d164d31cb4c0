"""CPU suite (-m "not gpu") of the ignore label: the fp64 statement of the masked loss that the GPU suite
(tests/test_ignore_label_gpu.py) compares the kernels with, proven here against torch and the oracle; the new entry points' declarations and
host-side argument checks; the profile over valid pixels; ScoreLog's ignored / bad bookkeeping; Meta.ignore_index and its way through a
checkpoint."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(os.path.dirname(__file__), 'golden')

NEW_ENTRY_POINTS = ('pylc_multiloss_stats_ex', 'pylc_multiloss_finalize_ex', 'pylc_multiloss_bwd_ex', 'pylc_logits_score_ex',
                    'pylc_confusion_matrix_ex', 'pylc_class_encode_resize_ex')


# ---- the statement: masked sums, as in the issue's Semantics table ------------------------------------------------------------------------
def valid_pixels(target, n_classes, ignore_index):
    """bool [..]: the target is a class index and is not the ignore label"""
    t = target.long()
    ok = (t >= 0) & (t < n_classes)
    return ok if ignore_index is None else ok & (t != ignore_index)


def masked_multiloss(logits, target, ignore_index, weights=(0.5, 0.5, 0.5), class_weights=None):
    """(total, ce, dice, focal) of [B,C,H,W] logits (any float dtype; differentiable) over the VALID pixels of target [B,H,W]:
    CE = sum w_t (-log p_t) / sum w_t, Dice with I_c, sum p_c and count_c over valid pixels (smooth 1, mean over all C classes), Focal the
    mean of -0.25 (1 - q)^2 log q, q = p_t + 1e-8.  Ignored and out-of-range pixels are removed; with no valid pixel everything is 0."""
    c = logits.shape[1]
    z = logits.permute(0, 2, 3, 1).reshape(-1, c)
    t = target.reshape(-1).long()
    keep = valid_pixels(t, c, ignore_index)
    z, t = z[keep], t[keep]
    if z.shape[0] == 0:
        zero = logits.sum() * 0
        return zero, zero, zero, zero
    logp = F.log_softmax(z, dim=1)
    p = logp.exp()
    nll = -logp.gather(1, t[:, None])[:, 0]
    w = torch.ones_like(nll) if class_weights is None else class_weights.to(z.dtype)[t]
    ce = (w * nll).sum() / w.sum()
    onehot = F.one_hot(t, c).to(z.dtype)
    inter = (p * onehot).sum(0)
    card = p.sum(0) + onehot.sum(0)
    dsc = (1 - (2 * inter + 1.0) / (card + 1.0)).mean()
    q = p.gather(1, t[:, None])[:, 0] + 1e-8
    fl = (-0.25 * (1 - q) ** 2 * torch.log(q)).mean()
    return weights[0] * ce + weights[1] * dsc + weights[2] * fl, ce, dsc, fl


def ignore_blobs(seed, shape, fraction, cell=4):
    """bool mask of `shape` [B,H,W]: whole cell x cell blobs (tests/_data.blob_masks) covering about `fraction` of the pixels"""
    b, h, w = shape
    k = 20
    return D.blob_masks(seed, b, h, w, k, cell=cell) < int(round(fraction * k))


def test_statement_ce_is_torch_cross_entropy_with_ignore_index():
    rs = np.random.RandomState(3)
    for c, ignore in ((9, 255), (3, -100), (11, 0), (2, 255)):
        z = torch.from_numpy(rs.standard_normal((2, c, 13, 11)) * 3)
        t = D.blob_masks(40 + c, 2, 13, 11, c, cell=3)
        t[ignore_blobs(41 + c, t.shape, 0.3, cell=3)] = ignore
        cw = torch.from_numpy(D.class_weights(c)).double()
        assert 0 < int(valid_pixels(t, c, ignore).sum()) < t.numel()
        for w in (None, cw):
            want = F.cross_entropy(z, t, weight=w, ignore_index=ignore, reduction='mean')
            got = masked_multiloss(z, t, ignore, class_weights=w)[1]
            assert abs(got.item() - want.item()) < 1e-12


def test_statement_without_ignored_pixels_is_the_oracle():
    import oracle
    rs = np.random.RandomState(4)
    for c in (2, 9, 16):
        z = torch.from_numpy(rs.standard_normal((2, c, 10, 9)) * 3)
        t = D.blob_masks(50 + c, 2, 10, 9, c, cell=3)
        cw = torch.from_numpy(D.class_weights(c)).double()
        for weighted in (False, True):
            want = oracle.multiloss(z, t, (0.5, 0.5, 0.5), cw, weighted)
            for ignore in (None, 255, -100):
                got = masked_multiloss(z, t, ignore, class_weights=cw if weighted else None)
                assert max(abs(a.item() - b.item()) for a, b in zip(got, want)) < 1e-12


def test_statement_with_no_valid_pixel_is_zero():
    z = torch.randn(1, 4, 3, 3, dtype=torch.float64, requires_grad=True)
    out = masked_multiloss(z, torch.full((1, 3, 3), 255), 255)
    out[0].backward()
    assert all(v.item() == 0.0 for v in out) and float(z.grad.abs().max()) == 0.0


# ---- the C ABI: declared, bound, argument errors before any launch -----------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_bound_and_the_abi_version_stays():
    from pylc_amd import lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
    assert L.ABI_VERSION == 15 and L.lib.pylc_abi_version() == 15


def test_loss_entry_points_refuse_bad_arguments_on_the_host():
    from pylc_amd import lib as L
    lib = L.lib
    P = 64                                          # a non-NULL, aligned "pointer": every call below returns before anything is launched

    def stats(logits=P, pitch=12, target=P, tbytes=1, n=100, c=9, ign=255, cw=None, st=P, ws=P, bad=None):
        return lib.pylc_multiloss_stats_ex(logits, pitch, target, tbytes, n, c, ign, cw, st, ws, bad, None)

    def bwd(logits=P, pitch=12, target=P, tbytes=1, n=100, c=9, ign=255, cw=None, st=P, dl=P, dpitch=12, amax=None):
        return lib.pylc_multiloss_bwd_ex(logits, pitch, target, tbytes, n, c, ign, cw, st, 0.5, 0.5, 0.5, None, dl, dpitch, amax, None)

    for call, name in ((stats, b'multiloss_stats_ex'), (bwd, b'multiloss_bwd_ex')):
        for kw, text in (({'tbytes': 2}, b'target_bytes=2'), ({'tbytes': 0}, b'target_bytes=0'), ({'tbytes': 4}, b'target_bytes=4'),
                         ({'target': None}, b'target is NULL'), ({'pitch': 8}, b'pitch=8'), ({'n': 0}, b'N=0'), ({'n': -5}, b'N=-5'),
                         ({'c': 1}, b'n_classes=1'), ({'c': 17}, b'n_classes=17'), ({'logits': None}, b'NULL'),
                         ({'target': 60, 'tbytes': 8}, b'aligned')):
            assert call(**kw) == 1, (name, kw)                                     # PYLC_ERR_ARG
            msg = lib.pylc_last_error()
            assert name in msg and text in msg, (kw, msg)
    assert bwd(dpitch=8) == 1 and b'dpitch=8' in lib.pylc_last_error()
    assert lib.pylc_multiloss_finalize_ex(None, 9, 0.5, 0.5, 0.5, P, None) == 1 and b'NULL' in lib.pylc_last_error()
    assert lib.pylc_multiloss_finalize_ex(P, 17, 0.5, 0.5, 0.5, P, None) == 1 and b'n_classes=17' in lib.pylc_last_error()


def test_score_and_encode_entry_points_refuse_bad_arguments_on_the_host():
    from pylc_amd import lib as L
    lib = L.lib
    P = 64

    def score(logits=P, pitch=12, target=P, tbytes=1, n=100, c=9, mask=P, ign=255, counts=P):
        return lib.pylc_logits_score_ex(logits, pitch, target, tbytes, n, c, mask, ign, counts, None)
    assert score(tbytes=2) == 1 and b'target_bytes=2' in lib.pylc_last_error()
    assert score(target=None, tbytes=0) == 1 and b'counts without target' in lib.pylc_last_error()
    assert score(pitch=8) == 1 and b'pitch=8' in lib.pylc_last_error()
    assert score(n=0) == 1 and score(c=17) == 1 and b'n_classes=17' in lib.pylc_last_error()

    def cm(yt=P, tb=1, yp=P, pb=1, n=100, c=9, out=P, skipped=None):
        return lib.pylc_confusion_matrix_ex(yt, tb, yp, pb, n, c, 1, out, 255, skipped, None)
    assert cm(yt=None) == 1 and cm(n=0) == 1 and cm(c=1) == 1 and cm(c=17) == 1 and b'confusion_matrix_ex' in lib.pylc_last_error()
    assert cm(tb=2) == 1 and b'uint8 or int64' in lib.pylc_last_error()

    def enc(rgb=P, pal=P, c=9, out=P, unmatched=255):
        return lib.pylc_class_encode_resize_ex(rgb, 10, 10, pal, c, out, 10, 10, unmatched, None)
    assert enc(unmatched=256) == 1 and b'unmatched_value=256' in lib.pylc_last_error()
    assert enc(unmatched=-1) == 1 and b'unmatched_value=-1' in lib.pylc_last_error()
    assert enc(rgb=None) == 1 and enc(c=17) == 1 and b'n_classes=17' in lib.pylc_last_error()


def test_python_argument_rules_without_gpu():
    from pylc_amd import dataset, photo
    with pytest.raises(ValueError, match="'ignore' together with an ignore_index"):
        photo.encode_mask(np.zeros((4, 4, 3), np.uint8), [[0, 0, 0]], device='cpu', unmatched='ignore')
    with pytest.raises(ValueError, match='0..255'):
        photo.encode_mask(np.zeros((4, 4, 3), np.uint8), [[0, 0, 0]], device='cpu', unmatched=300)
    for bad in (0, 8, 256, -100):                  # inside the class range, or not a uint8 value: the histogram cannot separate it
        with pytest.raises(ValueError, match='ignore_index=%d' % bad):
            dataset.TileSet(3, 9, 128, ignore_index=bad)
    ts = dataset.TileSet(3, 9, 128, ignore_index=255)
    assert ts.ignore_index == 255 and ts._hist.shape == (0, 10) and ts.partition(0, 0.5).ignore_index == 255
    assert dataset.TileSet(3, 9, 128).ignore_index is None
    with pytest.raises(ValueError, match='ignore_index=3'):
        dataset.extract_photo(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), [[0, 0, 0]] * 9, tile=4, ignore_index=3)


# ---- the profile over valid pixels ---------------------------------------------------------------------------------------------------------
def test_profile_from_sums_with_an_ignore_bin_equals_hand_arithmetic():
    from pylc_amd import dataset
    tile, c = 4, 3                                  # 16 pixels per tile
    hist = np.array([[6, 2, 0, 8], [4, 4, 8, 0], [0, 0, 1, 15]], np.int64)         # last bin: ignored pixels
    sums = np.array([[[16 * 10], [16 * 100 + 60]], [[16 * 20], [16 * 400 + 15]], [[16 * 30], [16 * 900 + 240]]], np.int64)
    p = dataset.profile_from_sums(sums, hist, tile, c, ignore=True)
    assert p['px_dist'] == [[6, 2, 0], [4, 4, 8], [0, 0, 1]] and p['dset_px_dist'] == [10, 6, 9]
    assert p['dset_px_count'] == 25 and p['ignored_px_count'] == 23 and p['tile_px_count'] == 16 and p['n_samples'] == 3
    probs = np.array([10 / 25, 6 / 25, 9 / 25])
    assert np.abs(np.array(p['probs']) - probs).max() < 1e-15
    w = 1 / np.log(1.02 + probs)
    assert np.abs(np.array(p['weights']) - w / w.max()).max() < 1e-15
    assert abs(p['m2'] - 1.5 * (1 - (probs ** 2).sum())) < 1e-15
    assert abs(p['jsd'] - dataset.jsd(probs, np.full(3, 1 / 3))) < 1e-15
    # px_mean / px_std do not depend on the labels: the same as without the ignore bin
    q = dataset.profile_from_sums(sums, np.array([[16, 0, 0], [0, 16, 0], [0, 0, 16]]), tile, c)
    assert p['px_mean'] == q['px_mean'] == [20.0] and p['px_std'] == q['px_std'] and 'ignored_px_count' not in q
    assert abs(p['px_std'][0] - (2.0 + 1.0 + 4.0) / 3) < 1e-12                      # sqrt((N SS - S^2) / (N (N - 1))) per tile: 2, 1, 4
    dataset.oversample_rates(dict(p), n_samples_ratio=2.0)                          # works on such a profile unchanged
    # ignore=False: a non-zero last bin still raises, a zero one is still accepted
    with pytest.raises(ValueError, match='does not match the tile count'):
        dataset.profile_from_sums(sums, hist, tile, c)
    full = np.array([[6, 2, 8, 0], [4, 4, 8, 0], [0, 0, 16, 0]], np.int64)
    assert dataset.profile_from_sums(sums, full, tile, c)['dset_px_count'] == 48
    assert dataset.profile_from_sums(sums, full, tile, c, ignore=True)['ignored_px_count'] == 0
    with pytest.raises(ValueError, match='n_classes \\+ 1'):
        dataset.profile_from_sums(sums, full[:, :3], tile, c, ignore=True)
    with pytest.raises(ValueError, match='without a labelled pixel'):
        dataset.profile_from_sums(sums, np.array([[0, 0, 0, 16]] * 3), tile, c, ignore=True)


# ---- ScoreLog ---------------------------------------------------------------------------------------------------------------------------------
def test_score_log_close_with_ignored_and_bad_counts():
    from pylc_amd import metrics
    cm = np.array([[50, 5, 0], [3, 40, 7], [0, 0, 0]], np.int64)
    log = metrics.ScoreLog(3, ignore_index=255)
    assert log.ignore_index == 255 and metrics.ScoreLog(3).ignore_index is None
    assert log._zeros('cpu').numel() == 11 and metrics.ScoreLog(3)._zeros('cpu').numel() == 10
    log.counts = torch.cat([torch.from_numpy(cm).reshape(-1), torch.tensor([0, 321])])
    row = log.close(7, 1)
    want = metrics.scores(cm)
    assert set(row) == {'iter', 'epoch', 'f1', 'iou', 'mcc', 'class_iou', 'class_f1', 'support', 'ignored'}
    assert row['ignored'] == 321 and (row['iou'], row['f1'], row['mcc']) == (want['iou'], want['f1'], want['mcc'])
    assert row['support'] == [55, 50, 0] and np.array_equal(log.last_counts.numpy(), cm) and int(log.counts.abs().sum()) == 0
    # bad targets still raise, ignored ones alone give no row
    log.counts = torch.cat([torch.from_numpy(cm).reshape(-1), torch.tensor([4, 9])])
    with pytest.raises(ValueError, match=r'\b4 validation targets'):
        log.close(8, 1)
    log.counts = torch.cat([torch.zeros(9, dtype=torch.int64), torch.tensor([0, 100])])
    assert log.close(9, 1) is None and len(log.rows) == 1


# ---- Meta and checkpoints ------------------------------------------------------------------------------------------------------------------
def test_meta_field_round_trips_through_update():
    from pylc_amd.model import Meta
    assert Meta().ignore_index is None and Meta(ignore_index=255).ignore_index == 255
    m = Meta().update({'ignore_index': 255, 'not_a_field': 1})
    assert m.ignore_index == 255 and not hasattr(m, 'not_a_field')
    assert Meta().update(m).ignore_index == 255 and Meta(ignore_index=7).update(Meta()).ignore_index is None


def test_checkpoint_carries_ignore_index_and_old_files_load_with_none(tmp_path):
    from pylc_amd.model import Model, Meta
    from pylc_amd import checkpoint as ck, metrics
    m = Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, ignore_index=255), 'cpu')
    m.scores = metrics.ScoreLog(4)
    m.build()
    assert m.crit.ignore_index == 255 and m.scores.ignore_index == 255
    assert Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1), 'cpu').build().crit.ignore_index is None
    path = str(tmp_path / 'checkpoint.pth')
    ck.save(m, path)
    raw = ck.load_reference_file(path)
    assert raw['meta'].ignore_index == 255 and ck.meta_from_reference(raw['meta']).ignore_index == 255
    del raw['meta'].__dict__['ignore_index']                       # a file written before the field existed
    old = ck.meta_from_reference(raw['meta'])
    assert old.ignore_index is None and old.n_classes == 4
    ref = ck.load_reference_file(os.path.join(HERE, 'ref_checkpoint_tiny.pth'))
    assert not hasattr(ref['meta'], 'ignore_index') and ck.meta_from_reference(ref['meta']).ignore_index is None


def test_custom_op_is_registered_with_a_fake():
    import pylc_amd  # noqa: F401
    from pylc_amd import torch_ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'multiloss_ignore' in torch_ops.REGISTERED and 'multiloss_ignore_backward' in torch_ops.REGISTERED
    with FakeTensorMode():
        losses, stats, bad = torch.ops.pylc_hip.multiloss_ignore(torch.empty(2, 9, 8, 8), torch.empty(2, 8, 8, dtype=torch.uint8), None,
                                                                 0.5, 0.5, 0.5, 255)
        assert tuple(losses.shape) == (4,) and tuple(stats.shape) == (30,) and tuple(bad.shape) == (1,) and bad.dtype == torch.int64
