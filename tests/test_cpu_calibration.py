"""Calibration without a GPU: the host-side scores and fit, the numpy yardstick, the argument checks of the entry
points through the C ABI, and the keyword errors raised before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _calibration as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('pylc_reliability_counts', 'pylc_logits_reliability', 'pylc_logits_nll_grid', 'pylc_logits_nll_grid_workspace_bytes',
                'pylc_blend_accumulate_t')


def _counts(c, bins, rows):
    """rows: (class, bin, n, hits, mean confidence as k / 2^24 numerator per pixel)"""
    out = np.zeros(K.n_cells(c, bins), np.int64)
    for cls, b, n, hits, q in rows:
        out[(cls * bins + b) * 3:(cls * bins + b) * 3 + 3] = n, hits, n * q
    return out


# ---- reliability_scores ------------------------------------------------------------------------------------------------------------------
def test_scores_of_a_perfectly_calibrated_table_are_zero():
    from pylc_amd import calibration as cal
    half, three_q = 1 << 23, 3 << 22
    counts = _counts(3, 4, [(0, 2, 100, 50, half), (1, 3, 40, 30, three_q), (2, 2, 8, 4, half)])
    r = cal.reliability_scores(counts, 3, 4)
    assert r['ece'] == 0.0 and r['mce'] == 0.0 and r['class_ece'] == [0.0, 0.0, 0.0]
    assert r['n'] == 148 and r['ignored'] == 0
    assert r['accuracy'] == pytest.approx(84 / 148) and r['mean_confidence'] == pytest.approx(84 / 148)
    assert r['table'].shape == (4, 3) and r['table'][2].tolist() == [108.0, 0.5, 0.5] and r['table'][0].tolist() == [0.0, 0.0, 0.0]


def test_scores_of_a_one_bin_table():
    from pylc_amd import calibration as cal
    counts = _counts(2, 1, [(0, 0, 10, 5, 3 << 22), (1, 0, 30, 30, 3 << 22)])
    r = cal.reliability_scores(counts, 2, 1)
    assert r['ece'] == pytest.approx(abs(35 / 40 - 0.75)) and r['mce'] == pytest.approx(r['ece'])
    assert r['class_ece'] == pytest.approx([0.25, 0.25])
    ref = K.scores_ref(counts, 2, 1)
    assert r['ece'] == pytest.approx(ref['ece'], abs=1e-15) and r['class_ece'] == pytest.approx(ref['class_ece'], abs=1e-15)


def test_scores_with_empty_bins_and_a_class_never_predicted():
    from pylc_amd import calibration as cal
    counts = _counts(4, 10, [(0, 9, 60, 30, 1 << 24), (2, 5, 20, 20, 1 << 23), (0, 1, 20, 0, 1 << 22)])
    counts[-2] = 7                                     # ignored pixels are reported, not an error
    r = cal.reliability_scores(counts, 4, 10)
    gaps = {9: 0.5, 5: 0.5, 1: 0.25}
    assert r['ece'] == pytest.approx(0.6 * 0.5 + 0.2 * 0.5 + 0.2 * 0.25) and r['mce'] == pytest.approx(max(gaps.values()))
    assert r['class_ece'][1] == 0.0 and r['class_ece'][3] == 0.0 and r['class_ece'][2] == pytest.approx(0.5)
    assert r['class_ece'][0] == pytest.approx(0.75 * 0.5 + 0.25 * 0.25)
    assert r['ignored'] == 7 and r['n'] == 100
    ref = K.scores_ref(counts, 4, 10)
    assert r['ece'] == pytest.approx(ref['ece'], abs=1e-15) and r['mce'] == pytest.approx(ref['mce'], abs=1e-15)
    empty = cal.reliability_scores(np.zeros(K.n_cells(4, 10), np.int64), 4, 10)
    assert empty['ece'] == 0.0 and empty['n'] == 0 and empty['class_ece'] == [0.0] * 4


def test_scores_raise_on_the_error_cells():
    from pylc_amd import calibration as cal
    for cell in (-3, -1):
        counts = _counts(2, 5, [(0, 0, 1, 1, 0)])
        counts[cell] = 2
        with pytest.raises(ValueError):
            cal.reliability_scores(counts, 2, 5)
    with pytest.raises(ValueError):
        cal.reliability_scores(np.zeros(7, np.int64), 2, 5)


# ---- the bin and q rules -----------------------------------------------------------------------------------------------------------------
def test_bin_rule_edge_cases():
    assert K.bin_of(np.float32(0.0), 10) == 0 and K.bin_of(np.float32(1.0), 10) == 9 and K.bin_of(np.float32(0.5), 10) == 5
    # float32(0.3) = 0.300000011920929 and the fp32 product with 10 rounds to 3.0 exactly: bin 3 (in float64 the product is 3.0000001)
    assert np.float32(0.3) * np.float32(10) == np.float32(3.0) and K.bin_of(np.float32(0.3), 10) == 3
    # float32(0.7) = 0.699999988 but the fp32 product rounds UP to 7.0: the rule is the fp32 product, not the real one
    assert K.bin_of(np.float32(0.7), 10) == int(np.float32(np.float32(0.7) * np.float32(10)))
    for c in range(2, 17):                             # all-equal logits: conf = 1 / C
        p = np.float32(1) / np.float32(c)
        for bins in (1, 10, 15, 32):
            assert K.bin_of(p, bins) == min(bins - 1, int(np.float32(p * np.float32(bins))))
    assert K.bin_of(np.float32(1.0), 1) == 0 and K.bin_of(np.float32(0.999), 1) == 0
    assert K.q_of(np.float32(1.0)) == 1 << 24 and K.q_of(np.float32(0.0)) == 0 and K.q_of(np.float32(0.5)) == 1 << 23
    p = np.float32(1) - np.float32(2.0 ** -24)         # the largest float below 1: every bit of it survives
    assert K.q_of(p) == (1 << 24) - 1
    assert K.q_of(np.float32(2.0 ** -25)) == 0         # truncation: at most 2^-24 is lost per pixel


def test_counts_ref_layout_and_tail_order():
    conf = np.array([0.05, 0.95, 1.0, np.nan, 0.5, np.inf, -0.1, 1.5, 0.5, 0.5], np.float32)
    pred = np.array([0, 1, 1, 0, 2, 0, 0, 0, 1, 1], np.uint8)
    truth = np.array([0, 0, 1, 0, 2, 255, 7, 0, 255, 1], np.int64)
    got = K.counts_ref(conf, pred, truth, 3, 10, ignore_index=255)
    assert got[-3:].tolist() == [1, 2, 2]              # truth 7; two ignored (one of them with conf inf); NaN and 1.5 with a class target
    cells = got[:-3].reshape(3, 10, 3)
    assert cells[0, 0].tolist() == [1, 1, K.q_of(np.float32(0.05))]
    assert cells[1, 9].tolist() == [2, 1, K.q_of(np.float32(0.95)) + (1 << 24)]
    assert cells[2, 5].tolist() == [1, 1, 1 << 23] and cells[1, 5].tolist() == [1, 1, 1 << 23]
    assert cells[:, :, 0].sum() == 5
    # an ignore label inside the class range is ignored, not scored
    got0 = K.counts_ref(conf, pred, truth, 3, 10, ignore_index=0)
    assert got0[-2] == 4 and got0[-3] == 3


# ---- the temperature fit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [9, 16])
def test_temperature_is_recovered_from_sampled_labels(c):
    from pylc_amd import calibration as cal
    betas = K.default_betas()
    assert np.array_equal(betas, cal.default_betas()) and betas[16] == 1.0 and len(betas) == 33
    worst = 0.0
    for s in (0.6, 1.0, 1.7, 2.5):
        for seed in range(3):
            z, labels = K.sampled(16384, c, s, seed)
            sums, tail, _ = K.nll_sums_ref(z, labels, betas, c)
            fit_np = K.fit_temperature(betas, sums, tail[0])
            fit = cal.fit_temperature(betas, sums, int(tail[0]))
            assert not fit['at_edge'] and not fit_np['at_edge']
            assert fit['temperature'] == pytest.approx(fit_np['temperature'], rel=1e-9) and fit['nll'] == pytest.approx(fit_np['nll'], rel=1e-9)
            assert fit['nll'] <= fit['nll_at_1'] + 1e-12 and fit['nll_at_1'] == pytest.approx(sums[16] / tail[0], rel=1e-12)
            worst = max(worst, abs(fit_np['temperature'] / s - 1))
            assert abs(fit_np['temperature'] / s - 1) < 0.03, (c, s, seed, fit_np)
    print('worst relative error of the fitted temperature, C=%d: %.4f' % (c, worst))


def test_fit_reports_the_edge():
    from pylc_amd import calibration as cal
    betas = K.default_betas()
    z, labels = K.sampled(4096, 9, 8.0, 0)
    sums, tail, _ = K.nll_sums_ref(z, labels, betas, 9)
    for fit in (K.fit_temperature(betas, sums, tail[0]), cal.fit_temperature(betas, sums, int(tail[0]))):
        assert fit['at_edge'] and fit['temperature'] == pytest.approx(4.0)
    with pytest.raises(ValueError):
        cal.fit_temperature(betas, sums, 0)
    with pytest.raises(ValueError):
        cal.fit_temperature(betas[:2], sums[:2], 10)


def test_default_betas():
    from pylc_amd import calibration as cal
    b = cal.default_betas(5, 0.5, 2.0)
    assert b[0] == 0.5 and b[-1] == 2.0 and b[2] == 1.0 and np.allclose(np.diff(np.log(b)), np.log(4) / 4)
    with pytest.raises(ValueError):
        cal.default_betas(2)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from pylc_amd import lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read(), flags=re.S)
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r'\b%s\s*\(' % name, hdr), '%s is not declared' % name
        assert hasattr(dll, name) and name in L.SIGNATURES
    assert L.ABI_VERSION == 15 and dll.pylc_abi_version() == 15
    assert L.SIGNATURES['pylc_blend_accumulate_t'][1][:-1] == L.SIGNATURES['pylc_blend_accumulate'][1]


class _Bufs:
    """host buffers standing in for device ones: an argument error returns before anything is launched or read"""

    def __init__(self):
        self.keep = [np.zeros(4096, np.uint8) for _ in range(6)]
        base = [(a.ctypes.data + 63) & ~63 for a in self.keep]
        self.logits, self.target, self.mask, self.conf, self.counts, self.ws = base


def _rc(fn, *args):
    from pylc_amd.lib import lib
    return getattr(lib, fn)(*args)


def test_reliability_counts_argument_checks():
    b = _Bufs()
    ok = dict(conf=b.conf, pred=b.mask, truth=b.target, tb=1, n=100, c=9, bins=15, hi=0, ign=0, counts=b.counts)

    def call(**kw):
        a = dict(ok, **kw)
        return _rc('pylc_reliability_counts', a['conf'], a['pred'], a['truth'], a['tb'], a['n'], a['c'], a['bins'], a['hi'], a['ign'], a['counts'], None)
    for kw in (dict(bins=0), dict(bins=33), dict(c=1), dict(c=17), dict(n=0), dict(n=(1 << 39) + 1), dict(tb=4), dict(conf=None), dict(pred=None),
               dict(truth=None), dict(counts=None), dict(conf=b.conf + 2), dict(counts=b.counts + 4), dict(tb=8, truth=b.target + 4), dict(hi=2)):
        assert call(**kw) == 1, kw


def test_logits_reliability_argument_checks():
    b = _Bufs()
    ok = dict(logits=b.logits, pitch=12, target=b.target, tb=1, n=100, c=9, bins=15, beta=1.0, hi=0, ign=0, mask=b.mask, conf=b.conf, counts=b.counts)

    def call(**kw):
        a = dict(ok, **kw)
        return _rc('pylc_logits_reliability', a['logits'], a['pitch'], a['target'], a['tb'], a['n'], a['c'], a['bins'], a['beta'], a['hi'], a['ign'],
                   a['mask'], a['conf'], a['counts'], None)
    for kw in (dict(bins=0), dict(bins=33), dict(c=1), dict(c=17), dict(beta=0.0), dict(beta=-1.0), dict(beta=float('nan')), dict(beta=float('inf')),
               dict(target=None, tb=0), dict(target=None), dict(tb=0), dict(pitch=8), dict(n=0), dict(logits=None),
               dict(mask=None, conf=None, counts=None), dict(logits=b.logits + 2), dict(counts=b.counts + 4), dict(conf=b.conf + 2),
               dict(tb=8, target=b.target + 4), dict(tb=2)):
        assert call(**kw) == 1, kw


def test_nll_grid_argument_checks():
    from pylc_amd.lib import lib
    b = _Bufs()
    good = (ctypes.c_float * 33)(*([1.0] * 33))
    ok = dict(logits=b.logits, pitch=12, target=b.target, tb=1, n=100, c=9, betas=good, k=3, hi=0, ign=0, ws=b.ws, sums=b.counts, tail=b.mask)

    def call(**kw):
        a = dict(ok, **kw)
        return _rc('pylc_logits_nll_grid', a['logits'], a['pitch'], a['target'], a['tb'], a['n'], a['c'], a['betas'], a['k'], a['hi'], a['ign'],
                   a['ws'], a['sums'], a['tail'], None)
    zero, neg, nan = ((ctypes.c_float * 3)(1.0, v, 1.0) for v in (0.0, -2.0, float('nan')))
    for kw in (dict(k=0), dict(k=33), dict(betas=zero), dict(betas=neg), dict(betas=nan), dict(c=1), dict(c=17), dict(target=None, tb=0),
               dict(ws=None), dict(sums=None), dict(tail=None), dict(sums=b.counts + 4), dict(ws=b.ws + 4), dict(tail=b.mask + 4),
               dict(logits=b.logits + 2), dict(tb=8, target=b.target + 4), dict(n=0), dict(pitch=8)):
        assert call(**kw) == 1, kw
    size = lib.pylc_logits_nll_grid_workspace_bytes
    assert size(0, 3) == 0 and size(100, 0) == 0 and size(100, 33) == 0
    assert size(1, 1) == 8 and size(1025, 32) == 2 * 32 * 8 and size(1 << 30, 32) == 512 * 32 * 8


def test_blend_accumulate_t_argument_checks():
    b = _Bufs()
    for beta in (0.0, -1.0, float('nan'), float('inf')):
        assert _rc('pylc_blend_accumulate_t', b.logits, 12, 0, 1, 16, 16, 16, 8, 9, 0, b.ws, 12, None, beta) == 1
    assert _rc('pylc_blend_accumulate_t', b.logits, 12, 0, 1, 16, 16, 16, 8, 1, 0, b.ws, 12, None, 1.0) == 1          # C = 1
    assert _rc('pylc_blend_accumulate_t', b.logits, 12, 0, 1, 16, 16, 16, 8, 17, 0, b.ws, 12, None, 1.0) == 1         # C = 17
    assert _rc('pylc_blend_accumulate_t', b.logits + 4, 12, 0, 1, 16, 16, 16, 8, 9, 0, b.ws, 12, None, 1.0) == 1      # misaligned


# ---- keyword errors before any launch ----------------------------------------------------------------------------------------------------
class _FakeModel:
    def __init__(self, arch='deeplab', temperature=None):
        from pylc_amd.model import Meta
        self.meta = Meta(arch=arch, temperature=temperature)
        self.scores = None
        self.device = torch.device('cpu')


def test_temperature_needs_the_mean_blend_on_a_deeplab():
    from pylc_amd import inference, photo
    img = torch.zeros((3, 64, 64), dtype=torch.uint8)
    with pytest.raises(ValueError, match="temperature needs blend='mean'"):
        inference.predict_image(_FakeModel(), img, tile=64, temperature=1.5)
    with pytest.raises(ValueError, match="temperature needs blend='mean'"):
        photo.segment_photo(_FakeModel(), np.zeros((64, 64, 3), np.uint8), tile=64, temperature='meta')


def test_temperature_meta_unset_and_bad_values_raise():
    from pylc_amd import inference, photo
    img = torch.zeros((3, 64, 64), dtype=torch.uint8)
    with pytest.raises(ValueError, match='meta.temperature is unset'):
        inference.predict_image(_FakeModel(), img, tile=64, blend='mean', temperature='meta')
    with pytest.raises(ValueError, match='meta.temperature is unset'):
        photo.segment_photo(_FakeModel(), np.zeros((64, 64, 3), np.uint8), tile=64, blend='mean', temperature='meta')
    with pytest.raises(ValueError, match='meta.temperature is unset'):
        inference.predict_blend_mean(_FakeModel('unet'), img, 64, 32, temperature='meta')
    for bad in (0.0, -2.0, float('nan'), float('inf'), 'auto'):
        with pytest.raises(ValueError):
            inference.resolve_temperature(_FakeModel(), bad)
    assert inference.resolve_temperature(_FakeModel(), None) is None
    assert inference.resolve_temperature(_FakeModel(), 2.0) == 0.5
    assert inference.resolve_temperature(_FakeModel(temperature=4.0), 'meta') == 0.25


def test_meta_temperature_defaults_to_none_and_survives_update():
    from pylc_amd.model import Meta
    m = Meta()
    assert m.temperature is None
    m.update({'n_classes': 5})                         # a checkpoint written before the field existed
    assert m.temperature is None
    m.update({'temperature': 1.3})
    assert m.temperature == 1.3 and vars(Meta(temperature=2.0))['temperature'] == 2.0


def test_calibration_bins_need_score():
    from pylc_amd import train
    with pytest.raises(ValueError, match='calibration_bins needs score=True'):
        train.trainer(_FakeModel(), [], [], 1, calibration_bins=15)


def test_bins_are_checked_where_they_are_given():
    from pylc_amd import metrics, photo
    pal = np.arange(27, dtype=np.uint8).reshape(9, 3)
    for bad in (0, 33, 1.5, True):
        with pytest.raises(ValueError):
            metrics.ScoreLog(9, calibration_bins=bad)
        with pytest.raises(ValueError):
            photo.PhotoEvaluator(9, pal, calibration_bins=bad)
    log = metrics.ScoreLog(9, calibration_bins=15)
    assert log.calibration_bins == 15 and len(log.betas) == 33
    assert metrics.ScoreLog(9).calibration_bins is None


def test_photo_evaluator_with_bins_needs_a_confidence():
    from pylc_amd import photo
    pal = np.arange(27, dtype=np.uint8).reshape(9, 3)
    ev = photo.PhotoEvaluator(9, pal, calibration_bins=10)
    geom = {'h_scaled': 8, 'w_scaled': 8}
    res = photo.PhotoResult(torch.zeros((8, 8), dtype=torch.uint8), None, geom, None, 8, None)
    with pytest.raises(ValueError, match='needs result.confidence'):
        ev.add(res, np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match='reliability counts are given exactly'):
        ev.add_counts(np.zeros((9, 9), np.int64))
    with pytest.raises(ValueError, match='reliability counts are given exactly'):
        photo.PhotoEvaluator(9, pal).add_counts(np.zeros((9, 9), np.int64), reliability_counts=np.zeros(K.n_cells(9, 10), np.int64))
