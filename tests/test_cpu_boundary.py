"""CPU suite (-m "not gpu") of the boundary scores (pylc_amd/boundary.py, csrc/boundary.hip): the numpy statement
of the rules (tests/_boundary.py) against the definition (an all-pairs search) and against scipy's exact Euclidean transform, the hand
cases of the scores, and what the package side can check without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _boundary as Bd
from tests import _regions as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = [(1, 1), (1, 9), (8, 1), (5, 7), (20, 23)]
RADII = [1, 2, 4, 7, 30]


def small_masks(h, w):
    out = {'noise2': R.noise(h, w, 2, 1), 'noise5': R.noise(h, w, 5, 2), 'constant': R.constant(h, w), 'checkerboard': R.checkerboard(h, w),
           'stripes_h': R.stripes_h(h, w), 'stripes_v': R.stripes_v(h, w)}
    if h >= 16 and w >= 16:
        out['blobs'] = R.blobs(h, w, 4, 3, radius=3)
    return out


# ---- the statement against the definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', RADII)
@pytest.mark.parametrize('hw', SMALL)
def test_statement_matches_all_pairs_search(hw, radius):
    for name, m in small_masks(*hw).items():
        want = Bd.brute_ref(m, radius)
        got = Bd.distance_ref(m, radius)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, hw, radius)
        assert got.min() >= 1 and got.max() <= radius * radius + 1
        mi = Bd.scatter_ignore(m, 0.1, seed=radius)
        got = Bd.distance_ref(mi, radius, ignore_index=255)
        assert np.array_equal(got, Bd.brute_ref(mi, radius, ignore_index=255)), (name, hw, radius, 'ignore')
        assert np.array_equal(got == -1, mi == 255)


def test_statement_ignore_inside_class_range_and_ignore_from():
    m = R.noise(12, 15, 3, 7)
    got = Bd.distance_ref(m, 4, ignore_index=0)
    assert np.array_equal(got, Bd.brute_ref(m, 4, ignore_index=0)) and np.array_equal(got == -1, m == 0)
    other = Bd.scatter_ignore(R.noise(12, 15, 3, 8), 0.2, seed=1)
    merged = np.where(other == 255, 255, m).astype(np.uint8)
    assert np.array_equal(Bd.distance_ref(m, 4, 255, ignore_from=other), Bd.brute_ref(merged, 4, 255))
    batch = np.stack([m, R.noise(12, 15, 3, 9)])
    got = Bd.distance_ref(batch, 3)
    assert got.shape == batch.shape and np.array_equal(got[1], Bd.brute_ref(batch[1], 3))


@pytest.mark.parametrize('radius', [2, 7, 30])
def test_statement_matches_scipy_edt(radius):
    ndi = pytest.importorskip('scipy.ndimage')
    for name, m in small_masks(20, 23).items():
        got = Bd.distance_ref(m, radius)
        want = np.full(m.shape, radius * radius + 1, np.int64)
        for c in np.unique(m):
            inside = m == c
            if inside.all():
                continue                              # scipy's transform of an all-true array has no background to measure from
            d2 = np.rint(ndi.distance_transform_edt(inside) ** 2).astype(np.int64)
            want[inside] = np.minimum(radius * radius + 1, d2[inside])
        assert np.array_equal(got, want), (name, radius)


def test_image_edge_is_no_border_and_uniform_saturates():
    m = R.constant(9, 11, 4)
    assert (Bd.distance_ref(m, 3) == 10).all() and not Bd.band_ref(m, 3).any()
    m[:, 6:] = 5                                      # a split at column 6: distances grow away from it, the edges add nothing
    d2 = Bd.distance_ref(m, 3)
    assert np.array_equal(d2[4], [10, 10, 10, 9, 4, 1, 1, 4, 9, 10, 10])
    assert (d2 == d2[4]).all()


# ---- the scores ------------------------------------------------------------------------------------------------------------------------
def issue_pair():
    truth = np.ones((40, 60), np.uint8)
    truth[:, 29:] = 2
    pred = np.ones((40, 60), np.uint8)
    pred[:, 30:] = 2
    return truth, pred


def test_hand_case_one_column_off():
    from pylc_amd import boundary, metrics
    truth, pred = issue_pair()
    counts = Bd.counts_ref(truth, pred, 3, 3)
    cm, inter, gband, pband, outside = Bd.split_counts(counts, 3)
    assert outside == 0
    assert list(gband) == [0, 120, 120] and list(pband) == [0, 120, 120] and list(inter) == [0, 80, 80]
    assert np.array_equal(cm[1:, 1:], [[120, 0], [40, 80]]) and cm[0].sum() == 0 and cm[:, 0].sum() == 0
    s = boundary.boundary_scores(counts, 3)
    assert np.allclose(s['class_boundary_iou'], [0.0, 0.5, 0.5], rtol=0, atol=1e-15)
    assert s['boundary_iou'] == 0.5 and s['boundary_iou_mean'] == 0.5 and s['band_px'] == 240
    ref = Bd.scores_ref(counts, 3)
    assert ref['boundary_iou'] == s['boundary_iou'] and ref['boundary_iou_mean'] == s['boundary_iou_mean']
    tri = metrics.scores(cm)
    assert s['trimap_iou'] == tri['iou'] and s['trimap_f1'] == tri['f1'] and s['trimap_mcc'] == tri['mcc']
    # what the whole-mask scores say of the same pair
    plain = np.zeros((3, 3), np.int64)
    np.add.at(plain, (truth.reshape(-1), pred.reshape(-1)), 1)
    iou = metrics.per_class(plain)['iou']
    assert abs(iou[1] - 0.9667) < 5e-5 and abs(iou[2] - 0.9677) < 5e-5


def test_uniform_mask_scores_zero():
    from pylc_amd import boundary
    m = R.constant(12, 17, 2)
    counts = Bd.counts_ref(m, m, 4, 3)
    assert not counts.any()
    s = boundary.boundary_scores(counts, 4)
    assert s['band_px'] == 0 and not s['class_boundary_iou'].any()
    assert all(s[k] == 0.0 for k in ('boundary_iou', 'boundary_iou_mean', 'trimap_iou', 'trimap_f1', 'trimap_mcc'))


def test_identical_masks_score_one():
    from pylc_amd import boundary
    m = R.blobs(40, 50, 5, 3, radius=4)
    counts = Bd.counts_ref(m, m, 6, 2)
    s = boundary.boundary_scores(counts, 6)
    present = np.bincount(m.reshape(-1), minlength=6) > 0
    assert present.sum() >= 3 and not present[5]
    assert np.array_equal(s['class_boundary_iou'], present.astype(np.float64))
    assert s['boundary_iou'] == 1.0 and s['boundary_iou_mean'] == 1.0 and s['trimap_iou'] == 1.0 and s['band_px'] > 0


def test_counts_with_ignore_and_out_of_range():
    from pylc_amd import boundary
    truth, pred = issue_pair()
    truth[5:9, 27:33] = 255
    counts = Bd.counts_ref(truth, pred, 3, 3, ignore_index=255)
    cm, inter, gband, pband, outside = Bd.split_counts(counts, 3)
    assert outside == 0 and cm.sum() == gband.sum()
    # the hole is a border for both masks: rows 2..11 gain band pixels around it, every other row is as in the hand case
    t2, p2 = issue_pair()
    base = Bd.counts_ref(t2[12:], p2[12:], 3, 3)
    assert np.array_equal(Bd.counts_ref(truth[12:], pred[12:], 3, 3, 255), base)
    pred[0, 0] = 7
    counts = Bd.counts_ref(truth, pred, 3, 3, ignore_index=255)
    assert counts[-1] == 1
    with pytest.raises(ValueError, match='outside'):
        boundary.boundary_scores(counts, 3)


def test_default_radius():
    from pylc_amd import boundary
    assert boundary.default_radius(3072, 4096) == 102
    assert boundary.default_radius(40, 60) == 1 and boundary.default_radius(1, 1) == 1
    assert boundary.default_radius(512, 512) == 14            # 0.02 * 724.08 = 14.48
    assert boundary.default_radius(512, 512, ratio=0.01) == 7
    assert boundary.default_radius(20000, 20000) == 254
    for hw in ((3072, 4096), (40, 60), (777, 1234)):
        assert boundary.default_radius(*hw) == Bd.default_radius_ref(*hw)


# ---- the package side that needs no device ---------------------------------------------------------------------------------------------
def test_bindings_exist():
    from pylc_amd import lib as L
    import pylc_amd
    assert pylc_amd.boundary.boundary_counts is not None
    hdr = open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name, nargs, res in (('pylc_boundary_workspace_bytes', 3, ctypes.c_size_t), ('pylc_boundary_distance', 10, ctypes.c_int),
                             ('pylc_boundary_counts', 11, ctypes.c_int), ('pylc_boundary_counts_maps', 10, ctypes.c_int)):
        assert re.search(r'\b%s\s*\(' % name, hdr) and hasattr(dll, name), name
        assert len(L.SIGNATURES[name][1]) == nargs and L.SIGNATURES[name][0] is res, name
    assert L.lib.pylc_abi_version() == L.ABI_VERSION


def test_entry_point_errors_without_gpu():
    """argument validation happens on the host before any launch"""
    from pylc_amd.lib import lib
    one = 1 << 12                                     # any non-NULL, aligned address: nothing is dereferenced
    ok = lib.pylc_boundary_workspace_bytes
    assert ok(1, 5, 7) >= 2 * 5 * 8 and ok(3, 4, 8) >= 2 * 3 * 4 * 8 and ok(1, 5, 7) % 4 == 0 and ok(0, 4, 4) == 0 and ok(1, 1 << 16, 1 << 15) == 0
    dist = lib.pylc_boundary_distance
    assert dist(None, 1, 4, 4, 3, -1, None, one, one, None) == 1 and b'NULL' in lib.pylc_last_error()
    assert dist(one, 1, 4, 4, 3, -1, None, None, one, None) == 1
    assert dist(one, 1, 4, 4, 3, -1, None, one, None, None) == 1
    assert dist(one, 1, 4, 4, 0, -1, None, one, one, None) == 1 and b'radius' in lib.pylc_last_error()
    assert dist(one, 1, 4, 4, 255, -1, None, one, one, None) == 1
    assert dist(one, 1, 4, 4, 3, 256, None, one, one, None) == 1
    assert dist(one, 1, 4, 4, 3, -2, None, one, one, None) == 1
    assert dist(one, 0, 4, 4, 3, -1, None, one, one, None) == 1
    assert dist(one, 2, 1 << 15, 1 << 15, 3, -1, None, one, one, None) == 1
    assert dist(one, 1, 4, 4, 3, -1, one, one, one, None) == 1 and b'ignore_from' in lib.pylc_last_error()
    cnt = lib.pylc_boundary_counts
    assert cnt(None, one, 1, 4, 4, 3, 3, -1, one, one, None) == 1
    assert cnt(one, one, 1, 4, 4, 0, 3, -1, one, one, None) == 1 and b'n_classes' in lib.pylc_last_error()
    assert cnt(one, one, 1, 4, 4, 256, 3, -1, one, one, None) == 1
    assert cnt(one, one, 1, 4, 4, 3, 0, -1, one, one, None) == 1
    assert cnt(one, one, 1, 4, 4, 3, 255, -1, one, one, None) == 1
    assert cnt(one, one, 1, 4, 4, 3, 3, 300, one, one, None) == 1
    assert cnt(one, one, 1, 4, 4, 3, 3, -1, None, one, None) == 1
    assert cnt(one, one, 1, 4, 4, 3, 3, -1, one + 4, one, None) == 1 and b'aligned' in lib.pylc_last_error()
    maps = lib.pylc_boundary_counts_maps
    assert maps(one, one, one, None, 16, 3, 3, -1, one, None) == 1
    assert maps(one, one, one, one, 0, 3, 3, -1, one, None) == 1
    assert maps(one, one, one, one, 16, 3, 0, -1, one, None) == 1
    assert maps(one, one, one, one, 16, 300, 3, -1, one, None) == 1


def test_python_argument_errors():
    from pylc_amd import boundary
    m = torch.zeros((4, 5), dtype=torch.uint8)
    for call in (lambda: boundary.boundary_distance(m, 3), lambda: boundary.boundary_band(m, 3), lambda: boundary.boundary_counts(m, m, 3, 3),
                 lambda: boundary.boundary_distance(m[None], 3, 255, ignore_from=m[None])):
        with pytest.raises(ValueError, match='device'):               # a host tensor: there is no CPU path
            call()
    with pytest.raises(TypeError):
        boundary.boundary_distance(m.to(torch.int64), 3)
    with pytest.raises(TypeError):
        boundary.boundary_distance(m.numpy(), 3)
    with pytest.raises(TypeError):
        boundary.boundary_counts(m, m.float(), 3, 3)
    with pytest.raises(TypeError):
        boundary.boundary_distance(m, 2.5)
    for radius in (0, 255, -1):
        with pytest.raises(ValueError, match='radius'):
            boundary.boundary_distance(m, radius)
        with pytest.raises(ValueError, match='radius'):
            boundary.boundary_counts(m, m, 3, radius)
    with pytest.raises(ValueError):
        boundary.boundary_distance(m, 3, ignore_index=256)
    with pytest.raises(ValueError):
        boundary.boundary_distance(m.reshape(-1), 3)                      # not 2-D or 3-D
    with pytest.raises(ValueError, match='ignore_index'):
        boundary.boundary_distance(m, 3, ignore_from=m)
    with pytest.raises(ValueError, match='match'):
        boundary.boundary_distance(m, 3, 255, ignore_from=m[:, :4])
    with pytest.raises(ValueError, match='match'):
        boundary.boundary_counts(m, m[:3], 3, 3)
    with pytest.raises(ValueError, match='match'):
        boundary.boundary_counts(m, m[None], 3, 3)
    for c in (0, 256):
        with pytest.raises(ValueError, match='n_classes'):
            boundary.boundary_counts(m, m, c, 3)
    with pytest.raises(ValueError, match='entries'):
        boundary.boundary_scores(np.zeros(5, np.int64), 3)


def test_defaults_leave_rows_and_results_as_they_are():
    """without a radius ScoreLog and PhotoEvaluator have exactly the keys they had before the boundary scores existed"""
    from pylc_amd import metrics, photo
    log = metrics.ScoreLog(3)
    assert log.boundary_radius is None
    log.counts = torch.tensor([5, 1, 0, 2, 7, 1, 0, 0, 4, 0], dtype=torch.int64)
    row = log.close(10, 1)
    assert sorted(row) == ['class_f1', 'class_iou', 'epoch', 'f1', 'iou', 'iter', 'mcc', 'support']
    log = metrics.ScoreLog(3, ignore_index=255)
    log.counts = torch.tensor([5, 1, 0, 2, 7, 1, 0, 0, 4, 0, 6], dtype=torch.int64)
    assert sorted(log.close(10, 1)) == ['class_f1', 'class_iou', 'epoch', 'f1', 'ignored', 'iou', 'iter', 'mcc', 'support']
    pal = [[0, 0, 0], [255, 0, 0], [0, 255, 0]]
    ev = photo.PhotoEvaluator(3, pal)
    assert ev.boundary_radius is None
    cm = np.array([[5, 1, 0], [2, 7, 1], [0, 0, 4]], np.int64)
    assert sorted(ev.add_counts(cm)) == ['cmatrix', 'f1', 'iou', 'mcc']
    assert sorted(ev.add_counts(cm, cm)) == ['cmatrix', 'f1', 'iou', 'mcc']
    assert sorted(ev.aggregate()) == ['cmatrix', 'f1', 'iou', 'mcc']
    with pytest.raises(ValueError, match='band counts'):
        ev.add_counts(cm, cm, np.zeros(19, np.int64))


def test_radius_options_on_the_host():
    """a ScoreLog row and a PhotoEvaluator result with a radius, from counts made by the statement (no device)"""
    from pylc_amd import boundary, metrics, photo
    truth, pred = issue_pair()
    band = Bd.counts_ref(truth, pred, 3, 3)
    plain = np.zeros((3, 3), np.int64)
    np.add.at(plain, (truth.reshape(-1), pred.reshape(-1)), 1)
    log = metrics.ScoreLog(3, boundary_radius=3)
    log.counts = torch.from_numpy(np.concatenate([plain.reshape(-1), [0]]))
    log.boundary_counts = torch.from_numpy(band.copy())
    row = log.close(4, 0)
    assert row['boundary_iou'] == 0.5 and row['class_boundary_iou'] == [0.0, 0.5, 0.5]
    assert row['trimap_iou'] == boundary.boundary_scores(band, 3)['trimap_iou']
    assert not log.boundary_counts.any()                              # zeroed for the next pass
    ev = photo.PhotoEvaluator(3, [[0, 0, 0], [255, 0, 0], [0, 255, 0]], boundary_radius='auto')
    one = ev.add_counts(plain, None, band)
    assert one['boundary_iou'] == 0.5 and one['band_px'] == 240
    ev.add_counts(plain, plain, band)
    agg = ev.aggregate()
    assert agg['boundary_iou'] == 0.5 and agg['band_px'] == 480
    with pytest.raises(ValueError, match='band counts'):
        ev.add_counts(plain, plain)
    for bad in (0, 255):
        with pytest.raises(ValueError, match='radius'):
            metrics.ScoreLog(3, boundary_radius=bad)
        with pytest.raises(ValueError, match='radius'):
            photo.PhotoEvaluator(3, [[0, 0, 0], [255, 0, 0], [0, 255, 0]], boundary_radius=bad)
    with pytest.raises(ValueError):
        metrics.ScoreLog(3, ignore_index=-100, boundary_radius=3)
