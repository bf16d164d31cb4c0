"""Boundary distance, band counts and their users on the GPU (-m gpu): pylc_amd/boundary.py and csrc/boundary.hip against the numpy statement
tests/_boundary.py, bit for bit.

Sizes are named from the kernels' tiles: the column pass works on 64 x 64 pixels (a thread on 4 columns), the row pass on 128 wide x 8 high,
so 63 / 64 / 65 rows, 127 / 128 / 129 columns, 7 / 8 / 9 rows and widths that are no multiple of 4 are the edges; 300 x 400 is several tiles
each way.  Radii: 1, 3, 70 (a halo wider than a column tile and more than half a row tile) and 254 where the window is larger than the
image."""
import functools

import numpy as np
import pytest
import torch

from tests import _boundary as Bd
from tests import _regions as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 9), (8, 1), (3, 600), (63, 127), (64, 128), (65, 129), (7, 130), (9, 255), (130, 66), (300, 400)]
RADII = [1, 3, 70]


@functools.lru_cache(maxsize=None)
def masks_for(h, w):
    out = {'noise2': R.noise(h, w, 2, 1), 'noise16': R.noise(h, w, 16, 2), 'constant': R.constant(h, w), 'checkerboard': R.checkerboard(h, w)}
    if h >= 16 and w >= 16:
        out['blobs9'] = R.blobs(h, w, 9, 4, radius=3, noise_frac=0.02)
        out['blobs3'] = R.blobs(h, w, 3, 5, radius=12)
    return out


@functools.lru_cache(maxsize=None)
def want_distance(h, w, name, radius, ignore):
    """the statement's map of one test mask; ignore: None, 255 (scattered at 10 %) or 0 (a class of the mask itself)"""
    m = masks_for(h, w)[name]
    if ignore == 255:
        m = Bd.scatter_ignore(m, 0.1, seed=h + w)
    return m, Bd.distance_ref(m, radius, ignore)


def gpu_distance(m, dev, radius, ignore_index=None, ignore_from=None):
    from pylc_amd import boundary
    f = None if ignore_from is None else torch.from_numpy(ignore_from).to(dev)
    out = boundary.boundary_distance(torch.from_numpy(m).to(dev), radius, ignore_index, f)
    assert out.dtype == torch.int32 and tuple(out.shape) == m.shape
    return out.cpu().numpy()


# ---- distance maps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', RADII)
@pytest.mark.parametrize('hw', SIZES)
def test_distance_matches_statement(dev, hw, radius):
    for name in masks_for(*hw):
        m, want = want_distance(*hw, name, radius, None)
        got = gpu_distance(m, dev, radius)
        assert np.array_equal(got, want), (name, hw, radius, int((got != want).sum()))
    assert (gpu_distance(R.constant(*hw), dev, radius) == radius * radius + 1).all()          # one class: saturated everywhere


@pytest.mark.parametrize('hw', [(3, 600), (40, 9)])
def test_distance_radius_254(dev, hw):
    """the window is larger than the image"""
    for name in masks_for(*hw):
        m, want = want_distance(*hw, name, 254, None)
        assert np.array_equal(gpu_distance(m, dev, 254), want), (name, hw)
    m = R.constant(*hw)
    m[0, 0] = 1                                        # one pixel of another class: every distance is the distance to that corner
    assert np.array_equal(gpu_distance(m, dev, 254), Bd.distance_ref(m, 254))


@pytest.mark.parametrize('radius', RADII)
@pytest.mark.parametrize('hw', [(1, 9), (8, 1), (3, 600), (65, 129), (300, 400)])
def test_distance_with_ignore(dev, hw, radius):
    for name in masks_for(*hw):
        m, want = want_distance(*hw, name, radius, 255)
        got = gpu_distance(m, dev, radius, 255)
        assert np.array_equal(got == -1, m == 255), (name, hw)
        assert np.array_equal(got, want), (name, hw, radius)
        m, want = want_distance(*hw, name, radius, 0)                 # an ignore label inside the class range
        got = gpu_distance(m, dev, radius, 0)
        assert np.array_equal(got == -1, m == 0) and np.array_equal(got, want), (name, hw, radius, 'ignore 0')


@pytest.mark.parametrize('radius', [3, 70])
def test_distance_ignore_from(dev, radius):
    h, w = 130, 197
    m = R.blobs(h, w, 5, 6, radius=4)
    other = Bd.scatter_ignore(R.blobs(h, w, 5, 7, radius=4), 0.05, seed=2)
    other[40:60, 100:150] = 255
    got = gpu_distance(m, dev, radius, 255, ignore_from=other)
    assert np.array_equal(got, Bd.distance_ref(m, radius, 255, ignore_from=other))
    assert np.array_equal(got == -1, other == 255)
    merged = np.where(other == 255, 255, m).astype(np.uint8)
    assert np.array_equal(got, gpu_distance(merged, dev, radius, 255))


def test_band(dev):
    from pylc_amd import boundary
    m = Bd.scatter_ignore(R.blobs(90, 140, 4, 8, radius=5), 0.03, seed=4)
    band = boundary.boundary_band(torch.from_numpy(m).to(dev), 4, ignore_index=255)
    assert band.dtype == torch.bool and np.array_equal(band.cpu().numpy(), Bd.band_ref(m, 4, 255))


# ---- batches -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', [3, 70])
def test_batch_equals_single_images(dev, radius):
    h, w = 70, 131
    imgs = np.stack([R.blobs(h, w, 9, 1, radius=3), R.noise(h, w, 4, 3), R.checkerboard(h, w)])
    got = gpu_distance(imgs, dev, radius)
    for k in range(3):
        assert np.array_equal(got[k], gpu_distance(imgs[k], dev, radius)), k
    assert np.array_equal(got, Bd.distance_ref(imgs, radius))
    uniform = np.stack([R.constant(h, w, v) for v in (0, 1, 2)])      # nothing leaks across the edge between two images
    assert (gpu_distance(uniform, dev, radius) == radius * radius + 1).all()
    ign = np.stack([Bd.scatter_ignore(k, 0.1, seed=5) for k in imgs])
    assert np.array_equal(gpu_distance(ign, dev, radius, 255), Bd.distance_ref(ign, radius, 255))


# ---- alignment and determinism -------------------------------------------------------------------------------------------------------------
def test_alignment_and_determinism(dev):
    from pylc_amd import boundary
    h, w = 100, 333
    m = Bd.scatter_ignore(R.blobs(h, w, 9, 5, radius=3, noise_frac=0.02), 0.05, seed=6)
    p = R.blobs(h, w, 9, 6, radius=3, noise_frac=0.02)
    flat, pflat = torch.from_numpy(m).to(dev).reshape(-1), torch.from_numpy(p).to(dev).reshape(-1)
    first = boundary.boundary_distance(flat.reshape(h, w), 5, 255)
    assert np.array_equal(first.cpu().numpy(), Bd.distance_ref(m, 5, 255))
    assert torch.equal(boundary.boundary_distance(flat.reshape(h, w), 5, 255), first)         # two runs: the same bytes
    counts = boundary.boundary_counts(flat.reshape(h, w), pflat.reshape(h, w), 9, 5, 255)
    assert torch.equal(boundary.boundary_counts(flat.reshape(h, w), pflat.reshape(h, w), 9, 5, 255), counts)
    for off in (1, 2, 3):
        buf = torch.zeros(h * w + 8, device=dev, dtype=torch.uint8)
        view = buf[off:off + h * w]
        view.copy_(flat)
        pbuf = torch.zeros(h * w + 8, device=dev, dtype=torch.uint8)
        pview = pbuf[4 - off:4 - off + h * w]
        pview.copy_(pflat)
        assert view.data_ptr() % 4 == off
        assert torch.equal(boundary.boundary_distance(view.reshape(h, w), 5, 255), first), off
        assert torch.equal(boundary.boundary_counts(view.reshape(h, w), pview.reshape(h, w), 9, 5, 255), counts), off


# ---- counts --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def count_pair(c, ignore):
    h, w = 150, 260
    truth = R.blobs(h, w, c, 10, radius=5)
    pred = R.blobs(h, w, c, 10, radius=5, noise_frac=0.03)
    pred = np.where(np.roll(truth, 2, axis=1) != truth, np.roll(pred, 1, axis=0), pred).astype(np.uint8)      # borders that disagree
    if ignore is not None:
        truth = Bd.scatter_ignore(truth, 0.05, seed=c, value=ignore)
        truth[20:40, 30:90] = ignore
        pred = pred.copy()
        pred[100:104, 200:230] = ignore              # a prediction equal to the ignore label: in no band of its own
    return truth, pred


@pytest.mark.parametrize('radius', [2, 70])
@pytest.mark.parametrize('ignore', [None, 255, 0])
@pytest.mark.parametrize('c', [2, 9, 40])
def test_counts_match_statement(dev, c, ignore, radius):
    """C = 40 counts past the LDS counters (above 32 classes the wave totals go to the int64 cells directly)"""
    from pylc_amd import boundary
    truth, pred = count_pair(c, ignore)
    want = Bd.counts_ref(truth, pred, c, radius, ignore)
    assert want[-1] == 0 and want[:c * c].sum() > 0 and want[c * c:c * c + c].sum() > 0
    t, p = torch.from_numpy(truth).to(dev), torch.from_numpy(pred).to(dev)
    got = boundary.boundary_counts(t, p, c, radius, ignore)
    assert got.dtype == torch.int64 and got.shape == (c * c + 3 * c + 1,)
    assert np.array_equal(got.cpu().numpy(), want), (c, ignore, radius)
    # the two-map form gives the same numbers
    d2t = boundary.boundary_distance(t, radius, ignore)
    d2p = boundary.boundary_distance(p, radius, ignore, ignore_from=t if ignore is not None else None)
    assert torch.equal(boundary.boundary_counts_from_maps(t, p, d2t, d2p, c, radius, ignore), got)
    s, ref = boundary.boundary_scores(got, c), Bd.scores_ref(want, c)
    assert s['boundary_iou'] == ref['boundary_iou'] and np.array_equal(s['class_boundary_iou'], ref['class_boundary_iou'])
    assert 0.0 < s['boundary_iou'] < 1.0 and s['band_px'] == int(want[:c * c].sum())


def test_counts_accumulate_batches_and_out_of_range(dev):
    from pylc_amd import boundary
    truth, pred = count_pair(9, 255)
    t, p = torch.from_numpy(truth).to(dev), torch.from_numpy(pred).to(dev)
    once = boundary.boundary_counts(t, p, 9, 3, 255)
    acc = once.clone()
    assert boundary.boundary_counts(t, p, 9, 3, 255, counts=acc) is acc
    assert torch.equal(acc, 2 * once)                                 # added into, not overwritten
    # a batch is the sum of its images
    t3, p3 = torch.stack([t, p, t]), torch.stack([p, t, t])
    want = sum(Bd.counts_ref(a, b, 9, 3, 255) for a, b in ((truth, pred), (pred, truth), (truth, truth)))
    assert np.array_equal(boundary.boundary_counts(t3, p3, 9, 3, 255).cpu().numpy(), want)
    # values outside 0..C-1 that are not the ignore label land in the last cell, and the scores refuse them
    bad_t, bad_p = truth.copy(), pred.copy()
    bad_t[5, 5:9] = 9
    bad_t[60, 60] = 200
    bad_t[70, 10:13] = 1
    bad_p[70, 10:13] = 77
    bad_p[20:40, 30:90] = 99                                          # under an ignored truth: not counted at all
    want = Bd.counts_ref(bad_t, bad_p, 9, 3, 255)
    assert want[-1] == 8
    got = boundary.boundary_counts(torch.from_numpy(bad_t).to(dev), torch.from_numpy(bad_p).to(dev), 9, 3, 255)
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match='outside'):
        boundary.boundary_scores(got, 9)
    with pytest.raises(ValueError, match='counts'):
        boundary.boundary_counts(t, p, 9, 3, 255, counts=torch.zeros(5, device=dev, dtype=torch.int64))


def test_hand_case_on_device(dev):
    from pylc_amd import boundary
    from tests.test_cpu_boundary import issue_pair
    truth, pred = issue_pair()
    got = boundary.boundary_counts(torch.from_numpy(truth).to(dev), torch.from_numpy(pred).to(dev), 3, 3)
    assert np.array_equal(got.cpu().numpy(), Bd.counts_ref(truth, pred, 3, 3))
    s = boundary.boundary_scores(got, 3)
    assert s['boundary_iou'] == 0.5 and s['band_px'] == 240


# ---- where users meet it -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ignore', [None, 255])
def test_score_log_with_radius(dev, ignore):
    from pylc_amd import metrics
    c, b, h, w = 5, 2, 48, 72
    rng = np.random.default_rng(3)
    log = metrics.ScoreLog(c, ignore_index=ignore, boundary_radius=3)
    plain = metrics.ScoreLog(c, ignore_index=ignore)
    want = np.zeros(Bd.n_cells(c), np.int64)
    for k in range(2):
        field = np.stack([R.blobs(h, w, c, 20 + 2 * k + i, radius=4) for i in range(b)])
        logits = rng.standard_normal((b, c, h, w)).astype(np.float32)
        np.put_along_axis(logits, field[:, None].astype(np.int64), 1.5, axis=1)            # mostly the blob field, with errors
        target = np.stack([R.blobs(h, w, c, 20 + 2 * k + i, radius=4, noise_frac=0.01) for i in range(b)])
        if ignore is not None:
            target = Bd.scatter_ignore(target, 0.05, seed=k, value=ignore)
        dtype = torch.int64 if k else torch.uint8
        x, t = torch.from_numpy(logits).to(dev), torch.from_numpy(target).to(dev).to(dtype)
        log.add(x, t)
        plain.add(x, t)
        want += Bd.counts_ref(target, logits.argmax(1).astype(np.uint8), c, 3, ignore)
    row, base = log.close(7, 1), plain.close(7, 1)
    ref = Bd.scores_ref(want, c)
    assert row['boundary_iou'] == ref['boundary_iou'] and row['class_boundary_iou'] == [float(v) for v in ref['class_boundary_iou']]
    assert 0.0 < row['boundary_iou'] < 1.0 and 0.0 < row['trimap_iou'] < 1.0
    extra = {'boundary_iou', 'trimap_iou', 'class_boundary_iou'}
    assert set(row) == set(base) | extra and all(row[k] == base[k] for k in base)      # the other columns are what they were
    assert not log.boundary_counts.any() and log.close(8, 1) is None


def test_photo_evaluator_with_radius(dev):
    from pylc_amd import boundary, photo
    pal = np.array([[0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    h, w = 96, 160
    truths = [R.blobs(h, w, 4, 30 + k, radius=5) for k in range(2)]
    preds = [R.blobs(h, w, 4, 30 + k, radius=5, noise_frac=0.02) for k in range(2)]
    for radius in (4, 'auto'):
        r = boundary.default_radius(h, w) if radius == 'auto' else radius
        assert r == (4 if radius == 'auto' else radius)               # 0.02 * 186.6 = 3.7
        ev = photo.PhotoEvaluator(4, pal, boundary_radius=radius)
        plain = photo.PhotoEvaluator(4, pal)
        total = np.zeros(Bd.n_cells(4), np.int64)
        for truth, pred in zip(truths, preds):
            geom = {'w_full': w, 'h_full': h, 'w_scaled': w, 'h_scaled': h, 'w_fitted': w, 'h_fitted': h, 'offset': 0}
            res = photo.PhotoResult(torch.from_numpy(pred).to(dev), None, geom, None, 64, None)
            one, base = ev.add(res, pal[truth]), plain.add(res, pal[truth])
            want = Bd.counts_ref(truth, pred, 4, r)
            total += want
            ref = Bd.scores_ref(want, 4)
            assert one['boundary_iou'] == ref['boundary_iou'] and one['band_px'] == int(want[:16].sum())
            assert all(np.array_equal(one[k], base[k]) for k in base)
        assert np.array_equal(ev.boundary_counts.cpu().numpy(), total)
        agg = ev.aggregate()
        assert agg['boundary_iou'] == Bd.scores_ref(total, 4)['boundary_iou'] and agg['iou'] == plain.aggregate()['iou']
        assert set(agg) == set(plain.aggregate()) | {'boundary_iou', 'boundary_iou_mean', 'class_boundary_iou', 'trimap_iou', 'trimap_f1',
                                                     'trimap_mcc', 'band_px'}


def test_entry_point_argument_errors_on_device(dev):
    from pylc_amd.lib import lib, ptr, stream
    m = torch.zeros((8, 8), device=dev, dtype=torch.uint8)
    d2 = torch.full((8, 8), 7, device=dev, dtype=torch.int32)
    ws = torch.zeros(64, device=dev, dtype=torch.int32)
    assert lib.pylc_boundary_distance(ptr(m), 1, 8, 8, 0, -1, None, ptr(d2), ptr(ws), stream()) == 1
    assert lib.pylc_boundary_distance(ptr(m), 1, 8, 8, 255, -1, None, ptr(d2), ptr(ws), stream()) == 1
    assert lib.pylc_boundary_distance(ptr(m), 1, 8, 8, 3, 256, None, ptr(d2), ptr(ws), stream()) == 1
    torch.cuda.synchronize()
    assert (d2 == 7).all()                                            # nothing was launched
