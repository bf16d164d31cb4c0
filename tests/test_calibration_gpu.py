"""Calibration on the GPU (csrc/calibration.hip) against the numpy yardstick tests/_calibration.py.

Sizes come from the kernels' geometry: a lane takes 4 pixels, a block 1024, a round of the grid 256 x 1024 = 262144; so 1, 3, 5 (below and
across one lane), 255, 1023, 1025 (across one block), 262144 + 5 (a second round for some blocks) and 2 * 262144 + 1027 (a third, the
ping-pong's two register sets both in use)."""
import numpy as np
import pytest
import torch

from tests import _calibration as K
from tests import _regions as R

pytestmark = pytest.mark.gpu

ROUND = 262144
SIZES = [1, 3, 5, 255, 1023, 1025, ROUND + 5, 2 * ROUND + 1027]
CLASSES = [2, 9, 16]
BINS = [1, 10, 15, 32]


def _nhwc(z, dev, pitch=None):
    """[N, C] float32 logits -> a [1, C, 1, N] device tensor with NHWC memory of the given pitch"""
    from pylc_amd import ops
    n, c = z.shape
    t = ops.zeros_nhwc(1, c, 1, n, dev, pitch=pitch)
    t.copy_(torch.from_numpy(np.ascontiguousarray(z.T)).view(1, c, 1, n))
    return t


def _targets(n, c, seed, dtype, ignore=None, outside=0):
    """a blob mask with some pixels set to the ignore label and `outside` pixels out of range"""
    t = K.blob_mask(n, c, seed).astype(np.int64)
    rng = np.random.default_rng(seed + 100)
    if ignore is not None and ignore >= c:
        t[rng.random(n) < 0.1] = ignore
    for i in rng.integers(0, n, outside):
        t[i] = c + 3 if dtype == np.uint8 else (-1 if i % 2 else 1 << 40)
    return t.astype(dtype)


def _planted_conf(n, bins, seed):
    """confidences in [0, 1] clustered near the top, with exact 0, 1 and bin edges k / bins planted"""
    rng = np.random.default_rng(seed)
    p = (1 - rng.random(n) ** 3 * 0.9).astype(np.float32)
    idx = rng.permutation(n)
    plant = [0.0, 1.0] + [k / bins for k in range(bins + 1)]
    for i, v in zip(idx, plant):
        p[i] = np.float32(v)
    return p


# ---- a. reliability_counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i,n', list(enumerate(SIZES)))
def test_reliability_counts_equal_the_model(dev, i, n):
    from pylc_amd import calibration as cal
    c, bins = CLASSES[i % 3], BINS[i % 4]
    for j, (tdtype, ignore) in enumerate([(np.uint8, None), (np.int64, 255), (np.uint8, 0)]):
        conf = _planted_conf(n, bins, i)
        if n >= 255:                                   # values no confidence may have: counted in the last cell, never binned
            conf[7:12] = [np.nan, np.inf, -0.1, 1.5, -np.inf]
        pred = (K.blob_mask(n, c, i + 1) if j != 1 else R.noise(1, n, c, i).reshape(-1)).astype(np.uint8)
        truth = _targets(n, c, i, tdtype, ignore, outside=3 if n >= 255 else 0)
        want = K.counts_ref(conf, pred, truth, c, bins, ignore)
        got = cal.reliability_counts(torch.from_numpy(conf).to(dev)[None], torch.from_numpy(pred).to(dev)[None],
                                     torch.from_numpy(truth).to(dev)[None], c, bins, ignore)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (n, c, bins, tdtype, ignore)
        assert want.sum() > 0 and want[:-3:3].sum() + want[-3:].sum() == n           # every pixel is counted exactly once


def test_reliability_counts_constant_mask_one_cell(dev):
    """the serialising case: every pixel in one cell (one class, one confidence, all hits), and the q sum past 2^32 within one wave's
    rounds (conf = 1: 256 pixels x 2^24)"""
    from pylc_amd import calibration as cal
    n = ROUND + 5
    for value in (np.float32(1.0), np.float32(0.93)):
        conf = np.full(n, value, np.float32)
        pred = np.full(n, 3, np.uint8)
        dp = torch.from_numpy(pred).to(dev)[None]
        got = cal.reliability_counts(torch.from_numpy(conf).to(dev)[None], dp, dp, 9, 15)
        want = K.counts_ref(conf, pred, pred, 9, 15)
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.count_nonzero(want) == 3 and want.max() == n * int(K.q_of(value))


def test_reliability_counts_unaligned_maps_and_accumulation(dev):
    """maps that start 1 element into their buffers (the pixel-by-pixel path) give the aligned path's counts; a second launch adds"""
    from pylc_amd import calibration as cal
    n, c, bins = 1025, 9, 10
    conf, pred, truth = _planted_conf(n + 1, bins, 3), K.blob_mask(n + 1, c, 4), _targets(n + 1, c, 5, np.int64, 255, 2)
    dc, dp, dt = (torch.from_numpy(a).to(dev) for a in (conf, pred, truth))
    got = cal.reliability_counts(dc[1:].view(1, n), dp[1:].view(1, n), dt[1:].view(1, n), c, bins, 255)
    want = K.counts_ref(conf[1:], pred[1:], truth[1:], c, bins, 255)
    assert np.array_equal(got.cpu().numpy(), want)
    cal.reliability_counts(dc[:n].view(5, 205), dp[:n].view(5, 205), dt[:n].view(5, 205), c, bins, 255, counts=got)
    assert np.array_equal(got.cpu().numpy(), want + K.counts_ref(conf[:n], pred[:n], truth[:n], c, bins, 255))


# ---- b. logits_reliability ---------------------------------------------------------------------------------------------------------------
def _check_logits_reliability(dev, z, target, c, bins, temperature, ignore, pitch=None):
    from pylc_amd import calibration as cal
    n = z.shape[0]
    x = _nhwc(z, dev, pitch)
    tgt = torch.from_numpy(target).to(dev).view(1, 1, n)
    counts, mask, conf = cal.logits_reliability(x, tgt, bins, temperature, ignore, return_mask=True, return_confidence=True)
    mask, conf, counts = mask.cpu().numpy().reshape(-1), conf.cpu().numpy().reshape(-1), counts.cpu().numpy()
    beta = 1.0 if temperature is None else np.float32(1.0 / temperature)
    assert np.array_equal(mask, z.argmax(1).astype(np.uint8))                                     # (i) first maximum
    err = np.abs(conf.astype(np.float64) - K.conf_f64(z, beta)).max()
    assert err <= (c + 8) * 2.0 ** -23, (err, c)                                                 # (ii)
    assert np.array_equal(counts, K.counts_ref(conf, mask, target, c, bins, ignore))              # (iii)
    assert counts[-1] == 0
    return conf, counts


@pytest.mark.parametrize('i,n', list(enumerate(SIZES)))
def test_logits_reliability_sizes(dev, i, n):
    c, bins = CLASSES[(i + 1) % 3], BINS[(i + 1) % 4]
    z = K.logits(n, c, 3.0, i)
    z[::7] = z[::7, :1]                                # ties: all-equal logits
    for tdtype, ignore, temperature in [(np.uint8, 255, None), (np.int64, 0, 2.5), (np.int64, None, 0.5)]:
        target = _targets(n, c, i, tdtype, ignore, outside=2 if n >= 255 and ignore is not None else 0)
        if ignore is None:
            target = np.minimum(target, c - 1)
        conf, counts = _check_logits_reliability(dev, z, target, c, bins, temperature, ignore)
        assert np.all(conf[::7] == np.float32(1) / np.float32(c))                                 # a tie: class 0 (checked above), conf 1 / C


@pytest.mark.parametrize('pitch', [9, 12])
def test_logits_reliability_pitches_and_saturation(dev, pitch):
    """C = 9 at pitch 9 (float-by-float loads) and 12 (16-byte loads); logits x 20 so that most pixels saturate to conf = 1"""
    n, c = 1025, 9
    z = K.logits(n, c, 3.0, 11)
    target = _targets(n, c, 2, np.uint8, 255, 2)
    for scale, temperature in [(1.0, None), (1.0, 0.5), (1.0, 2.5), (20.0, None)]:
        conf, counts = _check_logits_reliability(dev, (z * np.float32(scale)).astype(np.float32), target, c, 15, temperature, 255, pitch)
    assert (conf == 1.0).mean() > 0.5 and counts[-3] == 2


def test_logits_reliability_every_class_count(dev):
    for c in range(2, 17):
        _check_logits_reliability(dev, K.logits(1025, c, 2.0, c), _targets(1025, c, c, np.uint8), c, 15, None, None)


def test_logits_reliability_batch_of_images(dev):
    """a [2, C, 65, 129] batch as a net returns it"""
    from pylc_amd import calibration as cal, ops
    b, c, h, w = 2, 9, 65, 129
    z = K.logits(b * h * w, c, 3.0, 5)
    x = ops.zeros_nhwc(b, c, h, w, dev, pitch=12)
    x.copy_(torch.from_numpy(z.reshape(b, h, w, c)).permute(0, 3, 1, 2))
    target = _targets(b * h * w, c, 6, np.int64, 255, 1)
    counts, conf = cal.logits_reliability(x, torch.from_numpy(target).to(dev).view(b, h, w), 10, ignore_index=255, return_confidence=True)
    assert tuple(conf.shape) == (b, h, w)
    conf = conf.cpu().numpy().reshape(-1)
    assert np.abs(conf - K.conf_f64(z)).max() <= (c + 8) * 2.0 ** -23
    assert np.array_equal(counts.cpu().numpy(), K.counts_ref(conf, z.argmax(1), target, c, 10, 255))
    # maps only, without a target; counts are added into
    mask, = cal.logits_reliability(x, return_mask=True)[1:]
    assert np.array_equal(mask.cpu().numpy().reshape(-1), z.argmax(1).astype(np.uint8))
    twice = cal.logits_reliability(x, torch.from_numpy(target).to(dev).view(b, h, w), 10, ignore_index=255, counts=counts.clone())
    assert torch.equal(twice, 2 * counts)


@pytest.mark.parametrize('off', [1, 2, 3])
def test_logits_reliability_mask_out_past_a_dword(dev, off):
    """mask_out starting 1, 2 and 3 bytes past a dword, through the C ABI: the bytes before and after the mask are not written"""
    from pylc_amd.lib import lib, check, stream
    n, c, bins = 1025, 9, 15
    z = K.logits(n, c, 3.0, off)
    x = _nhwc(z, dev, 12)
    target = torch.from_numpy(_targets(n, c, off, np.uint8)).to(dev)
    buf = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
    conf = torch.full((n + 8,), -7.0, device=dev)
    counts = torch.zeros(K.n_cells(c, bins), dtype=torch.int64, device=dev)
    assert buf.data_ptr() % 4 == 0
    check(lib.pylc_logits_reliability(x.data_ptr(), 12, target.data_ptr(), 1, n, c, bins, 1.0, 0, 0, buf.data_ptr() + 4 + off,
                                      conf.data_ptr() + 4, counts.data_ptr(), stream()))
    got, cf = buf.cpu().numpy(), conf.cpu().numpy()
    assert np.all(got[:4 + off] == 0xEE) and np.all(got[4 + off + n:] == 0xEE)
    assert np.array_equal(got[4 + off:4 + off + n], z.argmax(1).astype(np.uint8))
    assert cf[0] == -7.0 and np.all(cf[1 + n:] == -7.0)
    assert np.array_equal(counts.cpu().numpy(), K.counts_ref(cf[1:1 + n], got[4 + off:4 + off + n], target.cpu().numpy(), c, bins))


# ---- c. nll_grid -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i,n', list(enumerate(SIZES)))
def test_nll_grid_sizes(dev, i, n):
    from pylc_amd import calibration as cal
    c = CLASSES[i % 3]
    betas = K.default_betas() if n <= 1025 else np.array([0.25, 1.0, 3.0])        # (33 betas: two launches of 17 and 16)
    tdtype, ignore = [(np.uint8, 255), (np.int64, 0), (np.int64, None)][i % 3]
    z = K.logits(n, c, 3.0, i)
    target = _targets(n, c, i, tdtype, ignore, outside=2 if n >= 255 and ignore is not None else 0)
    if ignore is None:
        target = np.minimum(target, c - 1)
    want, tail, bound = K.nll_sums_ref(z, target, betas.astype(np.float32), c, ignore)
    x, tgt = _nhwc(z, dev, 12 if c == 9 and i % 2 else None), torch.from_numpy(target).to(dev).view(1, 1, n)
    sums, got_tail = cal.nll_grid(x, tgt, betas, ignore)
    assert np.array_equal(got_tail.cpu().numpy(), tail) and tail.sum() == n
    diff = np.abs(sums.cpu().numpy() - want)
    print('nll_grid n=%d C=%d: worst |diff| / bound = %.3f' % (n, c, (diff / np.maximum(bound, 1e-300)).max()))
    assert np.all(diff <= bound), (diff, bound)
    again, _ = cal.nll_grid(x, tgt, betas, ignore)
    assert torch.equal(again.view(torch.int64), sums.view(torch.int64))           # bitwise reproducible


def test_nll_grid_half_batches_add_up(dev):
    from pylc_amd import calibration as cal
    n, c = 2 * 3000, 9
    betas = K.default_betas(9)
    z, target = K.logits(n, c, 4.0, 1), _targets(n, c, 1, np.uint8, 255)
    whole, tail = cal.nll_grid(_nhwc(z, dev), torch.from_numpy(target).to(dev).view(1, 1, n), betas, 255)
    sums = tail2 = None
    for part in (slice(0, n // 2), slice(n // 2, n)):
        sums, tail2 = cal.nll_grid(_nhwc(z[part], dev), torch.from_numpy(target[part]).to(dev).view(1, 1, n // 2), betas, 255, sums, tail2)
    assert torch.equal(tail, tail2)
    assert float(((sums - whole).abs() / whole.abs()).max()) <= 1e-12


# ---- d. end to end -----------------------------------------------------------------------------------------------------------------------
def test_fitted_temperature_end_to_end(dev):
    from pylc_amd import calibration as cal
    n, c, s, bins = 65536, 9, 1.7, 15
    z, labels = K.sampled(n, c, s, 0)
    betas = cal.default_betas()
    x, tgt = _nhwc(z, dev), torch.from_numpy(labels).to(dev).view(1, 1, n)
    sums, tail = cal.nll_grid(x, tgt, betas)
    fit = cal.fit_temperature(betas, sums, int(tail[0]))
    want, wtail, _ = K.nll_sums_ref(z, labels, betas.astype(np.float32), c)
    ref = K.fit_temperature(betas, want, wtail[0])
    assert not fit['at_edge'] and abs(fit['temperature'] / ref['temperature'] - 1) < 1e-3 and abs(fit['temperature'] / s - 1) < 0.03
    before = cal.reliability_scores(cal.logits_reliability(x, tgt, bins), c, bins)
    after = cal.reliability_scores(cal.logits_reliability(x, tgt, bins, temperature=fit['temperature']), c, bins)
    print('fitted T = %.4f (numpy %.4f, true %.1f); ECE %.4f -> %.4f' % (fit['temperature'], ref['temperature'], s, before['ece'], after['ece']))
    assert after['ece'] < before['ece'] and before['n'] == after['n'] == n
    assert abs(before['accuracy'] - after['accuracy']) < 1e-12 and after['mean_confidence'] < before['mean_confidence']


# ---- e. the blend --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [9, 16])
def test_blend_accumulate_t_against_the_plain_entry_point(dev, c):
    """a 3-by-2 grid of random logit tiles: beta = 1 gives pylc_blend_accumulate's bytes, beta = 0.5 those of the plain entry point fed
    0.5 * logits (halving is exact, so (z - max) * 0.5 == 0.5 z - max(0.5 z) bit for bit)"""
    from pylc_amd.lib import lib, check, stream
    out, stride, h, w = 16, 8, 24, 32
    cp = (c + 3) // 4 * 4
    rng = np.random.default_rng(c)
    z = np.zeros((6, out, out, cp), np.float32)
    z[..., :c] = rng.standard_normal((6, out, out, c)) * 4

    def run(tiles, beta, flip=0):
        t = torch.from_numpy(tiles).to(dev)
        acc = torch.zeros((h, w, cp), device=dev)
        for first, count in ((0, 4), (4, 2)):
            src = t[first:first + count].contiguous()
            if beta is None:
                check(lib.pylc_blend_accumulate(src.data_ptr(), cp, first, count, h, w, out, stride, c, flip, acc.data_ptr(), cp, stream()))
            else:
                check(lib.pylc_blend_accumulate_t(src.data_ptr(), cp, first, count, h, w, out, stride, c, flip, acc.data_ptr(), cp, stream(), beta))
        return acc
    plain = run(z, None)
    assert float(plain[..., :c].sum(-1).min()) > 0.99
    assert torch.equal(run(z, 1.0), plain) and torch.equal(run(z, 1.0, 1), run(z, None, 1))
    half = run((z * np.float32(0.5)).astype(np.float32), None)
    assert torch.equal(run(z, 0.5), half) and not torch.equal(half, plain)


@pytest.fixture(scope='module')
def deeplab(dev):
    import oracle
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    from tests import _data as D
    runtime.dropout_enabled = False
    img = D.learnable_tiles(21, 1, 192, 9, cell=16)[0][0, :, :128, :]          # [3,128,192]
    model = Model(Meta(), dev).build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec('deeplab', 'resnet', 9, 3), salt=2))
    model.net.eval()
    return {'model': model, 'img': img}


def test_temperature_one_gives_the_bytes_of_none(dev, deeplab):
    from pylc_amd import inference, photo
    model, img = deeplab['model'], deeplab['img']
    mask, conf = inference.predict_image(model, img, 64, 32, blend='mean', return_confidence=True)
    m1, c1 = inference.predict_image(model, img, 64, 32, blend='mean', return_confidence=True, temperature=1.0)
    assert torch.equal(m1, mask) and torch.equal(c1, conf)
    m2, c2 = inference.predict_image(model, img, 64, 32, blend='mean', return_confidence=True, temperature=2.0, flip=True)
    assert not torch.equal(c2, conf) and float(c2.mean()) < float(conf.mean())       # a higher temperature flattens the probabilities
    photo_img = img.permute(1, 2, 0).clamp(0, 255).to(torch.uint8).numpy()
    plain = photo.segment_photo(model, photo_img, 64, 32, blend='mean', return_confidence=True)
    model.meta.temperature = 1.0
    try:
        res = photo.segment_photo(model, photo_img, 64, 32, blend='mean', return_confidence=True, temperature='meta')
    finally:
        model.meta.temperature = None
    assert torch.equal(res.mask, plain.mask) and torch.equal(res.confidence, plain.confidence)


# ---- f. ScoreLog and PhotoEvaluator ------------------------------------------------------------------------------------------------------
def test_score_log_with_calibration_bins(dev):
    from pylc_amd import calibration as cal, metrics, ops
    c, bins, shapes = 9, 15, [(2, 33, 40), (1, 64, 64), (3, 17, 19)]
    zs, ts, batches = [], [], []
    for k, (b, h, w) in enumerate(shapes):
        z, labels = K.sampled(b * h * w, c, 1.7, k)
        labels[::11] = 255
        x = ops.zeros_nhwc(b, c, h, w, dev)
        x.copy_(torch.from_numpy(z.reshape(b, h, w, c)).permute(0, 3, 1, 2))
        batches.append((x, torch.from_numpy(labels).to(dev).view(b, h, w)))
        zs.append(z)
        ts.append(labels)
    z, labels = np.concatenate(zs), np.concatenate(ts)
    n = z.shape[0]
    plain, log = metrics.ScoreLog(c, 255), metrics.ScoreLog(c, 255, calibration_bins=bins)
    for x, t in batches:
        plain.add(x, t)
        log.add(x, t)
    whole, tgt = _nhwc(z, dev), torch.from_numpy(labels).to(dev).view(1, 1, n)
    want_counts = cal.logits_reliability(whole, tgt, bins, ignore_index=255)
    assert torch.equal(log.reliability_counts, want_counts)                       # counts exactly
    assert np.array_equal(log.nll_tail.cpu().numpy(), [(labels != 255).sum(), 0, (labels == 255).sum()])
    betas = cal.default_betas().astype(np.float32)
    ref, tail, bound = K.nll_sums_ref(z, labels, betas, c, 255)
    assert np.all(np.abs(log.nll_sums.cpu().numpy() - ref) <= bound)              # NLL by the per-pixel bound
    row0, row = plain.close(5, 1), log.close(5, 1)
    assert set(row) == set(row0) | {'ece', 'mce', 'nll', 'class_ece', 'temperature'}
    assert set(row0) == {'iter', 'epoch', 'f1', 'iou', 'mcc', 'class_iou', 'class_f1', 'support', 'ignored'}
    assert all(row[k] == row0[k] for k in row0)
    s = cal.reliability_scores(want_counts, c, bins)
    assert row['ece'] == s['ece'] and row['mce'] == s['mce'] and row['class_ece'] == [float(v) for v in s['class_ece']]
    fit = K.fit_temperature(betas, ref, tail[0])
    assert abs(row['temperature'] / fit['temperature'] - 1) < 1e-3 and abs(row['nll'] - ref[16] / tail[0]) <= bound[16] / tail[0]
    assert int(log.reliability_counts.sum()) == 0 and float(log.nll_sums.abs().sum()) == 0 and int(log.nll_tail.sum()) == 0     # zeroed for the next pass
    assert plain.reliability_counts is None and plain.nll_sums is None


def test_photo_evaluator_with_calibration_bins(dev):
    from pylc_amd import calibration as cal, photo
    c, bins, h, w = 9, 10, 48, 80
    pal = (np.arange(c, dtype=np.uint8)[:, None] * 20 + np.array([1, 2, 3], np.uint8)[None]).astype(np.uint8)
    ev, plain = photo.PhotoEvaluator(c, pal, calibration_bins=bins), photo.PhotoEvaluator(c, pal)
    total = np.zeros(K.n_cells(c, bins), np.int64)
    for k in range(2):
        truth = R.blobs(h, w, c, seed=k, radius=6)
        pred = np.where(np.random.default_rng(k).random((h, w)) < 0.8, truth, R.blobs(h, w, c, seed=k + 5, radius=6)).astype(np.uint8)
        conf = _planted_conf(h * w, bins, k).reshape(h, w)
        res = photo.PhotoResult(torch.from_numpy(pred).to(dev), None, {'h_scaled': h, 'w_scaled': w}, None, 64, None,
                                torch.from_numpy(conf).to(dev))
        got, base = ev.add(res, pal[truth]), plain.add(res, pal[truth])
        mine = K.counts_ref(conf, pred, truth, c, bins)
        total += mine
        want = cal.reliability_scores(mine, c, bins)
        assert got['ece'] == want['ece'] and got['mce'] == want['mce'] and got['class_ece'] == want['class_ece']
        assert set(got) == set(base) | {'ece', 'mce', 'class_ece'} and got['iou'] == base['iou']
    assert np.array_equal(ev.reliability_counts.cpu().numpy(), total)
    agg, want = ev.aggregate(), cal.reliability_scores(total, c, bins)
    assert agg['ece'] == want['ece'] and agg['mce'] == want['mce'] and agg['class_ece'] == want['class_ece']
    assert agg['ece'] == pytest.approx(K.scores_ref(total, c, bins)['ece'], abs=1e-12)
    assert 'ece' not in plain.aggregate()


def test_trainer_stores_the_fitted_temperature(dev, tmp_path):
    """trainer(score=True, calibration_bins=15): every validation row carries the calibration keys, and the last pass's fitted temperature
    is in model.meta (and so in the checkpoint written after it)"""
    import oracle
    from pylc_amd import checkpoint, runtime, train
    from pylc_amd.model import Meta, Model
    from tests import _data as D
    runtime.dropout_enabled = False
    model = Model(Meta(), dev).build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec('deeplab', 'resnet', 9, 3), salt=5))
    assert model.meta.temperature is None
    tr = [(D.tiles(80, 2, 3, 64, 64), D.blob_masks(90, 2, 64, 64, 9, cell=8))]
    va = [(D.tiles(85 + i, 2, 3, 64, 64), D.blob_masks(95 + i, 2, 64, 64, 9, cell=8)) for i in range(2)]
    train.trainer(model, tr, va, 1, save_dir=str(tmp_path), score=True, calibration_bins=15)
    rows = model.scores.rows
    assert len(rows) == 2 and all({'ece', 'mce', 'nll', 'class_ece', 'temperature'} <= set(r) for r in rows)
    assert 0.0 <= rows[-1]['ece'] <= rows[-1]['mce'] <= 1.0 and rows[-1]['nll'] > 0 and len(rows[-1]['class_ece']) == 9
    assert model.meta.temperature == rows[-1]['temperature'] and 0.25 <= model.meta.temperature <= 4.0
    saved = checkpoint.load_reference_file(str(tmp_path / model.model_id() / 'checkpoint.pth'))
    assert checkpoint.meta_from_reference(saved['meta']).temperature == model.meta.temperature
