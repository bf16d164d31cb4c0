"""Whole photographs, host side (no GPU): pylc_amd.photo.fit_geometry against a literal restatement of the reference's get_image and
adjust_to_tile size arithmetic, the reference's recorded 3453 x 4940 run, numpy restatements of OpenCV's INTER_AREA tables and resize
(the float64 exact value and the fp32 accumulation order of csrc/photo.hip; tests/test_photo_gpu.py compares the kernel with them), the
class_encode rule, and the --aggregate_metrics coverage rule against sklearn on the reference's concatenated, overwritten arrays."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- restatements of the reference ---------------------------------------------------------------------------------------------------
def reference_geometry(h, w, tile, stride, scale=None):
    """get_image (utils/tools.py:77-148) then adjust_to_tile (utils/tools.py:151-206), sizes only, line by line; None when a resize would
    upscale or a side would be 0 (pylc_amd.photo raises there)."""
    height, width = h, w
    height_resized, width_resized = height, width
    if scale:
        min_dim = min(height, width)
        if min_dim < tile:
            scale = tile / min_dim
        dim = (int(scale * width), int(scale * height))
        width_resized, height_resized = dim
    if height_resized > height or width_resized > width or height_resized == 0 or width_resized == 0:
        return None
    wa, ha = width_resized, height_resized
    aspect = wa / ha
    assert tile % stride == 0 and stride <= tile
    w_scaled = (wa // tile) * tile
    h_scaled = (math.ceil(w_scaled / aspect) // tile) * tile
    if w_scaled == 0 or h_scaled == 0 or h_scaled > ha:
        return None
    h_resized = h_scaled                                  # cv2.resize(img, (w_scaled, h_scaled)).shape[0]
    h_tgt = int(h_resized / tile) * tile
    h_crop = h_resized - h_tgt
    return {'w_full': width, 'h_full': height, 'w_scaled': width_resized, 'h_scaled': height_resized,
            'w_fitted': w_scaled, 'h_fitted': h_resized - h_crop, 'offset': h_crop}


def area_tab(ssize, dsize, exact=False):
    """computeResizeAreaTab: per output coordinate, the list of (source index, weight); float32 weights, or the double quotients when
    exact.  scale = 1 / (dsize / ssize), as cv::resize hands the area path dsize / ssize and inverts it."""
    scale = 1.0 / (dsize / ssize)
    cast = float if exact else np.float32
    tabs = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s2 = min(math.floor(f2), ssize - 1)
        s1 = min(math.ceil(f1), s2)
        t = []
        if s1 - f1 > 1e-3:
            t.append((s1 - 1, cast((s1 - f1) / cell)))
        for s in range(s1, s2):
            t.append((s, cast(1.0 / cell)))
        if f2 - s2 > 1e-3:
            t.append((s2, cast(min(min(f2 - s2, 1.0), cell) / cell)))
        tabs.append(t)
    return tabs


def _dense(tabs, dtype):
    """taps padded to the longest list with (index 0, weight 0): adding 0 * x leaves an fp32 sum of non-negative terms unchanged"""
    n = max(len(t) for t in tabs)
    idx = np.zeros((len(tabs), n), np.int64)
    wt = np.zeros((len(tabs), n), dtype)
    for d, t in enumerate(tabs):
        for k, (s, a) in enumerate(t):
            idx[d, k], wt[d, k] = s, a
    return idx, wt


def resize_area_np(img, oh, ow, exact=False):
    """INTER_AREA of a uint8 [H,W,C] image to [C,oh,ow].  exact=False: OpenCV's fp32 order (per source row ascending, the row's weighted
    sum over ascending columns, then acc += beta * rowsum) rounded half to even -> uint8.  exact=True: the float64 value, unrounded."""
    h, w, c = img.shape
    dt = np.float64 if exact else np.float32
    yi, yw = _dense(area_tab(h, oh, exact), dt)
    xi, xw = _dense(area_tab(w, ow, exact), dt)
    acc = np.zeros((oh, ow, c), dt)
    for a in range(yi.shape[1]):
        rows = img[yi[:, a]]                              # [oh, W, C] uint8
        r = np.zeros((oh, ow, c), dt)
        for b in range(xi.shape[1]):
            r = r + rows[:, xi[:, b]].astype(dt) * xw[None, :, b, None]
        acc = acc + yw[:, a, None, None] * r
    acc = acc.transpose(2, 0, 1)
    return acc if exact else np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def nearest_index(n, on):
    """cv2.INTER_NEAREST (resizeNN): min(floor(o * (1 / (on / n))), n - 1)"""
    return np.minimum(np.floor(np.arange(on) * (1.0 / (on / n))).astype(np.int64), n - 1)


def class_encode_np(rgb, palette):
    """class_encode (utils/tools.py:412-449): np.ones, then every palette index in turn overwrites its matches (the last match wins)."""
    flat = rgb.reshape(-1, 3)
    enc = np.ones(flat.shape[0])
    for idx, c in enumerate(palette):
        enc[np.all(flat == np.array(c), axis=1)] = idx
    return enc.reshape(rgb.shape[:2]).astype(np.uint8)


def encode_resize_np(rgb, palette, oh, ow):
    h, w = rgb.shape[:2]
    return class_encode_np(rgb[nearest_index(h, oh)][:, nearest_index(w, ow)], palette)


def reference_scores(y_true_list, y_pred_list, n_classes):
    """Evaluator.load (flattened uint8 masks appended), validate() with aggregate (concatenate, then y[idx] = idx for the first
    n_classes positions) and evaluate() (sklearn weighted F1, weighted Jaccard, MCC): utils/evaluate.py:64-176, utils/metrics.py:64-88."""
    from sklearn.metrics import f1_score, jaccard_score, matthews_corrcoef
    yt = np.concatenate([np.asarray(t).ravel() for t in y_true_list]).astype(np.int64)
    yp = np.concatenate([np.asarray(p).ravel() for p in y_pred_list]).astype(np.int64)
    for idx in range(n_classes):
        yt[idx] = idx
        yp[idx] = idx
    return {'f1': f1_score(yt, yp, average='weighted', zero_division=0), 'iou': jaccard_score(yt, yp, average='weighted'),
            'mcc': matthews_corrcoef(yt, yp)}


def counts_np(yt, yp, n, coverage):
    yt, yp = np.asarray(yt).ravel().astype(np.int64).copy(), np.asarray(yp).ravel().astype(np.int64).copy()
    if coverage:
        yt[:n] = np.arange(n)
        yp[:n] = np.arange(n)
    return np.bincount(yt * n + yp, minlength=n * n).reshape(n, n)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
SIZES = [(4940, 3453), (3453, 4940), (3000, 4000), (4000, 3000), (1023, 1537), (1537, 1023), (2048, 2048), (2049, 3071), (600, 4100),
         (4100, 600), (1200, 1100), (513, 700), (700, 513), (6000, 8000), (8001, 5999), (12000, 9000)]


@pytest.mark.parametrize('scale', [None, 0.2, 0.5, 1.0])
@pytest.mark.parametrize('tile,stride', [(512, 256), (1024, 512), (64, 32), (512, 512)])
def test_fit_geometry_matches_reference_arithmetic(scale, tile, stride):
    from pylc_amd import photo
    seen = 0
    for h, w in SIZES + [(300, 460), (150, 230), (333, 517)]:
        want = reference_geometry(h, w, tile, stride, scale)
        if want is None:
            with pytest.raises(ValueError):
                photo.fit_geometry(h, w, tile, stride, scale)
            continue
        got = photo.fit_geometry(h, w, tile, stride, scale)
        assert got == want, (h, w, tile, stride, scale)
        assert got['offset'] == 0
        assert got['h_fitted'] % tile == 0 and got['w_fitted'] % tile == 0
        assert got['h_fitted'] <= got['h_scaled'] <= h and got['w_fitted'] <= got['w_scaled'] <= w
        seen += 1
    assert seen >= 2


def test_recorded_reference_run():
    """hi-0027.tif, W x H 3453 x 4940 at scale 1.0: 'Fitted for Tiling 3072px x 4096px', 'Number of Tiles 165' (11 x 15); at tile 1024,
    stride 512 the same size in 5 x 7 = 35 tiles (the configs[4] inference leg)."""
    from pylc_amd import photo
    from pylc_amd.inference import tile_grid
    for scale in (None, 1.0):
        g = photo.fit_geometry(4940, 3453, 512, 256, scale)
        assert (g['h_fitted'], g['w_fitted'], g['h_scaled'], g['w_scaled'], g['offset']) == (4096, 3072, 4940, 3453, 0)
        assert tile_grid(g['h_fitted'], g['w_fitted'], 512, 256) == (15, 11)
    g = photo.fit_geometry(4940, 3453, 1024, 512)
    assert (g['h_fitted'], g['w_fitted']) == (4096, 3072)
    assert tile_grid(g['h_fitted'], g['w_fitted'], 1024, 512) == (7, 5)


def test_fit_geometry_errors():
    from pylc_amd import photo
    with pytest.raises(ValueError, match='upscale'):
        photo.fit_geometry(300, 400, 512, 256, scale=0.5)          # short side below the tile: the scale is raised to 512/300
    with pytest.raises(ValueError, match='upscale'):
        photo.fit_geometry(1000, 1200, 512, 256, scale=2.0)
    with pytest.raises(ValueError, match='multiple of stride'):
        photo.fit_geometry(1000, 1200, 512, 200)
    with pytest.raises(ValueError, match='multiple of stride'):
        photo.fit_geometry(1000, 1200, 512, 1024)
    with pytest.raises(ValueError, match='side of 0'):
        photo.fit_geometry(1000, 400, 512, 256)                    # narrower than one tile
    with pytest.raises(ValueError, match='side of 0'):
        photo.fit_geometry(300, 2000, 512, 256)                    # so flat that no tile row fits


# ---- INTER_AREA tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ssize,dsize', [(4940, 4096), (3453, 3072), (4940, 988), (3453, 690), (4940, 2470), (3453, 1726), (457, 333),
                                         (301, 211), (7, 3), (100, 100), (1000, 250), (9, 2)])
def test_area_tables(ssize, dsize):
    tabs = area_tab(ssize, dsize)
    exact = area_tab(ssize, dsize, exact=True)
    scale = 1.0 / (dsize / ssize)
    dropped_any = False
    for d, (t, e) in enumerate(zip(tabs, exact)):
        # the weights sum to 1 but for the slivers of <= 1e-3 source pixel that computeResizeAreaTab drops at either end of the cell
        f1, f2 = d * scale, d * scale + scale
        cell = min(scale, ssize - f1)
        lost = sum(x for x in (math.ceil(f1) - f1, f2 - math.floor(f2)) if 0 < x <= 1e-3 and math.floor(f2) <= ssize - 1)
        dropped_any |= lost > 0
        assert abs(sum(float(a) for _, a in t) - (1.0 - lost / cell)) < 1e-6
        assert abs(sum(a for _, a in e) - (1.0 - lost / cell)) < 1e-9
        idx = [s for s, _ in t]
        assert idx == list(range(idx[0], idx[0] + len(idx))) and 0 <= idx[0] and idx[-1] < ssize
    if (ssize, dsize) == (4940, 4096):
        assert dropped_any                                  # scale 1.2060546875: fractions of 1/1024 occur and are dropped
    covered = sorted(set(s for t in tabs for s, _ in t))
    assert covered == list(range(ssize))
    if ssize % dsize == 0:                                  # an integer factor: plain box means
        f = ssize // dsize
        assert all([s for s, _ in t] == list(range(d * f, d * f + f)) and all(a == np.float32(1.0 / f) for _, a in t)
                   for d, t in enumerate(tabs))


def test_area_resize_restatements():
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    assert np.array_equal(resize_area_np(img, 37, 53), img.transpose(2, 0, 1))              # equal sizes: the bytes
    half = resize_area_np(img[:36, :52], 18, 26)
    box = img[:36, :52].astype(np.float64).reshape(18, 2, 26, 2, 3).mean((1, 3)).transpose(2, 0, 1)
    assert np.array_equal(half, np.rint(box).astype(np.uint8))                                # factor 2: box mean, half to even
    got, ex = resize_area_np(img, 17, 29), resize_area_np(img, 17, 29, exact=True)
    assert np.abs(got.astype(np.float64) - ex).max() <= 0.5 + 1e-3


# ---- encoding and scores ---------------------------------------------------------------------------------------------------------------
def test_class_encode_rule():
    pal = [(0, 0, 0), (10, 20, 30), (40, 50, 60), (10, 20, 30)]           # colour 1 repeated at 3
    rgb = np.array([[[0, 0, 0], [10, 20, 30], [40, 50, 60], [1, 2, 3]]], np.uint8)
    assert class_encode_np(rgb, pal).tolist() == [[0, 3, 2, 1]]           # last match wins, no match -> 1
    assert nearest_index(10, 4).tolist() == [0, 2, 5, 7] and nearest_index(5, 5).tolist() == list(range(5))


def test_aggregate_coverage_rule_matches_reference():
    from pylc_amd import photo
    n = 9
    rs = np.random.RandomState(11)
    pal = rs.randint(0, 256, (n, 3))
    trues, preds = [], []
    ev = photo.PhotoEvaluator(n, pal)
    for k, (h, w) in enumerate([(40, 70), (33, 51), (64, 64)]):
        yt = rs.randint(0, n - 2, (h, w)).astype(np.uint8)                 # the last classes absent: coverage matters
        yp = np.where(rs.rand(h, w) < 0.7, yt, rs.randint(0, n, (h, w))).astype(np.uint8)
        trues.append(yt)
        preds.append(yp)
        per = ev.add_counts(counts_np(yt, yp, n, True), counts_np(yt, yp, n, False) if k else None)
        want = reference_scores([yt], [yp], n)
        for key in ('f1', 'iou', 'mcc'):
            assert abs(per[key] - want[key]) < 1e-12
    agg = ev.aggregate()
    want = reference_scores(trues, preds, n)
    for key in ('f1', 'iou', 'mcc'):
        assert abs(agg[key] - want[key]) < 1e-12, key
    # not the sum of per-image covered counts: validate() overwrites the concatenation's first n pixels once
    summed = sum(counts_np(t, p, n, True) for t, p in zip(trues, preds))
    assert not np.array_equal(summed, ev.cm)
    with pytest.raises(ValueError):
        photo.PhotoEvaluator(n, pal[:5])


def test_photo_entry_points_declared():
    from pylc_amd import lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read(), flags=re.S)
    for name in ('pylc_resize_area_u8', 'pylc_class_encode_resize', 'pylc_image_pack_tiles_ex'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in L.SIGNATURES
    assert L.ABI_VERSION == 15 and L.lib.pylc_abi_version() == 15
