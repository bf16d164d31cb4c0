"""The augmentation transform, host side (no GPU): a numpy restatement of the reference's augment_transform (perspective_shift +
channel_shift, utils/tools.py:452-594) with the dtypes the reference feeds it -- cv2.getPerspectiveTransform, cv2.warpPerspective (linear
with a 32-step interpolation table for the float32 image, nearest for the mask, BORDER_REFLECT_101), the 30-pixel crop, cv2.resize's
area-mode linear upscale and nearest, np.int16, the shift and the clip -- written out operation by operation (augment_params_np,
augment_np).  tests/test_augment_gpu.py compares pylc_augment_tiles with it bit for bit.  Here: pylc_amd.dataset.augment_params against
the restatement's draws, the oversampling layout and TileSet.oversample's bookkeeping on a stub of the device call, and the fact that
the separately rounded fp32 upscale leaves a flat region a hair below its value, which the truncation then makes visible."""
from fractions import Fraction

import numpy as np
import pytest
import torch

PTS1 = np.array([[56, 65], [368, 52], [28, 387], [389, 390]], np.float32)
SHIFTS = (19, 13, 12, 10)                                  # int(RandomState(j).uniform(10, 20)) after the eight point draws, j = 0..3
TIE = 1e-6                                                 # coordinates nearer than this to a rounding tie are not compared


# ---- restatement -------------------------------------------------------------------------------------------------------------------
def augment_draws_np(j, t):
    """(pts2 float32 [4,2], shift): the draws of augment_transform(.., RandomState(j)) on a tile of side t, in its order"""
    rs = np.random.RandomState(j)
    alpha = 0.06 * t
    pts2 = PTS1 + rs.uniform(-alpha, alpha, size=(4, 2)).astype(np.float32)
    assert pts2.dtype == np.float32
    return pts2, int(rs.uniform(10, 20))


def perspective_np(pts1, pts2):
    """cv2.getPerspectiveTransform's 8 x 8 system, solved EXACTLY (rational arithmetic on the float inputs): rows of Fractions [3][3]"""
    rows = []
    for k in (0, 1):
        for i in range(4):
            x, y, out = Fraction(float(pts1[i, 0])), Fraction(float(pts1[i, 1])), Fraction(float(pts2[i, k]))
            rows.append(([x, y, 1, 0, 0, 0] if k == 0 else [0, 0, 0, x, y, 1]) + [-x * out, -y * out, out])
    rows = [[Fraction(v) for v in r] for r in rows]
    for c in range(8):                                     # Gauss-Jordan
        p = next(r for r in range(c, 8) if rows[r][c] != 0)
        rows[c], rows[p] = rows[p], rows[c]
        for r in range(8):
            if r != c and rows[r][c] != 0:
                f = rows[r][c] / rows[c][c]
                rows[r] = [a - f * b for a, b in zip(rows[r], rows[c])]
    sol = [rows[i][8] / rows[i][i] for i in range(8)] + [Fraction(1)]
    return [sol[0:3], sol[3:6], sol[6:9]]


def inv3_np(m):
    """the inverse of a 3 x 3 matrix by its adjugate (as cv2.invert does for this size), exact, rounded to double at the end"""
    c = [[m[1][1] * m[2][2] - m[1][2] * m[2][1], m[0][2] * m[2][1] - m[0][1] * m[2][2], m[0][1] * m[1][2] - m[0][2] * m[1][1]],
         [m[1][2] * m[2][0] - m[1][0] * m[2][2], m[0][0] * m[2][2] - m[0][2] * m[2][0], m[0][2] * m[1][0] - m[0][0] * m[1][2]],
         [m[1][0] * m[2][1] - m[1][1] * m[2][0], m[0][1] * m[2][0] - m[0][0] * m[2][1], m[0][0] * m[1][1] - m[0][1] * m[1][0]]]
    det = m[0][0] * c[0][0] + m[0][1] * c[1][0] + m[0][2] * c[2][0]
    return np.array([[float(v / det) for v in row] for row in c])


def augment_params_np(j, t):
    pts2, shift = augment_draws_np(j, t)
    return inv3_np(perspective_np(PTS1, pts2)), shift


def warp_coords_np(minv, t, q):
    """fX, fY (float64 [t,t]) of warpPerspective's inverse map, interpolation-table size q; numpy rounds every operation on its own"""
    y, x = np.mgrid[0:t, 0:t]
    x, y = x.astype(np.float64), y.astype(np.float64)
    X0 = (minv[0, 0] * x + minv[0, 1] * y) + minv[0, 2]
    Y0 = (minv[1, 0] * x + minv[1, 1] * y) + minv[1, 2]
    W = (minv[2, 0] * x + minv[2, 1] * y) + minv[2, 2]
    with np.errstate(divide='ignore'):
        W = np.where(W != 0, q / W, 0.0)
    return X0 * W, Y0 * W


def near_tie(f):
    return np.abs((f - np.floor(f)) - 0.5) <= TIE


def refl_np(p, t):
    """BORDER_REFLECT_101, by its definition"""
    p = p.copy()
    while True:
        neg, big = p < 0, p >= t
        if not (neg.any() or big.any()):
            return p
        p[neg] = -p[neg]
        big = p >= t
        p[big] = 2 * t - 2 - p[big]


def resize_table_np(t):
    """cv2.resize from t - 60 to t in area mode (an upscale: its linear kernel): per output index the source index s and the float32
    weight f of s + 1; s alone is also INTER_NEAREST's index, min(floor(d * scale), t - 61)"""
    w = t - 60
    inv = t / w
    scale = 1.0 / inv
    s, f = np.zeros(t, np.int64), np.zeros(t, np.float32)
    for d in range(t):
        sd = int(np.floor(d * scale))
        fd = np.float32((d + 1) - (sd + 1) * inv)
        fd = np.float32(0) if fd <= 0 else np.float32(fd - np.floor(fd))
        if sd + 1 >= w:
            fd, sd = np.float32(0), w - 1
        assert sd == min(int(np.floor(d * scale)), w - 1)
        s[d], f[d] = sd, fd
    return s, f


def augment_np(img, mask, minv, shift):
    """img uint8 [C,t,t], mask uint8 [t,t] -> dict: img uint8 [C,t,t], mask uint8 [t,t], near_img / near_mask bool [t,t] (output pixels
    that read a warped pixel whose coordinate lies within TIE of a rounding tie), reflected (the share of the crop's warped image pixels
    that read a reflected source pixel)"""
    c, t = img.shape[0], img.shape[1]
    lo, hi = 30, t - 30
    # the mask: nearest
    fx, fy = warp_coords_np(minv, t, 1.0)
    mx, my = refl_np(np.rint(fx).astype(np.int64), t), refl_np(np.rint(fy).astype(np.int64), t)
    wmask = mask[my, mx][lo:hi, lo:hi]
    tie_m = (near_tie(fx) | near_tie(fy))[lo:hi, lo:hi]
    # the image: bilinear on a 1/32 grid
    fx, fy = warp_coords_np(minv, t, 32.0)
    X, Y = np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64)
    sx, sy, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31
    x0, x1, y0, y1 = refl_np(sx, t), refl_np(sx + 1, t), refl_np(sy, t), refl_np(sy + 1, t)
    reflected = ((sx < 0) | (sx + 1 >= t) | (sy < 0) | (sy + 1 >= t))[lo:hi, lo:hi]
    src = img.astype(np.int64)
    n = (32 - ax) * (32 - ay) * src[:, y0, x0] + ax * (32 - ay) * src[:, y0, x1] + (32 - ax) * ay * src[:, y1, x0] + ax * ay * src[:, y1, x1]
    warped = (n.astype(np.float32) / np.float32(1024))[:, lo:hi, lo:hi]
    assert np.array_equal(warped.astype(np.float64) * 1024, n[:, lo:hi, lo:hi])           # exact in fp32
    tie_i = (near_tie(fx) | near_tie(fy))[lo:hi, lo:hi]
    # the upscale: rows first, then columns; fp32, multiplies and adds rounded one by one
    s, f = resize_table_np(t)
    s1 = np.minimum(s + 1, t - 61)
    g = np.float32(1) - f
    rows = warped[:, :, s] * g + warped[:, :, s1] * f
    up = rows[:, s, :] * g[:, None] + rows[:, s1, :] * f[:, None]
    assert up.dtype == np.float32
    out = np.clip(up.astype(np.int16) + np.int16(shift), 0, 255).astype(np.uint8)
    near_img = tie_i[s][:, s] | tie_i[s1][:, s] | tie_i[s][:, s1] | tie_i[s1][:, s1]
    return {'img': out, 'mask': wmask[s][:, s], 'near_img': near_img, 'near_mask': tie_m[s][:, s], 'reflected': float(reflected.mean()),
            'upscaled': up}


def tiles_np(seed, n, c, t, n_classes=9):
    """n image tiles [n,c,t,t] with flat 255, flat 0 and flat 200 bands plus noise (they reach the clip at 255, the shift on black and the
    truncation below a flat value), and masks of random class indices with a few 255s"""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (n, c, t, t)).astype(np.uint8)
    q = t // 5
    img[:, :, q:2 * q] = 255
    img[:, :, 2 * q:3 * q] = 0
    img[:, :, 3 * q:4 * q] = 200
    mask = rs.randint(0, n_classes, (n, t, t)).astype(np.uint8)
    mask[rs.rand(n, t, t) < 0.01] = 255
    return img, mask


# ---- the host part -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [128, 200, 512, 1024])
def test_augment_params_match_the_restatement(t):
    from pylc_amd import dataset
    for j in range(4):
        pts2, shift = augment_draws_np(j, t)
        minv, got_shift = dataset.augment_params(j, t)
        assert got_shift == shift == SHIFTS[j]
        assert minv.dtype == np.float64 and minv.shape == (3, 3)
        want = augment_params_np(j, t)[0]
        assert np.all(np.abs(minv - want) <= 1e-12 * np.abs(want)), (j, t)
        # pts2 bit for bit: the matrix maps pts1 onto exactly the restatement's float32 points
        m = np.linalg.inv(minv)
        for p, q in zip(PTS1.astype(np.float64), pts2.astype(np.float64)):
            v = m @ np.array([p[0], p[1], 1.0])
            got = (v[:2] / v[2]).astype(np.float32)
            near = np.abs(v[:2] / v[2] - q) <= 1e-9
            assert near.all() and np.array_equal(got, q.astype(np.float32))
        assert abs(np.linalg.inv(minv)[2, 2] - 1.0) < 1e-12
    assert not np.array_equal(dataset.augment_params(0, 128)[0], dataset.augment_params(0, 512)[0])       # alpha = 0.06 t
    with pytest.raises(ValueError, match='below 128'):
        dataset.augment_params(0, 64)


def test_restatement_pieces():
    assert refl_np(np.array([-3, -1, 0, 7, 8, 9, 14, 15, 16, -15]), 8).tolist() == [3, 1, 0, 7, 6, 5, 0, 1, 2, 1]
    s, f = resize_table_np(128)
    assert s[0] == 0 and f[0] == 0 and s[-1] == 67 and f[-1] == 0 and np.all(np.diff(s) >= 0) and np.all((f >= 0) & (f < 1))
    # the identity warp: the transform is crop + upscale + shift, and the mask a nearest upscale of its crop
    img, mask = tiles_np(3, 1, 3, 128)
    out = augment_np(img[0], mask[0], np.eye(3), 0)
    assert np.array_equal(out['mask'], mask[0][30:98, 30:98][s][:, s]) and out['reflected'] == 0
    assert np.array_equal(out['img'][:, 0, 0], img[0][:, 30, 30]) and not out['near_mask'].any()
    # a translation by 2.5 pixels: every mask coordinate is a tie
    shifted = augment_np(img[0], mask[0], np.array([[1, 0, 2.5], [0, 1, 0], [0, 0, 1.0]]), 0)
    assert shifted['near_mask'].all() and not shifted['near_img'].any()


def test_flat_region_ends_below_its_value():
    """The two separately rounded fp32 passes (no FMA) leave a constant-200 region at 199.99997 on 7.1 % of its pixels; np.int16
    truncates, so those pixels come out as 199 + shift.  That is the reference's behaviour with an OpenCV whose resize does not contract;
    the kernel keeps it, and nobody is to 'fix' it by rounding."""
    t = 512
    minv, shift = augment_params_np(0, t)
    img = np.full((1, t, t), 200, np.uint8)
    out = augment_np(img, np.zeros((t, t), np.uint8), minv, shift)
    up = out['upscaled']
    below = up < 200
    assert 199.9999 < up.min() < 200 and up.max() < 200.0001
    assert below.mean() > 0 and round(float(below.mean()), 3) == 0.071
    assert np.array_equal(out['img'][0][below[0]], np.full(int(below.sum()), 199 + shift, np.uint8))
    assert np.array_equal(out['img'][0][~below[0]], np.full(int((~below).sum()), 200 + shift, np.uint8))


def test_ties_are_rare_on_the_reference_warps():
    """the share of output pixels the GPU comparison leaves out (a coordinate within 1e-6 of a rounding tie) stays far below its 1e-4 bound"""
    img, mask = tiles_np(5, 1, 3, 200)
    for j in range(4):
        minv, shift = augment_params_np(j, 200)
        out = augment_np(img[0], mask[0], minv, shift)
        assert out['near_img'].mean() <= 1e-4 and out['near_mask'].mean() <= 1e-4 and out['reflected'] == 0
        assert out['img'].max() == 255 and out['img'].min() == shift and (out['mask'] == 255).any()


# ---- the layout and the container ----------------------------------------------------------------------------------------------------
def test_oversample_layout():
    from pylc_amd import dataset
    src, copy = dataset.oversample_layout([0, 1, 4, 0, 2, 0])
    assert src.tolist() == [0, 1, 1, 2, 2, 2, 2, 2, 3, 4, 4, 4, 5]
    assert copy.tolist() == [-1, -1, 0, -1, 0, 1, 2, 3, -1, -1, 0, 1, -1]
    src, copy = dataset.oversample_layout(np.zeros(3, int))
    assert src.tolist() == [0, 1, 2] and copy.tolist() == [-1, -1, -1]
    assert dataset.oversample_layout([])[0].size == 0
    for bad in ([1, -1], [0.5, 1.0], [[1, 2]]):
        with pytest.raises(ValueError):
            dataset.oversample_layout(bad)


def _stub_augment(calls):
    """augment_tiles on the host: a copy is its source tile with pixel [0,0,0] set to 100 + copy index (and the mask's [0,0] to the copy
    index), statistics by numpy"""
    from tests.test_cpu_dataset import tile_sums_np

    def stub(img, mask, src_index, copy_index, band_rows=0, n_classes=None):
        calls.append((np.asarray(src_index).tolist(), np.asarray(copy_index).tolist()))
        a, m = img.numpy()[np.asarray(src_index, int)].copy(), mask.numpy()[np.asarray(src_index, int)].copy()
        a[:, 0, 0, 0] = 100 + np.asarray(copy_index)
        m[:, 0, 0] = np.asarray(copy_index)
        sums, hist = tile_sums_np(a, m, n_classes) if len(a) else (np.zeros((0, 2, a.shape[1]), np.int64), np.zeros((0, n_classes + 1), np.int64))
        return torch.from_numpy(a), torch.from_numpy(m), torch.from_numpy(sums), torch.from_numpy(hist)
    return stub


@pytest.mark.parametrize('chunk', [64, 2, 1])
def test_oversample_bookkeeping(monkeypatch, chunk):
    from pylc_amd import dataset
    from tests.test_cpu_dataset import tile_sums_np
    rs = np.random.RandomState(9)
    n, k, t = 6, 5, 8
    img = rs.randint(0, 256, (n, 3, t, t)).astype(np.uint8)
    mask = rs.randint(0, k, (n, t, t)).astype(np.uint8)
    sums, hist = tile_sums_np(img, mask, k)
    ts = dataset.TileSet(3, k, t, keep='host').from_arrays(img, mask, sums, hist)
    calls = []
    monkeypatch.setattr(dataset, 'augment_tiles', _stub_augment(calls))
    rates = [0, 1, 4, 0, 2, 0]
    out = ts.oversample(rates, chunk=chunk, device='cpu')
    assert out is not ts and len(ts) == n and len(out) == n + sum(rates) and out.keep == 'host' and out.tile == t and out.n_classes == k
    src, copy = dataset.oversample_layout(rates)
    want_img, want_mask = img[src].copy(), mask[src].copy()
    want_img[copy >= 0, 0, 0, 0] = 100 + copy[copy >= 0]
    want_mask[copy >= 0, 0, 0] = copy[copy >= 0]
    assert np.array_equal(out.img.numpy(), want_img) and np.array_equal(out.mask.numpy(), want_mask)
    want_sums, want_hist = tile_sums_np(want_img, want_mask, k)
    assert np.array_equal(out.sums, want_sums) and np.array_equal(out.hist, want_hist[:, :k])
    assert out.profile()['n_samples'] == 13
    assert len(calls) == -(-n // chunk) and sum(len(c[0]) for c in calls) == sum(rates)
    # a partition oversamples its own tiles
    part = ts.partition(0.5, 1.0).oversample(rates[3:], chunk=chunk, device='cpu')
    assert len(part) == 3 + 2 and np.array_equal(part.img.numpy()[[0, 1, 4]], img[3:])


def test_oversample_errors(monkeypatch):
    from pylc_amd import dataset
    from tests.test_cpu_dataset import tile_sums_np
    rs = np.random.RandomState(2)
    img = rs.randint(0, 256, (3, 1, 8, 8)).astype(np.uint8)
    mask = rs.randint(0, 4, (3, 8, 8)).astype(np.uint8)
    sums, hist = tile_sums_np(img, mask, 4)
    ts = dataset.TileSet(1, 4, 8, keep='host').from_arrays(img, mask, sums, hist)
    monkeypatch.setattr(dataset, 'augment_tiles', _stub_augment([]))
    with pytest.raises(ValueError, match='2 rates for 3 tiles'):
        ts.oversample([1, 1], device='cpu')
    with pytest.raises(ValueError):
        ts.oversample([1, -1, 0], device='cpu')
    with pytest.raises(ValueError, match='needs masks'):
        dataset.TileSet(1, 4, 8, keep='host').from_arrays(img, None, sums, None).oversample([0, 0, 0], device='cpu')
    # a copy that holds a class index >= n_classes: the stub writes the copy index into the mask
    with pytest.raises(ValueError, match='class index'):
        ts.oversample([0, 0, 4 + 1], device='cpu')
    assert len(ts.oversample([0, 0, 4], device='cpu')) == 7


def test_augment_entry_point_declared():
    import os
    import re
    from pylc_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'pylc_hip.h')).read(), flags=re.S)
    assert re.search(r'\bpylc_augment_tiles\s*\(', hdr) and 'pylc_augment_tiles' in L.SIGNATURES and hasattr(L.lib, 'pylc_augment_tiles')
    # the argument checks happen on the host before any launch: no GPU needed, never a fault
    P = 16

    def call(n_src=2, c=3, t=128, m=1, band=0, out_img=P, mask=P, out_mask=P, k=9, hist=P):
        return L.lib.pylc_augment_tiles(P, mask, n_src, c, t, P, P, P, m, band, out_img, out_mask, k, P, hist, None)
    assert call(t=64) == 1 and b'tile=64' in L.lib.pylc_last_error()
    assert call(t=1025) == 1
    assert call(c=2) == 1 and b'Cimg=2' in L.lib.pylc_last_error()
    assert call(out_img=None) == 1 and b'NULL' in L.lib.pylc_last_error()
    assert call(mask=None) == 1 and b'without mask tiles' in L.lib.pylc_last_error()
    assert call(k=17) == 1 and call(k=0) == 1
    assert call(t=512, band=129) == 1 and b'band_rows' in L.lib.pylc_last_error()
    assert call(n_src=0) == 1 and call(m=-1) == 1
    assert call(m=0) == 0                                                  # nothing to do, nothing launched
