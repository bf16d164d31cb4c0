"""Training tile sets from photographs: the reference's `pylc.py extract` (Extractor.extract -> __split -> class_encode -> coshuffle ->
profile, utils/extract.py:106-231, 279-310; utils/profile.py:21-150; utils/metrics.py:90-132) and the oversampling-rate search of
`pylc.py augment` (Augmentor.optimize, utils/augment.py:92-182), with every pixel-sized step on the GPU.

For each image / mask pair the reference
  1. reads the image and, with --scale, resizes it by cv2.INTER_AREA (get_image), optionally fits it to the tile grid (adjust_to_tile);
  2. reads the mask at the same scale by cv2.INTER_NEAREST;
  3. unfolds both into tile x tile tiles at `stride` (the remainder right and below is dropped) and class-encodes the mask tiles;
  4. later walks over all tiles once more for the profile: per-tile channel mean and std, per-tile class histogram, and from the
     histograms the class probabilities, the class weights of the weighted loss, M2 and the JSD against the uniform distribution.

Here steps 1-2 are photo.resize_area / photo.fit_image / photo.encode_mask (nearest-resize then encode: the same pixels as encode after
resize, since a nearest resize only selects pixels), step 3 is pylc_extract_tiles, which in the same pass leaves per tile the integer sums
the profile is made of (sum x, sum x^2 per channel, the class histogram); step 4 is double arithmetic on those exact integers on the host.
A TileSet keeps the tiles on the device (or in pinned host memory) and hands Model.train its batches.

The augmented copies those rates ask for (Augmentor.oversample -> augment_transform, utils/augment.py:184-239, utils/tools.py:452-594)
are made by pylc_augment_tiles: augment_params draws a copy's warp and brightness shift as the reference does, augment_tiles applies them
on the device, TileSet.oversample composes the class-balanced set.

Not in the reference: the per-step augmenter -- random scale, rotation, mirror image, crop and a tone curve drawn
anew for every batch: batch_augment_params draws, augment_batch applies them by one launch of pylc_batch_augment (exact integer
arithmetic), TileSet.batches(augment=...) feeds Model.train with them.

Out of scope: HDF5 files, file collation, print_meta."""
import math

import numpy as np
import torch

from . import lib as L
from . import photo
from .lib import lib, check, ptr, stream

MAX_CLASSES = photo.MAX_CLASSES


# ---- geometry (host) ---------------------------------------------------------------------------------------------------------------
def tile_grid_counts(h, w, tile, stride):
    """(rows, cols) of torch.unfold(0, tile, stride).unfold(1, tile, stride) on an h x w image: (h - tile) // stride + 1 and likewise;
    the remainder right and below is dropped.  ValueError when a side is below the tile."""
    if tile <= 0 or stride <= 0:
        raise ValueError('tile %d and stride %d must be positive' % (tile, stride))
    if h < tile or w < tile:
        raise ValueError('image %dx%d (HxW) is smaller than the tile %d' % (h, w, tile))
    return (h - tile) // stride + 1, (w - tile) // stride + 1


def _check_n_classes(n_classes):
    if not 1 <= int(n_classes) <= MAX_CLASSES:
        raise ValueError('n_classes=%s outside 1..%d' % (n_classes, MAX_CLASSES))
    return int(n_classes)


# ---- device steps --------------------------------------------------------------------------------------------------------------
def _u8(t, what):
    if t.dtype != torch.uint8:
        raise TypeError('%s must be uint8, got %s' % (what, t.dtype))
    return t.contiguous()


def cut_tiles(img, mask=None, tile=512, stride=None, n_classes=None, first_tile=0, n_tiles=None, band_rows=0):
    """pylc_extract_tiles on a device uint8 image [C,H,W] and, optionally, its class-index mask [H,W]: tiles first_tile ..
    first_tile + n_tiles - 1 of the grid (default: all).  Returns (img_tiles [n,C,t,t] uint8, mask_tiles [n,t,t] uint8 or None,
    sums int64 [n,2,C] -- sum x and sum x^2 per channel --, hist int64 [n, n_classes + 1] or None; the last bin counts every mask value
    >= n_classes).  band_rows (tile rows per block, 0: the default) changes the launch only, never the result."""
    L.init()
    img = _u8(img, 'the image')
    c, h, w = img.shape
    stride = tile if stride is None else stride
    n_all = 0
    if 0 < tile <= min(h, w) and stride > 0:
        rows, cols = tile_grid_counts(h, w, tile, stride)
        n_all = rows * cols
    n = max(n_all - first_tile, 0) if n_tiles is None else n_tiles
    dev = img.device
    out = torch.empty((max(n, 0), c, tile, tile), device=dev, dtype=torch.uint8)
    sums = torch.zeros((max(n, 0), 2, c), device=dev, dtype=torch.int64)
    mout = hist = None
    if mask is not None:
        mask = _u8(mask, 'the mask')
        if tuple(mask.shape) != (h, w):
            raise ValueError('mask %s does not match the image %dx%d' % (tuple(mask.shape), h, w))
        mout = torch.empty((max(n, 0), tile, tile), device=dev, dtype=torch.uint8)
        hist = torch.zeros((max(n, 0), (n_classes or 0) + 1), device=dev, dtype=torch.int64)
    check(lib.pylc_extract_tiles(ptr(img), c, h, w, ptr(mask), n_classes or 0, tile, stride, first_tile, n, band_rows, ptr(out), ptr(mout),
                                 ptr(sums), ptr(hist), stream()))
    return out, mout, sums, hist


def tile_stats(img, mask=None, n_classes=None, band_rows=0):
    """pylc_tile_stats: cut_tiles' sums and histograms for device tiles that already exist ([n,C,t,t] uint8, masks [n,t,t] uint8)."""
    L.init()
    img = _u8(img, 'tiles')
    if img.dim() != 4 or img.shape[2] != img.shape[3]:
        raise ValueError('tiles must be [n,C,t,t], got %s' % (tuple(img.shape),))
    n, c, t = img.shape[0], img.shape[1], img.shape[2]
    sums = torch.zeros((n, 2, c), device=img.device, dtype=torch.int64)
    hist = None
    if mask is not None:
        mask = _u8(mask, 'mask tiles')
        if tuple(mask.shape) != (n, t, t):
            raise ValueError('mask tiles %s do not match the tiles %s' % (tuple(mask.shape), tuple(img.shape)))
        hist = torch.zeros((n, (n_classes or 0) + 1), device=img.device, dtype=torch.int64)
    check(lib.pylc_tile_stats(ptr(img), n, c, t, ptr(mask), n_classes or 0, band_rows, ptr(sums), ptr(hist), stream()))
    return sums, hist


# ---- the augmentation transform ----------------------------------------------------------------------------------------------------
AUG_MIN_TILE = 128
_AUG_PTS = ((56, 65), (368, 52), (28, 387), (389, 390))         # perspective_shift's source points: fixed, whatever the tile


def augment_params(j, tile):
    """What augment_transform(img, mask, np.random.RandomState(j)) draws for a tile of side `tile`, in its order: the four points of
    perspective_shift (utils/tools.py:580-584) and channel_shift's brightness shift (:549).  Returns (minv, shift): minv float64 [3,3],
    the inverse of cv2.getPerspectiveTransform(pts1, pts2) -- what cv2.warpPerspective maps output pixels back with --, and the int shift.
    The seed is the copy's index j alone: copy j of every tile gets the same warp, as in the reference."""
    if tile < AUG_MIN_TILE:
        raise ValueError('tile %d is below %d: the transform crops 30 pixels on every side' % (tile, AUG_MIN_TILE))
    rs = np.random.RandomState(int(j))
    alpha = 0.06 * tile
    pts1 = np.float32(_AUG_PTS)
    pts2 = pts1 + rs.uniform(-alpha, alpha, size=pts1.shape).astype(np.float32)
    shift = int(rs.uniform(10, 20))
    a = np.zeros((8, 8))
    b = np.zeros(8)
    for i in range(4):                                     # getPerspectiveTransform's system, solved in double
        x, y, X, Y = float(pts1[i, 0]), float(pts1[i, 1]), float(pts2[i, 0]), float(pts2[i, 1])
        a[i] = (x, y, 1, 0, 0, 0, -x * X, -y * X)
        a[i + 4] = (0, 0, 0, x, y, 1, -x * Y, -y * Y)
        b[i], b[i + 4] = X, Y
    m = np.append(np.linalg.solve(a, b), 1.0).reshape(3, 3)
    return np.linalg.inv(m), shift


def warp_tiles(img, mask, src_index, minv, shift, n_classes=None, band_rows=0, stats=True):
    """pylc_augment_tiles with the matrices given: copy k is tile src_index[k] of the device uint8 tiles img [n,C,t,t] (and of the class-index
    masks [n,t,t], or None) under the inverse matrix minv[k] (float64 [m,3,3]) and the brightness shift[k].  Returns (img uint8 [m,C,t,t],
    mask uint8 [m,t,t] or None, sums int64 [m,2,C], hist int64 [m, n_classes + 1] or None when there is no mask or no n_classes); sums and
    hist are None with stats=False.  band_rows changes the launch only, never the result."""
    L.init()
    img = _u8(img, 'tiles')
    if img.dim() != 4 or img.shape[2] != img.shape[3]:
        raise ValueError('tiles must be [n,C,t,t], got %s' % (tuple(img.shape),))
    n, c, t = img.shape[0], img.shape[1], img.shape[2]
    src = np.asarray(src_index, dtype=np.int64).reshape(-1)
    m = src.shape[0]
    if m and (src.min() < 0 or src.max() >= n):
        raise ValueError('src_index outside 0..%d' % (n - 1))
    minv = np.ascontiguousarray(np.asarray(minv, dtype=np.float64).reshape(-1, 3, 3))
    shift = np.asarray(shift, dtype=np.int64).reshape(-1)
    if minv.shape[0] != m or shift.shape[0] != m:
        raise ValueError('%d source indices, %d matrices, %d shifts' % (m, minv.shape[0], shift.shape[0]))
    dev = img.device
    if mask is not None:
        mask = _u8(mask, 'mask tiles')
        if tuple(mask.shape) != (n, t, t):
            raise ValueError('mask tiles %s do not match the tiles %s' % (tuple(mask.shape), tuple(img.shape)))
    d_src = torch.from_numpy(src.astype(np.int32)).to(dev)
    d_minv = torch.from_numpy(minv).to(dev)
    d_shift = torch.from_numpy(shift.astype(np.int32)).to(dev)
    out = torch.empty((m, c, t, t), device=dev, dtype=torch.uint8)
    mout = torch.empty((m, t, t), device=dev, dtype=torch.uint8) if mask is not None else None
    sums = torch.zeros((m, 2, c), device=dev, dtype=torch.int64) if stats else None
    hist = None
    if stats and mask is not None and n_classes is not None:
        hist = torch.zeros((m, n_classes + 1), device=dev, dtype=torch.int64)
    check(lib.pylc_augment_tiles(ptr(img), ptr(mask), n, c, t, ptr(d_src), ptr(d_minv), ptr(d_shift), m, band_rows, ptr(out), ptr(mout),
                                 n_classes or 0, ptr(sums), ptr(hist), stream()))
    return out, mout, sums, hist


def augment_tiles(img, mask, src_index, copy_index, band_rows=0, n_classes=None):
    """The reference's augment_transform(tile src_index[k], RandomState(copy_index[k])) for every k, on the device: augment_params, then
    warp_tiles (whose returns these are)."""
    copy = np.asarray(copy_index, dtype=np.int64).reshape(-1)
    tile = int(img.shape[-1])
    params = {int(j): augment_params(int(j), tile) for j in np.unique(copy)}
    minv = np.stack([params[int(j)][0] for j in copy]) if copy.size else np.zeros((0, 3, 3))
    shift = [params[int(j)][1] for j in copy]
    return warp_tiles(img, mask, src_index, minv, shift, n_classes, band_rows)


def oversample_layout(rates):
    """Augmentor.oversample's order before its shuffle (utils/augment.py:206-232): every tile i, followed by its copies j = 0 ..
    rates[i] - 1.  Returns (src, copy), int64 [n + sum(rates)]: the tile each entry comes from and its copy index, -1 for the original."""
    rates = np.asarray(rates)
    if rates.size == 0:
        rates = rates.astype(np.int64)
    if rates.ndim != 1 or (rates.size and (not np.issubdtype(rates.dtype, np.integer) or rates.min() < 0)):
        raise ValueError('rates must be a list of non-negative integers, one per tile')
    src = np.repeat(np.arange(rates.size, dtype=np.int64), rates + 1)
    first = np.cumsum(rates + 1) - (rates + 1)
    copy = np.arange(src.size, dtype=np.int64) - first[src] - 1
    return src, copy


# ---- the per-step augmenter --------------------------------------------------------------------------------------------------------
Q24 = 1 << 24
BORDERS = {'constant': 0, 'reflect': 1}                    # PYLC_BORDER_* (include/pylc_hip.h)
MAT_LINEAR_MAX = 1 << 32                                   # |a00|, |a01|, |a10|, |a11| <= 2^32: a magnification of 1/256 at the least
MAT_SHIFT_LIMIT = 1 << 44                                  # |a02|, |a12| < 2^44: int64 cannot overflow for outputs up to 16384
AUG_MAX_OUT = 16384


def tone_lut(brightness=0.0, contrast=1.0, gamma=1.0, ch=3):
    """The photometric step of the per-step augmenter as a table, uint8 [ch, 256]: in float64, for v = 0..255,
    rint(255 * (clip(contrast * (v - 128) + 128 + brightness, 0, 255) / 255) ** gamma).  Each argument is a scalar or one value per
    channel.  The kernel does one lookup per byte, so any other per-channel curve fits the same table."""
    v = np.arange(256, dtype=np.float64)[None, :]

    def per_channel(a, what):
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        if a.size not in (1, ch):
            raise ValueError('%s: %d values for %d channels' % (what, a.size, ch))
        return np.broadcast_to(a, (ch,))[:, None]
    b, c, g = per_channel(brightness, 'brightness'), per_channel(contrast, 'contrast'), per_channel(gamma, 'gamma')
    if (g <= 0).any():
        raise ValueError('gamma must be positive')
    return np.rint(255.0 * (np.clip(c * (v - 128.0) + 128.0 + b, 0.0, 255.0) / 255.0) ** g).astype(np.uint8)


def affine_q24(src_hw, out_hw, scale=1.0, rotate_deg=0.0, flip_x=False, flip_y=False, centre_xy=None):
    """The inverse affine map of one sample, int64 [6] = (a00, a01, a02, a10, a11, a12) in Q24: output pixel (x, y) reads the source at
    L (x, y) + b with L = (1 / scale) [[cos, sin], [-sin, cos]] diag(-1 if flip_x else 1, -1 if flip_y else 1) and
    b = centre - L ((ow - 1) / 2, (oh - 1) / 2): the output's centre looks at centre_xy of the source (default: its centre,
    ((Ws - 1) / 2, (Hs - 1) / 2)), magnified by `scale` and turned by rotate_deg.  Every entry is rint(value * 2^24)."""
    (hs, ws), (oh, ow) = src_hw, out_hw
    if not scale > 0:
        raise ValueError('scale=%s must be positive' % (scale,))
    cx, cy = ((ws - 1) / 2.0, (hs - 1) / 2.0) if centre_xy is None else centre_xy
    t = math.radians(rotate_deg)
    lin = np.array([[math.cos(t), math.sin(t)], [-math.sin(t), math.cos(t)]]) / float(scale)
    lin = lin * np.array([-1.0 if flip_x else 1.0, -1.0 if flip_y else 1.0])[None, :]
    b = np.array([cx, cy], dtype=np.float64) - lin @ np.array([(ow - 1) / 2.0, (oh - 1) / 2.0])
    return np.rint(np.array([lin[0, 0], lin[0, 1], b[0], lin[1, 0], lin[1, 1], b[1]]) * Q24).astype(np.int64)


def _range(v, what):
    lo, hi = (v, v) if np.isscalar(v) else v
    if not lo <= hi:
        raise ValueError('%s range (%s, %s)' % (what, lo, hi))
    return float(lo), float(hi)


def batch_augment_params(rs, m, src_hw, out_hw, scale=(0.5, 2.0), rotate=0.0, flip=0.5, vflip=0.0, brightness=(0, 0), contrast=(1, 1),
                         gamma=(1, 1), ch=3):
    """The draws of m samples from the numpy RandomState rs -> (mats int64 [m,6], luts uint8 [m,ch,256], or None when the three tone
    ranges are all trivial -- (0, 0), (1, 1), (1, 1)).  Per sample, NINE draws in this order, every one of them made whatever the ranges:
        1. scale       rs.uniform(scale_lo, scale_hi)
        2. angle       rs.uniform(-rotate, rotate), degrees
        3. flip_x      rs.uniform() < flip
        4. flip_y      rs.uniform() < vflip
        5. ux          rs.uniform(-1, 1)
        6. uy          rs.uniform(-1, 1)
        7. brightness  rs.uniform(lo, hi)         8. contrast  rs.uniform(lo, hi)         9. gamma  rs.uniform(lo, hi)
    The window's centre is ((Ws - 1) / 2 + ux (Ws - ow / scale) / 2, (Hs - 1) / 2 + uy (Hs - oh / scale) / 2): the crop moves inside
    the source where it fits, and the source inside the crop where it does not.  The matrix is affine_q24 of these; the table is
    tone_lut of the three tone values, shared by the channels.  A range may be given as one number (no spread)."""
    (hs, ws), (oh, ow) = src_hw, out_hw
    s_lo, s_hi = _range(scale, 'scale')
    if not s_lo > 0:
        raise ValueError('scale range (%s, %s) must be positive' % (s_lo, s_hi))
    if rotate < 0 or not 0 <= flip <= 1 or not 0 <= vflip <= 1:
        raise ValueError('rotate=%s flip=%s vflip=%s' % (rotate, flip, vflip))
    tone = [_range(brightness, 'brightness'), _range(contrast, 'contrast'), _range(gamma, 'gamma')]
    with_lut = tone != [(0.0, 0.0), (1.0, 1.0), (1.0, 1.0)]
    mats = np.empty((m, 6), np.int64)
    luts = np.empty((m, ch, 256), np.uint8) if with_lut else None
    for k in range(m):
        sc = rs.uniform(s_lo, s_hi)
        angle = rs.uniform(-rotate, rotate)
        fx = rs.uniform() < flip
        fy = rs.uniform() < vflip
        ux, uy = rs.uniform(-1, 1), rs.uniform(-1, 1)
        b, c, g = (rs.uniform(lo, hi) for lo, hi in tone)
        centre = ((ws - 1) / 2.0 + ux * (ws - ow / sc) / 2.0, (hs - 1) / 2.0 + uy * (hs - oh / sc) / 2.0)
        mats[k] = affine_q24(src_hw, out_hw, sc, angle, fx, fy, centre)
        if with_lut:
            luts[k] = tone_lut(b, c, g, ch)
    return mats, luts


def check_affine_q24(mats):
    """ValueError for matrices pylc_batch_augment refuses: |a00|, |a01|, |a10|, |a11| > 2^32 or |a02|, |a12| >= 2^44."""
    mats = np.asarray(mats)
    if mats.dtype != np.int64 or mats.ndim != 2 or mats.shape[1] != 6:
        raise ValueError('matrices must be int64 [m,6] in Q24, got %s %s' % (mats.dtype, mats.shape))
    lin, shift = mats[:, [0, 1, 3, 4]], mats[:, [2, 5]]
    if mats.size and ((lin > MAT_LINEAR_MAX) | (lin < -MAT_LINEAR_MAX)).any():
        raise ValueError('a matrix entry a00, a01, a10 or a11 beyond 2^32 in Q24: a magnification below 1/256')
    if mats.size and ((shift >= MAT_SHIFT_LIMIT) | (shift <= -MAT_SHIFT_LIMIT)).any():
        raise ValueError('a matrix entry a02 or a12 at or beyond 2^44 in Q24: a translation of 2^20 pixels')
    return np.ascontiguousarray(mats)


def augment_batch(img, mask, src_index, mats, luts=None, out_hw=None, border='constant', fill=None, mask_fill=None, weights=None,
                  band_rows=0):
    """pylc_batch_augment: sample k is source src_index[k] of the device uint8 planes img [n,C,Hs,Ws] (C 1 or 3; tiles, or one whole
    photograph with n = 1), of the uint8 masks [n,Hs,Ws] and of the float32 weight maps [n,Hs,Ws] (either may be None), under the inverse
    affine map mats[k] (int64 [m,6] in Q24: affine_q24, batch_augment_params) and the tone tables luts[k] (uint8 [m,C,256] or None),
    at out_hw (default: the source's size).  The image is sampled bilinearly, mask and weights by the nearest pixel -- the SAME pixel.
    border='constant': outside the source the image is fill (one value per channel, default 0), the mask mask_fill (required with a
    mask: the ignore label) and the weight 0; border='reflect': BORDER_REFLECT_101.  src_index and mats are host arrays (they travel as
    kernel arguments, 32 samples per launch) or device tensors (int32 / int64: one launch; they are read back here to be checked).
    Returns (img uint8 [m,C,oh,ow], mask uint8 [m,oh,ow] or None, weights float32 [m,oh,ow] or None) on the device.  Everything the
    entry point refuses is refused here, with a ValueError, before anything is launched.  band_rows changes the launch only."""
    if img.dtype != torch.uint8 or img.dim() != 4:
        raise ValueError('sources must be uint8 [n,C,Hs,Ws], got %s %s' % (img.dtype, tuple(img.shape)))
    n, c, hs, ws = img.shape
    if c not in (1, 3):
        raise ValueError('C=%d, not 1 or 3' % c)
    if n < 1 or hs < 2 or ws < 2 or hs * ws >= 1 << 31:
        raise ValueError('%d sources of %dx%d (HxW): at least one, of 2x2 or more' % (n, hs, ws))
    oh, ow = (hs, ws) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if not (1 <= oh <= AUG_MAX_OUT and 1 <= ow <= AUG_MAX_OUT):
        raise ValueError('output %dx%d (HxW) outside 1..%d' % (oh, ow, AUG_MAX_OUT))
    if border not in BORDERS:
        raise ValueError("border must be 'constant' or 'reflect', got %r" % (border,))
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (n, hs, ws)):
        raise ValueError('masks must be uint8 %s, got %s %s' % ((n, hs, ws), mask.dtype, tuple(mask.shape)))
    if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (n, hs, ws)):
        raise ValueError('weights must be float32 %s, got %s %s' % ((n, hs, ws), weights.dtype, tuple(weights.shape)))
    if border == 'constant' and mask is not None and mask_fill is None:
        raise ValueError("border='constant' with a mask needs mask_fill (the ignore label)")
    mask_fill = 0 if mask_fill is None else int(mask_fill)
    if not 0 <= mask_fill <= 255:
        raise ValueError('mask_fill=%d outside 0..255' % mask_fill)
    fill = np.zeros(c, np.int64) if fill is None else np.asarray(fill).reshape(-1)
    if fill.size == 1:
        fill = np.repeat(fill, c)
    if fill.size != c or (fill < 0).any() or (fill > 255).any() or (fill != np.rint(fill)).any():
        raise ValueError('fill must be one uint8 value per channel, got %s' % (fill,))
    fill = np.ascontiguousarray(fill.astype(np.uint8))
    d_src = src_index if torch.is_tensor(src_index) and src_index.is_cuda else None
    if d_src is not None and (d_src.dtype != torch.int32 or not d_src.is_contiguous()):
        raise ValueError('a device src_index must be a contiguous int32 tensor')
    src = np.asarray(src_index.cpu() if torch.is_tensor(src_index) else src_index).reshape(-1)
    if src.size and not np.issubdtype(src.dtype, np.integer):
        raise ValueError('src_index must hold integers')
    m = src.shape[0]
    if m and (src.min() < 0 or src.max() >= n):
        raise ValueError('src_index outside 0..%d' % (n - 1))
    src = np.ascontiguousarray(src.astype(np.int32))
    d_mats = mats if torch.is_tensor(mats) and mats.is_cuda else None
    if d_mats is not None and not d_mats.is_contiguous():
        raise ValueError('device matrices must be contiguous')
    mats = check_affine_q24(mats.cpu().numpy() if torch.is_tensor(mats) else mats)
    if mats.shape[0] != m:
        raise ValueError('%d source indices, %d matrices' % (m, mats.shape[0]))
    if luts is not None:
        if not torch.is_tensor(luts):
            luts = torch.from_numpy(np.ascontiguousarray(luts))
        if luts.dtype != torch.uint8 or tuple(luts.shape) != (m, c, 256):
            raise ValueError('tone tables must be uint8 %s, got %s %s' % ((m, c, 256), luts.dtype, tuple(luts.shape)))
    L.init()
    dev = img.device
    img = img.contiguous()
    mask = mask.contiguous() if mask is not None else None
    weights = weights.contiguous() if weights is not None else None
    luts = luts.to(dev).contiguous() if luts is not None else None
    out = torch.empty((m, c, oh, ow), device=dev, dtype=torch.uint8)
    mout = torch.empty((m, oh, ow), device=dev, dtype=torch.uint8) if mask is not None else None
    wout = torch.empty((m, oh, ow), device=dev, dtype=torch.float32) if weights is not None else None
    check(lib.pylc_batch_augment(ptr(img), ptr(mask), ptr(weights), n, c, hs, ws, ptr(d_src) if d_src is not None else src.ctypes.data,
                                 ptr(d_mats) if d_mats is not None else mats.ctypes.data, ptr(luts), m, oh, ow, BORDERS[border],
                                 fill.ctypes.data, mask_fill, band_rows, ptr(out), ptr(mout), ptr(wout), stream()))
    return out, mout, wout


class Extracted:
    """extract_photo's output.  img: device uint8 [n,C,t,t]; mask: device uint8 [n,t,t] class indices or None; sums: device int64
    [n,2,C] (per tile and channel, sum x and sum x^2); hist: device int64 [n, n_classes + 1] or None (the last bin, values >= n_classes,
    is all zero: extract_photo raises otherwise -- or, with ignore_index, counts exactly the pixels that hold it); geometry: the
    reference's meta.extract fields (photo.fit_geometry's, plus n)."""

    def __init__(self, img, mask, sums, hist, geometry, tile, stride, n_classes, ignore_index=None):
        self.img, self.mask, self.sums, self.hist, self.geometry = img, mask, sums, hist, geometry
        self.tile, self.stride, self.n_classes, self.ignore_index = tile, stride, n_classes, ignore_index


def _check_ignore_index(ignore_index, n_classes):
    """An ignore label of a uint8 mask: the histograms keep it apart from the classes only in their last bin (values >= n_classes)."""
    ignore_index = int(ignore_index)
    if not n_classes <= ignore_index <= 255:
        raise ValueError('ignore_index=%d must lie in n_classes=%d..255 here: the class histogram cannot separate an ignore value inside the '
                         'class range, and masks are uint8' % (ignore_index, n_classes))
    return ignore_index


def _check_bad_classes(hist, n_classes, mask=None, ignore_index=None):
    bad = int(hist[:, -1].sum())
    if ignore_index is not None:
        ignored = int((mask == ignore_index).sum())          # every value >= n_classes must be the ignore value
        if bad != ignored:
            raise ValueError('%d mask pixels hold a class index >= n_classes=%d other than ignore_index=%d' % (bad - ignored, n_classes,
                                                                                                            ignore_index))
        return
    if bad:
        raise ValueError('%d mask pixels hold a class index >= n_classes=%d (one_hot in utils/profile.py:109 would raise)' % (bad, n_classes))


def extract_photo(image, mask_rgb=None, palette=None, tile=512, stride=None, scale=None, fit=False, n_classes=None, device='cuda',
                  ignore_index=None):
    """One image / mask pair through Extractor.extract (utils/extract.py:133-215): a decoded photograph ([H,W,3] RGB or [H,W] / [H,W,1]
    grayscale uint8) and, optionally, its RGB mask [H,W,3] with the schema palette -> Extracted.

    The image is uploaded once, scaled by get_image's arithmetic (photo.scaled_size, INTER_AREA) when `scale` is given, and cut by one
    launch of pylc_extract_tiles.  The mask is nearest-resized to the same scaled size and class-encoded (photo.encode_mask).  stride
    defaults to the tile (config.py:137); n_classes to the palette's length.  ignore_index (n_classes..255, not in the reference): a mask
    colour outside the palette is encoded as this value instead of class 1, and the tiles' last histogram bin counts those pixels.

    fit=True applies adjust_to_tile's second resize (photo.fit_image) and is allowed WITHOUT a mask only: the reference fits the image
    but not the mask (extract.py:154-156 against :188-195), so its own image and mask tile counts diverge there.

    ValueError: fit with a mask; a mask without a palette; n_classes outside 1..16; a resize that would upscale; image and mask scaled sizes
    that differ (the assertion at extract.py:191); a scaled side below the tile; a mask pixel whose class index is >= n_classes."""
    stride = tile if stride is None else stride
    if fit and mask_rgb is not None:
        raise ValueError('fit=True with a mask: the reference fits the image but not the mask (utils/extract.py:154-156, 188-195), so '
                         'their tiles would not correspond')
    if mask_rgb is not None and palette is None:
        raise ValueError('a mask needs the schema palette')
    if n_classes is None and palette is not None:
        n_classes = len(palette)
    if n_classes is not None:
        n_classes = _check_n_classes(n_classes)
    if ignore_index is not None:
        if n_classes is None:
            raise ValueError('ignore_index needs a mask with its palette')
        ignore_index = _check_ignore_index(ignore_index, n_classes)
    shape = tuple(image.shape)
    h, w = shape[0], shape[1]
    if fit:
        geom = photo.fit_geometry(h, w, tile, stride, scale)
        h_c, w_c = geom['h_fitted'], geom['w_fitted']
    else:
        h_s, w_s = photo.scaled_size(h, w, tile, scale)
        if h_s > h or w_s > w:
            raise ValueError('photograph %dx%d (HxW) at scale %s would be upscaled to %dx%d (short side below the tile %d?): INTER_AREA '
                             'downscales only here' % (h, w, scale, h_s, w_s, tile))
        if h_s == 0 or w_s == 0:
            raise ValueError('photograph %dx%d (HxW) at scale %s has a side of 0' % (h, w, scale))
        geom = {'w_full': w, 'h_full': h, 'w_scaled': w_s, 'h_scaled': h_s, 'w_fitted': w_s, 'h_fitted': h_s, 'offset': 0}
        h_c, w_c = h_s, w_s
    rows, cols = tile_grid_counts(h_c, w_c, tile, stride)
    if mask_rgb is not None:
        mh_s, mw_s = photo.scaled_size(mask_rgb.shape[0], mask_rgb.shape[1], tile, scale)
        if (mh_s, mw_s) != (geom['h_scaled'], geom['w_scaled']):
            raise ValueError('mask dims (%dpx x %dpx) do not match image dims (%dpx x %dpx) at scale %s' % (mw_s, mh_s, geom['w_scaled'],
                                                                                                             geom['h_scaled'], scale))
    L.init()
    if fit:
        img, _ = photo.fit_image(image, tile, stride, scale, device)
    else:
        img = photo.resize_area(photo._upload_photo(image, device), h_c, w_c)       # at its own size: a relayout to [C,H,W]
    mask = None
    if mask_rgb is not None:
        mask = photo.encode_mask(mask_rgb, palette, (h_c, w_c), img.device, unmatched=1 if ignore_index is None else ignore_index)
    tiles, mtiles, sums, hist = cut_tiles(img, mask, tile, stride, n_classes if mask is not None else None)
    if hist is not None:
        _check_bad_classes(hist, n_classes, mtiles, ignore_index)
    geom = dict(geom, n=rows * cols)
    return Extracted(tiles, mtiles, sums, hist, geom, tile, stride, n_classes, ignore_index)


# ---- the profile (host, double arithmetic on exact integers) ---------------------------------------------------------------------
def jsd(p, q):
    """utils/metrics.py:90-111, eps in the same places"""
    eps = 1e-8
    m = 0.5 * (p + q + eps)
    return 0.5 * np.sum(np.multiply(p, np.log(p / m + eps))) + 0.5 * np.sum(np.multiply(q, np.log(q / m + eps)))


def m2(p, n_classes):
    """utils/metrics.py:114-132"""
    if n_classes <= 1:
        raise ValueError('M2 variance needs more than one class')
    return (n_classes / (n_classes - 1)) * (1 - np.sum(p ** 2))


def profile_from_sums(sums, hist, tile, n_classes, ignore=False):
    """get_profile (utils/profile.py:92-148) from per-tile integer sums: sums int [n,2,C] (sum x, sum x^2), hist int [n, n_classes].

    ignore=True (not in the reference): hist is [n, n_classes + 1] and its last bin counts the pixels that carry the ignore label.  px_dist,
    dset_px_dist, probs, weights, m2 and jsd are then taken over the VALID pixels, dset_px_count is their number and ignored_px_count the
    others'; px_mean and px_std do not depend on labels and stay as they are.

    Per tile and channel, with N = tile^2: mean = S / N and the unbiased std = sqrt((N * SS - S^2) / (N * (N - 1))) -- torch.mean /
    torch.std over (0, 2, 3) of a [1,C,t,t] batch; for one channel the reference pools over the whole tile, which is the same thing.
    px_mean and px_std are the MEANS OVER TILES of these per-tile values: that is the reference's definition, which its networks were
    trained with; px_std is therefore NOT the standard deviation of the dataset's pixels (it leaves out the spread between tiles).

    Returns a dict under the reference's meta names: n_samples, tile_px_count, px_mean, px_std, px_dist [n][n_classes], dset_px_dist,
    dset_px_count, probs, weights (1 / ln(1.02 + probs), normalised by its maximum), m2, jsd (against the uniform distribution)."""
    sums = np.asarray(sums)
    hist = np.asarray(hist, dtype=np.int64)
    n, _, c = sums.shape
    if n == 0:
        raise ValueError('profile of an empty tile set')
    N = int(tile) * int(tile)
    mean = np.empty((n, c))
    std = np.empty((n, c))
    for i in range(n):                                   # python integers: N * SS and S^2 pass 2^63 from tiles of 8192^2 on
        for k in range(c):
            s, ss = int(sums[i, 0, k]), int(sums[i, 1, k])
            mean[i, k] = s / N
            std[i, k] = math.sqrt((N * ss - s * s) / (N * (N - 1)))
    px_dist = hist[:, :n_classes]
    dset_px_dist = np.sum(px_dist, axis=0)
    dset_px_count = np.sum(dset_px_dist)
    ignored = 0
    if ignore:
        if hist.shape[1] != n_classes + 1:
            raise ValueError('ignore=True needs histograms of n_classes + 1 = %d bins, got %d' % (n_classes + 1, hist.shape[1]))
        ignored = int(hist[:, n_classes].sum())
        if int(dset_px_count) == 0:
            raise ValueError('profile of a tile set without a labelled pixel')
    if int(dset_px_count) + ignored != n * N:
        raise ValueError('pixel distribution (%d) does not match the tile count (%d x %d)' % (int(dset_px_count), n, N))
    probs = dset_px_dist / dset_px_count
    weights = 1 / (np.log(1.02 + probs))
    weights = weights / np.max(weights)
    balanced = np.empty(n_classes)
    balanced.fill(1 / n_classes)
    return {'n_samples': n, 'tile_size': int(tile), 'tile_px_count': N, 'ch': c, 'n_classes': int(n_classes),
            'px_mean': (mean.sum(0) / n).tolist(), 'px_std': (std.sum(0) / n).tolist(),
            'px_dist': px_dist.tolist(), 'dset_px_dist': dset_px_dist.tolist(), 'dset_px_count': int(dset_px_count),
            'probs': probs.tolist(), 'weights': weights.tolist(), 'm2': float(m2(probs, n_classes)), 'jsd': float(jsd(probs, balanced)),
            **({'ignored_px_count': ignored} if ignore else {})}


def oversample_rates(profile, rate_coef_range=(1, 21), threshold_range=(0, 3.), rate_range=(0, 4), n_samples_ratio=0.36):
    """Augmentor.optimize (utils/augment.py:100-180) on a profile dict, in the same numpy dtypes and operation order: per-tile scores from
    the class histograms, a grid over rate coefficients (step 1) and thresholds (step 0.05), rates = int(coef * score) where the score
    passes the threshold, clipped to rate_range; of the candidates that add fewer than int(n_samples_ratio * n) tiles, the first one of
    least JSD against the uniform distribution.  Returns {'rates' (int array [n]: copies to add per tile), 'threshold', 'rate_coef',
    'probs', 'n_samples', 'aug_n_samples', 'jsd', 'm2'}.  ValueError where the reference asserts 'No augmentation optimization found'."""
    eps = 1e-8
    px_dist = np.array(profile['px_dist'], dtype='long')
    px_count = profile['tile_px_count']
    n_classes = px_dist.shape[1]
    input_size = px_dist.shape[0]
    dset_probs = np.array(profile['probs'], dtype='float32') + eps
    oversample_filter = np.clip(1 / n_classes - dset_probs, a_min=0, a_max=1.)
    probs = px_dist / px_count
    probs_weighted = np.multiply(np.multiply(probs, 1 / dset_probs), oversample_filter)
    scores = np.sqrt(np.sum(probs_weighted, axis=1))
    rate_coefs = np.arange(min(rate_coef_range), max(rate_coef_range), 1.)
    thresholds = np.arange(min(threshold_range), max(threshold_range), 0.05)
    balanced = np.empty(n_classes)
    balanced.fill(1 / n_classes)
    jsds, found = [], []
    for rate_coef in rate_coefs:
        for threshold in thresholds:
            over_sample = scores > threshold
            rates = np.multiply(over_sample, rate_coef * scores).astype(int)
            rates = np.clip(rates, rate_range[0], rate_range[1])
            if np.sum(rates) < int(n_samples_ratio * input_size):
                aug_px_dist = np.multiply(np.expand_dims(rates, axis=1), px_dist)
                full_px_dist = px_dist + aug_px_dist
                full_px_probs = np.sum(full_px_dist, axis=0) / np.sum(full_px_dist)
                m2_sample = m2(full_px_probs, n_classes)
                jsd_sample = jsd(full_px_probs, balanced)
                jsds.append(jsd_sample)
                found.append({'probs': full_px_probs, 'threshold': float(threshold), 'rate_coef': float(rate_coef), 'rates': rates,
                              'n_samples': int(np.sum(full_px_dist) / px_count), 'aug_n_samples': int(np.sum(rates)),
                              'jsd': float(jsd_sample), 'm2': float(m2_sample)})
    if not jsds:
        raise ValueError('No augmentation optimization found.')
    return found[int(np.argmin(np.asarray(jsds)))]


# ---- the container -------------------------------------------------------------------------------------------------------------
def _pinned(shape):
    t = torch.empty(shape, dtype=torch.uint8)
    return t.pin_memory() if torch.cuda.is_available() else t


class _Batches:
    """re-iterable over a TileSet's (img uint8 [B,C,t,t], mask uint8 [B,t,t]) batches"""

    def __init__(self, tiles, batch_size, drop_last):
        self.tiles, self.batch_size, self.drop_last = tiles, int(batch_size), drop_last
        if self.batch_size <= 0:
            raise ValueError('batch_size=%s' % batch_size)

    def __len__(self):
        n = len(self.tiles)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        ts = self.tiles
        img, mask = ts._storage()
        for k in range(len(self)):
            lo = ts.start + k * self.batch_size
            hi = min(lo + self.batch_size, ts.end)
            if ts.keep == 'device':
                idx = torch.arange(lo, hi, device=img.device)
                yield img.index_select(0, idx), (mask.index_select(0, idx) if mask is not None else None)
            else:
                yield img[lo:hi].numpy(), (mask[lo:hi].numpy() if mask is not None else None)


class _AugmentedBatches:
    """re-iterable over a TileSet's batches, each augmented anew (batch_augment_params -> augment_batch): device (img uint8 [B,C,oh,ow],
    mask uint8 [B,oh,ow] or None).  ONE RandomState(seed) belongs to the iterable and advances across iterations: every epoch differs, and
    a run with the same seed repeats."""

    def __init__(self, tiles, batch_size, drop_last, augment, seed, out, device):
        self.plain = _Batches(tiles, batch_size, drop_last)
        self.tiles, self.augment, self.device = tiles, dict(augment), device
        self.out_hw = (tiles.tile, tiles.tile) if out is None else ((int(out), int(out)) if np.isscalar(out) else (int(out[0]), int(out[1])))
        batch_augment_params(np.random.RandomState(0), 0, (tiles.tile, tiles.tile), self.out_hw, ch=tiles.ch, **self.augment)      # the keywords
        self.rs = np.random.RandomState(seed)

    def __len__(self):
        return len(self.plain)

    def __iter__(self):
        ts, bs = self.tiles, self.plain.batch_size
        img, mask = ts._storage()
        kw = {'border': 'reflect'}
        if ts.ignore_index is not None:
            mean = ts.sums[:, 0, :].sum(0) / float(len(ts) * ts.tile * ts.tile)
            kw = {'border': 'constant', 'mask_fill': ts.ignore_index, 'fill': np.rint(mean)}
        for k in range(len(self)):
            lo = ts.start + k * bs
            hi = min(lo + bs, ts.end)
            mats, luts = batch_augment_params(self.rs, hi - lo, (ts.tile, ts.tile), self.out_hw, ch=ts.ch, **self.augment)
            if ts.keep == 'device':
                s_img, s_mask, src = img, mask, np.arange(lo, hi)
            else:
                s_img = img[lo:hi].to(self.device, non_blocking=True)
                s_mask = mask[lo:hi].to(self.device, non_blocking=True) if mask is not None else None
                src = np.arange(hi - lo)
            x, y, _ = augment_batch(s_img, s_mask, src, mats, luts, self.out_hw, **kw)
            yield x, y


class TileSet:
    """Tiles of one size with their integer statistics, resident on the device (keep='device') or in pinned host memory (keep='host');
    the statistics always end on the host (numpy int64).  add() appends extract_photo's output, from_arrays() takes tiles cut elsewhere
    (their statistics come from pylc_tile_stats), coshuffle() permutes everything alike, partition() is a view, batches() feeds
    Model.train and profile() is the reference's dataset profile.  ignore_index (n_classes..255): masks may hold this value for pixels
    without a label; the histograms then have a last column with their count per tile, and the profile is taken over the other pixels."""

    def __init__(self, ch, n_classes, tile, keep='device', ignore_index=None):
        if keep not in ('device', 'host'):
            raise ValueError("keep must be 'device' or 'host', got %r" % (keep,))
        if ch not in (1, 3):
            raise ValueError('ch must be 1 or 3, got %s' % ch)
        self.ch, self.n_classes, self.tile, self.keep = int(ch), _check_n_classes(n_classes), int(tile), keep
        self.ignore_index = None if ignore_index is None else _check_ignore_index(ignore_index, self.n_classes)
        self._own = self                       # partitions share their parent's storage
        self._img, self._mask = [], []         # chunks; _storage() joins them
        self._sums = np.zeros((0, 2, self.ch), np.int64)
        self._hist = np.zeros((0, self.n_classes + (0 if self.ignore_index is None else 1)), np.int64)
        self._lo, self._hi = 0.0, 1.0

    # -- filling
    def _append(self, img, mask, sums, hist):
        if self._own is not self:
            raise ValueError('a partition is a view: add to the tile set it came from')
        n = img.shape[0]
        if tuple(img.shape[1:]) != (self.ch, self.tile, self.tile):
            raise ValueError('tiles %s do not fit a [n,%d,%d,%d] set' % (tuple(img.shape), self.ch, self.tile, self.tile))
        if (mask is None) != (hist is None):
            raise ValueError('mask tiles and class histograms come together')
        if self._img and (mask is None) != (not self._mask):
            raise ValueError('a tile set holds masks for all of its tiles or for none')
        if mask is not None and tuple(mask.shape) != (n, self.tile, self.tile):
            raise ValueError('mask tiles %s do not match the tiles %s' % (tuple(mask.shape), tuple(img.shape)))
        sums = np.asarray(sums.cpu() if torch.is_tensor(sums) else sums, dtype=np.int64).reshape(n, 2, self.ch)
        if hist is not None:
            hist = np.asarray(hist.cpu() if torch.is_tensor(hist) else hist, dtype=np.int64).reshape(n, -1)
            if self.ignore_index is not None:
                if hist.shape[1] != self.n_classes + 1:
                    raise ValueError('histograms of %d bins in a set of %d classes with an ignore label' % (hist.shape[1], self.n_classes))
                _check_bad_classes(hist, self.n_classes, mask, self.ignore_index)
            elif hist.shape[1] == self.n_classes + 1:
                if hist[:, -1].any():
                    raise ValueError('%d mask pixels hold a class index >= n_classes=%d' % (int(hist[:, -1].sum()), self.n_classes))
                hist = hist[:, :self.n_classes]
            if hist.shape[1] != self._hist.shape[1]:
                raise ValueError('histograms of %d bins in a set of %d classes' % (hist.shape[1], self.n_classes))
            self._hist = np.concatenate([self._hist, hist])
        self._sums = np.concatenate([self._sums, sums])

        def hold(t):
            if self.keep == 'device':
                if not t.is_cuda:
                    raise L.PylcError("keep='device' holds device tensors")
                return t
            p = _pinned(t.shape)
            p.copy_(t)
            return p
        self._img.append(hold(img))
        if mask is not None:
            self._mask.append(hold(mask))
        return self

    def add(self, extracted):
        """Append extract_photo's tiles and statistics."""
        if extracted.tile != self.tile:
            raise ValueError('tiles of %d in a set of %d' % (extracted.tile, self.tile))
        if extracted.mask is not None and extracted.n_classes != self.n_classes:
            raise ValueError('tiles of %s classes in a set of %d' % (extracted.n_classes, self.n_classes))
        if extracted.mask is not None and getattr(extracted, 'ignore_index', None) not in (None, self.ignore_index):
            raise ValueError('tiles with ignore_index=%s in a set with %s' % (extracted.ignore_index, self.ignore_index))
        return self._append(extracted.img, extracted.mask, extracted.sums, extracted.hist)

    def from_arrays(self, img, mask=None, sums=None, hist=None, device='cuda'):
        """Append existing tiles (uint8 [n,C,t,t], masks uint8 [n,t,t]; numpy or tensors, host or device).  Their statistics are computed
        on the device by pylc_tile_stats unless given (sums int [n,2,C], hist int [n, n_classes])."""
        img = torch.as_tensor(img)
        mask = torch.as_tensor(mask) if mask is not None else None
        if sums is None:
            d_img = img.to(device)
            d_mask = mask.to(device) if mask is not None else None
            sums, hist = tile_stats(d_img, d_mask, self.n_classes)
            if self.keep == 'device':
                img, mask = d_img, d_mask
        elif self.keep == 'device':
            img, mask = img.to(device), (mask.to(device) if mask is not None else None)
        return self._append(img.contiguous(), mask.contiguous() if mask is not None else None, sums, hist)

    # -- access
    def _storage(self):
        own = self._own
        for name in ('_img', '_mask'):
            chunks = getattr(own, name)
            if len(chunks) > 1:
                if own.keep == 'device':
                    joined = torch.cat(chunks)
                else:
                    joined = _pinned((sum(c.shape[0] for c in chunks),) + tuple(chunks[0].shape[1:]))
                    torch.cat(chunks, out=joined)
                setattr(own, name, [joined])
        return (own._img[0] if own._img else None), (own._mask[0] if own._mask else None)

    @property
    def start(self):
        return int(math.ceil(self._lo * self._own._sums.shape[0]))          # db/database.py:89-90

    @property
    def end(self):
        return int(math.ceil(self._hi * self._own._sums.shape[0]))

    def __len__(self):
        return self.end - self.start

    @property
    def img(self):
        t = self._storage()[0]
        return None if t is None else t[self.start:self.end]

    @property
    def mask(self):
        t = self._storage()[1]
        return None if t is None else t[self.start:self.end]

    @property
    def sums(self):
        return self._own._sums[self.start:self.end]

    @property
    def hist(self):
        return self._own._hist[self.start:self.end] if self._own._mask else None

    def coshuffle(self, seed):
        """One np.random.RandomState(seed).permutation applied to images, masks and statistics alike (coshuffle, utils/tools.py:361-385,
        seeded).  Partitions taken before see the new order."""
        if self._own is not self:
            raise ValueError('a partition is a view: shuffle the tile set it came from')
        n = self._sums.shape[0]
        perm = np.random.RandomState(seed).permutation(n)
        img, mask = self._storage()
        idx = torch.from_numpy(perm)

        def take(t):
            if t is None:
                return []
            if self.keep == 'device':
                return [t.index_select(0, idx.to(t.device))]
            out = _pinned(t.shape)
            torch.index_select(t, 0, idx, out=out)
            return [out]
        self._img, self._mask = take(img), take(mask)
        self._sums = self._sums[perm]
        if self._hist.shape[0] == n:
            self._hist = self._hist[perm]
        return self

    def partition(self, lo, hi):
        """The tiles ceil(lo * n) .. ceil(hi * n) - 1 as a view (MLPDataset(partition=(0, 0.8)), db/database.py:89-91)."""
        if not 0 <= lo <= hi <= 1:
            raise ValueError('partition (%s, %s) outside 0 <= lo <= hi <= 1' % (lo, hi))
        view = object.__new__(TileSet)
        view.ch, view.n_classes, view.tile, view.keep, view.ignore_index = self.ch, self.n_classes, self.tile, self.keep, self.ignore_index
        view._own = self._own
        span = self._hi - self._lo
        view._lo, view._hi = self._lo + lo * span, self._lo + hi * span
        return view

    def batches(self, batch_size, drop_last=True, augment=None, seed=0, out=None, device='cuda'):
        """A re-iterable of (img uint8 [B,C,t,t], mask uint8 [B,t,t] or None): device tensors gathered by index (keep='device', what
        Model.train takes as is), or host arrays out of the pinned store (keep='host', what data.TileFeeder takes).

        augment: a dict of batch_augment_params' keywords (scale, rotate, flip, vflip, brightness, contrast, gamma; {} for its defaults).
        Every batch is then drawn anew and made by one launch of pylc_batch_augment, and the iterable yields DEVICE (img, mask) of size
        `out` ((oh, ow) or one side; default: the tile) -- a host set uploads the batch's tiles to `device` first.  With an ignore_index
        the border is constant: pixels the map takes outside the tile get that label and the image there is rint(the set's px mean);
        without one the tile is mirrored (BORDER_REFLECT_101).  One RandomState(seed) belongs to the iterable and advances across
        epochs.  augment=None: the stored tiles as they are (seed, out and device are not used)."""
        if augment is None:
            return _Batches(self, batch_size, drop_last)
        return _AugmentedBatches(self, batch_size, drop_last, augment, seed, out, device)

    def oversample(self, rates, chunk=64, device='cuda'):
        """Augmentor.oversample (utils/augment.py:184-239) without its shuffle: a NEW tile set of the same keep mode that holds, for every
        tile i in order, the tile followed by rates[i] augmented copies (augment_tiles with copy indices 0 .. rates[i] - 1; rates as
        oversample_rates returns them).  The originals carry their statistics over; the copies' are computed on the device by the launch
        that makes them.  `chunk` source tiles are worked on at a time (a host set uploads them to `device`), so that the temporaries stay at
        chunk * (1 + max(rates)) tiles.  Follow with coshuffle(seed) and profile().
        ValueError: len(rates) != len(self), a set without masks, a copy with a class index >= n_classes."""
        src, copy = oversample_layout(rates)
        n = len(self)
        if len(rates) != n:
            raise ValueError('%d rates for %d tiles' % (len(rates), n))
        if self.hist is None:
            raise ValueError('oversampling needs masks: the rates come from their class histograms')
        if chunk <= 0:
            raise ValueError('chunk=%s' % chunk)
        out = TileSet(self.ch, self.n_classes, self.tile, self.keep, self.ignore_index)
        img, mask = self.img, self.mask
        pad = 1 if self.ignore_index is None else 0         # (with an ignore label the stored histograms have the last bin already)
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            sel = (src >= lo) & (src < hi)
            c_src, c_copy = src[sel] - lo, copy[sel]
            aug = c_copy >= 0
            d_img, d_mask = img[lo:hi], mask[lo:hi]
            if self.keep == 'host':
                d_img, d_mask = d_img.to(device, non_blocking=True), d_mask.to(device, non_blocking=True)
            a_img, a_mask, a_sums, a_hist = augment_tiles(d_img, d_mask, c_src[aug], c_copy[aug], n_classes=self.n_classes)
            # entry k of the chunk: original c_src[k], or the next copy in launch order
            pick = np.where(aug, (hi - lo) + np.cumsum(aug) - 1, c_src)
            idx = torch.from_numpy(pick).to(a_img.device)
            sums = np.concatenate([self.sums[lo:hi], a_sums.cpu().numpy()])[pick]
            hist = np.concatenate([np.pad(self.hist[lo:hi], ((0, 0), (0, pad))), a_hist.cpu().numpy()])[pick]
            out._append(torch.cat([d_img, a_img]).index_select(0, idx), torch.cat([d_mask, a_mask]).index_select(0, idx), sums, hist)
        return out

    def profile(self):
        """The reference's dataset profile (profile_from_sums) of these tiles, as a dict under its meta names: Meta.update(profile) picks
        up px_mean, px_std and weights.  Note px_std: the mean over tiles of the per-tile std, not the dataset's."""
        if self.hist is None:
            raise ValueError('a profile needs masks')
        return profile_from_sums(self.sums, self.hist, self.tile, self.n_classes, ignore=self.ignore_index is not None)
