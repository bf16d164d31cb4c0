"""The per-step training augmenter (pylc_batch_augment, csrc/batch_augment.hip) restated in numpy: exact int64
arithmetic, nothing rounded twice, so the kernel is compared with it bit for bit and no pixel is left out.

Output sample k is made from source plane set src_index[k] under the inverse affine map mats[k] = (a00, a01, a02, a10, a11, a12), six
int64 numbers in Q24 fixed point.  For output pixel (x, y), pixel centres at integers:

    X = a00 x + a01 y + a02        Y = a10 x + a11 y + a12
    image:  sx = X >> 24, fx = (X >> 19) & 31, likewise sy, fy       (arithmetic shifts: floor)
            N  = (t(sy,sx)(32-fx) + t(sy,sx+1) fx)(32-fy) + (t(sy+1,sx)(32-fx) + t(sy+1,sx+1) fx) fy
            v  = (N + 512) >> 10;  out = lut[k][c][v]                 (lut None: the identity)
    mask, weights (nearest):  mx = (X + 2^23) >> 24, my likewise;  out = mask[my][mx], w[my][mx]

border 'constant': a tap outside the source reads fill[c], a mask pixel outside is mask_fill, a weight outside 0.0f.
border 'reflect':  BORDER_REFLECT_101 on the indices (period 2(n-1)), for any integer."""
import numpy as np

Q = 24
ONE = 1 << Q
MAT_LINEAR_MAX = 1 << 32                  # |a00|, |a01|, |a10|, |a11| above this are refused (a magnification below 1/256)
MAT_SHIFT_LIMIT = 1 << 44                 # |a02|, |a12| at or above this are refused
BORDERS = {'constant': 0, 'reflect': 1}


def reflect101(p, n):
    """BORDER_REFLECT_101 of any integer index array p into 0..n-1 (n >= 2)"""
    period = 2 * (n - 1)
    q = np.abs(p) % period
    return np.where(q < n, q, period - q)


def batch_augment_np(img, mask, weights, src_index, mats, lut, out_hw, border, fill=None, mask_fill=None):
    """img uint8 [n,C,Hs,Ws]; mask uint8 [n,Hs,Ws] or None; weights float32 [n,Hs,Ws] or None; src_index int [m]; mats int64 [m,6];
    lut uint8 [m,C,256] or None; border 'constant' (fill uint8 [C], mask_fill 0..255) or 'reflect'.
    Returns (uint8 [m,C,oh,ow], uint8 [m,oh,ow] or None, float32 [m,oh,ow] or None)."""
    img = np.asarray(img)
    n, C, Hs, Ws = img.shape
    oh, ow = out_hw
    mats = np.asarray(mats, dtype=np.int64).reshape(-1, 6)
    m = mats.shape[0]
    src_index = np.asarray(src_index, dtype=np.int64).reshape(-1)
    assert src_index.shape[0] == m and border in BORDERS
    out = np.empty((m, C, oh, ow), np.uint8)
    out_mask = np.empty((m, oh, ow), np.uint8) if mask is not None else None
    out_w = np.empty((m, oh, ow), np.float32) if weights is not None else None
    x = np.arange(ow, dtype=np.int64)[None, :]
    y = np.arange(oh, dtype=np.int64)[:, None]
    for k in range(m):
        a00, a01, a02, a10, a11, a12 = (int(v) for v in mats[k])
        s = int(src_index[k])
        X = a00 * x + a01 * y + a02
        Y = a10 * x + a11 * y + a12
        sx, fx = X >> Q, (X >> (Q - 5)) & 31
        sy, fy = Y >> Q, (Y >> (Q - 5)) & 31

        def taps(plane, outside, yy, xx):
            if border == 'reflect':
                return plane[reflect101(yy, Hs), reflect101(xx, Ws)].astype(np.int64)
            inside = (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
            got = plane[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)].astype(np.int64)
            return np.where(inside, got, outside)

        for c in range(C):
            p = img[s, c]
            f = int(fill[c]) if border == 'constant' else 0
            top = taps(p, f, sy, sx) * (32 - fx) + taps(p, f, sy, sx + 1) * fx
            bot = taps(p, f, sy + 1, sx) * (32 - fx) + taps(p, f, sy + 1, sx + 1) * fx
            v = (top * (32 - fy) + bot * fy + 512) >> 10
            out[k, c] = v.astype(np.uint8) if lut is None else np.asarray(lut)[k, c][v]
        if mask is not None or weights is not None:
            mx, my = (X + (ONE >> 1)) >> Q, (Y + (ONE >> 1)) >> Q
            if border == 'reflect':
                iy, ix = reflect101(my, Hs), reflect101(mx, Ws)
                inside = np.ones((oh, ow), bool)
            else:
                inside = (my >= 0) & (my < Hs) & (mx >= 0) & (mx < Ws)
                iy, ix = np.clip(my, 0, Hs - 1), np.clip(mx, 0, Ws - 1)
            if mask is not None:
                out_mask[k] = np.where(inside, mask[s][iy, ix], 0 if mask_fill is None else mask_fill).astype(np.uint8)
            if weights is not None:
                out_w[k] = np.where(inside, weights[s][iy, ix], np.float32(0)).astype(np.float32)
    return out, out_mask, out_w


def smooth_image(n, C, Hs, Ws, seed):
    """a smooth uint8 image (a few low-frequency waves): neighbour differences of a few grey levels"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
    out = np.empty((n, C, Hs, Ws), np.uint8)
    for i in range(n):
        for c in range(C):
            fx, fy, ph = rs.uniform(0.02, 0.08, 2), rs.uniform(0.02, 0.08, 2), rs.uniform(0, 6.28, 2)
            v = 128 + 60 * np.sin(fx[0] * xx + fy[0] * yy + ph[0]) + 50 * np.cos(fx[1] * xx - fy[1] * yy + ph[1])
            out[i, c] = np.rint(np.clip(v, 0, 255)).astype(np.uint8)
    return out


def sources(n, C, Hs, Ws, seed, n_classes=5):
    """seeded sources: random uint8 image planes, a blocky class mask, positive float32 weights"""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (n, C, Hs, Ws)).astype(np.uint8)
    mask = rs.randint(0, n_classes, (n, Hs // 4 + 1, Ws // 4 + 1)).astype(np.uint8).repeat(4, 1).repeat(4, 2)[:, :Hs, :Ws]
    weights = rs.uniform(0.25, 4.0, (n, Hs, Ws)).astype(np.float32)
    return img, np.ascontiguousarray(mask), weights
