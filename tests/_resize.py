"""The fp32 pooling and resize kernels of pylc_amd/csrc/pool_resize.hip stated in numpy, from the formulas of include/pylc_hip.h and the
comments of that file, with the per-element bounds tests/test_pool_resize_abi_gpu.py uses.  Tensors are NHWC,
[B, H, W, C].  Not a test module.

Bilinear, align_corners=True.  The index pair and weight pair of an output position are computed in float32 exactly as the kernels'
lerp_of / ac_scale state PyTorch's rule (lerp_f32); the interpolation and its transpose are then taken in float64 WITH THOSE float32
WEIGHTS.  An index that flips where scale * dst lands a rounding away from an integer is thereby part of the model, not an error of the
kernel.  u = 2^-24; bounds are first-order worst-case: (roundings on the path) x u x sum |w x|.
"""
import numpy as np

U = 2.0 ** -24
f32 = np.float32


# ---- bilinear -------------------------------------------------------------------------------------------------------------------------------
def ac_scale(n_in, n_out):
    return f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)


def lerp_f32(dst, n_in, n_out):
    """(i0, i1, w0, w1) of the output positions `dst` (int array): src = scale * dst in float32, i0 = (int)src clamped to n_in - 1,
    i1 = i0 + (i0 < n_in - 1), w1 = src - i0, w0 = 1 - w1 (float32)."""
    src = ac_scale(n_in, n_out) * np.asarray(dst).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = src - i0.astype(np.float32)
    w0 = f32(1) - w1
    assert w0.dtype == w1.dtype == np.float32
    return i0, i1, w0, w1


def lerp_matrix(n_in, n_out):
    """(A [n_out, n_in] float64 holding the float32 weights exactly -- both on one pixel where i1 == i0 --, hits [n_in]: how many output
    positions reference each input pixel)."""
    i0, i1, w0, w1 = lerp_f32(np.arange(n_out), n_in, n_out)
    A = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(A, (o, i0), w0.astype(np.float64))
    np.add.at(A, (o, i1), w1.astype(np.float64))
    ref = np.zeros((n_out, n_in), bool)
    ref[o, i0] = True
    ref[o, i1] = True
    return A, ref.sum(0)


def bilinear64(x, OH, OW):
    Ah, _ = lerp_matrix(x.shape[1], OH)
    Aw, _ = lerp_matrix(x.shape[2], OW)
    return np.einsum('oh,bhwc,pw->bopc', Ah, x.astype(np.float64), Aw)


def bilinear_fwd_bound(x, OH, OW):
    """r = wh0 (ww0 v00 + ww1 v01) + wh1 (ww0 v10 + ww1 v11): a value passes its product with ww (1 rounding), the inner sum (1), the
    product with wh (1) and the outer sum (1): 4u sum |w x|."""
    Ah, _ = lerp_matrix(x.shape[1], OH)
    Aw, _ = lerp_matrix(x.shape[2], OW)
    return 4 * U * np.einsum('oh,bhwc,pw->bopc', np.abs(Ah), np.abs(x.astype(np.float64)), np.abs(Aw))


def bilinear_f32(x, OH, OW):
    """The forward in float32, in the kernels' expression order (both launch forms evaluate the same expression)."""
    h0, h1, a0, a1 = lerp_f32(np.arange(OH), x.shape[1], OH)
    w0, w1, b0, b1 = lerp_f32(np.arange(OW), x.shape[2], OW)
    a0, a1 = a0[None, :, None, None], a1[None, :, None, None]
    b0, b1 = b0[None, None, :, None], b1[None, None, :, None]
    v00, v01 = x[:, h0][:, :, w0], x[:, h0][:, :, w1]
    v10, v11 = x[:, h1][:, :, w0], x[:, h1][:, :, w1]
    t0 = b0 * v00
    t0 = t0 + b1 * v01
    t1 = b0 * v10
    t1 = t1 + b1 * v11
    r = a0 * t0 + a1 * t1
    assert r.dtype == np.float32
    return r


def bilinear_bwd64(dy, H, W):
    """The transpose: dx = Ah^T dy Aw."""
    Ah, _ = lerp_matrix(H, dy.shape[1])
    Aw, _ = lerp_matrix(W, dy.shape[2])
    return np.einsum('oh,bopc,pw->bhwc', Ah, dy.astype(np.float64), Aw)


def bilinear_bwd_bound(dy, H, W, separable):
    """Direct kernel: a term (wh ww) dy carries wh resp. ww (u each only where both weights of a border position were added: counted
    always), their product (1), the product with dy (1), and at most T - 1 additions, T = Th[h] Tw[w] the number of output positions that
    reference the pixel: (T + 3) u sum |w dy|.
    Separable: the pass along W leaves (Tw + 1) u on every term (weight, product, Tw - 1 additions), the pass along H adds (Th + 1) u:
    (Th + Tw + 2) u sum |w dy|."""
    Ah, th = lerp_matrix(H, dy.shape[1])
    Aw, tw = lerp_matrix(W, dy.shape[2])
    mag = np.einsum('oh,bopc,pw->bhwc', np.abs(Ah), np.abs(dy.astype(np.float64)), np.abs(Aw))
    k = (th[:, None] + tw[None, :] + 2) if separable else (th[:, None] * tw[None, :] + 3)
    return k[None, :, :, None] * U * mag


def continuity_bound(x, OH, OW):
    """|model - exact align_corners interpolation| where the float32 source coordinate is off by dsrc: along one axis the interpolant is
    piecewise linear and continuous, so the value moves by at most |dsrc| x the largest neighbour difference along that axis (for both
    axes: the sum).  dsrc <= 2u x coordinate (the scale's division and the product), plus u for the weight 1 - w1."""
    x = x.astype(np.float64)
    B, H, W, C = x.shape
    dh = np.abs(np.diff(x, axis=1)).max() if H > 1 else 0.0
    dw = np.abs(np.diff(x, axis=2)).max() if W > 1 else 0.0
    return 3 * U * (max(H - 1, 1) * dh + max(W - 1, 1) * dw) + 3 * U * np.abs(x).max()


# ---- max pool -------------------------------------------------------------------------------------------------------------------------------
def pool_out(n, k, s, pad):
    return (n + 2 * pad - k) // s + 1


def maxpool_fwd(x, k, s, pad):
    """(y, idx): the maximum and its scan-order code kh * k + kw; the first valid element seeds, then `v > best` replaces: the first
    maximum wins (and -0 / +0 compare equal: the earlier one stays)."""
    B, H, W, C = x.shape
    OH, OW = pool_out(H, k, s, pad), pool_out(W, k, s, pad)
    y = np.zeros((B, OH, OW, C), x.dtype)
    idx = np.zeros((B, OH, OW, C), np.uint8)
    for oh in range(OH):
        for ow in range(OW):
            first = True
            for kh in range(k):
                h = oh * s - pad + kh
                if not 0 <= h < H:
                    continue
                for kw in range(k):
                    w = ow * s - pad + kw
                    if not 0 <= w < W:
                        continue
                    v = x[:, h, w, :]
                    take = np.ones(v.shape, bool) if first else v > y[:, oh, ow, :]
                    y[:, oh, ow, :] = np.where(take, v, y[:, oh, ow, :])
                    idx[:, oh, ow, :] = np.where(take, kh * k + kw, idx[:, oh, ow, :])
                    first = False
    return y, idx


def maxpool_bwd64(dy, idx, H, W, k, s, pad, add=None, window=None):
    """(dx, magnitude, terms): the fp64 gather dx[h, w] = sum of dy over the windows whose code points at (h, w), plus `add` inside
    window = (h0, w0, AH, AW); the sum of the magnitudes and the number of summed terms per element."""
    B, OH, OW, C = dy.shape
    dx, mag = np.zeros((B, H, W, C)), np.zeros((B, H, W, C))
    cnt = np.zeros((B, H, W, C), np.int64)
    d = dy.astype(np.float64)
    for oh in range(OH):
        for ow in range(OW):
            for kh in range(k):
                h = oh * s - pad + kh
                if not 0 <= h < H:
                    continue
                for kw in range(k):
                    w = ow * s - pad + kw
                    if not 0 <= w < W:
                        continue
                    hit = idx[:, oh, ow, :] == kh * k + kw
                    dx[:, h, w, :] += np.where(hit, d[:, oh, ow, :], 0.0)
                    mag[:, h, w, :] += np.where(hit, np.abs(d[:, oh, ow, :]), 0.0)
                    cnt[:, h, w, :] += hit
    if add is not None:
        h0, w0, AH, AW = window
        dx[:, h0:h0 + AH, w0:w0 + AW] += add.astype(np.float64)
        mag[:, h0:h0 + AH, w0:w0 + AW] += np.abs(add.astype(np.float64))
        cnt[:, h0:h0 + AH, w0:w0 + AW] += 1
    return dx, mag, cnt


def maxpool_bwd_bound(mag, cnt):
    """T summed terms take T - 1 additions whose partial sums the magnitudes bound (the first lands on an exact zero): (T - 1) u sum |term|.
    Non-overlapping 2 x 2 windows give T <= 1 without `add`: exact."""
    return np.maximum(cnt - 1, 0) * U * mag


# ---- global average pool --------------------------------------------------------------------------------------------------------------------
def gap_fwd_bound(x):
    """gap_fwd_kernel: row lane ty sums rows ty, ty + 16, ... in fp32 (R = ceil(HW / 16) additions at most), the 16 lane sums are added
    (15), the sum is multiplied (1) by a rounded 1 / HW (1): (R + 17) u mean |x|.  x: [B, HW, C]."""
    hw = x.shape[1]
    return (-(-hw // 16) + 17) * U * np.abs(x.astype(np.float64)).mean(1)


def gap_bwd_bound(dy, hw, dx0=None):
    """dy * (1 / HW): the rounded reciprocal and the product, 2u |dy| / HW.  accumulate: the addition to what dx held rounds once more,
    u |dy / HW + dx0| (three roundings on the path: where dx0 is small against dy / HW the result is off by up to 3u of itself)."""
    d = dy.astype(np.float64)[:, None, :] / hw
    b = 2 * U * np.abs(d)
    return b if dx0 is None else b + U * np.abs(d + dx0.astype(np.float64))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
# (H, W) -> (OH, OW): up- and down-sampling, extents of 1 along one axis only and along both, the identity, a strong down- and up-sampling
RESIZE_PAIRS = [((8, 8), (29, 29)), ((7, 5), (20, 11)), ((20, 20), (10, 30)), ((1, 1), (8, 8)), ((1, 6), (5, 6)), ((6, 1), (6, 9)),
                ((9, 9), (1, 1)), ((5, 7), (5, 7)), ((2, 2), (65, 3))]
RESIZE_PAIRS_BWD = RESIZE_PAIRS + [((64, 3), (3, 64))]


def wide(seed, *shape):
    """N(0,1) with per-channel scales spread over 2^-6 .. 2^6: a max-norm tolerance would hide the small channels."""
    r = np.random.RandomState(seed)
    return (r.standard_normal(shape) * np.exp2(np.linspace(-6.0, 6.0, shape[-1]))).astype(np.float32)


def pool_input(seed, B, H, W, C):
    """Post-ReLU values on a coarse grid (many ties, many zeros); channel 1 holds -0.0 / +0.0 only, channel 2 -inf only."""
    r = np.random.RandomState(seed)
    x = np.maximum(np.round(r.standard_normal((B, H, W, C)) * 2.0) / 2.0, 0.0).astype(np.float32)
    x[..., 1] = np.where(r.randint(0, 2, (B, H, W)) == 1, np.float32(-0.0), np.float32(0.0))
    x[..., 2] = -np.inf
    return x
