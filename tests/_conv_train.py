"""The dense convolution's training entries -- pylc_conv2d_dgrad, pylc_conv2d_dgrad_add, pylc_conv2d_fwd, pylc_conv2d_fwd_stats -- stated in
numpy float64 / float32 / float16 from include/pylc_hip.h (PylcConvDesc, "fp16 planes"), not from the kernels, with the comparison helpers
tests/test_conv_train_abi_gpu.py applies to what the GPU wrote and tests/test_cpu_conv_train_ref.py applies to corrupted copies of a perfect
output.  Not a test module.  Geometry, operands, plane placement and the element-wise comparisons are those of tests/_eval_conv.py.

What the kernel sees.  A plane operand (dy of the data gradient, x of the forward, the prepared filter) is built on the host
(tests/_planes.py); the values behind it are  t^ = join(h0, h1, s)  (precision mode 2, f16x3) resp. join(h0, None, s)  (mode 3, one plane).
For the fp32-tensor entries the operands are the fp32 values themselves.

Data gradient, in float64, in the SCATTER form of the definition (every output pixel of the forward hands its gradient to the input pixels
its taps read; no parity classes, no gather):
    dx[b, ho stride - pad + r dil, wo stride - pad + s dil, c] += sum_k dy^[b, ho, wo, k] w^[k, r, s, c]     for targets inside the image
    dxa = the same with absolute values: the scale every error is measured in
Epilogues:  fresh  v = dx;   accumulate  v = old + dx, mag = dxa + |old|;   add  v = dx + add_src;   masked add  v = dx + (bit ? add_src : 0),
mag = dxa + |what was added|.  The bit of (pixel m, channel c) is read from the 1-bit ReLU mask by the model tests/_bn.py unpack_relu_bits
states (mask_bits below is its numpy form; the CPU test pins the two against each other).
One-plane output (out_fmt = 1):  out_bound = bits(float(Kp R S) * dy_bound * w_amax), two fp32 multiplies in that order (no add: nothing to
contract), Kp = roundup4(Cout); for the forward  float(Cin R S) * x_bound * w_amax.  Decoded with scale_for(out_bound).

Forward statistics:  z = y - bias, the conv sum BEFORE the bias; per tile of pixel rows  sum z  and  sum z^2  in float64 (stats64).  The
linear-tile forms give row r the pixels [r bm, (r + 1) bm), bm in {128, 256} read off the returned row count (tile_height); the halo forms
(plh, plhn) return the patch count and the patch order is not documented, so only the COLUMN TOTALS over all rows are compared there.
Bounds, from quantities the project already uses (no new constant), summed over the pixels of the tile:
    sum       sum(TOL_C mag) + sum_bound(z)
    squares   sum(2 |z| TOL_C mag + (TOL_C mag)^2) + sum_bound(z^2)
(sum_bound: n 2^-24 sum|.| for an any-order fp32 sum of n terms; for the column totals n is the tile height 256, the rows themselves being
added here in float64.)

Tolerance.  TOL_C starts from the project's own figure for these kernels, 1e-6 * sum|a||b| (tests/_eval_conv.py TOL, test_fullsize_ops_gpu.py,
test_ops_gpu.py test_conv_precision_modes), plus 2^-23 for the one extra rounding of an accumulate / add epilogue, measured against mag.  It
was to be halved while the worst measured ratio over all cases stayed below 0.25 (a slack of 4 x or more).  Measured on an MI355X
(profiles/conv_train_abi.txt): worst 0.403 on fp32 tensors (pylc_conv2d_dgrad, fp32 MFMA, the stride-2 3x3 with Cin 76), 0.291 on plane
operands (pylc_conv2d_fwd, plp, mode 2) -- a slack of 2.5 x, so the final value is the starting one, TOL_C = 1e-6 + 2^-23 = 1.119e-6."""
import numpy as np

from tests import _eval_conv as E
from tests import _planes as P

F64, F32, F16 = np.float64, np.float32, np.float16
GUARD = E.GUARD
TOL_C = 1e-6 + 2.0 ** -23                  # final = starting figure: the measured worst ratio is 0.403 (module docstring)
Geom = E.Geom


def roundup4(v):
    return (v + 3) & ~3


# ---- data -----------------------------------------------------------------------------------------------------------------------------------
def make_train_data(g, seed):
    """dy [B][OH][OW][Cout] by the recipe of _eval_conv.make_data's x (N(0,1) 2^U(-12,0)), w [Cout][k k][Cin] ~ N(0, 2 / (Cin k^2)), old and
    add_src [B H W][Cin] ~ N(0,1), the mask bytes of B H W x Cin bits, each set with probability 0.55; fp32, fixed seeds."""
    r = np.random.RandomState(seed)
    shape = (g.b, g.oh, g.ow, g.cout)
    dy = (r.standard_normal(shape) * 2.0 ** r.uniform(-12.0, 0.0, shape)).astype(F32)
    w = (r.standard_normal((g.cout, g.k * g.k, g.cin)) * np.sqrt(2.0 / g.klen)).astype(F32)
    mi = g.b * g.h * g.w
    old = r.standard_normal((mi, g.cin)).astype(F32)
    add = r.standard_normal((mi, g.cin)).astype(F32)
    mask = pack_mask(r.random_sample((mi, g.cin)) < 0.55) if g.cin % 8 == 0 else None
    return dict(dy=dy, w=w, old=old, add=add, mask=mask)


def w_crsk(w):
    """The fp32 transposed filter [Cin][R S][Kp] of w [Cout][R S][Cin] (pylc_weight_transpose), Kp = roundup4(Cout), zero pad columns."""
    k, rs, c = w.shape
    out = np.zeros((c, rs, roundup4(k)), dtype=F32)
    out[:, :, :k] = np.asarray(w, dtype=F32).transpose(2, 1, 0)
    return out


# ---- the 1-bit mask ---------------------------------------------------------------------------------------------------------------------------
def mask_bits(mask_bytes, m, c):
    """bool [m][c] of the mask bytes: byte (row C/4 + q) / 2 holds the nibbles of the channel quads q (even: low nibble, odd: high nibble),
    bit k of a nibble is channel 4 q + k."""
    assert c % 8 == 0
    b = np.asarray(mask_bytes, dtype=np.uint8).reshape(m, c // 8).astype(np.int32)
    nib = np.stack((b & 15, b >> 4), axis=2).reshape(m, c // 4)
    return (np.stack([(nib >> k) & 1 for k in range(4)], axis=2).reshape(m, c)) != 0


def pack_mask(bits):
    """The inverse of mask_bits: uint8 [m c / 8]."""
    m, c = bits.shape
    assert c % 8 == 0
    nib = (bits.reshape(m, c // 4, 4).astype(np.int32) << np.arange(4)).sum(2)
    pair = nib.reshape(m, c // 8, 2)
    return (pair[:, :, 0] | (pair[:, :, 1] << 4)).astype(np.uint8).ravel()


# ---- the data gradient --------------------------------------------------------------------------------------------------------------------------
def _tap_range(k_idx, g, size, osize):
    """Forward output positions o in [lo, hi) whose tap k_idx reads an input position o stride - pad + k_idx dil inside [0, size), and the
    first such input position."""
    lo = max(0, -((k_idx * g.dil - g.pad) // g.stride))
    hi = min(osize, (size - 1 + g.pad - k_idx * g.dil) // g.stride + 1)
    return lo, hi, lo * g.stride - g.pad + k_idx * g.dil


def dgrad64(dy_seen, w_seen, g):
    """(dx, dxa) [B H W][Cin] float64 of dy [B][OH][OW][Cout] (or [B OH OW][Cout]) and w [Cout][k k][Cin]: every tap scatters the gradient of
    the forward's output pixels onto the input pixels it read."""
    dy = np.asarray(dy_seen, dtype=F64).reshape(g.b, g.oh, g.ow, g.cout)
    w = np.asarray(w_seen, dtype=F64)
    dya, wa = np.abs(dy), np.abs(w)
    dx = np.zeros((g.b, g.h, g.w, g.cin), dtype=F64)
    dxa = np.zeros_like(dx)
    for r in range(g.k):
        lo, hi, i0 = _tap_range(r, g, g.h, g.oh)
        if hi <= lo:
            continue
        for s in range(g.k):
            lo2, hi2, j0 = _tap_range(s, g, g.w, g.ow)
            if hi2 <= lo2:
                continue
            to = (slice(None), slice(i0, i0 + (hi - lo - 1) * g.stride + 1, g.stride), slice(j0, j0 + (hi2 - lo2 - 1) * g.stride + 1, g.stride))
            n = g.b * (hi - lo) * (hi2 - lo2)
            shape = (g.b, hi - lo, hi2 - lo2, g.cin)
            dx[to] += (dy[:, lo:hi, lo2:hi2].reshape(n, g.cout) @ w[:, r * g.k + s, :]).reshape(shape)
            dxa[to] += (dya[:, lo:hi, lo2:hi2].reshape(n, g.cout) @ wa[:, r * g.k + s, :]).reshape(shape)
    return dx.reshape(-1, g.cin), dxa.reshape(-1, g.cin)


def reached(g):
    """bool [B H W]: the input pixels at least one tap of one output pixel reads.  The others -- whole parity classes of a stride-2 1x1 or of an
    even dilation -- have the data gradient 0 by definition, whatever dy holds."""
    one = Geom(1, 1, g.k, g.stride, g.pad, g.dil, g.b, g.h, g.w)
    return dgrad64(np.ones((g.b, g.oh, g.ow, 1)), np.ones((1, g.k * g.k, 1)), one)[1].ravel() > 0


def dgrad_epilogue64(dx, dxa, old=None, add=None, mask=None):
    """(v, mag) float64: old != None is accumulate = 1; add (with the optional mask BYTES) is pylc_conv2d_dgrad_add's add_src / add_mask."""
    assert old is None or add is None
    if old is not None:
        o = np.asarray(old, dtype=F64)
        return o + dx, dxa + np.abs(o)
    if add is not None:
        a = np.asarray(add, dtype=F64)
        if mask is not None:
            a = np.where(mask_bits(mask, *a.shape), a, 0.0)
        return dx + a, dxa + np.abs(a)
    assert mask is None
    return dx, dxa


def product_bound(klen, a_bits, b_bits):
    """{bits} of float(klen) * a * b: two fp32 multiplies in that order."""
    return {P.bits_of(F32(F32(F32(float(klen)) * P.float_of(a_bits)) * P.float_of(b_bits)))}


def check_classes(y, old_f32, g, accumulate, what):
    """The input pixels no tap reaches, in the fp32 dx [B H W][Cin] as read back: exact zeros when accumulate = 0, `old` bit for bit when 1."""
    dead = ~reached(g)
    got = np.ascontiguousarray(y[dead]).view(np.uint32)
    if accumulate:
        want = np.ascontiguousarray(np.asarray(old_f32, dtype=F32)[dead]).view(np.uint32)
        bad = got != want
        msg = 'does not hold the old value bit for bit'
    else:
        bad = (got << 1) != 0
        msg = 'is not zero'
    if bad.any():
        i = E._first(bad)
        raise AssertionError('%s: pixel %d channel %d, which no tap reaches, %s: %#010x (%d of %d)' %
                             (what, int(np.nonzero(dead)[0][i[0]]), i[1], msg, int(got[i]), int(bad.sum()), bad.size))
    return int(dead.sum())


# ---- forward statistics ---------------------------------------------------------------------------------------------------------------------------
def tile_height(m, rows):
    """bm in {128, 256} with ceil(M / bm) == rows."""
    fit = [bm for bm in (128, 256) if -(-m // bm) == rows]
    assert fit, 'stats_rows %d is neither ceil(%d / 128) nor ceil(%d / 256)' % (rows, m, m)
    return fit[0]


def linear_tiles(m, bm):
    return [slice(r * bm, min((r + 1) * bm, m)) for r in range(-(-m // bm))]


def stats64(z, rows_of_tile):
    """(sum z, sum z^2) float64 [tiles][C]; rows_of_tile: one slice / index array of pixel rows per tile."""
    z = np.asarray(z, dtype=F64)
    return (np.stack([z[t].sum(0) for t in rows_of_tile]), np.stack([(z[t] ** 2).sum(0) for t in rows_of_tile]))


def stats_bounds(z, mag, rows_of_tile, n_terms=None, tol=None):
    """The module docstring's bounds, [tiles][C] each; n_terms: the length of the fp32 sum when it is not the tile's row count."""
    tol = TOL_C if tol is None else tol
    z, e = np.asarray(z, dtype=F64), tol * np.asarray(mag, dtype=F64)
    bs, bq = [], []
    for t in rows_of_tile:
        zt, et = z[t], e[t]
        k = 1.0 if n_terms is None else n_terms / float(zt.shape[0])      # P.sum_bound counts the rows it is given
        bs.append(et.sum(0) + k * P.sum_bound(zt))
        bq.append((2.0 * np.abs(zt) * et + et ** 2).sum(0) + k * P.sum_bound(zt ** 2))
    return np.stack(bs), np.stack(bq)


def check_stats(buf, floats, rows, c, z, mag, what, halo=False, tol=None, guard=GUARD):
    """The statistics buffer [guard | `floats` floats | guard], NaN-filled before the call, laid out [rows][2][roundup4(C)]: rows [0, rows)
    finite and within the bounds of sum z / sum z^2 per tile (halo: the column totals over all rows, against one tile holding every pixel),
    every float past them and both guards still NaN.  Returns the worst error / bound."""
    buf = np.asarray(buf, dtype=F32)
    c4 = roundup4(c)
    m = z.shape[0]
    assert buf.size == floats + 2 * guard and 0 < rows and rows * 2 * c4 <= floats, '%s: %d rows of 2 x %d do not fit %d floats' % (what, rows, c4, floats)
    assert np.isnan(buf[:guard]).all() and np.isnan(buf[guard + floats:]).all(), '%s: a guard around the statistics was written' % what
    body = buf[guard:guard + floats]
    past = body[rows * 2 * c4:]
    if not np.isnan(past).all():
        i = int(np.nonzero(~np.isnan(past))[0][0]) + rows * 2 * c4
        raise AssertionError('%s: float %d of the statistics (row %d) lies past the %d rows reported and was written' % (what, i, i // (2 * c4), rows))
    got = body[:rows * 2 * c4].reshape(rows, 2, c4)[:, :, :c].astype(F64)
    if not np.isfinite(got).all():
        i = E._first(~np.isfinite(got))
        raise AssertionError('%s: statistics row %d (%s) channel %d was not written' % (what, i[0], ('sum', 'squares')[i[1]], i[2]))
    if halo:
        tiles = [slice(0, m)]
        got = got.sum(0, keepdims=True)
        bs, bq = stats_bounds(z, mag, tiles, n_terms=256, tol=tol)
    else:
        tiles = linear_tiles(m, tile_height(m, rows))
        bs, bq = stats_bounds(z, mag, tiles, tol=tol)
    ws, wq = stats64(z, tiles)
    worst = 0.0
    for name, g_, w_, b_ in (('sum', got[:, 0], ws, bs), ('sum of squares', got[:, 1], wq, bq)):
        err = np.abs(g_ - w_)
        bad = ~(err <= b_)
        if bad.any():
            i = E._first(bad)
            raise AssertionError('%s: %s of statistics row %d channel %d is off by %.6g, allowed %.6g (%d of %d fail)' %
                                 (what, name, i[0], i[1], err[i], b_[i], int(bad.sum()), bad.size))
        live = b_ > 0
        if live.any():
            worst = max(worst, float((err[live] / b_[live]).max()))
    return worst


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
# Geometry (Cin, Cout, k, stride, pad, dil, B, H, W).  For a data gradient the GEMM has rows M = B H W, columns N = Cin and the reduction
# Kp = roundup4(Cout) per tap.  The forms were derived for 256 compute units; each is asserted through pylc_debug_last_conv_form after the call
# (stride 2: the form of the last parity class launched).  If a shape stops reaching its form, the shape changes, never the assertion.
#   plhn  3x3 / unit steps, patches * 2048 <= M * 9 and patches * ceil(N / 64) >= 512 (patches = B ceil(H/16) ceil(W/16))
#   plh   the same geometry with N > 64, below plhn's count and patches * ceil(N / 128) >= 128
#   pl256 one tap, ceil(K / 32) >= 24 K-steps and ceil(M / 256) * ceil(N / 128) >= 256 tiles
#   plp   one tap, no padding, M % 128 == 0, N % 128 == 0, more than 512 tiles of 128 rows, at least two K-steps; fp32 output, no bias
#   everything else takes 128-row tiles, in the narrow wave layout when N <= 64
DGRAD_CASES = [
    ('plhn', (64, 16, 3, 1, 1, 1, 2, 256, 256), '512 patches x 1 column tile >= 512'),
    ('plhn', (64, 64, 3, 1, 0, 1, 2, 252, 252), 'valid conv: dx is 252^2, ragged patches; 512 * 2048 <= 127008 * 9; border pixels read dy rows outside the map'),
    ('plhn', (136, 32, 3, 1, 1, 1, 1, 256, 256), '256 patches x 3 column tiles = 768; the last tile has 8 channels'),
    ('plh', (72, 32, 3, 1, 1, 1, 1, 184, 184), '144 patches: x 2 = 288 < 512, x 1 >= 128; 144 * 2048 <= 33856 * 9'),
    ('pl256', (256, 768, 1, 1, 0, 1, 2, 128, 128), '24 K-steps, 128 * 2 = 256 tiles'),
    ('plp', (256, 72, 1, 1, 0, 1, 1, 257, 128), 'M = 32896 = 257 * 128: 257 * 2 = 514 tiles > 512; 3 K-steps (2 in mode 3); Kp % 32 != 0: separate planes'),
    ('plp', (128, 128, 1, 1, 0, 1, 1, 513, 128), '513 tiles; chunk-interleaved dy and w_planes_t'),
    ('pl128', (200, 40, 1, 1, 0, 1, 2, 33, 31), 'ragged M and N'),
    ('pl128', (128, 32, 3, 1, 6, 6, 1, 16, 16), 'dilation 6: tap skipping'),
    ('pl128', (128, 32, 3, 1, 18, 18, 1, 16, 16), 'dilation 18: only the centre tap is ever valid'),
    ('pl128', (72, 32, 3, 2, 1, 1, 2, 45, 44), 'stride 2, all four classes live, odd and even size'),
    ('pl128', (128, 64, 1, 2, 0, 1, 2, 17, 16), 'stride-2 1x1 shortcut: three empty classes'),
    ('pl128', (72, 32, 3, 2, 2, 2, 1, 21, 20), 'stride 2, even dilation: classes all-or-none'),
    ('pl128-narrow', (16, 24, 1, 1, 0, 1, 1, 40, 36), '1x1, M = 1440'),
    ('pl128-narrow', (64, 64, 3, 1, 1, 1, 1, 20, 24), 'multi-tap 3x3 on 4 patches: too few for the halo kernels'),
]
# pylc_conv2d_dgrad on fp32 tensors (dy_fmt = 0): (form, modes, geometry, dy pitch, note)
DGRAD32_CASES = [
    ('igemm', (0, 1, 2), (64, 9, 1, 1, 0, 1, 2, 12, 12), 12, '9-class head: dy channels 9 .. 11 zero, as the forward writes them'),
    ('igemm', (0, 1, 2), (4, 64, 7, 2, 3, 1, 2, 40, 40), 64, 'the thin-input stem, stride 2'),
    ('igemm', (0, 1, 2), (76, 32, 3, 2, 1, 1, 1, 19, 19), 32, 'stride 2, odd size'),
    ('pp', (2,), (128, 32, 3, 1, 1, 1, 3, 128, 128), 32, '192 tiles of 256 x 128; once with w_planes_t, once with the fp32 transposed filter alone'),
]
# pylc_conv2d_fwd / pylc_conv2d_fwd_stats on plane x: (form, modes, geometry, statistics, bias, out_fmt, note)
FWD_CASES = [
    ('plp', (2, 3), (72, 128, 1, 1, 0, 1, 1, 513, 128), True, False, 0, 'persistent kernel, epilogue kind 1'),
    ('plp', (2, 3), (72, 128, 1, 1, 0, 1, 1, 513, 128), False, False, 0, 'persistent kernel, epilogue kind 0'),
    ('plhn', (2, 3), (32, 136, 3, 1, 1, 1, 1, 256, 256), True, False, 0, 'patch statistics: column totals'),
    ('pl128', (2, 3), (40, 200, 1, 1, 0, 1, 2, 33, 31), True, False, 0, 'ragged both ways'),
    ('pl128', (2, 3), (40, 200, 1, 1, 0, 1, 2, 33, 31), True, True, 0, 'statistics before the bias: a bias of 50 x the spread'),
    ('pl128-narrow', (2, 3), (64, 64, 3, 1, 0, 1, 1, 20, 20), False, True, 0, 'the U-Net valid conv'),
    ('pl256', (2, 3), (768, 256, 1, 1, 0, 1, 2, 128, 128), True, False, 0, '24 K-steps, 256 tiles'),
    ('pl128', (3,), (32, 72, 3, 2, 1, 1, 2, 45, 45), False, False, 1, 'one-plane output'),
]
CASES = ([('pylc_conv2d_dgrad_add', f, geo, note) for f, geo, note in DGRAD_CASES] +
         [('pylc_conv2d_dgrad', f, geo, note) for f, _, geo, _, note in DGRAD32_CASES] +
         [('pylc_conv2d_fwd_stats' if st else 'pylc_conv2d_fwd', f, geo, note) for f, _, geo, st, _, _, note in FWD_CASES])
FULL_PRODUCT_MAX_M = 8192                  # data-gradient cases up to this many dx pixels take every epilogue option


def big_bias(z, cout, seed):
    """A bias of 50 x the spread of the conv sums."""
    r = np.random.RandomState(seed)
    return (50.0 * float(np.asarray(z).std()) * (1.0 + 0.1 * r.standard_normal(cout))).astype(F32)
