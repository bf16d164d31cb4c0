"""The fused inference convolution -- pylc_conv2d_fwd_bnact_ex and its fp32-tensor sibling pylc_conv2d_fwd_bnact: conv + eval BatchNorm +
residual + ReLU on fp16-plane tensors -- stated in numpy float64 / float32 / float16 from include/pylc_hip.h (PylcConvDesc, PylcFwdEp,
"fp16 planes"), not from the kernels, with the comparison helpers tests/test_eval_conv_abi_gpu.py applies to what the GPU wrote and
tests/test_cpu_eval_conv_ref.py applies to corrupted copies of a perfect output.  Not a test module.

What the kernel sees.  Every operand is built on the host as planes (tests/_planes.py): x split under the bound the case chooses, the filter
through filter_planes, a plane residual like x.  The values behind them are  x^ = join(h0, h1, s)  (precision mode 2, f16x3) resp.
join(h0, None, s)  (mode 3, one plane), and w^, r^ alike; for the fp32-tensor entry the operands are the fp32 values themselves.

Reference, all in float64, per output element (pixel m, channel n):
    z = sum x^ w^            v = (z + bias) scale + shift + r^            y = max(v, 0) if relu
    mag = |scale| (sum |x^| |w^| + |bias|) + |shift| + |r^|               the scale every error is measured in
A kernel that forms the products exactly and accumulates in fp32 in any order stays within  tol * mag,  tol = TOL below.

Output bound (plane outputs), in fp32 in the header's order:
    b = float(Cin R S) * x_true * w_amax;      b = b * scale_amax + shift_amax;      b += res_amax   (with a residual)
x_true = *x_true_amax, or *d->x_amax when that pointer is NULL.  A compiler may contract the second line into one fused multiply-add:
bound_candidates returns both bit patterns.  The output is scaled with scale_for(bits(b)).

Placement of a plane output: dense [M][Cout] halves; two planes chunk-interleaved iff planes_stride says 32 (plane 1 at + 32 inside each
64-half line), else plane 1 at + M Cout; one plane: plane 0 alone."""
from fractions import Fraction

import numpy as np

from tests import _planes as P

F64, F32, F16 = np.float64, np.float32, np.float16
GUARD = 64                                  # sentinel elements in front of and behind every device buffer
# the project's own figure for these kernels, 1e-6 * sum|a||b| (tests/test_fullsize_ops_gpu.py tol_fwd, test_ops_gpu.py
# test_conv_precision_modes), plus 2^-22 for the four roundings of the epilogue (bias add, scale multiply, shift add, residual add)
TOL = 1e-6 + 2.0 ** -22


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------
class Geom:
    """(Cin, Cout, k, stride, pad, dil, B, H, W) with the derived output size."""

    def __init__(self, cin, cout, k, stride, pad, dil, b, h, w):
        self.cin, self.cout, self.k, self.stride, self.pad, self.dil, self.b, self.h, self.w = cin, cout, k, stride, pad, dil, b, h, w
        self.oh = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1
        self.ow = (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
        self.m = b * self.oh * self.ow
        self.klen = cin * k * k

    def __repr__(self):
        return '(%d,%d,%dx%d s%d p%d d%d, B%d %dx%d)' % (self.cin, self.cout, self.k, self.k, self.stride, self.pad, self.dil, self.b, self.h, self.w)


def planes_stride(m, c, nplanes):
    """include/pylc_hip.h pylc_planes_stride: 32 (chunk-interleaved) iff two planes, C % 32 == 0 and 4 M C < 2^31; else M * C."""
    return 32 if nplanes == 2 and c % 32 == 0 and 4 * m * c < 2 ** 31 else m * c


# ---- data -----------------------------------------------------------------------------------------------------------------------------------
def make_data(g, seed):
    """x [B][H][W][Cin] ~ N(0,1) 2^U(-12,0), w [Cout][k k][Cin] ~ N(0, 2 / (Cin k^2)), scale = 1 + 0.3 N, shift = 0.2 N, bias = 0.5 N,
    residual [M][Cout] ~ N(0,1); fp32, fixed seeds."""
    r = np.random.RandomState(seed)
    x = (r.standard_normal((g.b, g.h, g.w, g.cin)) * 2.0 ** r.uniform(-12.0, 0.0, (g.b, g.h, g.w, g.cin))).astype(F32)
    w = (r.standard_normal((g.cout, g.k * g.k, g.cin)) * np.sqrt(2.0 / g.klen)).astype(F32)
    scale = (1.0 + 0.3 * r.standard_normal(g.cout)).astype(F32)
    shift = (0.2 * r.standard_normal(g.cout)).astype(F32)
    bias = (0.5 * r.standard_normal(g.cout)).astype(F32)
    res = r.standard_normal((g.m, g.cout)).astype(F32)
    return dict(x=x, w=w, scale=scale, shift=shift, bias=bias, res=res)


class Operand:
    """A tensor as the planes the kernel reads: pieces h0 / h1 under scale_for(bound bits), and the float64 values behind them."""

    def __init__(self, t, bound_bits, nplanes):
        self.bits, self.nplanes = int(bound_bits), nplanes
        self.s = P.scale_for(self.bits)
        self.h0, self.h1 = P.split(t, self.s)
        self.seen = P.join(self.h0, self.h1 if nplanes == 2 else None, self.s).astype(F64)


def amax_bits(t):
    return P.bits_of(np.abs(np.asarray(t, dtype=F32)).max())


def times_pow2(bits, mult):
    """bits of `mult` (a power of two) times the float behind `bits`."""
    return P.bits_of(F32(P.float_of(bits) * F32(mult)))


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def conv64(xs, ws, g):
    """(z, za) [M][Cout] float64: sum x w and sum |x| |w| of xs [B][H][W][Cin], ws [Cout][k k][Cin], one tap at a time (zero padding: a tap
    outside the image contributes nothing)."""
    xs, ws = np.asarray(xs, dtype=F64), np.asarray(ws, dtype=F64)
    xa, wa = np.abs(xs), np.abs(ws)
    z = np.zeros((g.b, g.oh, g.ow, g.cout), dtype=F64)
    za = np.zeros_like(z)
    for r in range(g.k):
        # output rows whose input row o * stride - pad + r * dil lies inside the image
        lo = max(0, -((r * g.dil - g.pad) // g.stride))
        hi = min(g.oh, (g.h - 1 + g.pad - r * g.dil) // g.stride + 1)
        if hi <= lo:
            continue
        i0 = lo * g.stride - g.pad + r * g.dil
        for s in range(g.k):
            lo2 = max(0, -((s * g.dil - g.pad) // g.stride))
            hi2 = min(g.ow, (g.w - 1 + g.pad - s * g.dil) // g.stride + 1)
            if hi2 <= lo2:
                continue
            j0 = lo2 * g.stride - g.pad + s * g.dil
            sl = (slice(None), slice(i0, i0 + (hi - lo - 1) * g.stride + 1, g.stride), slice(j0, j0 + (hi2 - lo2 - 1) * g.stride + 1, g.stride))
            n = g.b * (hi - lo) * (hi2 - lo2)
            z[:, lo:hi, lo2:hi2] += (xs[sl].reshape(n, g.cin) @ ws[:, r * g.k + s, :].T).reshape(g.b, hi - lo, hi2 - lo2, g.cout)
            za[:, lo:hi, lo2:hi2] += (xa[sl].reshape(n, g.cin) @ wa[:, r * g.k + s, :].T).reshape(g.b, hi - lo, hi2 - lo2, g.cout)
    return z.reshape(g.m, g.cout), za.reshape(g.m, g.cout)


def epilogue64(z, za, scale, shift, bias=None, res=None, relu=False):
    """(y, mag) float64 of the module docstring from the conv sums; bias / res None = absent."""
    scale, shift = np.asarray(scale, dtype=F64), np.asarray(shift, dtype=F64)
    b = np.zeros_like(scale) if bias is None else np.asarray(bias, dtype=F64)
    r = 0.0 if res is None else np.asarray(res, dtype=F64)
    v = (z + b) * scale + shift + r
    mag = np.abs(scale) * (za + np.abs(b)) + np.abs(shift) + np.abs(r)
    return (np.maximum(v, 0.0) if relu else v), mag


# ---- the output bound -------------------------------------------------------------------------------------------------------------------------
def _rn32(q):
    """The fp32 nearest (ties to even) to the exact rational q > 0 inside the normal range."""
    q = Fraction(q)
    assert q > 0
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    n = round(q / Fraction(2) ** (e - 23))              # Fraction.__round__: half to even
    v = float(n) * 2.0 ** (e - 23)
    assert -126 <= e <= 126 and float(F32(v)) == v
    return F32(v)


def bound_candidates(klen, x_true_bits, w_bits, scale_bits, shift_bits, res_bits=None):
    """The set of fp32 bit patterns the output bound may have: the affine step as two roundings, or contracted into one."""
    xt, wa, sa, sh = (P.float_of(b) for b in (x_true_bits, w_bits, scale_bits, shift_bits))
    b = F32(F32(F32(float(klen)) * xt) * wa)
    two = F32(F32(b * sa) + sh)
    one = _rn32(Fraction(float(b)) * Fraction(float(sa)) + Fraction(float(sh)))
    out = set()
    for v in (two, one):
        if res_bits is not None:
            v = F32(v + P.float_of(res_bits))
        out.add(P.bits_of(v))
    return out


# ---- plane outputs ------------------------------------------------------------------------------------------------------------------------------
def plane_halves(m, c, nplanes):
    """Halves a dense plane tensor occupies."""
    return nplanes * m * c


def plane_index(m, c, nplanes):
    """(addresses of plane 0, addresses of plane 1 or None) of the flat elements 0 .. M C - 1, in halves from the tensor's start."""
    stride = planes_stride(m, c, nplanes)
    at = P.phys(np.arange(m * c, dtype=np.int64), nplanes == 2 and stride == 32)
    return at, (at + stride if nplanes == 2 else None)


def encode_planes(t, s, nplanes, out=None, base=0):
    """The uint16 image of t [M][C] (fp32) as a plane tensor under the scale s, written into out[base ..] (default: a fresh buffer)."""
    m, c = t.shape
    h0, h1 = P.split(t, s)
    if out is None:
        out = np.zeros(plane_halves(m, c, nplanes), dtype=np.uint16)
    stride = planes_stride(m, c, nplanes)
    return P.place(h0, h1 if nplanes == 2 else None, nplanes == 2 and stride == 32, out=out, base=base, stride=stride)


def decode_planes(buf, m, c, nplanes, s, base=0):
    """(h0, h1 or None, fp32 values [M][C]) read from a uint16 buffer at the model's placement."""
    a0, a1 = plane_index(m, c, nplanes)
    h0 = buf[base + a0].view(F16).reshape(m, c)
    h1 = buf[base + a1].view(F16).reshape(m, c) if nplanes == 2 else None
    with np.errstate(invalid='ignore'):
        return h0, h1, P.join(h0, h1, s)


# ---- comparison helpers: each raises AssertionError with the first offender, or returns the worst error / (tol * mag) ----------------------------
def _first(bad):
    return tuple(int(k[0]) for k in np.nonzero(bad))


def _ratio(err, allow, mag, tol, what):
    bad = ~(err <= allow)                                # NaN counts as a failure
    if bad.any():
        i = _first(bad)
        raise AssertionError('%s: element %s is off by %.6g, allowed %.6g (%d of %d elements fail)' % (what, i, err[i], allow[i], int(bad.sum()), bad.size))
    live = mag > 0
    return float((err[live] / (tol * mag[live])).max()) if live.any() else 0.0


def check_f32(buf, m, c, pitch, c0, y64, mag, what, tol=TOL, guard=GUARD):
    """An fp32 output inside its NaN-filled buffer [guard | M x pitch | guard], channels [c0, c0 + C) of every row: every element within
    tol * mag of y64; channels [C, roundup4(C)) exact zeros where the pitch holds them; every other float still NaN.  Returns
    (worst error / (tol mag), the output as [M][C] fp32)."""
    buf = np.asarray(buf, dtype=F32)
    assert buf.size == m * pitch + 2 * guard
    body = buf[guard:guard + m * pitch].reshape(m, pitch)
    c4 = min((c + 3) & ~3, pitch - c0)
    assert np.isnan(buf[:guard]).all() and np.isnan(buf[guard + m * pitch:]).all(), '%s: a guard around the fp32 output was written' % what
    assert np.isnan(body[:, :c0]).all() and np.isnan(body[:, c0 + c4:]).all(), '%s: a channel outside the output slice was written' % what
    pad = body[:, c0 + c:c0 + c4]
    assert pad.size == 0 or (pad.view(np.uint32) << 1 == 0).all(), '%s: a padding channel [C, roundup4(C)) is not zero' % what
    y = body[:, c0:c0 + c]
    err = np.abs(y.astype(F64) - y64)
    return _ratio(err, tol * mag, mag, tol, what), y


def check_planes(buf, m, c, nplanes, out_bits, y64, mag, what, tol=TOL, same_as=None, guard=GUARD):
    """A plane output inside its 0x7e00-filled buffer [guard | 2 M C halves | guard] (a one-plane tensor uses the first M C halves: where a
    second plane would be must stay filled): decoded at the model's placement with scale_for(out_bits), every element within
    tol * mag + round_trip_bound(y64) of y64; every half that is no element still filled.  same_as: the [M][C] fp32 output of the same call
    with an fp32 result -- the plane bytes must be its split under the same scale (through canon).  Returns the worst
    (error - round-trip bound) / (tol mag), at least 0."""
    buf = np.asarray(buf, dtype=np.uint16)
    assert buf.size == 2 * m * c + 2 * guard
    s = P.scale_for(out_bits)
    used = np.zeros(buf.size, dtype=bool)
    a0, a1 = plane_index(m, c, nplanes)
    used[guard + a0] = True
    if a1 is not None:
        used[guard + a1] = True
    if not (buf[~used] == P.FILL16).all():
        i = int(np.nonzero(~used & (buf != P.FILL16))[0][0])
        raise AssertionError('%s: half %d (buffer of %d, output at %d .. %d) is no element of the output and was written: %#06x' %
                             (what, i, buf.size, guard, guard + plane_halves(m, c, nplanes), buf[i]))
    h0, h1, y = decode_planes(buf, m, c, nplanes, s, base=guard)
    err = np.abs(y.astype(F64) - y64)
    rt = P.round_trip_bound(y64, s, nplanes)
    _ratio(err, tol * mag + rt, mag, tol, what)
    worst = float(np.maximum((err - rt) / np.where(mag > 0, tol * mag, 1.0), 0.0).max())
    if same_as is not None:
        w0, w1 = P.split(same_as, s)
        for name, got, want in (('plane 0', h0, w0), ('plane 1', h1, w1))[:nplanes]:
            gu, wu = P.canon(got.view(np.uint16)), P.canon(want.view(np.uint16))
            if not np.array_equal(gu, wu):
                i = _first(gu != wu)
                raise AssertionError('%s: %s of element %s is %#06x, the split of the fp32 run gives %#06x (%d differ)' % (what, name, i, gu[i], wu[i], int((gu != wu).sum())))
    return worst


def check_bound(out_bits, candidates, true_max, what):
    """The returned scale bound: one of the model's bit patterns, and a bound."""
    assert int(out_bits) in candidates, '%s: out_bound %#010x is none of the model\'s %s' % (what, int(out_bits), ', '.join('%#010x' % b for b in sorted(candidates)))
    assert float(P.float_of(int(out_bits))) >= float(true_max), '%s: out_bound %.6g is below the true maximum %.6g' % (what, P.float_of(int(out_bits)), true_max)


def check_amax(amax_bits_got, y_f32_run, what):
    """amax_out after a run from 0: exactly the bits of max|y| of the fp32-output run of the same call."""
    want = amax_bits(y_f32_run)
    assert int(amax_bits_got) == want, '%s: amax_out %#010x (%.8g), max|y| of the fp32 run is %#010x (%.8g)' % (
        what, int(amax_bits_got), P.float_of(int(amax_bits_got)), want, P.float_of(want))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
# (form the case must reach -- asserted through pylc_debug_last_conv_form, not restated from the dispatcher --, geometry, with a bias in
# the four-combination set, note).  The smallest shapes that reach each form on the 256 compute units the dispatch counts with; the
# arithmetic that got them there:
#   plhn  needs 3x3 / unit steps, patches * 256 * 8 <= M * 9 and patches * ceil(Cout / 64) >= 512 (patches = B ceil(OH/16) ceil(OW/16))
#   plh   the same geometry with Cout > 64, below plhn's count and patches * ceil(Cout / 128) >= 128
#   pl256 needs one tap, ceil(Cin / 32) >= 24 K-steps and ceil(M / 256) * ceil(Cout / 128) >= 256 tiles
#   everything else takes 128-row tiles, in the narrow wave layout when Cout <= 64
EX_CASES = [
    ('plhn', (8, 64, 3, 1, 1, 1, 2, 256, 256), False, 'narrow: 2 * 16 * 16 = 512 patches of 16^2; Cin shorter than one K-step'),
    ('plhn', (64, 64, 3, 1, 0, 1, 2, 252, 252), True, 'narrow, ragged patches: P = Q = 250 (the U-Net valid conv), 512 * 2048 <= 125000 * 9'),
    ('plhn', (32, 136, 3, 1, 1, 1, 1, 256, 256), False, 'column tiles: 256 patches * 3 tiles = 768, the last tile with 8 channels'),
    ('plh', (32, 72, 3, 1, 1, 1, 1, 184, 184), False, '12 * 12 = 144 patches: * 2 column tiles of 64 = 288 < 512, * 1 of 128 >= 128; 144 * 2048 <= 33856 * 9'),
    ('pl128-narrow', (24, 16, 1, 1, 0, 1, 1, 40, 36), False, '1x1, M = 1440'),
    ('pl128-narrow', (64, 64, 3, 1, 1, 1, 1, 20, 24), False, 'multi-tap 3x3 on 4 patches: too few for the halo kernels'),
    ('pl128', (40, 200, 1, 1, 0, 1, 2, 33, 31), False, 'M = 2046, ragged N'),
    ('pl128', (32, 72, 3, 2, 1, 1, 2, 45, 45), False, 'stride 2: 23 x 23 outputs'),
    ('pl128', (32, 128, 3, 1, 6, 6, 1, 16, 16), False, 'dilation 6: tap skipping'),
    ('pl128', (32, 128, 3, 1, 18, 18, 1, 16, 16), False, 'dilation 18 on 16^2: only the centre tap is ever valid'),
    ('pl256', (768, 256, 1, 1, 0, 1, 2, 128, 128), False, 'exactly 128 * 2 = 256 tiles, 24 K-steps'),
    ('pl256', (776, 264, 1, 1, 0, 1, 2, 130, 127), False, 'ragged M (33020) and N; Cin % 32 = 8: separate planes'),
]
FULL_PRODUCT_MAX_M = 8192                  # cases up to this many output pixels take every combination of the epilogue options
# pylc_conv2d_fwd_bnact (fp32 tensors): (geometry, y pitch, with bias, note)
F32_CASES = [
    ((64, 12, 1, 1, 0, 1, 2, 12, 12), 12, True, 'head-like 1x1 into a 12-float pitch'),
    ((64, 9, 1, 1, 0, 1, 2, 12, 12), 12, True, '9 classes in the 12-float pitch: channels 9 .. 11 are written as zeros'),
    ((4, 64, 7, 2, 3, 1, 2, 40, 40), 64, False, 'the thin-input stem'),
    ((32, 76, 3, 1, 1, 1, 1, 10, 10), 76, False, 'Cout % 8 = 4, which the plane form refuses'),
]
