"""The depthwise 3x3 convolution of include/pylc_hip.h (the comment above PylcDwDesc and the one-plane section) stated in numpy: float64
statements, the range bounds in the kernels' own float32 association, per-element first-order rounding bounds, bit-exact float32 models
and the inputs tests/test_cpu_dw_ref.py and tests/test_dw_abi_gpu.py run on.  Taken from the header, not from the kernels; the scale rule,
rn16 and the planted edges come from tests/_planes.py, the mask layout from tests/_bn.py.  Not a test module.

The operation (NHWC, w[C][3][3], fixed_padding: a pad of `dil` on each side, OH = (H - 1) / stride + 1):
    y[b, oh, ow, c]  = sum_{kr, ks} w[c, kr, ks] x[b, oh stride + (kr - 1) dil, ow stride + (ks - 1) dil, c]        (taps outside x: nothing)
    dx               = the transpose: x-position (h, w) receives w[c, kr, ks] dy[b, oh, ow, c] from every (oh, ow, kr, ks) that reads it
    dw[c, kr, ks]    = sum_{b, oh, ow} dy[b, oh, ow, c] x[b, oh stride + (kr - 1) dil, ow stride + (ks - 1) dil, c]
The data gradient may accumulate (dx += ...) and, in the masked-residual form, adds (mask ? add_src : 0).

One-plane operands: element = rn16(s v), s = P.scale_for(bound bits).  The output's bound is the float32 expression (9.f * w_amax) * in
(+ acc_bound when accumulating), in that association; the _eval form takes the TRUE maximum of x in place of the bound x was scaled with.

The bounds.  u = 2^-24, gamma(n) = n u / (1 - n u).  A sum of products evaluated with n roundings on its longest path is within
gamma(n) sum|w x| of the exact sum.
  * fp32 forward / data gradient (separate multiply and add; the file is built with -ffp-contract=off): L live taps make L roundings on the
    longest path (the first product's rounding and L - 1 additions: 0 + p is exact).  The tiled kernels fuse: L fmas, L roundings again --
    one fewer per TERM, the same on the longest path, so the same figure serves both.  Each accumulate / masked add is one more rounding,
    of a partial result the magnitudes bound: gamma(L + extras) (sum|w x| + |old| + |add|).
  * a half output adds P.bound1(|ref| + that bound, s_out): half an fp16 ulp of the value rounded.  The old content of an accumulating half
    dx is re-scaled by a power of two (exact); its rounding is the addition counted above.
  * filter gradient: depth(wgrad) = the per-thread chain length (from the Python statement of make_slab / make_strips / make_tiles(_g)
    below) + the product rounding of the unfused kernels + the in-block adds + the one final rounding of the fp64 combine.
  * statistics: the same with the chain of the statistics accumulators; sums of squares carry the product's rounding too.
"""
import collections

import numpy as np

from tests import _planes as P

F32, F16, F64 = np.float32, np.float16, np.float64
U = 2.0 ** -24
SLABS = 1024                  # the strip kernels' block limit and the tiled kernels' group limit
ROW_SLABS = 512               # make_slab's default limit
CHUNK = 128                   # channels per block of the tiled kernels


def gamma(n):
    n = np.asarray(n, dtype=F64)
    return n * U / (1.0 - n * U)


def cdiv(a, b):
    return -(-a // b)


class Desc(collections.namedtuple('Desc', 'B H W C stride dil x_pitch y_pitch')):
    """PylcDwDesc; pitches default to C."""
    __slots__ = ()

    def __new__(cls, B, H, W, C, stride=1, dil=1, x_pitch=None, y_pitch=None):
        return super().__new__(cls, B, H, W, C, stride, dil, x_pitch or C, y_pitch or C)

    OH = property(lambda d: (d.H - 1) // d.stride + 1)
    OW = property(lambda d: (d.W - 1) // d.stride + 1)
    dense = property(lambda d: d.x_pitch == d.C and d.y_pitch == d.C)


# ---- the taps ------------------------------------------------------------------------------------------------------------------------------
def fwd_terms(x, stride, dil, pad=None):
    """The nine operands of the forward sum, tap order (kr, ks): [(term[B, OH, OW, C], live[1, OH, OW, 1])]; taps outside x are zeros / not
    live.  pad: the padding on each side (the header: dil; a mutant passes another)."""
    B, H, W, C = x.shape
    pad = dil if pad is None else pad
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    m = 2 * dil + 1
    xp = np.zeros((B, H + 2 * m, W + 2 * m, C), dtype=x.dtype)
    lp = np.zeros((H + 2 * m, W + 2 * m), dtype=bool)
    xp[:, m:m + H, m:m + W] = x
    lp[m:m + H, m:m + W] = True
    out = []
    for kr in range(3):
        for ks in range(3):
            h0, w0 = m - pad + kr * dil, m - pad + ks * dil
            hs, ws = slice(h0, h0 + (OH - 1) * stride + 1, stride), slice(w0, w0 + (OW - 1) * stride + 1, stride)
            out.append((xp[:, hs, ws, :], lp[hs, ws][None, :, :, None]))
    return out


def dgrad_terms(dy, H, W, stride, dil, wshift=0):
    """The nine operands of the data gradient, in the forward's tap order: term t is dy scattered to the x-positions tap t reads.  wshift:
    a mutant's column offset (1 swaps the column parity at stride 2)."""
    B, OH, OW, C = dy.shape
    out = []
    for kr in range(3):
        for ks in range(3):
            h, w = np.arange(OH) * stride + (kr - 1) * dil, np.arange(OW) * stride + (ks - 1) * dil + wshift
            okh, okw = (h >= 0) & (h < H), (w >= 0) & (w < W)
            t = np.zeros((B, H, W, C), dtype=dy.dtype)
            live = np.zeros((H, W), dtype=bool)
            ih, iw = h[okh][:, None], w[okw][None, :]
            t[:, ih, iw, :] = dy[:, np.arange(OH)[okh][:, None], np.arange(OW)[okw][None, :], :]
            live[ih, iw] = True
            out.append((t, live[None, :, :, None]))
    return out


def nlive(terms):
    return sum(l.astype(np.int64) for _, l in terms)


# ---- float64 statements -------------------------------------------------------------------------------------------------------------------
def conv64(terms, w, absolute=False):
    w = np.asarray(w, dtype=F64).reshape(-1, 9)
    acc = 0.0
    for t, (term, _) in enumerate(terms):
        p = w[:, t] * term.astype(F64)
        acc = acc + (np.abs(p) if absolute else p)
    return acc


def fwd64(x, w, stride, dil):
    return conv64(fwd_terms(x, stride, dil), w)


def dgrad64(dy, w, H, W, stride, dil, old=None, add_src=None, add_mask=None):
    """dx (+ old: the accumulating form) (+ mask ? add_src : 0: the masked-residual form)."""
    dx = conv64(dgrad_terms(dy, H, W, stride, dil), w)
    if old is not None:
        dx = dx + old.astype(F64)
    if add_src is not None:
        dx = dx + np.where(add_mask, add_src.astype(F64), 0.0)
    return dx


def wgrad64(x, dy, stride, dil, absolute=False):
    """dw[C][9] (absolute: the sum of the terms' magnitudes, what the bound scales with)."""
    dy = dy.astype(F64)
    cols = []
    for term, _ in fwd_terms(x, stride, dil):
        p = dy * term.astype(F64)
        cols.append((np.abs(p) if absolute else p).sum((0, 1, 2)))
    return np.stack(cols, 1)


def stats64(y):
    """Per-channel (sum, sum of squares, sum of magnitudes) of what was stored."""
    y = y.astype(F64).reshape(-1, y.shape[-1])
    return y.sum(0), (y * y).sum(0), np.abs(y).sum(0)


# ---- range bounds in the kernels' arithmetic ---------------------------------------------------------------------------------------------------
def bound_bits(w_amax, in_bound, acc_bound=None, nine=9.0):
    """Bits of (9.f * w_amax) * in (+ acc) in float32, that association.  For the _eval form pass the true maximum as `in_bound`."""
    b = F32(F32(nine) * F32(w_amax)) * F32(in_bound)
    if acc_bound is not None:
        b = F32(b + F32(acc_bound))
    return P.bits_of(b)


# ---- per-element bounds --------------------------------------------------------------------------------------------------------------------------
def elem_bound(terms, w, extras=()):
    """gamma(L + len(extras)) (sum|w x| + sum|extras|), L the live taps of the element."""
    mag = conv64(terms, w, absolute=True)
    for e in extras:
        mag = mag + np.abs(e.astype(F64))
    return gamma(nlive(terms) + len(extras)) * mag


def half_bound(ref, acc, s_out):
    """The accumulation bound plus the rounding of the stored half."""
    return acc + P.bound1(np.abs(ref) + acc, s_out)


# ---- exact float32 arithmetic ---------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a b + c) with one rounding, a and c float32, b a float32 holding an fp16 value: the float64 product is exact (24 + 11 bits); the
    float64 sum is corrected to round-to-odd with the TwoSum residual, after which the conversion to float32 rounds once."""
    p = np.asarray(a, dtype=F32).astype(F64) * np.asarray(b, dtype=F32).astype(F64)
    c = np.broadcast_to(np.asarray(c, dtype=F32).astype(F64), p.shape)
    s = p + c
    bb = s - p
    r = (p - (s - bb)) + (c - bb)
    bits = np.array(s, dtype=F64).view(np.uint64).copy()
    inexact = r != 0.0
    down = inexact & (np.signbit(r) != np.signbit(s))
    bits[down] -= np.uint64(1)
    bits[inexact] |= np.uint64(1)
    return bits.view(F64).astype(F32)


def rn16(v):
    return np.asarray(v, dtype=F32).astype(F16)


def rz16(v):
    """A mutant's conversion: truncation toward zero."""
    v = np.asarray(v, dtype=F32)
    h = v.astype(F16)
    over = np.abs(h.astype(F32)) > np.abs(v)
    u = h.view(np.uint16).copy()
    u[over] -= np.uint16(1)
    return u.view(F16)


def canon32(a):
    """float32 values with -0 replaced by +0."""
    return np.asarray(a, dtype=F32) + F32(0.0)


# ---- bit-exact float32 models ----------------------------------------------------------------------------------------------------------------------
FWD_ORDER = tuple(range(9))
ROT_ORDER = tuple(range(8, -1, -1))           # the stride-1 tiled data gradient walks the filter rotated by 180 degrees


def chain32(terms, w, in_inv=None):
    """General and strip kernels: taps in order kr, ks; acc = acc + k * x with both roundings; half inputs de-scaled first (exact)."""
    w = np.asarray(w, dtype=F32).reshape(-1, 9)
    acc = None
    for t in FWD_ORDER:
        xt = terms[t][0].astype(F32)
        if in_inv is not None:
            xt = xt * F32(in_inv)
        p = w[:, t] * xt
        acc = p + F32(0.0) if acc is None else acc + p
    return acc


def chain_fma(terms, w, order=FWD_ORDER):
    """Tiled kernels: an fma chain on the raw halves in `order` (the stride-2 data gradient takes its parity subset in the forward's order:
    the other taps are zeros here and leave the accumulator as it is)."""
    w = np.asarray(w, dtype=F32).reshape(-1, 9)
    acc = np.zeros(terms[0][0].shape, dtype=F32)
    for t in order:
        acc = fma32(w[:, t], terms[t][0].astype(F32), acc)
    return acc


def finish32(acc, in_inv=None, old=None, old_inv=None, add_src=None, add_mask=None, s_out=None, cvt=rn16):
    """acc (* in_inv: tiled) (+ old (* old_inv: a half dx)) (+ mask ? src : 0), then rn16(. * s_out) for a half output."""
    v = np.asarray(acc, dtype=F32)
    if in_inv is not None:
        v = v * F32(in_inv)
    if old is not None:
        v = v + (old.astype(F32) * F32(old_inv) if old_inv is not None else old.astype(F32))
    if add_src is not None:
        v = v + np.where(add_mask, add_src.astype(F32), F32(0.0))
    return v if s_out is None else cvt(v * F32(s_out))


def model(terms, w, path, grad=False, stride=1, in_scale=None, **fin):
    """The float32 model of one forward / data-gradient launch on `path` ('general' | 'strip' | 'tile' | 'tileg'); terms hold fp32 values, or
    the raw halves when in_scale (the operand's scale) is given."""
    inv = None if in_scale is None else F32(1.0) / F32(in_scale)
    if path in ('tile', 'tileg'):
        order = ROT_ORDER if (grad and stride == 1) else FWD_ORDER
        return finish32(chain_fma(terms, w, order), in_inv=inv, **fin)
    return finish32(chain32(terms, w, inv), **fin)


Expect = collections.namedtuple('Expect', 'bits s out ref bound')      # out: the model's halves (or fp32 values when s is None)


def expect_fwd(x, w, d):
    """fp32 forward: (model, fp64, bound)."""
    t = fwd_terms(x, d.stride, d.dil)
    return Expect(None, None, chain32(t, w), conv64(t, w), elem_bound(t, w))


def expect_dgrad(dy, w, d, old=None):
    t = dgrad_terms(dy, d.H, d.W, d.stride, d.dil)
    ex = () if old is None else (old,)
    return Expect(None, None, finish32(chain32(t, w), old=old), conv64(t, w) + (0.0 if old is None else old.astype(F64)), elem_bound(t, w, ex))


def expect_fwd_h(xh, w, wa_bits, d, path, true_bits=None, cvt=rn16, nine=9.0):
    """pylc_dwconv3x3_fwd_h (true_bits: _fwd_h_eval) on the Half xh."""
    bits = bound_bits(P.float_of(wa_bits), P.float_of(xh.bits if true_bits is None else true_bits), nine=nine)
    s = P.scale_for(bits)
    out = model(fwd_terms(xh.h, d.stride, d.dil), w, path, in_scale=xh.s, s_out=s, cvt=cvt)
    tv = fwd_terms(xh.v, d.stride, d.dil)
    ref = conv64(tv, w)
    return Expect(bits, s, out, ref, half_bound(ref, elem_bound(tv, w), s))


def expect_dgrad_h(dyh, w, wa_bits, d, path, old=None, half_out=True, add_src=None, add_mask=None, rescale_bug=False):
    """pylc_dwconv3x3_dgrad_h / _dgrad_h_add: old = a Half (accumulating half dx; its bound joins the new one) or an fp32 array (accumulating
    fp32 dx) or None; half_out False: an fp32 dx, no bound written."""
    old_half = isinstance(old, Half)
    assert not old_half or half_out
    bits = s = None
    if half_out:
        bits = bound_bits(P.float_of(wa_bits), P.float_of(dyh.bits), P.float_of(old.bits) if old_half else None)
        s = P.scale_for(bits)
    fin = dict(s_out=s)
    if old_half:
        fin.update(old=old.h, old_inv=F32(1.0) / (s if rescale_bug else old.s))
    elif old is not None:
        fin.update(old=old)
    if add_src is not None:
        fin.update(add_src=add_src, add_mask=add_mask)
    out = model(dgrad_terms(dyh.h, d.H, d.W, d.stride, d.dil), w, path, grad=True, stride=d.stride, in_scale=dyh.s, **fin)
    tv = dgrad_terms(dyh.v, d.H, d.W, d.stride, d.dil)
    oldv = None if old is None else (old.v if old_half else old.astype(F64))
    ref = dgrad64(dyh.v, w, d.H, d.W, d.stride, d.dil, oldv, add_src, add_mask)
    extras = [e for e in (oldv, None if add_src is None else np.where(add_mask, add_src, 0.0)) if e is not None]
    acc = elem_bound(tv, w, extras)
    return Expect(bits, s, out, ref, half_bound(ref, acc, s) if half_out else acc)


# ---- the path each shape takes ---------------------------------------------------------------------------------------------------------------------
def valid(d):
    return (min(d.B, d.H, d.W, d.C) > 0 and d.C % 4 == 0 and d.stride in (1, 2) and d.dil >= 1 and d.x_pitch >= d.C and d.y_pitch >= d.C and
            d.x_pitch % 4 == 0 and d.y_pitch % 4 == 0 and d.B * d.H * d.W < 2 ** 31)


def fast(d):
    """The strip kernels, against the general ones."""
    return d.stride == 1 and d.dil == 1 and d.W >= 2


def tile_dense(d):
    return d.C % 8 == 0 and d.dense and d.B * d.H * d.W * d.C * 2 < 2 ** 31


def tile_ok(d, knob=3):
    return bool(knob & 1) and tile_dense(d) and d.stride == 1 and d.dil == 1


def tileg_ok(d, knob=3):
    return bool(knob & 2) and tile_dense(d) and ((d.stride == 2 and d.dil == 1 and d.H % 2 == 0 and d.W % 2 == 0) or (d.stride == 1 and d.dil == 2))


def half_ok(d, knob=3):
    """A half kernel exists for the shape: strips, or one of the tiled kernels."""
    return valid(d) and d.dense and (fast(d) or tile_ok(d, knob) or tileg_ok(d, knob))


def bn_ok(d, knob=3):
    return valid(d) and (tile_ok(d, knob) or tileg_ok(d, knob))


def add_ok(d, knob=3):
    return valid(d) and tile_ok(d, knob)


def half_path(d, knob=3):
    return 'tile' if tile_ok(d, knob) else 'tileg' if tileg_ok(d, knob) else 'strip' if (fast(d) and d.dense) else None


def f32_path(d):
    return 'strip' if fast(d) else 'general'


Slab = collections.namedtuple('Slab', 'CV cols RL rows_per_slab nslab')
Strips = collections.namedtuple('Strips', 'nseg seg pairs n_strips strips_per_block blocks')
Tiles = collections.namedtuple('Tiles', 'tiles_w tiles_h n_tiles groups chunks th')


def make_slab(M, C):
    CV = C // 4
    cols = min(CV, 256)
    RL = 256 // cols
    rps = cdiv(max(cdiv(M, ROW_SLABS), RL * 8), RL) * RL
    return Slab(CV, cols, RL, rps, cdiv(M, rps))


def make_strips(d, g):
    pairs, seg, waves = (d.H + 1) // 2, 32, (g.cols * g.RL + 63) // 64
    while True:
        nseg = cdiv(d.W, seg)
        sg = cdiv(d.W, nseg)
        n = d.B * pairs * nseg
        if seg <= 8 or cdiv(n, g.RL) * waves >= 256 * 12:
            break
        seg //= 2
    spb = g.RL * cdiv(n, g.RL * SLABS)
    return Strips(nseg, sg, pairs, n, spb, cdiv(n, spb))


def make_tiles(d, mode=0):
    """Tiles of the half kernels: stride-1 / dilation-1 and every data gradient tile 8 x 16 of the tensor written; the stride-2 forward and
    filter gradient tile 4 x 16 of the output, dilation 2 tiles 8 x 16 of it."""
    if (d.stride, d.dil) == (1, 1) or mode == 1:
        H, W, th = d.H, d.W, 8
    else:
        H, W, th = d.OH, d.OW, (4 if d.stride == 2 else 8)
    tw, t_h = cdiv(W, 16), cdiv(H, th)
    n = d.B * t_h * tw
    return Tiles(tw, t_h, n, min(n, SLABS), cdiv(d.C, CHUNK), th)


def f32_stats_rows(d):
    if not (valid(d) and fast(d)):
        return 0
    return make_strips(d, make_slab(d.B * d.OH * d.OW, d.C)).blocks


def half_stats_rows(d, knob=3):
    if not half_ok(d, knob):
        return 0
    p = half_path(d, knob)
    return make_tiles(d).groups if p in ('tile', 'tileg') else f32_stats_rows(d)


def depths(d, path, mode):
    """(rows written, chain length per thread, in-block adds) of the per-block partials: mode 0 the statistics of the forward, mode 2 the
    filter gradient.  `rows` is also what the workspace must hold."""
    if path == 'general':
        g = make_slab(d.B * d.OH * d.OW, d.C)
        return g.nslab, cdiv(g.rows_per_slab, g.RL), g.RL - 1
    if path == 'strip':
        g = make_slab(d.B * d.OH * d.OW, d.C)
        s = make_strips(d, g)
        return s.blocks, (s.strips_per_block // g.RL) * 2 * s.seg, g.RL - 1
    t = make_tiles(d, mode)
    per = cdiv(t.n_tiles, t.groups)
    if mode == 2:
        return t.groups, per * t.th * 2, 7                  # a thread owns two columns of every tile row; 8 pixel threads per channel quad
    return t.groups, per * t.th, 16                         # after the lane swap one pixel per tile row; 16 contributions per channel


def wgrad_bound(x, dy, d, path):
    """Per (c, tap): gamma(chain + product rounding of the unfused kernels + in-block adds + the final rounding) sum|dy x|, plus an
    absolute floor for results below 2^-126: a product, a partial row or the result that is an fp32 subnormal is rounded to 2^-150 at
    most (reached only by the terms 2^-100 below the largest of the small-corner case)."""
    rows, chain, inblock = depths(d, path, 2)
    n = chain + inblock + 1 + (0 if path in ('tile', 'tileg') else 1)
    return gamma(n) * wgrad64(x, dy, d.stride, d.dil, absolute=True) + (d.B * d.OH * d.OW + rows + 1) * 2.0 ** -150


def stats_bound(stored, d, path):
    """(d sum, d sum of squares) of the summed partial rows against stats64(stored)."""
    _, chain, inblock = depths(d, path, 0)
    _, s2, sa = stats64(stored)
    return gamma(chain + inblock) * sa, gamma(chain + inblock + 1) * s2


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def wide(seed, shape, mag=1.0, mult=1.0):
    """fp32 NHWC, P.wide with P.plant's edges (zeros of both signs, +-max, ties, elements down to 2^-30 of the scaled bound) for the range
    scalar mult x max|x|; mag (a power of two) places the whole tensor.  Returns (x, bits of the range scalar)."""
    c = shape[-1]
    x, bits = P.plant(P.wide(seed, int(np.prod(shape[:-1])), c) * F32(mag), mult)
    return x.reshape(shape), bits


Half = collections.namedtuple('Half', 'h bits s v')          # the stored halves, the bound's bits, the scale, the fp64 values the kernels see


def to_half(x, bits):
    s = P.scale_for(bits)
    h = P.split(x, s)[0]
    return Half(h, bits, s, h.astype(F64) / float(s))


def wide_half(seed, shape, mag=1.0, mult=1.0):
    return to_half(*wide(seed, shape, mag, mult))


def filt(seed, C, scale=0.4):
    """w[C][3][3] ~ scale N(0, 1) with per-channel magnitudes spread over 2^-6 .. 1, and the bits of max|w|."""
    r = np.random.RandomState(1000 + seed)
    w = (scale * r.standard_normal((C, 3, 3)) * 2.0 ** r.uniform(-6.0, 0.0, (C, 1, 1))).astype(F32)
    return w, P.bits_of(np.abs(w).max())


def one_hot(C, tap, val):
    w = np.zeros((C, 9), dtype=F32)
    w[:, tap] = val
    return w.reshape(C, 3, 3), P.bits_of(val)


def pack_mask(keep):
    """The 1-bit mask of PylcBnExtra.relu_mask from bool [M][C] (tests/_bn.py unpack_relu_bits is its inverse): byte (row C/4 + cv) / 2, the
    even quad in the low nibble, bit k of a nibble = channel 4 cv + k -- element e is bit e & 7 of byte e >> 3."""
    k = np.asarray(keep, dtype=np.uint8).reshape(-1, 8)
    return (k << np.arange(8, dtype=np.uint8)).sum(1).astype(np.uint8)


# (B, H, W, C, stride, dil): the smallest shapes at which each mechanism can fail
F32_CASES = [
    (1, 1, 2, 4, 1, 1),            # the smallest strip
    (2, 5, 7, 8, 1, 1),            # odd H, one segment
    (2, 9, 70, 20, 1, 1),          # several ragged segments, odd vector count
    (2, 9, 11, 728, 1, 1),         # 182 columns, idle threads
    (1, 4, 6, 1028, 1, 1),         # a second column pass with one live column
    (1, 6, 1, 12, 1, 1),           # W = 1: the general kernel at stride 1
    (2, 7, 9, 16, 2, 1), (2, 8, 10, 16, 2, 1),
    (1, 9, 10, 24, 1, 2),
    (1, 5, 6, 8, 1, 4),
    (1, 3, 3, 8, 1, 3),            # only the centre tap is live
    (1, 6, 7, 8, 2, 2),
]
WS_CASE = (200, 1, 9, 8, 1, 1)             # the filter gradient's 4 strip blocks exceed make_slab's 2 row slabs: the workspace check
# strips_per_block = 2 (1026 strips on 513 blocks: a thread walks two strips, the filter gradient's accumulators carry across them) at 14 MB
# instead of the 67 MB of (2, 66, 130, 1024, 1, 1): 256 columns and one row lane need more than 1024 strips, which many short images
# give as well as one large one.  Two-row pairs and a last single-row pair; 513 blocks against make_slab's 428 slabs.
F32_SPB2 = (342, 5, 2, 1024, 1, 1)
HALF_CASES = [
    (1, 8, 16, 8, 1, 1),           # exactly one tile
    (1, 9, 17, 8, 1, 1),           # four ragged tiles, odd last column
    (2, 19, 37, 136, 1, 1),        # the second chunk holds 8 channels
    (1, 5, 6, 12, 1, 1),           # C % 8 == 4: strips whatever the knob says
    (1, 9, 1, 8, 1, 1),            # W = 1: tiled only
    (1, 8, 32, 8, 2, 1), (2, 10, 34, 136, 2, 1),
    (1, 8, 16, 8, 1, 2), (2, 11, 19, 136, 1, 2), (1, 2, 3, 8, 1, 2),
]
HALF_BIG = (1, 264, 512, 8, 1, 1)           # 1056 tiles against 1024 groups
