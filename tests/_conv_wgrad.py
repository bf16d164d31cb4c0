"""The dense convolution's filter gradient -- pylc_conv2d_wgrad, pylc_conv2d_wgrad_slabs, pylc_splitk_reduce_batch -- stated in numpy float64
from include/pylc_hip.h (PylcConvDesc, "fp16 planes", the pylc_conv2d_wgrad* comments), not from the kernels, with the comparison helpers
tests/test_conv_wgrad_abi_gpu.py applies to what the GPU wrote and tests/test_cpu_conv_wgrad_ref.py applies to corrupted copies of a perfect
output.  Not a test module.  Geometry, operands, plane placement and the fp32 comparison are those of tests/_eval_conv.py.

What the kernel sees.  A plane operand (x_fmt = dy_fmt = 1) is built on the host (tests/_planes.py); the values behind it are
t^ = join(h0, h1, s)  (precision mode 2, f16x3) resp. join(h0, None, s)  (mode 3, plane 0 alone).  An fp32 operand is its own values.

Filter gradient, in float64, in the GATHER form of the definition (every tap collects, over the output pixels, the product of the gradient
and the input pixel that tap read; no tiles, no splits):
    dw[n, r, s, c] = sum over (b, ho, wo) of dy^[b, ho, wo, n] x^[b, ho stride - pad + r dil, wo stride - pad + s dil, c]   source inside the image
    dwa = the same with absolute values: the scale every error is measured in
A tap no output pixel reads inside the image (tap_reached) has dw == 0 by definition: exact zeros are asserted there.
pylc_splitk_reduce_batch:  dw[i] = sum over the slabs k of slabs[k][i]  (slab_sum64), an fp32 sum in the kernel's own fixed order: within
_planes.sum_bound of the float64 sum.

Tolerance.  TOL_W starts from the project's figure for these kernels, TOL_C = 1e-6 + 2^-23 of dwa (tests/_conv_train.py), and the rule of
DESIGN.md 5.24.1: halved if the worst measured ratio over all cases stays below 0.25, kept otherwise.  Measured on an MI355X
(profiles/conv_wgrad_abi.txt): worst 0.795 on fp32 operands (fp32 MFMA chain, the 7x7 stem: 800 pixels in one split), 0.633 with bf16x6,
0.370 with f16x3 on fp32 operands, 0.379 on plane operands (mode 2, the dilation-6 case) -- a slack of 1.26 x, so the final value is the
starting one.  No form exceeded 1.0: the term for the final fp32 sum of the splits' partials (_planes.sum_bound) was not needed and is not
part of the bound (check_dw's `extra` stays unused by the GPU test).

The plan.  plan() transliterates the host-only arithmetic the workspace size follows from (tile configuration by channel counts, split
count by the fill of the resident-block slots of 256 compute units, the cap of `max_steps` K-steps of 32 pixels per block of a multi-tap
filter) so that every table row can record HOW its configuration, geometry path and split count were derived; the rows hold the derived
figures as literals, tests/test_cpu_conv_wgrad_ref.py asserts literal == plan() == what pylc_conv2d_wgrad_workspace returns, and the GPU test
asserts the workspace figure again before each launch.  If a shape stops reaching its plan, the shape changes, never the assertion."""
import numpy as np

from tests import _conv_train as T
from tests import _eval_conv as E
from tests import _planes as P

F64, F32 = np.float64, np.float32
GUARD = E.GUARD
Geom = E.Geom
TOL_W = T.TOL_C                            # final = starting figure 1e-6 + 2^-23: the measured worst ratio is 0.795 (module docstring)
KNOB_DEFAULTS = dict(m16=2, dma=1, sets=1, acc1=0, flags=0, max_steps=256)


# ---- data -----------------------------------------------------------------------------------------------------------------------------------
def make_wgrad_data(g, seed):
    """x [B][H][W][Cin] and dy [B][OH][OW][Cout], each N(0,1) 2^U(-12,0) per element (the 12-binade spread of _conv_train.make_train_data, so
    that plane 1 and fp16 subnormal pieces matter); fp32, fixed seeds."""
    r = np.random.RandomState(seed)
    xs, ys = (g.b, g.h, g.w, g.cin), (g.b, g.oh, g.ow, g.cout)
    x = (r.standard_normal(xs) * 2.0 ** r.uniform(-12.0, 0.0, xs)).astype(F32)
    dy = (r.standard_normal(ys) * 2.0 ** r.uniform(-12.0, 0.0, ys)).astype(F32)
    return dict(x=x, dy=dy)


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def _tap_range(k_idx, g, size, osize):
    """Output positions o in [lo, hi) whose tap k_idx reads the input position o stride - pad + k_idx dil inside [0, size), and the first such
    input position."""
    lo = max(0, -((k_idx * g.dil - g.pad) // g.stride))
    hi = min(osize, (size - 1 + g.pad - k_idx * g.dil) // g.stride + 1)
    return lo, hi, lo * g.stride - g.pad + k_idx * g.dil


def wgrad64(dy_seen, x_seen, g, pixels=None):
    """(dw, dwa) float64 [Cout][k k][Cin] of dy [B][OH][OW][Cout] (or [M][Cout]) and x [B][H][W][Cin] (or [B H W][Cin]).  pixels: bool [M],
    the output pixels that take part in the reduction (default all) -- what a kernel that dropped a row or a split would have summed."""
    dy = np.asarray(dy_seen, dtype=F64).reshape(g.b, g.oh, g.ow, g.cout)
    x = np.asarray(x_seen, dtype=F64).reshape(g.b, g.h, g.w, g.cin)
    if pixels is not None:
        dy = dy * np.asarray(pixels, dtype=F64).reshape(g.b, g.oh, g.ow, 1)
    dya, xa = np.abs(dy), np.abs(x)
    dw = np.zeros((g.cout, g.k * g.k, g.cin), dtype=F64)
    dwa = np.zeros_like(dw)
    for r in range(g.k):
        lo, hi, i0 = _tap_range(r, g, g.h, g.oh)
        if hi <= lo:
            continue
        for s in range(g.k):
            lo2, hi2, j0 = _tap_range(s, g, g.w, g.ow)
            if hi2 <= lo2:
                continue
            src = (slice(None), slice(i0, i0 + (hi - lo - 1) * g.stride + 1, g.stride), slice(j0, j0 + (hi2 - lo2 - 1) * g.stride + 1, g.stride))
            n = g.b * (hi - lo) * (hi2 - lo2)
            dw[:, r * g.k + s, :] = dy[:, lo:hi, lo2:hi2].reshape(n, g.cout).T @ x[src].reshape(n, g.cin)
            dwa[:, r * g.k + s, :] = dya[:, lo:hi, lo2:hi2].reshape(n, g.cout).T @ xa[src].reshape(n, g.cin)
    return dw, dwa


def tap_reached(g):
    """bool [k k]: the taps at least one output pixel reads inside the image."""
    out = np.zeros(g.k * g.k, dtype=bool)
    for r in range(g.k):
        lo, hi, _ = _tap_range(r, g, g.h, g.oh)
        for s in range(g.k):
            lo2, hi2, _ = _tap_range(s, g, g.w, g.ow)
            out[r * g.k + s] = hi > lo and hi2 > lo2
    return out


def slab_sum64(slabs):
    """(sum, bound) float64 [n] of slabs [splits][n]: the float64 sum over the slabs and _planes.sum_bound of an any-order fp32 sum of them."""
    s = np.asarray(slabs, dtype=F64)
    return s.sum(0), P.sum_bound(s, axis=0)


# ---- operands as the kernel reads them ----------------------------------------------------------------------------------------------------------
PITCH_EXTRA, PITCH_C0 = 32, 16              # pitched operands: channels [16, 16 + C) of a C + 32 wide buffer


def plane_image(t, s, nplanes, pitched, extra=PITCH_EXTRA):
    """(uint16 buffer, offset of element (0, 0) in halves) of t [M][C] as a plane tensor under the scale s.  Dense: the placement of
    _eval_conv.encode_planes (chunk-interleaved where pylc_planes_stride says so).  Pitched: channels [16, 16 + C) of [nplanes][M][C + extra]
    halves, separate planes M (C + extra) halves apart, every other half 0x7e00."""
    m, c = t.shape
    if not pitched:
        return E.encode_planes(t, s, nplanes), 0
    pitch = c + extra
    h0, h1 = P.split(t, s)
    out = np.full(nplanes * m * pitch, P.FILL16, dtype=np.uint16)
    index = (np.arange(m, dtype=np.int64)[:, None] * pitch + PITCH_C0 + np.arange(c, dtype=np.int64)[None, :]).ravel()
    P.place(h0, h1 if nplanes == 2 else None, False, out=out, stride=m * pitch, index=index)
    return out, PITCH_C0


def f32_image(t, pitch, c0=0, fill=np.nan, zero_to=None):
    """fp32 buffer [M][pitch] holding t [M][C] in channels [c0, c0 + C), `fill` elsewhere; zero_to: channels [c0 + C, c0 + zero_to) hold zeros
    (what pylc_conv2d_fwd writes into [Cout, roundup4(Cout)))."""
    m, c = t.shape
    out = np.full((m, pitch), fill, dtype=F32)
    out[:, c0:c0 + c] = t
    if zero_to is not None:
        out[:, c0 + c:c0 + zero_to] = 0.0
    return out


# ---- the host-only plan -------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def plan(g, max_steps=256, cus=256, planes=True):
    """(cfg, fast, splits, m_per_split) of a filter gradient: cfg 0 = 128 x 128 tiles, 1 = 64 x 64, 2 = 32 (Cout) x 128 (Cin), 3 = the thin-input
    tile (Cin == 4, multi-tap: columns are (tap, 4 channels)); fast = geometry path (1: OW % 32 == 0, 2: OW >= 16, 0: the division path --
    OW < 16 or cfg 3); the split count fills whole rounds of resident blocks (2 per compute unit for cfg 0, else 4) with at least 512 pixels
    per block, the smallest count within 4 % of the best fill, at least ceil(M / (32 max_steps)) for a multi-tap filter."""
    t, m = g.k * g.k, g.m
    cin4 = g.cin == 4 and t > 1
    if cin4:
        cfg, bn, bc = 3, 64, 64
    elif g.cout <= 32:
        cfg, bn, bc = 2, 32, 128
    elif g.cout <= 64 or g.cin <= 64:
        cfg, bn, bc = 1, 64, 64
    else:
        cfg, bn, bc = 0, 128, 128
    tiles = _cdiv(g.cout, bn) * (_cdiv(t * 4, bc) if cin4 else _cdiv(g.cin, bc) * t)
    slots = (2 if cfg == 0 else 4) * cus
    max_splits = min(max(_cdiv(m, 512), 1), 256)
    min_splits = 1
    if t > 1 and not cin4 and max_steps > 0:
        min_splits = min(_cdiv(m, 32 * max_steps), max_splits)
    s, best = min_splits, -1.0
    for c in range(min_splits, max_splits + 1):
        blocks = tiles * c
        eff = blocks / float(_cdiv(blocks, slots) * slots)
        if eff > best + 0.04:
            best, s = eff, c
    mps = _cdiv(_cdiv(m, s), 32) * 32
    s = _cdiv(m, mps)
    fast = 0 if cin4 or g.ow < 16 else (1 if g.ow % 32 == 0 else 2)
    return cfg, fast, s, mps


def split_of_pixel(g, mps):
    """int [M]: the split that reduces each output pixel."""
    return np.arange(g.m) // mps


# ---- comparison helpers: each raises AssertionError with the offending element, or returns the worst error / (tol * dwa) -------------------------
def _where(i, g):
    t = g.k * g.k
    n, e = divmod(int(i), t * g.cin)
    return 'row %d tap %d channel %d' % (n, e // g.cin, e % g.cin)


def check_dw(buf, g, dw64, dwa, what, tol=None, extra=None, guard=GUARD):
    """The fp32 dw inside its NaN-filled buffer [guard | Cout k k Cin | guard]: both guards still NaN, EVERY element written (not NaN), exact
    zeros in the taps no pixel reaches, and every element within tol * dwa (+ extra, an array like dw64) of dw64.  Returns (worst error /
    (tol dwa), dw as [Cout][k k][Cin] fp32)."""
    tol = TOL_W if tol is None else tol
    buf = np.asarray(buf, dtype=F32)
    n = g.cout * g.k * g.k * g.cin
    assert buf.size == n + 2 * guard, '%s: a buffer of %d floats for %d elements' % (what, buf.size, n)
    for name, part in (('in front of', buf[:guard]), ('behind', buf[guard + n:])):
        if not np.isnan(part).all():
            raise AssertionError('%s: the guard %s dw was written (float %d of it)' % (what, name, int(np.nonzero(~np.isnan(part))[0][0])))
    flat = buf[guard:guard + n]
    if np.isnan(flat).any():
        i = int(np.nonzero(np.isnan(flat))[0][0])
        raise AssertionError('%s: %s was not written (NaN; %d of %d elements)' % (what, _where(i, g), int(np.isnan(flat).sum()), n))
    dw = flat.reshape(g.cout, g.k * g.k, g.cin)
    dead = ~tap_reached(g)
    if dead.any():
        bad = np.zeros(dw.shape, dtype=bool)
        bad[:, dead, :] = (dw[:, dead, :].view(np.uint32) << 1) != 0
        if bad.any():
            i = int(np.nonzero(bad.ravel())[0][0])
            raise AssertionError('%s: %s, a tap no pixel reaches, holds %.6g instead of 0 (%d elements)' % (what, _where(i, g), flat[i], int(bad.sum())))
    err = np.abs(dw.astype(F64) - dw64)
    allow = tol * dwa + (0.0 if extra is None else extra)
    bad = ~(err <= allow)
    if bad.any():
        i = int(np.nonzero(bad.ravel())[0][0])
        raise AssertionError('%s: %s is off by %.6g, allowed %.6g (value %.8g, float64 %.8g; %d of %d elements fail)' %
                             (what, _where(i, g), err.ravel()[i], allow.ravel()[i], flat[i], dw64.ravel()[i], int(bad.sum()), n))
    live = allow > 0
    return (float((err[live] / allow[live]).max()) if live.any() else 0.0), dw


def check_slab_sum(buf, slabs, what, guard=GUARD):
    """dw of one pylc_splitk_reduce_batch entry inside [guard | 4 n4 floats | guard] against slab_sum64 of slabs [splits][4 n4]: guards NaN,
    every element written and within sum_bound.  Returns the worst error / bound."""
    buf = np.asarray(buf, dtype=F32)
    n = slabs.shape[1]
    assert buf.size == n + 2 * guard
    if not (np.isnan(buf[:guard]).all() and np.isnan(buf[guard + n:]).all()):
        raise AssertionError('%s: a guard around dw was written' % what)
    got = buf[guard:guard + n]
    if np.isnan(got).any():
        i = int(np.nonzero(np.isnan(got))[0][0])
        raise AssertionError('%s: element %d is NaN: not written, or a float of the slab padding reached it (%d of %d)' % (what, i, int(np.isnan(got).sum()), n))
    want, bound = slab_sum64(slabs)
    err = np.abs(got.astype(F64) - want)
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError('%s: element %d is off by %.6g, allowed %.6g (%d of %d fail)' % (what, i, err[i], bound[i], int(bad.sum()), n))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def synthetic_slabs(seed, splits, n4, pad):
    """(buffer [splits][4 n4 + pad] fp32 with NaN in the padding, slabs [splits][4 n4]): N(0,1) 2^U(-12,0); slab 1 all -0.0 when asked by the
    caller (it overwrites)."""
    r = np.random.RandomState(seed)
    n = 4 * n4
    slabs = (r.standard_normal((splits, n)) * 2.0 ** r.uniform(-12.0, 0.0, (splits, n))).astype(F32)
    buf = np.full((splits, n + pad), np.nan, dtype=F32)
    buf[:, :n] = slabs
    return buf, slabs


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
# Geometry (Cin, Cout, k, stride, pad, dil, B, H, W).  The GEMM of a filter gradient has rows N = Cout, columns Cin per tap and the reduction
# M = B OH OW pixels, cut into `splits` ranges of m_per_split pixels (the last one shorter).  (geometry, max_steps or None = the default 256,
# cfg, fast, splits, m_per_split, note); derived for 256 compute units by plan() -- slots = 512 resident blocks for cfg 0, 1024 otherwise;
# a count c of splits fills tiles * c / (ceil(tiles * c / slots) * slots) of them:
#   (256,256,3x3) 48x32     M 1536: tiles 2 * 2 * 9 = 36, at most ceil(1536 / 512) = 3 splits, fills .07 .14 .21 -> 3 of 512; OW 32 -> FAST 1
#   (256,256,3x3) 40x40     M 1600, max_steps 4: at least ceil(1600 / 128) = 13, capped by ceil(1600 / 512) = 4 -> 4 of ceil(400 / 32) 32 = 416, last 352
#   (136,136,3x3) 33x31 x2  M 2046, max_steps 4: 4 of 512, last 510 = 15 K-steps of 32 and one of 30; two 128-tiles each way, 8 channels in the last
#   (768,512,1x1) 24x32 x2  M 1536: tiles 4 * 6 = 24, fills .047 .094 .141 -> 3 of 512; Cin > Cout; both operands % 32: chunk-interleaved
#   (200,136,1x1) 33x31 x2  M 2046: tiles 2 * 2 = 4, fills .008 .016 .023 .031: only the first clears the 4 % step -> 1 split
#   (128,256,1x1 s2) 64x64  M 2048 (32 x 32 outputs): tiles 2, fills .004 ..: 1 split; OW 32 -> FAST 1
#   (72,40,3x3 s2) 45x44 x2 M 2 * 23 * 22 = 1012, max_steps 4: min(ceil(1012 / 128), ceil(1012 / 512)) = 2 of 512, last 500; Cout <= 64 -> cfg 1
#   the rest: M <= 2048 with few tiles on 1024 slots -> 1 split
PLANE_CASES = [
    ((256, 256, 3, 1, 1, 1, 1, 48, 32), None, 0, 1, 3, 512, 'aligned multi-tap, two staging sets, M16 + DMA default'),
    ((256, 256, 3, 1, 1, 1, 1, 40, 40), 4, 0, 2, 4, 416, 'row wraps, shorter last split (352)'),
    ((136, 136, 3, 1, 1, 1, 2, 33, 31), 4, 0, 2, 4, 512, 'ragged M: the last tile holds 30 pixels; ragged N and C, 8 channels in the last tile; odd OW'),
    ((768, 512, 1, 1, 0, 1, 2, 24, 32), None, 0, 1, 3, 512, 'single tap (one staging set), Cin > Cout rasterisation, chunk-interleaved planes'),
    ((200, 136, 1, 1, 0, 1, 2, 33, 31), None, 0, 2, 1, 2048, 'no workspace; separate planes (C % 32 != 0); dw written directly'),
    ((128, 256, 1, 2, 0, 1, 2, 64, 64), None, 0, 1, 1, 2048, 'stride-2 1x1 shortcut, in_sw = 2'),
    ((72, 40, 3, 2, 1, 1, 2, 45, 44), 4, 1, 2, 2, 512, 'stride 2, odd and even size; last split 500'),
    ((64, 64, 3, 1, 0, 1, 1, 20, 24), None, 1, 2, 1, 416, 'U-Net valid conv, M = 396'),
    ((304, 48, 1, 1, 0, 1, 1, 20, 44), None, 1, 2, 1, 896, 'decoder conv1: Cin % 32 != 0, half-empty column tile'),
    ((256, 32, 1, 1, 0, 1, 2, 32, 32), None, 2, 1, 1, 2048, 'A_ALL == false: only rows < 32 load dy'),
    ((128, 24, 3, 1, 6, 6, 1, 20, 20), None, 2, 2, 1, 416, 'dilation 6: taps partly outside'),
    ((128, 16, 3, 1, 18, 18, 1, 16, 16), None, 2, 2, 1, 256, 'dilation 18: only the centre tap is reached; the other eight slices must be exact zeros'),
    ((64, 128, 2, 2, 0, 1, 2, 32, 32), None, 1, 2, 1, 512,
     'the U-Net 2x2 transposed conv, roles swapped as ops/conv.py calls it: x = dy of the up-conv, dy = its input, dw = [Cin_t][2][2][Cout_t]'),
]
SPLIT_PLANE_CASES = [0, 1, 2, 3]            # the cfg-0 cases with 3 or 4 splits: every dispatched form runs on them
# fp32 operands: (geometry, dy pitch, max_steps, cfg, fast, splits, m_per_split, note)
F32_CASES = [
    ((64, 9, 1, 1, 0, 1, 2, 24, 20), 12, None, 2, 2, 1, 960, 'the 9-class head: dy channels 9 .. 11 zero as the forward writes them; no dw row past 8'),
    ((4, 64, 7, 2, 3, 1, 2, 40, 40), 64, None, 3, 0, 1, 800, 'the thin-input stem'),
    ((4, 64, 3, 1, 0, 1, 2, 36, 36), 64, None, 3, 0, 1, 2336, 'U-Net first conv; one column tile, 36 of 64 columns used'),
    ((76, 40, 3, 2, 1, 1, 1, 19, 19), 40, None, 1, 0, 1, 128, 'the division path (OW = 10 < 16) on a dense filter, Cin % 8 != 0'),
    ((256, 256, 3, 1, 1, 1, 2, 24, 24), 256, None, 0, 2, 3, 384, 'split-K on fp32 operands in all three arithmetic modes'),
    ((136, 136, 3, 1, 1, 1, 2, 32, 32), 136, None, 0, 1, 4, 512, 'ragged channel tiles'),
]
# pylc_splitk_reduce_batch on synthetic slabs, one launch: (splits, n4, padding floats behind each slab); one tile beside 129 tiles
SLAB_ENTRIES = [(9, 33, 4), (2, 1, 12), (256, 4097, 8), (33, 100, 20)]
