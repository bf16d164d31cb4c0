"""The fp16-plane format and the range kernels at the C ABI against the bit-exact model of tests/_planes.py (-m gpu; DESIGN.md section
5.17): every producer's planes bit for bit at their physical addresses, both layouts, one and two planes, pitched buffers whose unused
lanes and surroundings must stay as they were filled (fp32: NaN; halves: 0x7e00); every consumer against the model's rebuilt values and
the derived bounds per element resp. per channel; the range scalars as exact bits / true upper bounds; one scale rule for writers and readers.

Sections print their worst figure as error / bound (lines PL-A .. PL-H; 1.0 = at the bound, attained by the planted ties).  The
implementing run on an MI355X, worst over the cases of each section:
  PL-A  planes and rebuilt values bit for bit in all 84 cases; round trip 1.000 for every shape of 37 rows and more, both plane counts and
        every range scalar (the planted ties attain the bound), 0.036 / 0.000 for the 1 x 8 tensor (one / two planes), all-zero tensor exact
  PL-B  333952 halves bit for bit for interleave 0 and 1, pad columns zero, 704 sentinel halves intact
  PL-C  planes = split of pylc_maxpool_fwd's output, idx equal, 8 cases        PL-D  planes = split of [pylc_bilinear_fwd | crop], 4 cases
  PL-E  bit-identical to pylc_gap_fwd of pylc_from_planes in all 70 cases; mean against float64 0.22 (C 40, two planes), 0.16-0.20 elsewhere
  PL-F  0.14 (20 x 2056), 0.003 and below for the other shapes
  PL-G  pylc_amax exact on the three paths (negative maximum, -0, +inf, zeros; exponent field 0 for denormals); pylc_range_product / exact - 1
        in [1.1e-7, 3.4e-7] of an allowed [0, 2^-20 = 9.5e-7], with and without `add`
  PL-H  0.011 of the harness's tolerance; with the reader's own copy of the scale rule (clamp 254) the same test gave 46 x the tolerance
One finding became part of the contract: for x = -0 the kernels store h1 = -0 where the stated formula gives +0 (the compiler forms the
rn16(s x) that the residual is taken against as a fused multiply-add with a +0 addend); no value depends on it, so pieces are compared with
the sign of ZERO pieces cleared (tests/_planes.py canon) and rebuilt fp32 zeros with either sign -- nothing else is relaxed.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _planes as P

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 64                      # sentinel halves in front of, between and behind half regions


# ---- buffers -------------------------------------------------------------------------------------------------------------------------------
def _L():
    from pylc_amd import lib as L
    L.init()
    return L


def _dev_f32(a, dev, pitch=None):
    """numpy [M][C] fp32 -> ([M][pitch] NaN-filled device buffer, view of the values), bits preserved."""
    m, c = a.shape
    pitch = pitch or c
    buf = torch.full((m, pitch), NAN, device=dev)
    buf[:, :c] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return buf, buf[:, :c]


def _out_f32(dev, m, c, pitch=None):
    buf = torch.full((m, pitch or c), NAN, device=dev)
    return buf, buf[:, :c]


def _lanes_clean(buf, c, what):
    assert torch.isnan(buf[:, c:]).all(), '%s: a lane beyond C was written' % what


def _bits(v, dev):
    """Device int32[1] holding the uint32 bit pattern v."""
    return torch.from_numpy(np.array([v], dtype=np.uint32).view(np.int32)).to(dev)


def _hbuf(dev, n):
    """n halves with GUARD sentinel halves on either side, everything filled with 0x7e00; returns (whole buffer, the n halves)."""
    buf = torch.full((n + 2 * GUARD,), P.FILL16, dtype=torch.int16, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _want(n):
    return np.full(n + 2 * GUARD, P.FILL16, dtype=np.uint16)


def _same_halves(buf, want, what):
    """Bit for bit, guards included; the sign of a zero piece apart (tests/_planes.py canon)."""
    got, want = P.canon(buf.cpu().numpy().view(np.uint16)), P.canon(want)
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        raise AssertionError('%s: half %d of %d (guards included) is %#06x, the model says %#06x; %d halves differ%s' %
                             (what, i, got.size, got[i], want[i], int((got != want).sum()), ' -- the fill was overwritten' if want[i] == P.FILL16 else ''))


def _same_bits(got, want, what, zero_sign=True):
    """fp32 device tensor against a numpy fp32 array, bit for bit.  zero_sign = False: -0 and +0 count as equal (what is rebuilt from zero
    pieces: their signs are not part of the format, tests/_planes.py)."""
    g, w = got.contiguous().cpu().numpy(), np.ascontiguousarray(want, dtype=np.float32).reshape(tuple(got.shape))
    if not zero_sign:
        g, w = g + np.float32(0.0), w + np.float32(0.0)
    g, w = g.view(np.uint32), w.view(np.uint32)
    if not np.array_equal(g, w):
        i = tuple(int(k[0]) for k in np.nonzero(g != w))
        raise AssertionError('%s: element %s is %#010x, the model says %#010x; %d differ' % (what, i, g[i], w[i], int((g != w).sum())))


def _ratio(err, bound, what):
    """err <= bound everywhere (zero bound: exact); returns the worst err / bound."""
    err, bound = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(err))
    assert not np.isnan(err).any(), '%s: NaN' % what
    bad = err > bound
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad & ((err - bound) == (err - bound)[bad].max())))
        raise AssertionError('%s: index %s err %.6g > bound %.6g; %d over the bound' % (what, i, err[i], bound[i], int(bad.sum())))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _index(m, c, pitch):
    return (np.arange(m, dtype=np.int64)[:, None] * pitch + np.arange(c, dtype=np.int64)[None, :]).ravel()


class _Planes:
    """A planes tensor of M x C (pitch p) on the device, with its guards: stride 'rule' = what pylc_planes_stride returns, 'sep' = two plane
    arrays M * pitch halves apart."""

    def __init__(self, dev, m, c, pitch, nplanes, stride):
        L = _L()
        self.m, self.c, self.pitch, self.npl = m, c, pitch, nplanes
        self.stride = L.lib.pylc_planes_stride(m, c, nplanes) if stride == 'rule' else m * pitch
        if stride == 'rule':
            assert pitch == c and self.stride == (32 if nplanes == 2 and c % 32 == 0 else m * c), 'pylc_planes_stride: not the documented rule'
        self.il = nplanes == 2 and self.stride == 32
        self.n = 2 * m * c if self.il else (self.stride + m * pitch if nplanes == 2 else m * pitch)
        self.buf, self.view = _hbuf(dev, self.n)

    def expect(self, h0, h1, what):
        want = _want(self.n)
        P.place(h0, h1 if self.npl == 2 else None, self.il, out=want, base=GUARD, stride=self.stride, index=_index(self.m, self.c, self.pitch))
        _same_halves(self.buf, want, what)

    def fill(self, h0, h1):
        """Write the model's pieces (for the consumers' tests)."""
        want = _want(self.n)
        P.place(h0, h1 if self.npl == 2 else None, self.il, out=want, base=GUARD, stride=self.stride, index=_index(self.m, self.c, self.pitch))
        self.buf.copy_(torch.from_numpy(want.view(np.int16)).to(self.buf.device))
        self.want = want
        return self


def k_to_planes(x, x_pitch, pl, bits_t):
    L = _L()
    L.check(L.lib.pylc_to_planes(L.ptr(x), x_pitch, L.ptr(pl.view), pl.pitch, pl.stride, pl.m, pl.c, L.ptr(bits_t), pl.npl, L.stream()))


def k_from_planes(pl, bits_t, x_pitch=None):
    L = _L()
    obuf, out = _out_f32(pl.view.device, pl.m, pl.c, x_pitch)
    L.check(L.lib.pylc_from_planes(L.ptr(pl.view), pl.pitch, pl.stride, L.ptr(out), x_pitch or pl.c, pl.m, pl.c, L.ptr(bits_t), pl.npl, L.stream()))
    _lanes_clean(obuf, pl.c, 'from_planes')
    return out


def k_amax(t, rows, cols, pitch):
    L = _L()
    out = torch.full((3,), -1, dtype=torch.int32, device=t.device)
    L.check(L.lib.pylc_amax(L.ptr(t), rows, cols, pitch, L.ptr(out[1:2]), L.stream()))
    assert out[0].item() == -1 and out[2].item() == -1, 'amax wrote beside its scalar'
    return int(out[1:2].cpu().numpy().view(np.uint32)[0])


def _scaled_to(x, target):
    """x times the power of two that puts its maximum into [2^target, 2^(target + 1)) (fp32: what falls below 2^-149 is lost)."""
    e = int(np.floor(np.log2(float(np.abs(x).max()))))
    return (x.astype(np.float64) * 2.0 ** (target - e)).astype(np.float32)


def _range_cases(seed, m, c):
    """(name, x, bits) over the range scalars of section PL-A."""
    base = P.wide(seed, m, c)
    for mult in (1.0, 2.0, 32.0, 4096.0):
        x, bits = P.plant(base, mult)
        yield 'x%g' % mult, x, bits
    for target in (120, -110):
        x, bits = P.plant(_scaled_to(base, target))
        assert float(P.scale_for(bits)) == (2.0 ** -106 if target == 120 else 2.0 ** 115)
        yield '2^%d' % target, x, bits
    yield 'zero', np.zeros((m, c), dtype=np.float32), 0


# ---- PL-A  pylc_to_planes / pylc_from_planes ---------------------------------------------------------------------------------------------------
#        M,  C, plane pitch, stride, fp32 pitch
PLA = [(1, 8, 8, 'sep', 8),                   # smallest
       (37, 72, 72, 'sep', 72), (37, 72, 80, 'sep', 76),          # separate planes only (72 % 32 != 0), dense and pitched
       (64, 96, 96, 'rule', 96), (64, 96, 96, 'sep', 100),        # the same tensor chunk-interleaved and as two arrays
       (1031, 32, 32, 'rule', 32)]            # several blocks, four grid-stride turns, a tail


@pytest.mark.parametrize('nplanes', [2, 1])
@pytest.mark.parametrize('m,c,pp,stride,xp', PLA)
def test_pla_to_and_from_planes(dev, m, c, pp, stride, xp, nplanes):
    worst = {}
    for name, x, bits in _range_cases(m + c, m, c):
        what = 'PL-A %dx%d pitch %d %s %d plane(s) %s' % (m, c, pp, stride, nplanes, name)
        s = P.scale_for(bits)
        h0, h1 = P.split(x, s)
        xbuf, xv = _dev_f32(x, dev, xp)
        bits_t = _bits(bits, dev)
        pl = _Planes(dev, m, c, pp, nplanes, stride)
        k_to_planes(xv, xp, pl, bits_t)
        pl.expect(h0, h1, what + ': to_planes')
        back = k_from_planes(pl, bits_t, xp + 4)
        want = P.join(h0, h1 if nplanes == 2 else None, s)
        _same_bits(back, want, what + ': from_planes', zero_sign=False)
        err = np.abs(back.cpu().numpy().astype(np.float64) - x.astype(np.float64))
        worst[name] = _ratio(err, P.round_trip_bound(x, s, nplanes), what + ': round trip')
    print('PL-A %4d x %2d pitch %2d %-4s %d plane(s)  err / bound  ' % (m, c, pp, stride, nplanes) + '  '.join('%s %.3f' % kv for kv in worst.items()))


# ---- PL-B  pylc_weight_prepare --------------------------------------------------------------------------------------------------------------
#         K, RS,  C, range scalar / maximum, data scale
PLB = [(9, 1, 64, 1.0, 0),            # Kp = 12: three zero pad columns
       (136, 1, 256, 2.0, -12),       # forward interleaved, transposed (Kp = 136) not
       (64, 9, 64, 32.0, 7),          # both interleaved
       (48, 1, 40, 4096.0, -3),       # neither; a partial tile in K and in C
       (32, 9, 32, 1.0, 20)]


@pytest.mark.parametrize('interleave', [0, 1])
def test_plb_weight_prepare(dev, interleave):
    L = _L()
    amax_index = [3, 0, 4, 1, 2]                                   # every filter reads its own slot of the range table
    ws, bits, src_off, regions, n_src, n_half, tiles = [], [0] * 5, [], [], 4, GUARD, 0
    entries = []
    for i, (K, RS, Cc, mult, sh) in enumerate(PLB):
        w, b = P.plant(P.wide(50 + i, K * RS, Cc) * np.float32(2.0 ** sh), mult)
        w = w.reshape(K, RS, Cc)
        ws.append(w)
        bits[amax_index[i]] = b
        Kp = (K + 3) & ~3
        nf, nt = 2 * K * RS * Cc, 2 * Cc * RS * Kp
        fwd_off, t_off = n_half, n_half + nf + GUARD
        n_half = t_off + nt + GUARD
        regions.append((fwd_off, nf, t_off, nt))
        src_off.append(n_src)
        entries.append(L.WPrepEntry(n_src, fwd_off, t_off, tiles, K, RS, Cc, amax_index[i]))
        tiles += RS * ((K + 31) // 32) * ((Cc + 31) // 32)
        n_src += (w.size + 3) // 4 * 4 + 4
    base = torch.full((n_src,), NAN, device=dev)
    for w, o in zip(ws, src_off):
        base[o:o + w.size] = torch.from_numpy(w.ravel()).to(dev)
    planes = torch.full((n_half,), P.FILL16, dtype=torch.int16, device=dev)
    arr = (L.WPrepEntry * len(entries))(*entries)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(dev)
    amax = torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.int32)).to(dev)
    L.check(L.lib.pylc_weight_prepare(L.ptr(base), L.ptr(table), len(entries), tiles, L.ptr(amax), L.ptr(planes), interleave, L.stream()))
    got = planes.cpu().numpy().view(np.uint16)
    want = np.full(n_half, P.FILL16, dtype=np.uint16)
    for i, (w, (fo, nf, to, nt)) in enumerate(zip(ws, regions)):
        K, RS, Cc = w.shape
        Kp = (K + 3) & ~3
        fwd, tr = P.filter_planes(w, P.scale_for(bits[amax_index[i]]), interleave)
        assert fwd.size == nf and tr.size == nt
        want[fo:fo + nf], want[to:to + nt] = fwd, tr
        what = 'PL-B filter %d (K %d RS %d C %d, interleave %d)' % (i, K, RS, Cc, interleave)
        for name, g, wnt in (('forward', P.canon(got[fo:fo + nf]), P.canon(fwd)), ('transposed', P.canon(got[to:to + nt]), P.canon(tr))):
            if not np.array_equal(g, wnt):
                j = int(np.nonzero(g != wnt)[0][0])
                raise AssertionError('%s: %s planes, half %d is %#06x, the model says %#06x; %d differ' % (what, name, j, g[j], wnt[j], int((g != wnt).sum())))
        if Kp > K:                                                 # the pad columns [K, Kp) of the transposed layout, both planes: zeros
            il_t = bool(interleave) and Kp % 32 == 0
            e = (np.arange(Cc * RS, dtype=np.int64)[:, None] * Kp + np.arange(K, Kp, dtype=np.int64)[None, :]).ravel()
            at = to + P.phys(e, il_t)
            assert not got[at].any() and not got[at + (32 if il_t else Cc * RS * Kp)].any(), what + ': a pad column is not zero'
    assert np.array_equal(got == P.FILL16, want == P.FILL16) and np.array_equal(P.canon(got), P.canon(want)), 'PL-B: a sentinel between the regions was overwritten'
    print('PL-B interleave %d: 5 filters, %d halves bit for bit, %d sentinel halves intact' % (interleave, int((want != P.FILL16).sum()), int((want == P.FILL16).sum())))


# ---- PL-C  pylc_maxpool_fwd_planes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nplanes', [2, 1])
@pytest.mark.parametrize('c', [8, 32])
@pytest.mark.parametrize('k,s,pad', [(2, 2, 0), (3, 2, 1)])
def test_plc_maxpool_planes(dev, k, s, pad, c, nplanes):
    L = _L()
    b, h, w = 2, 9, 10
    oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    x, _ = P.plant(P.wide(k + c, b * h * w, c))
    _, xv = _dev_f32(x, dev)
    bits = k_amax(xv, b * h * w, c, c)
    assert bits == P.bits_of(np.abs(x).max())
    bits_t = _bits(bits, dev)
    m = b * oh * ow
    ybuf, y = _out_f32(dev, m + 2, c)                                                # one guard row on either side
    idx = torch.full((m * c + 32,), 0xA5, dtype=torch.uint8, device=dev)
    L.check(L.lib.pylc_maxpool_fwd(L.ptr(xv), L.ptr(y[1:]), L.ptr(idx[16:]), b, h, w, c, k, s, pad, oh, ow, L.stream()))
    assert torch.isnan(ybuf[0]).all() and torch.isnan(ybuf[-1]).all()
    y = y[1:m + 1]
    ref = F.max_pool2d(xv.view(b, h, w, c).permute(0, 3, 1, 2), k, s, pad).permute(0, 2, 3, 1).reshape(m, c)
    assert torch.equal(y, ref)
    pl = _Planes(dev, m, c, c, nplanes, 'rule')
    assert pl.il == (nplanes == 2 and c == 32)
    idx2 = torch.full_like(idx, 0xA5)
    L.check(L.lib.pylc_maxpool_fwd_planes(L.ptr(xv), L.ptr(pl.view), pl.stride, nplanes, L.ptr(bits_t), L.ptr(idx2[16:]), b, h, w, c, k, s, pad, oh, ow,
                                          L.stream()))
    h0, h1 = P.split(y.cpu().numpy(), P.scale_for(bits))
    pl.expect(h0, h1, 'PL-C k %d s %d pad %d C %d %d plane(s)' % (k, s, pad, c, nplanes))
    assert torch.equal(idx, idx2) and (idx2[:16] == 0xA5).all() and (idx2[-16:] == 0xA5).all() and int(idx2[16:-16].max()) < k * k


# ---- PL-D  pylc_upsample2_crop_concat_planes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nplanes', [2, 1])
@pytest.mark.parametrize('c1,c2', [(8, 16), (32, 32)])
def test_pld_upsample_crop_concat_planes(dev, c1, c2, nplanes):
    L = _L()
    b, h, w, hh, ww = 2, 5, 6, 13, 14
    oh, ow = 2 * h, 2 * w
    h0_, w0_ = (hh - oh) // 2, (ww - ow) // 2
    assert h0_ % 2 == 1 and w0_ % 2 == 1
    z, br = P.wide(c1, b * h * w, c1), P.wide(c2 + 1, b * hh * ww, c2)
    bits = max(P.bits_of(np.abs(z).max()), P.bits_of(np.abs(br).max()))          # one bound for both sources
    z, br = P.plant(z, bits=bits)[0], P.plant(br, bits=bits)[0]
    zp, bp = c1 + 4, c2 + 8
    _, zv = _dev_f32(z, dev, zp)
    _, bv = _dev_f32(br, dev, bp)
    bits_t = _bits(bits, dev)
    m = b * oh * ow
    ubuf, up = _out_f32(dev, m, c1, c1 + 4)
    L.check(L.lib.pylc_bilinear_fwd(L.ptr(zv), zp, L.ptr(up), c1 + 4, b, h, w, c1, oh, ow, L.stream()))
    _lanes_clean(ubuf, c1, 'bilinear_fwd')
    crop = br.reshape(b, hh, ww, c2)[:, h0_:h0_ + oh, w0_:w0_ + ow].reshape(m, c2)
    cat = np.concatenate([up.cpu().numpy(), crop], 1)
    pl = _Planes(dev, m, c1 + c2, c1 + c2, nplanes, 'rule')
    L.check(L.lib.pylc_upsample2_crop_concat_planes(L.ptr(zv), zp, b, h, w, c1, L.ptr(bv), bp, hh, ww, c2, L.ptr(pl.view), pl.stride, nplanes,
                                                    L.ptr(bits_t), L.stream()))
    hp0, hp1 = P.split(cat, P.scale_for(bits))
    pl.expect(hp0, hp1, 'PL-D C1 %d C2 %d %d plane(s)' % (c1, c2, nplanes))


# ---- PL-E  pylc_gap_fwd_planes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nplanes', [2, 1])
@pytest.mark.parametrize('c', [8, 40, 64])
def test_ple_gap_from_planes(dev, c, nplanes):
    L = _L()
    b, worst = 2, 0.0
    for hw in (1, 15, 16, 130, 300):                               # either side of the 16 row lanes and of the 128-row unroll
        for mult in (1.0, 32.0):
            x, bits = P.plant(P.wide(hw + c, b * hw, c), mult)
            s = P.scale_for(bits)
            h0, h1 = P.split(x, s)
            seen = P.join(h0, h1 if nplanes == 2 else None, s).astype(np.float64).reshape(b, hw, c)
            bits_t = _bits(bits, dev)
            for stride in (('rule', 'sep') if nplanes == 2 and c % 32 == 0 else ('sep',)):
                what = 'PL-E HW %d C %d %d plane(s) %s x%g' % (hw, c, nplanes, stride, mult)
                pl = _Planes(dev, b * hw, c, c, nplanes, stride).fill(h0, h1)
                ybuf, y = _out_f32(dev, b + 2, c)
                L.check(L.lib.pylc_gap_fwd_planes(L.ptr(pl.view), pl.stride, nplanes, L.ptr(bits_t), L.ptr(y[1:]), b, hw, c, L.stream()))
                assert torch.isnan(ybuf[0]).all() and torch.isnan(ybuf[-1]).all(), what + ': wrote outside y[B][C]'
                x32 = k_from_planes(pl, bits_t)
                rbuf, r = _out_f32(dev, b, c)
                L.check(L.lib.pylc_gap_fwd(L.ptr(x32), L.ptr(r), b, hw, c, L.stream()))
                _same_bits(y[1:b + 1], r.cpu().numpy(), what + ': against gap_fwd of from_planes')
                err = np.abs(y[1:b + 1].cpu().numpy().astype(np.float64) - seen.mean(1))
                worst = max(worst, _ratio(err, P.mean_bound(seen, 1), what + ': against float64'))
    print('PL-E C %2d %d plane(s): mean err / bound %.3f' % (c, nplanes, worst))


# ---- PL-F  pylc_planes_colsum ---------------------------------------------------------------------------------------------------------------
#         M,    C, pitch, stride
PLF = [(1, 8, 8, 'sep'),                  # smallest
       (4100, 8, 8, 'sep'),               # three row slabs with a tail
       (700, 48, 48, 'sep'), (700, 48, 56, 'sep'),      # 6 column lanes, which do not divide 256; pitched
       (513, 64, 64, 'rule'),             # chunk-interleaved (two planes)
       (20, 2056, 2056, 'sep')]           # the channel loop runs twice


@pytest.mark.parametrize('nplanes', [2, 1])
@pytest.mark.parametrize('m,c,pp,stride', PLF)
def test_plf_planes_colsum(dev, m, c, pp, stride, nplanes):
    L = _L()
    x, bits = P.plant(P.wide(m + c, m, c), 2.0)
    s = P.scale_for(bits)
    h0, h1 = P.split(x, s)
    seen = P.join(h0, h1 if nplanes == 2 else None, s).astype(np.float64)
    pl = _Planes(dev, m, c, pp, nplanes, stride).fill(h0, h1)
    bits_t = _bits(bits, dev)
    sums = torch.full((c + 16,), NAN, device=dev)
    ws = torch.empty(L.lib.pylc_planes_colsum_workspace_floats(c), device=dev)
    L.check(L.lib.pylc_planes_colsum(L.ptr(pl.view), pp, pl.stride, nplanes, L.ptr(bits_t), m, c, L.ptr(sums[8:]), L.ptr(ws), L.stream()))
    assert torch.isnan(sums[:8]).all() and torch.isnan(sums[8 + c:]).all(), 'planes_colsum wrote outside sums[C]'
    err = np.abs(sums[8:8 + c].cpu().numpy().astype(np.float64) - seen.sum(0))
    r = _ratio(err, P.sum_bound(seen), 'PL-F %dx%d pitch %d %s %d plane(s)' % (m, c, pp, stride, nplanes))
    _same_halves(pl.buf, pl.want, 'PL-F: the planes were written to')
    print('PL-F %4d x %4d pitch %4d %-4s %d plane(s): sum err / bound %.2g' % (m, c, pp, stride, nplanes, r))


# ---- PL-G  range scalars --------------------------------------------------------------------------------------------------------------------
def _amax_paths(dev, a):
    """max|a| of a[rows][cols] through the three forms of pylc_amax; what the kernel may not read holds 1e30 (the float4 path documents that
    it reads the pad lanes up to roundup4(cols) inside the pitch: those hold zeros)."""
    rows, cols = a.shape
    t = torch.from_numpy(a).to(dev)
    out = {}
    dense = torch.full((rows * cols + 8,), 1e30, device=dev)             # aligned float4 path (cols % 4 == 0) or, cols % 4 != 0, the flat path
    dense[4:4 + rows * cols] = t.reshape(-1)
    out['dense'] = k_amax(dense[4:], rows, cols, cols)
    pitch = (cols + 3) // 4 * 4 + 8                                      # a pitched view at channel 4 of a wider buffer: cols % 4 != 0 inside the pitch
    wide_ = torch.full((rows, pitch), 1e30, device=dev)
    wide_[:, 4:4 + (cols + 3) // 4 * 4] = 0.0
    wide_[:, 4:4 + cols] = t
    out['pitched'] = k_amax(wide_[:, 4:], rows, cols, pitch)
    flat = torch.full((rows * cols + 9,), 1e30, device=dev)              # unaligned base, pitch == cols: the flat path
    flat[5:5 + rows * cols] = t.reshape(-1)
    out['flat'] = k_amax(flat[5:], rows, cols, cols)
    return out


@pytest.mark.parametrize('rows,cols', [(37, 12), (301, 9), (2100, 7)])
def test_plg_amax_exact_bits(dev, rows, cols):
    a = P.wide(rows, rows, cols)
    top = np.float32(np.abs(a).max())
    a[rows // 2, cols - 1] = -2 * top                                    # a planted negative maximum in the last column
    a[0, 0] = -0.0
    for name, got in _amax_paths(dev, a).items():
        assert got == P.bits_of(2 * top), 'amax %s: %#010x, want %#010x' % (name, got, P.bits_of(2 * top))
    a[rows - 1, cols - 1] = np.inf
    for name, got in _amax_paths(dev, a).items():
        assert got == 0x7f800000, 'amax %s with +inf: %#010x' % (name, got)
    z = np.zeros((rows, cols), dtype=np.float32)
    z[1, 1] = -0.0
    for name, got in _amax_paths(dev, z).items():
        assert got == 0, 'amax %s of zeros: %#010x' % (name, got)
    # fp32 denormals only: any consumer reads the exponent field alone
    d = (np.random.RandomState(rows).randint(1, 1 << 23, (rows, cols)).astype(np.uint32) | (np.random.RandomState(cols).randint(0, 2, (rows, cols)).astype(np.uint32) << 31)).view(np.float32)
    for name, got in _amax_paths(dev, d).items():
        assert (got >> 23) & 0xFF == 0 and got >> 31 == 0, 'amax %s of denormals: %#010x' % (name, got)


@pytest.mark.parametrize('with_add', [False, True])
def test_plg_range_product_is_a_tight_upper_bound(dev, with_add):
    L = _L()
    r = np.random.RandomState(9 + with_add)
    n = 200
    a, b, f, cc = [(2.0 ** r.uniform(-40, 40, n) * r.uniform(1, 2, n)).astype(np.float32) for _ in range(4)]
    f = (2.0 ** r.uniform(0, 12, n)).astype(np.float32)                   # a reduction length
    ta, tb, tc = [torch.from_numpy(v.view(np.int32)).to(dev) for v in (a, b, cc)]
    out = torch.full((n + 2,), -1, dtype=torch.int32, device=dev)
    for i in range(n):
        L.check(L.lib.pylc_range_product(L.ptr(ta[i:]), L.ptr(tb[i:]), float(f[i]), L.ptr(tc[i:]) if with_add else None, L.ptr(out[1 + i:]), L.stream()))
    assert out[0].item() == -1 and out[-1].item() == -1
    got = out[1:-1].cpu().numpy().view(np.float32).astype(np.float64)
    exact = f.astype(np.float64) * a.astype(np.float64) * b.astype(np.float64) + (cc.astype(np.float64) if with_add else 0.0)
    assert (got >= exact).all(), 'range_product below the exact bound at %s' % np.nonzero(got < exact)[0][:5]
    assert (got <= (1.0 + 2.0 ** -20) * exact).all(), 'range_product looser than 2^-20: worst %.3g' % (got / exact - 1).max()
    print('PL-G range_product add %d: result / exact - 1 in [%.3g, %.3g]' % (with_add, (got / exact - 1).min(), (got / exact - 1).max()))


# ---- PL-H  one scale rule for writers and readers -----------------------------------------------------------------------------------------
def test_plh_one_plane_reader_uses_the_writers_scale(dev):
    """A one-plane tensor written by pylc_to_planes under a bound of 2^-110 (the clamped scale 2^115) and read by the half depthwise kernel:
    the harness, reference and tolerance of tests/test_round3_gpu.py::test_half_depthwise_kernels_against_fp64."""
    L = _L()
    from pylc_amd import ops
    b, c, h, w = 1, 64, 8, 8
    d = ops._dw_desc(torch.empty(b, c, h, w, device='meta'), 1, 1, c, c)
    assert L.lib.pylc_dwconv3x3_half_ok(C.byref(d))
    x = _scaled_to(P.wide(11, b * h * w, c), -111)
    xb = 2.0 ** -110
    assert float(np.abs(x).max()) <= xb
    s = P.scale_for(P.bits_of(xb))
    assert float(s) == 2.0 ** 115
    _, xv = _dev_f32(x, dev)
    xb_t = _bits(P.bits_of(xb), dev)
    pl = _Planes(dev, b * h * w, c, c, 1, 'sep')
    k_to_planes(xv, c, pl, xb_t)
    h0, _ = P.split(x, s)
    pl.expect(h0, None, 'PL-H to_planes')
    xq = torch.from_numpy(h0.astype(np.float64) / float(s)).view(b, h, w, c)                    # what the kernel must see
    wt = torch.from_numpy(np.random.RandomState(3).standard_normal((c, 1, 3, 3)).astype(np.float32) * 0.4)
    wa = float(wt.abs().max())
    wt_d, wa_t = wt.to(dev), _bits(P.bits_of(wa), dev)
    y_ref = F.conv2d(xq.permute(0, 3, 1, 2), wt.double(), padding=1, groups=c).permute(0, 2, 3, 1)
    rows = L.lib.pylc_dwconv3x3_fwd_h_stats_rows(C.byref(d))
    assert rows > 0
    ybuf, y_h = _hbuf(dev, b * h * w * c)
    yb = torch.zeros(1, dtype=torch.int32, device=dev)
    sums = torch.full((rows, 2 * c), NAN, device=dev)
    L.check(L.lib.pylc_dwconv3x3_fwd_h(C.byref(d), L.ptr(pl.view), L.ptr(xb_t), L.ptr(wt_d), L.ptr(wa_t), L.ptr(y_h), L.ptr(yb), L.ptr(sums), L.stream()))
    bound = float(yb.view(torch.float32).item())
    assert abs(bound - 9 * wa * xb) <= 1e-5 * bound and float(y_ref.abs().max()) <= bound
    got = ybuf.cpu().numpy().view(np.uint16)
    assert (got[:GUARD] == P.FILL16).all() and (got[-GUARD:] == P.FILL16).all()
    y = torch.from_numpy(got[GUARD:-GUARD].view(np.float16).astype(np.float64) / float(P.scale_for(P.bits_of(bound)))).view(b, h, w, c)
    err = (y - y_ref).abs().max().item()
    print('PL-H bound 2^-110: max err / (2^-10 bound) %.3g' % (err / (2.0 ** -10 * bound)))
    assert err <= 2.0 ** -10 * bound            # one fp16 rounding at the tensor's scale (+ fp32 accumulation)
