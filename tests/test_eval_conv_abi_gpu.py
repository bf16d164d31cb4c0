"""The fused inference convolution at the C ABI against the float64 model of tests/_eval_conv.py (-m gpu): pylc_conv2d_fwd_bnact_ex on
fp16-plane tensors in precision modes 2 (f16x3, two planes) and 3 (one plane), and its fp32-tensor sibling pylc_conv2d_fwd_bnact in modes
0 / 1 / 2.  Operands are built on the host as planes (no GPU producer in the loop); every device buffer lies between sentinel regions (fp32:
NaN, halves: 0x7e00) that must be intact after the call, inputs must be bit for bit what was uploaded, and EVERY output element is compared:
    fp32 output     |y - y64| <= TOL mag
    plane output    decoded at the model's placement with the scale of the returned out_bound: |y^ - y64| <= TOL mag + round-trip bound,
                    and the plane bytes equal the split of the SAME call's fp32-output run (one epilogue computes one value before it splits)
    out_bound       one of the model's two bit patterns (affine step contracted or not), and >= the true maximum
    amax_out        the exact bits of max|y| of the fp32-output run, in the plane run too; a larger preset stays, 0 is overwritten
Every case asserts the kernel form it was built to reach through pylc_debug_last_conv_form (tests/_eval_conv.py EX_CASES records the
arithmetic), instead of restating the dispatcher's thresholds.

Each test prints one line `EC <form> mode <m> ...: worst error / (TOL mag)`; profiles/eval_conv_abi.txt keeps those of the implementing run on
an MI355X: at most 0.28 on plane operands (plhn, mode 2), 0.35 on fp32 tensors (bf16x6, the 7x7 shape) -- the starting tolerance is slack by
2.9 x, below the 4 x from which it was to be tightened, so it stays; plane bytes equal to the split of the fp32 run in every case.
A residual whose interleaving differs from the output's cannot be expressed at this ABI: the entry derives both plane strides from ONE rule
(pylc_planes_stride of the same M x Cout), so the two always agree; what the cross product does cover is a plane residual (either layout)
beside an fp32 output."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import _eval_conv as E
from tests import _planes as P

pytestmark = pytest.mark.gpu

GUARD = E.GUARD
NAN = float('nan')
UNSET = -1                                   # what scalar slots and their neighbours hold before a call


def _L():
    from pylc_amd import lib as L
    L.init()
    return L


@pytest.fixture
def set_mode(dev):
    L = _L()
    prev = L.lib.pylc_get_conv_precision()

    def go(mode):
        L.check(L.lib.pylc_set_conv_precision(mode))
    yield go
    L.check(L.lib.pylc_set_conv_precision(prev))


# ---- buffers ----------------------------------------------------------------------------------------------------------------------------------
class _Buf:
    """A device buffer between GUARD sentinel elements (+ `lead` more in front: a deliberately misaligned start), with a copy of what was
    uploaded: `same()` says whether the device still holds exactly that."""

    def __init__(self, dev, values, fill, lead=0):
        values = np.ascontiguousarray(values).ravel()
        host = np.full(values.size + 2 * GUARD + lead, fill, dtype=values.dtype)
        host[GUARD + lead:GUARD + lead + values.size] = values
        as_int = host.view(np.int32 if host.dtype.itemsize == 4 else np.int16)
        self.buf = torch.from_numpy(as_int.copy()).to(dev)
        self.was = self.buf.clone()
        self.view = self.buf[GUARD + lead:GUARD + lead + values.size]
        self.dtype = values.dtype

    def ptr(self, offset=0):
        return self.view.data_ptr() + offset * self.view.element_size()

    def same(self):
        return torch.equal(self.buf, self.was)

    def host(self):
        return self.buf.cpu().numpy().view(self.dtype)


def _f32(dev, values, lead=0):
    return _Buf(dev, np.asarray(values, dtype=np.float32), NAN, lead)


def _u16(dev, values):
    return _Buf(dev, np.asarray(values, dtype=np.uint16), P.FILL16)


class _Scalars:
    """Device uint32 scalars, each between two UNSET words."""

    def __init__(self, dev, **bits):
        self.names = list(bits)
        host = np.full(2 * len(bits) + 1, UNSET, dtype=np.int64)
        host[1::2] = [b if b < 2 ** 31 else b - 2 ** 32 for b in bits.values()]
        self.t = torch.from_numpy(host.astype(np.int32)).to(dev)

    def ptr(self, name):
        return self.t.data_ptr() + 4 * (1 + 2 * self.names.index(name))

    def read(self):
        h = self.t.cpu().numpy()
        assert (h[0::2] == UNSET).all(), 'a word beside a device scalar was written'
        return dict(zip(self.names, (int(v) for v in h[1::2].view(np.uint32))))


# ---- one case on the device --------------------------------------------------------------------------------------------------------------------
_HOST = {}


def _host(geo, mode, x_mult, seed):
    """The operands of a case as planes and the float64 conv sums, computed once per (geometry, mode, x bound)."""
    key = (geo, mode, x_mult, seed)
    if key not in _HOST:
        g = E.Geom(*geo)
        npl = 2 if mode == 2 else 1
        d = E.make_data(g, seed)
        h = dict(g=g, npl=npl, d=d)
        h['x'] = E.Operand(d['x'], E.times_pow2(E.amax_bits(d['x']), x_mult), npl)
        h['w'] = E.Operand(d['w'], E.amax_bits(d['w']), npl)
        h['r'] = E.Operand(d['res'], E.times_pow2(E.amax_bits(d['res']), 2.0), npl)      # a residual scaled under twice its maximum
        h['z'], h['za'] = E.conv64(h['x'].seen, h['w'].seen, g)
        h['wp'] = P.filter_planes(d['w'], h['w'].s, mode == 2)[0]                         # f16x3: chunk-interleaved where Cin % 32 == 0, as the product prepares them
        h['w_fmt'] = 1 if mode == 2 and g.cin % 32 == 0 else 0
        h['xp'] = E.encode_planes(d['x'].reshape(-1, g.cin), h['x'].s, npl)
        h['rp'] = E.encode_planes(d['res'], h['r'].s, npl)
        _HOST.clear()                                                                      # (one case at a time: the large ones hold 100s of MB)
        _HOST[key] = h
    return _HOST[key]


class _Case:
    def __init__(self, dev, geo, mode, x_mult=1.0, seed=3):
        L = self.L = _L()
        h = self.h = _host(geo, mode, x_mult, seed)
        g, d, npl = h['g'], h['d'], h['npl']
        self.g, self.mode, self.npl, self.dev = g, mode, npl, dev
        assert L.lib.pylc_planes_stride(g.b * g.h * g.w, g.cin, npl) == E.planes_stride(g.b * g.h * g.w, g.cin, npl)
        assert L.lib.pylc_planes_stride(g.m, g.cout, npl) == E.planes_stride(g.m, g.cout, npl), 'pylc_planes_stride: not the documented rule'
        self.x, self.wp, self.w32 = _u16(dev, h['xp']), _u16(dev, h['wp']), _f32(dev, d['w'])
        self.res32, self.resp = _f32(dev, d['res']), _u16(dev, h['rp'])
        self.coef = {lead: {k: _f32(dev, d[k], lead) for k in ('scale', 'shift', 'bias')} for lead in (0, 1)}
        self.bits = dict(x=h['x'].bits, x_true=E.amax_bits(d['x']), w=h['w'].bits, scale=E.amax_bits(d['scale']), shift=E.amax_bits(d['shift']),
                         res_scale=h['r'].bits, res=E.amax_bits(d['res']))
        self.inputs = [self.x, self.wp, self.w32, self.res32, self.resp] + [b for c in self.coef.values() for b in c.values()]

    def reference(self, res, bias, relu):
        h, d = self.h, self.h['d']
        seen = None if res == 'none' else (h['r'].seen if res == 'planes' else d['res'].astype(np.float64))
        return E.epilogue64(h['z'], h['za'], d['scale'], d['shift'], d['bias'] if bias else None, seen, relu)

    def call(self, out, res, bias, relu, *, lead=0, x_true=True, w32=False, pitch=None, c0=0, preset=0, res_buf=None, expect_rc=0, breakit=None):
        """One pylc_conv2d_fwd_bnact_ex.  Returns (host copy of the output buffer, scalars read back, form)."""
        L, g = self.L, self.g
        pitch = pitch or g.cout
        sc = _Scalars(self.dev, out_bound=0xFFFFFFFF, amax_out=preset, **self.bits)
        y = _u16(self.dev, np.full(2 * g.m * g.cout, P.FILL16, dtype=np.uint16)) if out == 'planes' else _f32(self.dev, np.full(g.m * pitch, NAN, dtype=np.float32))
        d = L.ConvDesc(g.b, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.dil, g.oh, g.ow, g.cin, pitch)
        d.x_amax, d.w_amax, d.w_planes, d.w_planes_fmt, d.x_fmt = sc.ptr('x'), sc.ptr('w'), self.wp.ptr(), self.h['w_fmt'], 1
        d.out_bound = sc.ptr('out_bound')
        d.out_fmt = 0 if out == 'f32' else (2 if self.mode == 2 else 1)
        ep = L.FwdEp()
        co = self.coef[lead]
        ep.scale, ep.shift, ep.scale_amax, ep.shift_amax = co['scale'].ptr(), co['shift'].ptr(), sc.ptr('scale'), sc.ptr('shift')
        if res != 'none':
            ep.residual = (res_buf or (self.resp if res == 'planes' else self.res32)).ptr(c0 if res_buf else 0)
            ep.res_fmt = 0 if res == 'f32' else (2 if self.mode == 2 else 1)
            ep.res_scale_bound = sc.ptr('res_scale') if res == 'planes' else None
            ep.res_amax = sc.ptr('res')
        ep.x_true_amax = sc.ptr('x_true') if x_true else None
        ep.relu, ep.amax_out = int(relu), sc.ptr('amax_out')
        if breakit:
            breakit(d, ep)
        before = sc.t.clone()
        rc = L.lib.pylc_conv2d_fwd_bnact_ex(C.byref(d), self.x.ptr(), self.w32.ptr() if w32 else None, co['bias'].ptr() if bias else None, C.byref(ep),
                                            y.ptr(c0), L.stream())
        form = L.CONV_FORMS[L.lib.pylc_debug_last_conv_form()]
        torch.cuda.synchronize()
        if expect_rc is None:
            assert rc != 0, 'the call was accepted'
            assert y.same() and torch.equal(sc.t, before), 'a refused call wrote to its outputs'
        else:
            assert rc == 0, L.lib.pylc_last_error().decode()
        for b in self.inputs + ([res_buf] if res_buf else []):
            assert b.same(), 'an input buffer or its guards changed'
        got = sc.read()
        for k, v in self.bits.items():
            assert got[k] == v, 'the input scalar %s changed' % k
        return y.host(), got, form

    def run(self, form, out, res, bias, relu, *, label='', **kw):
        """The fp32-output run of a combination and, for out == 'planes', the plane run of the same call checked against it and the model.
        Returns (fp32 ratio, plane ratio or None)."""
        g = self.g
        what = 'EC %s mode %d %r out %s res %s bias %d relu %d %s' % (form, self.mode, g, out, res, bias, relu, label)
        y64, mag = self.reference(res, bias, relu)
        buf, sc, ran = self.call('f32', res, bias, relu, **kw)
        assert ran == form, '%s: took the %s form' % (what, ran)
        assert sc['out_bound'] == 0xFFFFFFFF, what + ': an fp32 output has no bound to write'
        r32, y32 = E.check_f32(buf, g.m, g.cout, g.cout, 0, y64, mag, what + ' [fp32 run]')
        E.check_amax(sc['amax_out'], y32, what + ' [fp32 run]')
        if out != 'planes':
            return r32, None
        buf, scp, ran = self.call('planes', res, bias, relu, **kw)
        assert ran == form, '%s: the plane run took the %s form' % (what, ran)
        x_true = self.bits['x_true'] if kw.get('x_true', True) else self.bits['x']
        cand = E.bound_candidates(g.klen, x_true, self.bits['w'], self.bits['scale'], self.bits['shift'], self.bits['res'] if res != 'none' else None)
        E.check_bound(scp['out_bound'], cand, np.abs(y32).max(), what)
        rpl = E.check_planes(buf, g.m, g.cout, self.npl, scp['out_bound'], y64, mag, what, same_as=y32)
        assert scp['amax_out'] == sc['amax_out'], what + ': the true maximum of the plane run is not the fp32 run\'s'
        return r32, rpl


def _combos(g, with_bias):
    if g.m <= E.FULL_PRODUCT_MAX_M:
        return list(itertools.product(('f32', 'planes'), ('none', 'f32', 'planes'), (False, True), (False, True)))
    return [('planes', 'planes', False, True),            # planes residual + planes out + relu (on the 3x3 forms: a planes residual on a halo kernel)
            ('f32', 'f32', True, False),                  # fp32 out + bias + fp32 residual
            ('planes', 'planes', True, False),            # bias + planes residual: the general-path combination
            ('planes', 'none', with_bias, True)]          # the plain conv + BatchNorm + ReLU of most layers


def _report(form, mode, g, what, worst):
    print('EC %-12s mode %d %-40r %-24s worst error / (TOL mag): fp32 out %.3f   plane out %.3f   plane bytes == split(fp32 run)' %
          (form, mode, g, what, worst[0], worst[1]))


CASE_IDS = ['%s-%r' % (c[0], E.Geom(*c[1])) for c in E.EX_CASES]


@pytest.mark.parametrize('mode', [2, 3], ids=['f16x3', 'mode3'])
@pytest.mark.parametrize('idx', range(len(E.EX_CASES)), ids=CASE_IDS)
def test_ex_against_float64(dev, set_mode, idx, mode):
    form, geo, with_bias, _ = E.EX_CASES[idx]
    set_mode(mode)
    # the bound x is scaled with: the true maximum (even cases) or twice it (odd cases: the scale bound and the true maximum then differ, which
    # is what tells *x_true_amax from *d->x_amax in the output bound)
    case = _Case(dev, geo, mode, x_mult=2.0 if idx % 2 else 1.0)
    g = case.g
    worst = [0.0, 0.0]

    def take(r):
        worst[0] = max(worst[0], r[0])
        worst[1] = max(worst[1], r[1] or 0.0)
    for n, (out, res, bias, relu) in enumerate(_combos(g, with_bias)):
        take(case.run(form, out, res, bias, relu, w32=(n == 0)))              # (the first combination also hands over the fp32 filter)
    if idx % 2:
        take(case.run(form, 'planes', 'none', True, True, lead=1, label='coefficients off 16-byte alignment'))
        take(case.run(form, 'planes', 'planes', False, True, lead=1, label='coefficients off 16-byte alignment'))
        take(case.run(form, 'planes', 'none', False, True, x_true=False, label='x_true_amax NULL'))
        take(case.run(form, 'planes', 'planes', False, False, x_true=False, label='x_true_amax NULL'))
        # an fp32 output into channels [16, 16 + Cout) of a buffer Cout + 32 wide, the fp32 residual in the same geometry
        pitch = g.cout + 32
        wide = np.full((g.m, pitch), NAN, dtype=np.float32)
        wide[:, 16:16 + g.cout] = case.h['d']['res']
        res_buf = _f32(dev, wide)
        y64, mag = case.reference('f32', True, True)
        buf, sc, ran = case.call('f32', 'f32', True, True, pitch=pitch, c0=16, res_buf=res_buf)
        assert ran == form
        r, y32 = E.check_f32(buf, g.m, g.cout, pitch, 16, y64, mag, 'EC %s mode %d %r channel slice' % (form, mode, g))
        E.check_amax(sc['amax_out'], y32, 'channel slice')
        take((r, None))
    # the true maximum is max-ACCUMULATED: a larger preset stays
    big = P.bits_of(2.0 ** 20)
    for out in ('f32', 'planes'):
        _, sc, _ = case.call(out, 'none', False, True, preset=big)
        assert sc['amax_out'] == big, 'amax_out: a larger preset was overwritten (%s output)' % out
    _report(form, mode, g, 'all combinations', worst)


SMALL = [i for i, c in enumerate(E.EX_CASES) if E.Geom(*c[1]).m <= E.FULL_PRODUCT_MAX_M]


@pytest.mark.parametrize('mode', [2, 3], ids=['f16x3', 'mode3'])
@pytest.mark.parametrize('idx', SMALL, ids=[CASE_IDS[i] for i in SMALL])
def test_ex_under_a_loose_input_bound(dev, set_mode, idx, mode):
    """x split under 4 x its true maximum (two bits fewer in plane 0): the reference follows the planes, the output bound the TRUE maximum."""
    form, geo, _, _ = E.EX_CASES[idx]
    set_mode(mode)
    case = _Case(dev, geo, mode, x_mult=4.0, seed=4)
    worst = [0.0, 0.0]
    for kw in (dict(), dict(x_true=False, label='x_true_amax NULL')):
        for res, bias in (('planes', True), ('none', False)):
            r = case.run(form, 'planes', res, bias, True, **kw)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    _report(form, mode, case.g, 'x bound = 4 max|x|', worst)


# ---- argument errors: refused, and nothing launched -------------------------------------------------------------------------------------------
def _no_res_bound(d, ep):
    ep.res_scale_bound = None


def _no_out_bound(d, ep):
    d.out_bound = None


def _no_scale_amax(d, ep):
    ep.scale_amax = None


def _fp32_x(d, ep):
    d.x_fmt = 0


def _no_scale(d, ep):
    ep.scale = None


@pytest.mark.parametrize('mode', [2, 3], ids=['f16x3', 'mode3'])
def test_ex_refuses_bad_arguments(dev, set_mode, mode):
    set_mode(mode)
    case = _Case(dev, (24, 16, 1, 1, 0, 1, 1, 40, 36), mode)
    for out, res, breakit in (('f32', 'planes', _no_res_bound), ('planes', 'planes', _no_res_bound), ('planes', 'none', _no_out_bound),
                              ('planes', 'none', _no_scale_amax), ('f32', 'none', _fp32_x), ('planes', 'none', _fp32_x), ('f32', 'none', _no_scale),
                              ('planes', 'f32', _no_scale)):
        case.call(out, res, False, True, expect_rc=None, breakit=breakit)
    odd = _Case(dev, (24, 12, 1, 1, 0, 1, 1, 40, 36), mode)                    # Cout % 8 == 4: no partner lane for the last channel quad
    odd.call('planes', 'none', False, True, expect_rc=None)
    odd.call('f32', 'planes', False, True, expect_rc=None)
    buf, sc, form = odd.call('f32', 'f32', True, True)                         # ... while the fp32 form of the same shape runs
    y64, mag = odd.reference('f32', True, True)
    E.check_f32(buf, odd.g.m, 12, 12, 0, y64, mag, 'Cout 12, fp32 output')


# ---- the fp32-tensor sibling --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1, 2], ids=['fp32', 'bf16x6', 'f16x3'])
@pytest.mark.parametrize('idx', range(len(E.F32_CASES)), ids=[repr(E.Geom(*c[0])) for c in E.F32_CASES])
def test_fp32_tensor_form_against_float64(dev, set_mode, idx, mode):
    """pylc_conv2d_fwd_bnact: the operands are the fp32 values themselves; same reference, same tolerance."""
    L = _L()
    geo, pitch, with_bias, _ = E.F32_CASES[idx]
    set_mode(mode)
    g = E.Geom(*geo)
    d = E.make_data(g, 5)
    z, za = E.conv64(d['x'], d['w'], g)
    x, w = _f32(dev, d['x']), _f32(dev, d['w'])
    coef = {k: _f32(dev, d[k]) for k in ('scale', 'shift', 'bias')}
    wide = np.zeros((g.m, pitch), dtype=np.float32)                            # the residual has y's geometry: its padding channels are zeros
    wide[:, :g.cout] = d['res']
    res = _f32(dev, wide)
    worst = 0.0
    for with_res, relu in itertools.product((False, True), (False, True)):
        what = 'EC igemm mode %d %r res %d bias %d relu %d' % (mode, g, with_res, with_bias, relu)
        sc = _Scalars(dev, x=E.amax_bits(d['x']), w=E.amax_bits(d['w']), amax_out=0)
        y = _f32(dev, np.full(g.m * pitch, NAN, dtype=np.float32))
        desc = L.ConvDesc(g.b, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.dil, g.oh, g.ow, g.cin, pitch)
        desc.x_amax, desc.w_amax = sc.ptr('x'), sc.ptr('w')
        L.check(L.lib.pylc_conv2d_fwd_bnact(C.byref(desc), x.ptr(), w.ptr(), coef['bias'].ptr() if with_bias else None, coef['scale'].ptr(), coef['shift'].ptr(),
                                            res.ptr() if with_res else None, int(relu), y.ptr(), sc.ptr('amax_out'), L.stream()))
        form = L.CONV_FORMS[L.lib.pylc_debug_last_conv_form()]
        torch.cuda.synchronize()
        assert form == 'igemm', what + ': took the %s form' % form
        for b in [x, w, res] + list(coef.values()):
            assert b.same(), what + ': an input buffer or its guards changed'
        y64, mag = E.epilogue64(z, za, d['scale'], d['shift'], d['bias'] if with_bias else None, d['res'] if with_res else None, relu)
        r, y32 = E.check_f32(y.host(), g.m, g.cout, pitch, 0, y64, mag, what)
        E.check_amax(sc.read()['amax_out'], y32, what)
        worst = max(worst, r)
    print('EC %-12s mode %d %-40r %-24s worst error / (TOL mag): fp32 out %.3f' % ('igemm', mode, g, 'fp32 tensors', worst))
