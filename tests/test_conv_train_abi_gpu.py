"""The dense convolution's training entries at the C ABI against the float64 model of tests/_conv_train.py (-m gpu): the data gradient
pylc_conv2d_dgrad / pylc_conv2d_dgrad_add on fp16-plane dy in precision modes 2 (f16x3, two planes) and 3 (one plane) and on fp32 tensors in
modes 0 / 1 / 2, the forward pylc_conv2d_fwd / pylc_conv2d_fwd_stats on plane x, and two feeders of the data gradient, pylc_weight_transpose and
pylc_relu_bwd_bits.  Operands are built on the host as planes (no GPU producer in the loop); every device buffer lies between sentinel regions
(fp32: NaN, halves: 0x7e00) that must be intact after the call, inputs -- add_src, the mask bytes and every range scalar included -- must be bit
for bit what was uploaded, and EVERY output element is compared:
    fp32 dx / y      |v - v64| <= TOL_C mag, v64 and mag by epilogue (fresh, accumulate, add, masked add; y = z + bias)
    one-plane dx / y decoded with the scale of the returned out_bound: |v^ - v64| <= TOL_C mag + round-trip bound; out_bound has exactly the bits of
                     float(reduction length) * operand bound * filter bound and is >= the true maximum
    stride 2         pixels no tap reaches: exact zeros (accumulate = 0), `old` bit for bit (accumulate = 1)
    statistics       rows [0, *stats_rows) finite and within the model's bounds per tile (halo forms: the column totals only, their patch order
                     is not documented), everything past them still NaN; y of the statistics run == y of the plain run bit for bit
Every case asserts the kernel form it was built to reach through pylc_debug_last_conv_form (tests/_conv_train.py records the arithmetic).

Which epilogue code the options reach (not asserted): the ragged cases -- pl128 33 x 31, the 252^2 and the 136-channel plhn -- run full and edge
tiles in one launch, i.e. both the lean and the general path of pl_epilogue; the aligned ones (plp, pl256, the 256^2 plhn) the lean path alone.
fresh / accumulate / add / masked add are pl_epilogue_lean<.., PV = 0 / 1 / 2> and the general path's counterparts on the per-tile kernels and
plp_epilogue_lean<0 .. 2> (kinds 0, 2, 3; kind 1 = statistics, the forward case) on the persistent one.

Each check prints one line `CT <entry> <form> mode <m> <geometry> <option>: worst error / (TOL_C mag)`; profiles/conv_train_abi.txt keeps those of
the implementing run on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _conv_train as T
from tests import _eval_conv as E
from tests import _planes as P
from tests.test_eval_conv_abi_gpu import _Buf, _f32, _L, _Scalars, _u16, set_mode      # noqa: F401  (set_mode: a fixture)

pytestmark = pytest.mark.gpu

GUARD = E.GUARD
NAN = float('nan')
DGRAD = 'pylc_conv2d_dgrad_add'


def _bytes(dev, raw):
    """Bytes between 128 guard bytes on either side (as halves, so that _Buf's bit comparison covers them); returns (buffer, device pointer)."""
    raw = np.asarray(raw, dtype=np.uint8).ravel()
    host = np.full(raw.size + (raw.size & 1), 0xA5, dtype=np.uint8)
    host[:raw.size] = raw
    b = _u16(dev, host.view(np.uint16))
    return b, b.ptr()


def _report(entry, form, mode, g, option, ratio):
    print('CT %s %s mode %d %r %s: worst error / (TOL_C mag) %.3f' % (entry, form, mode, g, option, ratio))


def _form(L):
    return L.CONV_FORMS[L.lib.pylc_debug_last_conv_form()]


# ---- the data gradient on plane dy -------------------------------------------------------------------------------------------------------------
_HOST = {}


def _host(idx, mode):
    """The operands of a data-gradient case as planes and the float64 sums, computed once per (case, mode); one case at a time is kept."""
    key = (idx, mode)
    if key not in _HOST:
        form, geo, _ = T.DGRAD_CASES[idx]
        g = E.Geom(*geo)
        npl = 2 if mode == 2 else 1
        assert g.cout % 8 == 0 and g.cin % 8 == 0
        d = T.make_train_data(g, 7)
        h = dict(g=g, npl=npl, d=d, form=form)
        # odd cases: dy split under twice its true maximum
        h['dy'] = E.Operand(d['dy'], E.times_pow2(E.amax_bits(d['dy']), 2.0 if idx % 2 else 1.0), npl)
        h['w'] = E.Operand(d['w'], E.amax_bits(d['w']), npl)
        h['dx'], h['dxa'] = T.dgrad64(h['dy'].seen, h['w'].seen, g)
        h['wt'] = P.filter_planes(d['w'], h['w'].s, mode == 2)[1]                         # chunk-interleaved where Kp % 32 == 0, as the product prepares them
        h['w_fmt'] = 2 if mode == 2 and g.cout % 32 == 0 else 0
        h['dyp'] = E.encode_planes(d['dy'].reshape(-1, g.cout), h['dy'].s, npl)
        _HOST.clear()
        _HOST[key] = h
    return _HOST[key]


class _DCase:
    def __init__(self, dev, idx, mode):
        L = self.L = _L()
        h = self.h = _host(idx, mode)
        g, d = h['g'], h['d']
        self.g, self.mode, self.dev, self.form = g, mode, dev, h['form']
        self.mi = g.b * g.h * g.w
        assert L.lib.pylc_planes_stride(g.m, g.cout, h['npl']) == E.planes_stride(g.m, g.cout, h['npl'])
        self.dy, self.wt, self.w32 = _u16(dev, h['dyp']), _u16(dev, h['wt']), _f32(dev, T.w_crsk(d['w']))
        self.add = _f32(dev, d['add'])
        self.mask, self.mask_ptr = _bytes(dev, d['mask'])
        self.bits = dict(dy=h['dy'].bits, w=h['w'].bits)
        self.inputs = [self.dy, self.wt, self.w32, self.add, self.mask]

    def reference(self, kind):
        h, d = self.h, self.h['d']
        return T.dgrad_epilogue64(h['dx'], h['dxa'], old=d['old'] if kind == 'acc' else None, add=d['add'] if kind in ('add', 'addmask') else None,
                                  mask=d['mask'] if kind == 'addmask' else None)

    def call(self, *, accumulate=0, add=False, mask=False, pitched=False, half=False, dy_fmt=1, planes_t=True, w32='as needed', y_pitch=None,
             refused=False, either=False):
        """One pylc_conv2d_dgrad_add.  Returns (host copy of the dx buffer, scalars, form, rc)."""
        L, g, d_ = self.L, self.g, self.h['d']
        pitch, c0 = (g.cin + 32, 16) if pitched else (g.cin, 0)
        if half:
            out = _u16(self.dev, np.full(2 * self.mi * g.cin, P.FILL16, dtype=np.uint16))
        else:
            host = np.full((self.mi, pitch), NAN, dtype=np.float32)
            if accumulate:
                host[:, c0:c0 + g.cin] = d_['old']
            out = _f32(self.dev, host)
        sc = _Scalars(self.dev, out_bound=0xFFFFFFFF, **self.bits)
        d = L.ConvDesc(g.b, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.dil, g.oh, g.ow, pitch, y_pitch or g.cout)
        d.dy_amax, d.w_amax, d.dy_fmt = sc.ptr('dy'), sc.ptr('w'), dy_fmt
        if planes_t:
            d.w_planes_t, d.w_planes_fmt = self.wt.ptr(), self.h['w_fmt']
        if half:
            d.out_fmt, d.out_bound = 1, sc.ptr('out_bound')
        needs = L.lib.pylc_conv2d_dgrad_needs_f32_weights(C.byref(d))
        # (0 exactly when the prepared planes are all a plane-dy launch reads; 1 in modes 0 / 1 and for a descriptor it cannot vouch for)
        want = 0 if planes_t and dy_fmt == 1 and y_pitch is None and L.lib.pylc_get_conv_precision() >= 2 else 1
        assert needs == want, 'pylc_conv2d_dgrad_needs_f32_weights says %d' % needs
        give = bool(needs) if w32 == 'as needed' else w32
        before = sc.t.clone()
        rc = L.lib.pylc_conv2d_dgrad_add(C.byref(d), self.dy.ptr(), self.w32.ptr() if give else None, out.ptr(c0), int(accumulate),
                                         self.add.ptr() if add else None, self.mask_ptr if mask else None, L.stream())
        form = _form(L)
        torch.cuda.synchronize()
        if refused or (either and rc != 0):
            assert rc != 0, 'the call was accepted'
            assert out.same() and torch.equal(sc.t, before), 'a refused call wrote to its outputs'
        else:
            assert rc == 0, L.lib.pylc_last_error().decode()
        for b in self.inputs:
            assert b.same(), 'an input buffer or its guards changed'
        got = sc.read()
        for k, v in self.bits.items():
            assert got[k] == v, 'the input scalar %s changed' % k
        return out.host(), got, form, rc

    def run(self, kind, *, pitched=False, half=False):
        """One option of the case against the model; returns the worst error / (TOL_C mag)."""
        g = self.g
        option = kind + (' pitched dx' if pitched else '') + (' one-plane dx' if half else '')
        what = 'CT %s %s mode %d %r %s' % (DGRAD, self.form, self.mode, g, option)
        v, mag = self.reference(kind)
        buf, sc, ran, rc = self.call(accumulate=kind == 'acc', add=kind in ('add', 'addmask'), mask=kind == 'addmask', pitched=pitched, half=half,
                                     either=half and self.mode == 2)
        if rc != 0:                                        # (a one-plane output in mode 2: the entry may refuse it, and then has written nothing)
            print(what + ': refused, nothing written')
            return 0.0
        assert ran == self.form, '%s: took the %s form' % (what, ran)
        if half:
            kp = T.roundup4(g.cout)
            E.check_bound(sc['out_bound'], T.product_bound(kp * g.k * g.k, self.bits['dy'], self.bits['w']), np.abs(v).max(), what)
            r = E.check_planes(buf, self.mi, g.cin, 1, sc['out_bound'], v, mag, what, tol=T.TOL_C)
        else:
            assert sc['out_bound'] == 0xFFFFFFFF, what + ': an fp32 output has no bound to write'
            pitch, c0 = (g.cin + 32, 16) if pitched else (g.cin, 0)
            r, y = E.check_f32(buf, self.mi, g.cin, pitch, c0, v, mag, what, tol=T.TOL_C)
            if g.stride == 2:
                T.check_classes(y, self.h['d']['old'], g, kind == 'acc', what)
        _report(DGRAD, self.form, self.mode, g, option, r)
        return r


DGRAD_IDS = ['%s-%r' % (c[0], E.Geom(*c[1])) for c in T.DGRAD_CASES]


@pytest.mark.parametrize('mode', [2, 3], ids=['f16x3', 'mode3'])
@pytest.mark.parametrize('idx', range(len(T.DGRAD_CASES)), ids=DGRAD_IDS)
def test_dgrad_on_planes_against_float64(dev, set_mode, idx, mode):
    set_mode(mode)
    case = _DCase(dev, idx, mode)
    g = case.g
    empty = not T.reached(g).all()
    case.run('fresh')
    case.run('acc')
    if g.stride == 1:
        case.run('addmask')
        if case.mi <= T.FULL_PRODUCT_MAX_M:
            case.run('add')
            case.run('fresh', half=True)
    if idx % 2:
        # channels [16, 16 + Cin) of a Cin + 32 wide NaN buffer
        if g.stride == 2 and empty:                        # zeroing the empty classes of a pitched dx would need a strided fill: refused
            case.call(pitched=True, refused=True)
        else:
            case.run('fresh', pitched=True)
        case.run('acc', pitched=True)


# ---- the data gradient on fp32 tensors ----------------------------------------------------------------------------------------------------------
D32 = [(i, m) for i, c in enumerate(T.DGRAD32_CASES) for m in c[1]]


@pytest.mark.parametrize('idx,mode', D32, ids=['%s-%r-mode%d' % (T.DGRAD32_CASES[i][0], E.Geom(*T.DGRAD32_CASES[i][2]), m) for i, m in D32])
def test_dgrad_on_fp32_tensors_against_float64(dev, set_mode, idx, mode):
    """pylc_conv2d_dgrad with dy_fmt = 0: the operands are the fp32 values themselves; same reference, same tolerance."""
    L = _L()
    form, _, geo, y_pitch, _ = T.DGRAD32_CASES[idx]
    set_mode(mode)
    g = E.Geom(*geo)
    mi, kp = g.b * g.h * g.w, T.roundup4(g.cout)
    d = T.make_train_data(g, 9)
    dx, dxa = T.dgrad64(d['dy'], d['w'], g)
    wide = np.zeros((g.m, y_pitch), dtype=np.float32)                          # channels [Cout, pitch) zero, as the forward writes them
    wide[:, :g.cout] = d['dy'].reshape(g.m, g.cout)
    dy, w32 = _f32(dev, wide), _f32(dev, T.w_crsk(d['w']))
    bits = dict(dy=E.amax_bits(d['dy']), w=E.amax_bits(d['w']))
    wt = _u16(dev, P.filter_planes(d['w'], P.scale_for(bits['w']), True)[1])
    for planes_t in ((True, False) if form == 'pp' else (False,)):
        for acc in (0, 1):
            option = ('accumulate' if acc else 'fresh') + (' w_planes_t' if planes_t else '')
            what = 'CT pylc_conv2d_dgrad %s mode %d %r %s' % (form, mode, g, option)
            sc = _Scalars(dev, **bits)
            host = np.full((mi, g.cin), NAN, dtype=np.float32)
            if acc:
                host[:] = d['old']
            out = _f32(dev, host)
            desc = L.ConvDesc(g.b, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.dil, g.oh, g.ow, g.cin, y_pitch)
            desc.dy_amax, desc.w_amax = sc.ptr('dy'), sc.ptr('w')
            if planes_t:
                desc.w_planes_t, desc.w_planes_fmt = wt.ptr(), 2 if kp % 32 == 0 else 0
            needs = L.lib.pylc_conv2d_dgrad_needs_f32_weights(C.byref(desc))
            assert needs == (0 if planes_t else 1), what + ': pylc_conv2d_dgrad_needs_f32_weights says %d' % needs
            if not needs:
                assert L.lib.pylc_conv2d_dgrad(C.byref(desc), dy.ptr(), None, out.ptr(), acc, L.stream()) == 0, L.lib.pylc_last_error().decode()
            else:
                rc = L.lib.pylc_conv2d_dgrad(C.byref(desc), dy.ptr(), None, out.ptr(), acc, L.stream())      # without the filter it says it needs: refused
                torch.cuda.synchronize()
                assert rc != 0 and out.same(), what + ': ran without the fp32 transposed filter it asked for'
                L.check(L.lib.pylc_conv2d_dgrad(C.byref(desc), dy.ptr(), w32.ptr(), out.ptr(), acc, L.stream()))
            ran = _form(L)
            torch.cuda.synchronize()
            assert ran == form, '%s: took the %s form' % (what, ran)
            for b in (dy, w32, wt):
                assert b.same(), what + ': an input buffer or its guards changed'
            assert sc.read() == bits, what + ': an input scalar changed'
            v, mag = T.dgrad_epilogue64(dx, dxa, old=d['old'] if acc else None)
            r, y = E.check_f32(out.host(), mi, g.cin, g.cin, 0, v, mag, what, tol=T.TOL_C)
            if g.stride == 2:
                T.check_classes(y, d['old'], g, acc, what)
            _report('pylc_conv2d_dgrad', form, mode, g, option, r)


# ---- the forward and its statistics ---------------------------------------------------------------------------------------------------------------
_FHOST = {}


def _fwd_host(geo, mode):
    key = (geo, mode)
    if key not in _FHOST:
        g = E.Geom(*geo)
        npl = 2 if mode == 2 else 1
        d = E.make_data(g, 13)
        h = dict(g=g, npl=npl, d=d)
        h['x'] = E.Operand(d['x'], E.amax_bits(d['x']), npl)
        h['w'] = E.Operand(d['w'], E.amax_bits(d['w']), npl)
        h['z'], h['za'] = E.conv64(h['x'].seen, h['w'].seen, g)
        h['wp'] = P.filter_planes(d['w'], h['w'].s, mode == 2)[0]
        h['w_fmt'] = 1 if mode == 2 and g.cin % 32 == 0 else 0
        h['xp'] = E.encode_planes(d['x'].reshape(-1, g.cin), h['x'].s, npl)
        _FHOST.clear()
        _FHOST[key] = h
    return _FHOST[key]


FWD = [(i, m) for i, c in enumerate(T.FWD_CASES) for m in c[1]]


def _fwd_id(i, m):
    form, _, geo, stats, bias, out_fmt, _ = T.FWD_CASES[i]
    return '%s-%r-stats%d-bias%d-out%d-mode%d' % (form, E.Geom(*geo), stats, bias, out_fmt, m)


@pytest.mark.parametrize('idx,mode', FWD, ids=[_fwd_id(i, m) for i, m in FWD])
def test_fwd_and_statistics_against_float64(dev, set_mode, idx, mode):
    L = _L()
    form, _, geo, with_stats, with_bias, out_fmt, _ = T.FWD_CASES[idx]
    set_mode(mode)
    h = _fwd_host(geo, mode)
    g, d = h['g'], h['d']
    x, wp = _u16(dev, h['xp']), _u16(dev, h['wp'])
    bias_h = None
    if with_bias:
        bias_h = T.big_bias(h['z'], g.cout, 1) if with_stats else d['bias']
    bias = _f32(dev, bias_h) if with_bias else None
    bits = dict(x=h['x'].bits, w=h['w'].bits)
    y64 = h['z'] + (bias_h.astype(np.float64) if with_bias else 0.0)
    mag = h['za'] + (np.abs(bias_h.astype(np.float64)) if with_bias else 0.0)
    opt = ('statistics' if with_stats else 'plain') + (' bias' if with_bias else '') + (' one-plane y' if out_fmt else '')

    def launch(stats):
        sc = _Scalars(dev, out_bound=0xFFFFFFFF, **bits)
        y = _u16(dev, np.full(2 * g.m * g.cout, P.FILL16, dtype=np.uint16)) if out_fmt else _f32(dev, np.full(g.m * g.cout, NAN, dtype=np.float32))
        desc = L.ConvDesc(g.b, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.dil, g.oh, g.ow, g.cin, g.cout)
        desc.x_amax, desc.w_amax, desc.w_planes, desc.w_planes_fmt, desc.x_fmt = sc.ptr('x'), sc.ptr('w'), wp.ptr(), h['w_fmt'], 1
        if out_fmt:
            desc.out_fmt, desc.out_bound = 1, sc.ptr('out_bound')
        st = rows = None
        if stats:
            floats = L.lib.pylc_conv2d_fwd_stats_floats(C.byref(desc))
            assert floats == -(-g.m // 128) * 2 * T.roundup4(g.cout)
            st, rows = _f32(dev, np.full(floats, NAN, dtype=np.float32)), C.c_int(-1)
            L.check(L.lib.pylc_conv2d_fwd_stats(C.byref(desc), x.ptr(), None, bias.ptr() if bias else None, y.ptr(), st.ptr(), C.byref(rows), L.stream()))
        else:
            L.check(L.lib.pylc_conv2d_fwd(C.byref(desc), x.ptr(), None, bias.ptr() if bias else None, y.ptr(), L.stream()))
        ran = _form(L)
        torch.cuda.synchronize()
        what = 'CT %s %s mode %d %r %s' % ('pylc_conv2d_fwd_stats' if stats else 'pylc_conv2d_fwd', form, mode, g, opt)
        assert ran == form, '%s: took the %s form' % (what, ran)
        for b in [x, wp] + ([bias] if bias else []):
            assert b.same(), what + ': an input buffer or its guards changed'
        got = sc.read()
        assert {k: got[k] for k in bits} == bits, what + ': an input scalar changed'
        return y.host(), got, (st.host() if stats else None), (rows.value if stats else None), what

    buf, sc, _, _, what = launch(False)
    if out_fmt:
        E.check_bound(sc['out_bound'], T.product_bound(g.klen, bits['x'], bits['w']), np.abs(y64).max(), what)
        r = E.check_planes(buf, g.m, g.cout, 1, sc['out_bound'], y64, mag, what, tol=T.TOL_C)
    else:
        assert sc['out_bound'] == 0xFFFFFFFF
        r, _ = E.check_f32(buf, g.m, g.cout, g.cout, 0, y64, mag, what, tol=T.TOL_C)
    _report('pylc_conv2d_fwd', form, mode, g, opt.replace('statistics', 'plain'), r)
    if with_stats:
        buf2, _, st, rows, what = launch(True)
        assert np.array_equal(buf2.view(np.uint32), buf.view(np.uint32)), what + ': y differs from the plain run\'s'
        floats = st.size - 2 * GUARD
        rs = T.check_stats(st, floats, rows, g.cout, h['z'], h['za'], what, halo=form in ('plh', 'plhn'))
        print('CT pylc_conv2d_fwd_stats %s mode %d %r %s (%d rows): worst statistics error / bound %.3f' % (form, mode, g, opt, rows, rs))


# ---- argument errors: refused, and nothing written -------------------------------------------------------------------------------------------------
S1_IDX = 14            # (64, 64, 3x3, stride 1) 20 x 24
S2_IDX = 11            # the stride-2 1x1 shortcut: three empty classes


def test_dgrad_refuses_bad_arguments(dev, set_mode):
    set_mode(2)
    one = _DCase(dev, S1_IDX, 2)
    one.call(add=True, accumulate=1, refused=True)
    one.call(add=True, pitched=True, refused=True)
    one.call(mask=True, refused=True)                                           # add_mask without add_src
    one.call(half=True, accumulate=1, refused=True)
    one.call(planes_t=False, w32=False, refused=True)                           # no filter at all
    one.call(add=True, dy_fmt=0, planes_t=False, refused=True)                  # add_src with fp32 dy (the pointer then stands for an fp32 dy: refused before any read)
    one.call(y_pitch=56, refused=True)                                          # dy pitch below roundup4(Cout)
    two = _DCase(dev, S2_IDX, 2)
    two.call(add=True, refused=True)
    two.call(half=True, refused=True)
    two.call(pitched=True, refused=True)
    for mode in (0, 1):                                                         # plane dy needs precision mode 2 or 3
        set_mode(mode)
        one.call(refused=True)
        one.call(accumulate=1, refused=True)


def test_fwd_refuses_a_plane_output_with_a_bias(dev, set_mode):
    L = _L()
    set_mode(3)
    h = _fwd_host((64, 64, 3, 1, 0, 1, 1, 20, 20), 3)
    g = h['g']
    x, wp, bias = _u16(dev, h['xp']), _u16(dev, h['wp']), _f32(dev, h['d']['bias'])
    sc = _Scalars(dev, out_bound=0xFFFFFFFF, x=h['x'].bits, w=h['w'].bits)
    y = _u16(dev, np.full(2 * g.m * g.cout, P.FILL16, dtype=np.uint16))
    desc = L.ConvDesc(g.b, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.dil, g.oh, g.ow, g.cin, g.cout)
    desc.x_amax, desc.w_amax, desc.w_planes, desc.x_fmt, desc.out_fmt, desc.out_bound = sc.ptr('x'), sc.ptr('w'), wp.ptr(), 1, 1, sc.ptr('out_bound')
    before = sc.t.clone()
    rc = L.lib.pylc_conv2d_fwd(C.byref(desc), x.ptr(), None, bias.ptr(), y.ptr(), L.stream())
    torch.cuda.synchronize()
    assert rc != 0 and y.same() and torch.equal(sc.t, before)
    L.check(L.lib.pylc_conv2d_fwd(C.byref(desc), x.ptr(), None, None, y.ptr(), L.stream()))      # ... while the same call without the bias runs
    torch.cuda.synchronize()
    assert sc.read()['out_bound'] in T.product_bound(g.klen, h['x'].bits, h['w'].bits)


# ---- two feeders ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [4, 72])
@pytest.mark.parametrize('rs', [1, 9])
@pytest.mark.parametrize('k', [9, 64, 136])
def test_weight_transpose_is_the_numpy_transpose(dev, k, rs, c):
    L = _L()
    w = np.random.RandomState(k * 100 + rs * 10 + c).standard_normal((k, rs, c)).astype(np.float32)
    want = T.w_crsk(w)
    src, dst = _f32(dev, w), _f32(dev, np.full(want.size, NAN, dtype=np.float32))
    L.check(L.lib.pylc_weight_transpose(src.ptr(), dst.ptr(), k, rs, c, L.stream()))
    torch.cuda.synchronize()
    assert src.same()
    got = dst.host()
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + want.size:]).all(), 'a guard around the transposed filter was written'
    assert np.array_equal(got[GUARD:GUARD + want.size].view(np.uint32), want.ravel().view(np.uint32))


@pytest.mark.parametrize('c', [8, 72, 256])
@pytest.mark.parametrize('m', [1, 127, 4096])
def test_relu_bwd_bits_selects_by_the_mask(dev, m, c):
    L = _L()
    r = np.random.RandomState(m + c)
    dout = r.standard_normal((m, c)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 2.0 ** -140], dtype=np.float32)
    at = r.randint(0, m * c, max(8, m * c // 16))
    dout.ravel()[at] = special[r.randint(0, special.size, at.size)]
    bits = r.random_sample((m, c)) < 0.55
    raw = T.pack_mask(bits)
    assert np.array_equal(T.mask_bits(raw, m, c), bits)
    src, dst = _f32(dev, dout), _f32(dev, np.full(m * c, NAN, dtype=np.float32))
    mask, mask_ptr = _bytes(dev, raw)
    L.check(L.lib.pylc_relu_bwd_bits(src.ptr(), mask_ptr, dst.ptr(), m, c, L.stream()))
    torch.cuda.synchronize()
    assert src.same() and mask.same()
    got = dst.host()
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + m * c:]).all(), 'a guard around g_out was written'
    gu = got[GUARD:GUARD + m * c].view(np.uint32).reshape(m, c)
    du = dout.view(np.uint32)
    if not np.array_equal(gu[bits], du[bits]):
        i = E._first(bits & (gu != du))
        raise AssertionError('g_out%s is %#010x where the bit is set, dout is %#010x' % (i, gu[i], du[i]))
    if not (gu[~bits] << 1 == 0).all():                                          # +0 or -0, never NaN * 0
        i = E._first(~bits & (gu << 1 != 0))
        raise AssertionError('g_out%s is %#010x where the bit is clear (dout %#010x)' % (i, gu[i], du[i]))
