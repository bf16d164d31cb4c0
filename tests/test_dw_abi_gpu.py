"""The kernels of pylc_amd/csrc/dwconv.hip at the C ABI (ctypes only) against the statements, bounds and bit-exact models of tests/_dw.py
(-m gpu).  Every tensor lies in a NaN-filled buffer with two guard rows before and after; the fp32 entry points
get x_pitch = C + 4 and y_pitch = C + 8: gaps and guards must stay NaN and the outputs must hold no NaN, so a read of a gap shows up.  The
half entry points are dense, in fp16-NaN (P.FILL16) guards, and run under pylc_debug_dw_tiles(3) and (0).  Errors are judged per element
against the derived bound, or bit for bit (the sign of a zero aside, as the header allows); no tolerance is tuned to the device's output.

Sections print their worst figure as error / bound (1.0 = at the bound):
  DW-A  pylc_dwconv3x3_fwd / _fwd_stats / _dgrad / _dgrad_acc: bit-equal to the float32 model, within the bound of fp64; statistics rows
  DW-B  pylc_dwconv3x3_wgrad: per tap within the derived bound; workspace rows beyond those used untouched; the workspace refusal
  DW-C  one-hot filters: fp32 y and dx equal the shifted operand; the halves equal the exactly known rounding, ties included
  DW-D  pylc_dwconv3x3_fwd_h / _fwd_h_eval: the bound's bits, the halves' bits, the statistics of the stored halves
  DW-E  pylc_dwconv3x3_dgrad_h in its four forms and _dgrad_h_add
  DW-F  pylc_dwconv3x3_wgrad_h, with the small corner of the window of bounds
  DW-G  the _bn forms against pylc_bn_apply_ex + the plain forms: torch.equal
  DW-H  the eligibility predicates and statistics-row counts against the yardstick's statement; the refusal of an ineligible shape
The implementing run on an MI355X, worst over the cases of each section:
  DW-A  bit-equal to the float32 model in all 13 cases; fwd 0.941 (two strips per block), dgrad 0.989 (stride 2), fwd_stats sums 0.274 (C 1028)
  DW-B  0.264 (C 1028), 0.142 with two strips per thread; the 200 x 1 x 9 x 8 case writes 4 rows where make_slab counts 2 (342 x 5 x 2 x 1024:
        513 against 428): the parent's size check let such a launch into a workspace of less, fixed in this change
  DW-C  exact everywhere
  DW-D  bound and halves bit-equal in all 15 runs; 1.000 (bound1 is attained at ties); statistics 0.150
  DW-E  bit-equal in every form; 1.000 half, 0.999 fp32 (stride 2, 136 channels)
  DW-F  0.191; the small corner 0.090 (tiled) / 0.119 (strips)
  DW-G  identical          DW-H  37 descriptors x 4 knob values agree (W == 1 joined pylc_dwconv3x3_half_ok in this change)
The 91 cases took 6.1 s together in that run (pytest's own total on the GPU host, float64 references included; the slowest, 0.9 s, is the
two-strips-per-block case of DW-A).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _dw as D
from tests import _planes as P

pytestmark = pytest.mark.gpu

NAN = float('nan')
GR = 2                          # guard rows
ERR_ARG, ERR_WORKSPACE = 1, 3


def _L():
    from pylc_amd import lib as L
    L.init()
    return L


class _T:
    """rows x c values at `pitch` inside a NaN-filled buffer with GR guard rows on either side (float16: the pattern P.FILL16)."""

    def __init__(self, dev, rows, c, pitch=None, a=None, dtype=torch.float32):
        self.rows, self.c, self.pitch = rows, c, pitch or c
        self.buf = torch.full((rows + 2 * GR, self.pitch), NAN, dtype=dtype, device=dev)
        self.v = self.buf[GR:GR + rows, :c]
        if a is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(rows, c)))
        assert self.v.data_ptr() % 16 == 0 or c % 4

    def untouched(self):
        return bool(torch.isnan(self.v).all())

    def get(self, what, shape=None):
        assert torch.isnan(self.buf[:GR]).all() and torch.isnan(self.buf[GR + self.rows:]).all(), '%s: a guard row was written' % what
        assert torch.isnan(self.buf[:, self.c:]).all(), '%s: a lane beyond C was written' % what
        a = self.v.contiguous().cpu().numpy()
        return a.reshape(shape) if shape else a


def test_fill_pattern(dev):
    assert int(torch.full((1,), NAN, dtype=torch.float16, device=dev).view(torch.int16).item()) == P.FILL16


def _ratio(got, ref, bound, what):
    got = np.asarray(got)
    assert not np.isnan(got).any(), '%s: NaN in the output' % what
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError('%s: element %s is %.9g, fp64 says %.9g: err %.4g > bound %.4g; %d over the bound' %
                             (what, i, got[i], ref[i], err[i], bound[i], int(bad.sum())))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _same_bits(got, want, what):
    """float32 (-0 cleared) or float16 (P.canon) patterns."""
    if np.asarray(got).dtype == np.float16:
        g, w = P.canon(np.ascontiguousarray(got).view(np.uint16)), P.canon(np.ascontiguousarray(want, dtype=np.float16).view(np.uint16))
    else:
        g, w = D.canon32(got).view(np.uint32), D.canon32(want).view(np.uint32)
    if not np.array_equal(g, w):
        i = tuple(int(k[0]) for k in np.nonzero(g != w))
        raise AssertionError('%s: element %s is %#x, the model says %#x; %d differ' % (what, i, g[i], w[i], int((g != w).sum())))


def _desc(L, d):
    return L.DwDesc(d.B, d.H, d.W, d.C, d.stride, d.dil, d.OH, d.OW, d.x_pitch, d.y_pitch)


def _scalar(dev, bits):
    return torch.from_numpy(np.array([bits], dtype=np.uint32).view(np.int32)).to(dev)


class _Out:
    """A device scalar an entry point writes, between two words that must stay as they are."""

    def __init__(self, dev):
        self.t = torch.full((3,), -1, dtype=torch.int32, device=dev)
        self.p = self.t[1:]

    def bits(self, what):
        a = self.t.cpu().numpy()
        assert a[0] == -1 and a[2] == -1, '%s: a word next to the bound was written' % what
        return int(a[1:2].view(np.uint32)[0])

    def untouched(self):
        return bool((self.t == -1).all())


def _ids(c):
    return 'x'.join(map(str, c))


def _pitched(case):
    return D.Desc(*case, x_pitch=case[3] + 4, y_pitch=case[3] + 8)


def _f32_inputs(case, seed=0):
    d = D.Desc(*case)
    x, _ = D.wide(seed + 1, (d.B, d.H, d.W, d.C))
    dy, _ = D.wide(seed + 2, (d.B, d.OH, d.OW, d.C), mag=2.0 ** -8)
    w, _ = D.filt(seed + 3, d.C)
    return x, dy, w


def _wt(dev, w):
    return torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32).reshape(-1, 9)).to(dev)


def _sum_rows(st, rows, c, what):
    a = st.get(what, (rows, 2, c))
    assert np.isfinite(a).all(), '%s: a statistics row is not finite' % what
    a = a.astype(np.float64).sum(0)
    return a[0], a[1]


def _check_stats(st, rows, stored, d, path, what):
    s1, s2 = _sum_rows(st, rows, d.C, what)
    r1, r2, _ = D.stats64(stored)
    b1, b2 = D.stats_bound(stored, d, path)
    return max(_ratio(s1, r1, b1, what + ' sum'), _ratio(s2, r2, b2, what + ' sum of squares'))


# ---- DW-A  the fp32 forward and data gradient -----------------------------------------------------------------------------------------------------
def _dwa(dev, d, x, dy, w, what='DW-A'):
    L = _L()
    lib, dd = L.lib, _desc(L, d)
    wt = _wt(dev, w)
    xt, dyt = _T(dev, d.B * d.H * d.W, d.C, d.x_pitch, x), _T(dev, d.B * d.OH * d.OW, d.C, d.y_pitch, dy)
    worst = {}
    rows = lib.pylc_dwconv3x3_fwd_stats_rows(C.byref(dd))
    assert rows == D.f32_stats_rows(d) and (rows > 0) == (D.f32_path(d) == 'strip')

    def cmp(got, e, name):
        _same_bits(got, e.out, '%s %s' % (what, name))
        worst[name] = _ratio(got, e.ref, e.bound, '%s %s' % (what, name))

    e = D.expect_fwd(x, w, d)
    yt = _T(dev, d.B * d.OH * d.OW, d.C, d.y_pitch)
    L.check(lib.pylc_dwconv3x3_fwd(C.byref(dd), L.ptr(xt.v), L.ptr(wt), L.ptr(yt.v), L.stream()))
    y = yt.get(what + ' y', (d.B, d.OH, d.OW, d.C))
    cmp(y, e, 'fwd')
    yt2, st = _T(dev, d.B * d.OH * d.OW, d.C, d.y_pitch), _T(dev, max(rows, 1), 2 * d.C)
    rc = lib.pylc_dwconv3x3_fwd_stats(C.byref(dd), L.ptr(xt.v), L.ptr(wt), L.ptr(yt2.v), L.ptr(st.v), L.stream())
    if rows:
        L.check(rc)
        _same_bits(yt2.get(what + ' fwd_stats y', y.shape), y, what + ' fwd_stats y against fwd')
        worst['stats'] = _check_stats(st, rows, y, d, 'strip', what + ' fwd_stats')          # the row after the last is a guard row
    else:
        assert rc == ERR_ARG and yt2.untouched() and st.untouched(), what + ': fwd_stats on a shape without a fused form'
    xt.get(what + ' x')
    del e
    for name, acc in (('dgrad', None), ('dgrad_acc 0', 0), ('dgrad_acc 1', 1)):
        old = D.wide(9, x.shape)[0] if acc else None
        if acc != 0:                                   # dgrad and dgrad_acc 0 share one expectation
            e = D.expect_dgrad(dy, w, d, old)
        dxt = _T(dev, d.B * d.H * d.W, d.C, d.x_pitch, old)
        if acc is None:
            L.check(lib.pylc_dwconv3x3_dgrad(C.byref(dd), L.ptr(dyt.v), L.ptr(wt), L.ptr(dxt.v), L.stream()))
        else:
            L.check(lib.pylc_dwconv3x3_dgrad_acc(C.byref(dd), L.ptr(dyt.v), L.ptr(wt), L.ptr(dxt.v), acc, L.stream()))
        cmp(dxt.get('%s %s' % (what, name), x.shape), e, name)
    dyt.get(what + ' dy')
    return worst


@pytest.mark.parametrize('case', D.F32_CASES, ids=_ids)
def test_dwa_fp32_forward_and_data_gradient(dev, case):
    d = _pitched(case)
    worst = _dwa(dev, d, *_f32_inputs(case))
    print('DW-A %-18s %-7s bit-equal to the float32 model; err / bound %s' %
          (_ids(case), D.f32_path(d), '  '.join('%s %.3f' % kv for kv in worst.items())))


def test_dwa_two_strips_per_block(dev):
    """strips_per_block = 2: every thread of the strip kernels walks two strips (D.F32_SPB2 says why this shape stands for the 67 MB one).
    Pitched like the other cases; every entry point, every element."""
    d = _pitched(D.F32_SPB2)
    st = D.make_strips(d, D.make_slab(d.B * d.H * d.W, d.C))
    assert st.strips_per_block == 2 and st.blocks < st.n_strips
    worst = _dwa(dev, d, *_f32_inputs(D.F32_SPB2), what='DW-A spb 2')
    print('DW-A %s: bit-equal to the float32 model; err / bound %s' % (_ids(D.F32_SPB2), '  '.join('%s %.3f' % kv for kv in worst.items())))


# ---- DW-B  the fp32 filter gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', D.F32_CASES + [D.WS_CASE, D.F32_SPB2], ids=_ids)
def test_dwb_fp32_filter_gradient(dev, case):
    L = _L()
    d = _pitched(case)
    lib, dd = L.lib, _desc(L, d)
    x, dy, _ = _f32_inputs(case)
    what = 'DW-B ' + _ids(case)
    path = D.f32_path(d)
    used = D.depths(d, path, 2)[0]
    nbytes = lib.pylc_dwconv3x3_wgrad_workspace(C.byref(dd))
    assert nbytes == D.SLABS * 9 * d.C * 4 and used <= D.SLABS
    xt, dyt = _T(dev, d.B * d.H * d.W, d.C, d.x_pitch, x), _T(dev, d.B * d.OH * d.OW, d.C, d.y_pitch, dy)
    ws, dwt = _T(dev, D.SLABS, 9 * d.C), _T(dev, d.C, 9)
    rc = lib.pylc_dwconv3x3_wgrad(C.byref(dd), L.ptr(xt.v), L.ptr(dyt.v), L.ptr(dwt.v), L.ptr(ws.v), used * 9 * d.C * 4 - 4, L.stream())
    assert rc == ERR_WORKSPACE and dwt.untouched() and ws.untouched(), what + ': a workspace one word short'
    L.check(lib.pylc_dwconv3x3_wgrad(C.byref(dd), L.ptr(xt.v), L.ptr(dyt.v), L.ptr(dwt.v), L.ptr(ws.v), nbytes, L.stream()))
    rows = ws.get(what + ' workspace')
    assert not np.isnan(rows[:used]).any() and np.isnan(rows[used:]).all(), what + ': workspace rows beyond the %d used were written' % used
    r = _ratio(dwt.get(what + ' dw'), D.wgrad64(x, dy, d.stride, d.dil), D.wgrad_bound(x, dy, d, path), what)
    xt.get(what + ' x'), dyt.get(what + ' dy')
    print('DW-B %-18s %-7s %4d workspace rows; err / bound %.3f' % (_ids(case), path, used, r))


# ---- half harness -----------------------------------------------------------------------------------------------------------------------------------
class _Knob:
    def __init__(self, L, knob):
        self.L, self.knob = L, knob

    def __enter__(self):
        self.L.lib.pylc_debug_dw_tiles(self.knob)

    def __exit__(self, *a):
        self.L.lib.pylc_debug_dw_tiles(3)


def _ht(dev, rows, c, a=None):
    return _T(dev, rows, c, None, a, dtype=torch.float16)


HALF_RUNS = [(c, k) for c in D.HALF_CASES for k in (3, 0) if D.half_path(D.Desc(*c), k)]
# the path property each case exists for
assert [D.half_path(D.Desc(*c), k) for c, k in HALF_RUNS] == ['tile', 'strip', 'tile', 'strip', 'tile', 'strip', 'strip', 'strip', 'tile'] + ['tileg'] * 5


def _half_ids(v):
    return _ids(v) if isinstance(v, tuple) else 'knob%d' % v


def _fwd_h(L, dev, d, xh, w, wa, stats=True, true_bits=None, what=''):
    """One pylc_dwconv3x3_fwd_h (true_bits: _fwd_h_eval) launch: (halves, bound bits, statistics buffer, rows)."""
    lib, dd = L.lib, _desc(L, d)
    m = d.B * d.OH * d.OW
    xt, yt, yb = _ht(dev, d.B * d.H * d.W, d.C, xh.h), _ht(dev, m, d.C), _Out(dev)
    xb, wab, wt = _scalar(dev, xh.bits), _scalar(dev, wa), _wt(dev, w)
    rows = lib.pylc_dwconv3x3_fwd_h_stats_rows(C.byref(dd))
    st = _T(dev, max(rows, 1), 2 * d.C) if stats else None
    if true_bits is None:
        L.check(lib.pylc_dwconv3x3_fwd_h(C.byref(dd), L.ptr(xt.v), L.ptr(xb), L.ptr(wt), L.ptr(wab), L.ptr(yt.v), L.ptr(yb.p),
                                         L.ptr(st.v) if stats else None, L.stream()))
    else:
        tb = _scalar(dev, true_bits)
        L.check(lib.pylc_dwconv3x3_fwd_h_eval(C.byref(dd), L.ptr(xt.v), L.ptr(xb), L.ptr(tb), L.ptr(wt), L.ptr(wab), L.ptr(yt.v), L.ptr(yb.p), L.stream()))
    torch.cuda.synchronize()
    xt.get(what + ' x')
    return yt.get(what + ' y', (d.B, d.OH, d.OW, d.C)), yb.bits(what), st, rows


# ---- DW-C  one-hot filters --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(2, 5, 7, 8, 1, 1), (2, 7, 9, 16, 2, 1), (1, 9, 10, 24, 1, 2)], ids=_ids)
def test_dwc_one_hot_fp32(dev, case):
    L = _L()
    d = _pitched(case)
    lib, dd = L.lib, _desc(L, d)
    x, dy, _ = _f32_inputs(case)
    xt, dyt = _T(dev, d.B * d.H * d.W, d.C, d.x_pitch, x), _T(dev, d.B * d.OH * d.OW, d.C, d.y_pitch, dy)
    ft, gt = D.fwd_terms(x, d.stride, d.dil), D.dgrad_terms(dy, d.H, d.W, d.stride, d.dil)
    for tap in range(9):
        wt = _wt(dev, D.one_hot(d.C, tap, 1.0)[0])
        yt, dxt = _T(dev, d.B * d.OH * d.OW, d.C, d.y_pitch), _T(dev, d.B * d.H * d.W, d.C, d.x_pitch)
        L.check(lib.pylc_dwconv3x3_fwd(C.byref(dd), L.ptr(xt.v), L.ptr(wt), L.ptr(yt.v), L.stream()))
        L.check(lib.pylc_dwconv3x3_dgrad(C.byref(dd), L.ptr(dyt.v), L.ptr(wt), L.ptr(dxt.v), L.stream()))
        _same_bits(yt.get('DW-C y', dy.shape), ft[tap][0], 'DW-C %s tap %d: y against the shifted x' % (_ids(case), tap))
        _same_bits(dxt.get('DW-C dx', x.shape), gt[tap][0], 'DW-C %s tap %d: dx against the shifted dy' % (_ids(case), tap))
    print('DW-C %s fp32: y and dx equal the shifted operand for all nine taps' % _ids(case))


@pytest.mark.parametrize('case,knob', [((1, 9, 17, 8, 1, 1), 3), ((1, 9, 17, 8, 1, 1), 0), ((1, 8, 32, 8, 2, 1), 3), ((1, 8, 16, 8, 1, 2), 3)],
                         ids=_half_ids)
def test_dwc_one_hot_half(dev, case, knob):
    L = _L()
    d = D.Desc(*case)
    lib, dd = L.lib, _desc(L, d)
    xh = D.wide_half(1, (d.B, d.H, d.W, d.C))
    dyh = D.wide_half(2, (d.B, d.OH, d.OW, d.C), 2.0 ** -8)
    ft, gt = D.fwd_terms(xh.h, d.stride, d.dil), D.dgrad_terms(dyh.h, d.H, d.W, d.stride, d.dil)
    ties = 0
    with _Knob(L, knob):
        for val in (1.0, 1.5):
            for tap in range(9):
                w, wa = D.one_hot(d.C, tap, val)
                what = 'DW-C %s knob %d tap %d value %.1f' % (_ids(case), knob, tap, val)
                y, bits, _, _ = _fwd_h(L, dev, d, xh, w, wa, stats=False, what=what)
                assert bits == D.bound_bits(val, P.float_of(xh.bits)), what
                exact = ft[tap][0].astype(np.float64) * val * (float(P.scale_for(bits)) / float(xh.s))
                _same_bits(y, exact.astype(np.float16), what + ': y against the one rounding of the exact value')
                ties += int((exact.astype(np.float16).astype(np.float64) != exact).sum())
                dyt, dxt, db = _ht(dev, d.B * d.OH * d.OW, d.C, dyh.h), _ht(dev, d.B * d.H * d.W, d.C), _Out(dev)
                dyb, wab, wt = _scalar(dev, dyh.bits), _scalar(dev, wa), _wt(dev, w)
                L.check(lib.pylc_dwconv3x3_dgrad_h(C.byref(dd), L.ptr(dyt.v), L.ptr(dyb), L.ptr(wt), L.ptr(wab), L.ptr(dxt.v), L.ptr(db.p), 0, None, L.stream()))
                bits = db.bits(what)
                assert bits == D.bound_bits(val, P.float_of(dyh.bits)), what
                exact = gt[tap][0].astype(np.float64) * val * (float(P.scale_for(bits)) / float(dyh.s))
                _same_bits(dxt.get(what + ' dx', exact.shape), exact.astype(np.float16), what + ': dx against the one rounding of the exact value')
    print('DW-C %s knob %d half: 2 x 9 taps equal the exactly known halves (%d of the forward outputs are rounded)' % (_ids(case), knob, ties))


# ---- DW-D  the half forward ---------------------------------------------------------------------------------------------------------------------------
def _dwd(dev, case, knob, mults=(1.0, 128.0)):
    L = _L()
    d = D.Desc(*case)
    path = D.half_path(d, knob)
    w, wa = D.filt(3, d.C)
    worst = {}
    with _Knob(L, knob):
        for mult in mults:
            what = 'DW-D %s knob %d bound x%g' % (_ids(case), knob, mult)
            xh = D.wide_half(1, (d.B, d.H, d.W, d.C), mult=mult)
            e = D.expect_fwd_h(xh, w, wa, d, path)
            y, bits, st, rows = _fwd_h(L, dev, d, xh, w, wa, what=what)
            assert rows == D.half_stats_rows(d, knob) and rows > 0, what
            assert bits == e.bits, '%s: y_bound_out is %#x, the header says %#x' % (what, bits, e.bits)
            _same_bits(y, e.out, what)
            stored = y.astype(np.float64) / float(e.s)
            worst['x%g' % mult] = _ratio(stored, e.ref, e.bound, what)
            worst['stats x%g' % mult] = _check_stats(st, rows, stored, d, path, what + ' statistics')
            y2, bits2, _, _ = _fwd_h(L, dev, d, xh, w, wa, stats=False, what=what + ' without statistics')
            assert bits2 == bits
            _same_bits(y2, y, what + ': with against without statistics')
        # inference: x scaled with a bound 2^7 x its true maximum, which the output's bound follows
        xh = D.wide_half(1, (d.B, d.H, d.W, d.C), mult=128.0)
        true_bits = P.bits_of(np.abs(xh.v).max())
        assert P.float_of(true_bits) * 100 < P.float_of(xh.bits)
        what = 'DW-D %s knob %d eval' % (_ids(case), knob)
        e = D.expect_fwd_h(xh, w, wa, d, path, true_bits=true_bits)
        y, bits, _, _ = _fwd_h(L, dev, d, xh, w, wa, stats=False, true_bits=true_bits, what=what)
        assert bits == e.bits == D.bound_bits(P.float_of(wa), P.float_of(true_bits)), what
        _same_bits(y, e.out, what)
        worst['eval'] = _ratio(y.astype(np.float64) / float(e.s), e.ref, e.bound, what)
    return path, worst


@pytest.mark.parametrize('case,knob', HALF_RUNS, ids=_half_ids)
def test_dwd_half_forward(dev, case, knob):
    path, worst = _dwd(dev, case, knob)
    print('DW-D %-18s knob %d %-5s bound and halves bit-equal; err / bound %s' % (_ids(case), knob, path, '  '.join('%s %.3f' % kv for kv in worst.items())))


def test_dwd_more_tiles_than_groups(dev):
    t = D.make_tiles(D.Desc(*D.HALF_BIG))
    assert t.n_tiles > t.groups == D.SLABS
    path, worst = _dwd(dev, D.HALF_BIG, 3, mults=(1.0,))
    print('DW-D %s %d tiles on %d groups: err / bound %s' % (_ids(D.HALF_BIG), t.n_tiles, t.groups, '  '.join('%s %.3f' % kv for kv in worst.items())))


# ---- DW-E  the half data gradient ----------------------------------------------------------------------------------------------------------------------
def _dgrad_h(L, dev, d, dyh, w, wa, what, old=None, half_out=True, accumulate=0, acc_bits=None, add_src=None, add_mask=None):
    lib, dd = L.lib, _desc(L, d)
    n = d.B * d.H * d.W
    dyt = _ht(dev, d.B * d.OH * d.OW, d.C, dyh.h)
    dxt = _ht(dev, n, d.C, old) if half_out else _T(dev, n, d.C, None, old)
    dyb, wab, wt, db = _scalar(dev, dyh.bits), _scalar(dev, wa), _wt(dev, w), _Out(dev)
    ab = _scalar(dev, acc_bits) if acc_bits is not None else None
    if add_src is not None:
        src, mk = _T(dev, n, d.C, None, add_src), torch.from_numpy(D.pack_mask(add_mask)).to(dev)
        L.check(lib.pylc_dwconv3x3_dgrad_h_add(C.byref(dd), L.ptr(dyt.v), L.ptr(dyb), L.ptr(wt), L.ptr(wab), L.ptr(dxt.v), L.ptr(src.v), L.ptr(mk), L.stream()))
        src.get(what + ' add_src')
    else:
        L.check(lib.pylc_dwconv3x3_dgrad_h(C.byref(dd), L.ptr(dyt.v), L.ptr(dyb), L.ptr(wt), L.ptr(wab), L.ptr(dxt.v), L.ptr(db.p) if half_out else None,
                                           accumulate, L.ptr(ab), L.stream()))
    torch.cuda.synchronize()
    dyt.get(what + ' dy')
    dx = dxt.get(what, (d.B, d.H, d.W, d.C))
    if half_out:
        return dx, db.bits(what)
    assert db.untouched(), what
    return dx, None


@pytest.mark.parametrize('case,knob', HALF_RUNS + [(D.HALF_BIG, 3)], ids=_half_ids)
def test_dwe_half_data_gradient(dev, case, knob):
    L = _L()
    d = D.Desc(*case)
    path = D.half_path(d, knob)
    w, wa = D.filt(3, d.C)
    shape = (d.B, d.H, d.W, d.C)
    worst = {}
    big = case == D.HALF_BIG
    with _Knob(L, knob):
        assert L.lib.pylc_dwconv3x3_dgrad_h_add_ok(C.byref(_desc(L, d))) == int(D.add_ok(d, knob)) == int(path == 'tile')
        for mult in (1.0,) if big else (1.0, 128.0):
            dyh = D.wide_half(2, (d.B, d.OH, d.OW, d.C), 2.0 ** -8, mult)
            new = float(P.float_of(D.bound_bits(P.float_of(wa), P.float_of(dyh.bits))))
            mag = 2.0 ** round(np.log2(new / 4.0))
            old32 = D.wide(9, shape, mag)[0]
            forms = [('fresh half', {}, dict()),
                     ('fresh fp32', dict(half_out=False), dict()),
                     ('accumulating fp32', dict(old=old32, half_out=False), dict(accumulate=1))]
            if not big:
                for name, k in (('accumulating half, old 2^8 larger', 2.0 ** 8), ('accumulating half, old 2^8 smaller', 2.0 ** -8)):
                    oldh = D.wide_half(10, shape, mag * k)
                    forms.append((name, dict(old=oldh), dict(accumulate=1, acc_bits=oldh.bits)))
                # accumulate == 0 with an acc_bound: the scalar is not read
                forms.append(('fresh half, acc_bound given', {}, dict(accumulate=0, acc_bits=P.bits_of(1e30))))
                if path == 'tile':
                    keep = np.random.RandomState(5).rand(*shape) > 0.4
                    forms.append(('masked residual', dict(half_out=False, add_src=old32, add_mask=keep), dict(add_src=old32, add_mask=keep)))
            for name, ekw, rkw in forms:
                what = 'DW-E %s knob %d bound x%g %s' % (_ids(case), knob, mult, name)
                e = D.expect_dgrad_h(dyh, w, wa, d, path, **ekw)
                old = ekw.get('old')
                half_out = ekw.get('half_out', True)
                dx, bits = _dgrad_h(L, dev, d, dyh, w, wa, what, old.h if isinstance(old, D.Half) else old, half_out,
                                    **{k: v for k, v in rkw.items()})
                assert bits == e.bits, '%s: dx_bound_out is %s, the header says %s' % (what, bits, e.bits)
                _same_bits(dx, e.out, what)
                got = dx.astype(np.float64) / (float(e.s) if half_out else 1.0)
                worst[name] = max(worst.get(name, 0.0), _ratio(got, e.ref, e.bound, what))
    print('DW-E %-18s knob %d %-5s bit-equal in every form; err / bound %s' % (_ids(case), knob, path, '  '.join('%s %.3f' % kv for kv in worst.items())))


# ---- DW-F  the half filter gradient --------------------------------------------------------------------------------------------------------------------
def _wgrad_h(L, dev, d, xh, dyh, what, bn=None):
    lib, dd = L.lib, _desc(L, d)
    xt, dyt = _ht(dev, d.B * d.H * d.W, d.C, xh.h), _ht(dev, d.B * d.OH * d.OW, d.C, dyh.h)
    xb, dyb = _scalar(dev, xh.bits), _scalar(dev, dyh.bits)
    nbytes = lib.pylc_dwconv3x3_wgrad_workspace(C.byref(dd))
    ws, dwt = _T(dev, D.SLABS, 9 * d.C), _T(dev, d.C, 9)
    if bn is None:
        L.check(lib.pylc_dwconv3x3_wgrad_h(C.byref(dd), L.ptr(xt.v), L.ptr(xb), L.ptr(dyt.v), L.ptr(dyb), L.ptr(dwt.v), L.ptr(ws.v), nbytes, L.stream()))
    else:
        yb, sc, sh, relu = bn
        L.check(lib.pylc_dwconv3x3_wgrad_h_bn(C.byref(dd), L.ptr(xt.v), L.ptr(yb), L.ptr(sc), L.ptr(sh), relu, L.ptr(xb), L.ptr(dyt.v), L.ptr(dyb),
                                              L.ptr(dwt.v), L.ptr(ws.v), nbytes, L.stream()))
    torch.cuda.synchronize()
    xt.get(what + ' x'), dyt.get(what + ' dy')
    return dwt.get(what + ' dw'), ws.get(what + ' workspace')


# x and dy placed at 1 / 2^-8 and at the small corner of the window of bounds
CORNER = (2.0 ** -22, 2.0 ** -42)           # the magnitudes; the bounds come out near 2^-20 and 2^-40


@pytest.mark.parametrize('case,knob', HALF_RUNS + [(D.HALF_BIG, 3)], ids=_half_ids)
def test_dwf_half_filter_gradient(dev, case, knob):
    L = _L()
    d = D.Desc(*case)
    path = D.half_path(d, knob)
    used = D.depths(d, path, 2)[0]
    worst = {}
    with _Knob(L, knob):
        for name, (mx, mdy) in [('', (1.0, 2.0 ** -8))] + ([('corner', CORNER)] if case == (2, 19, 37, 136, 1, 1) else []):
            what = 'DW-F %s knob %d %s' % (_ids(case), knob, name)
            xh, dyh = D.wide_half(1, (d.B, d.H, d.W, d.C), mx), D.wide_half(2, (d.B, d.OH, d.OW, d.C), mdy)
            if name:
                assert 2.0 ** -22 <= P.float_of(xh.bits) <= 2.0 ** -18 and 2.0 ** -42 <= P.float_of(dyh.bits) <= 2.0 ** -38
            dw, rows = _wgrad_h(L, dev, d, xh, dyh, what)
            assert not np.isnan(rows[:used]).any() and np.isnan(rows[used:]).all(), what + ': workspace rows beyond the %d used were written' % used
            worst[name or 'plain'] = _ratio(dw, D.wgrad64(xh.v, dyh.v, d.stride, d.dil), D.wgrad_bound(xh.v, dyh.v, d, path), what)
    print('DW-F %-18s knob %d %-5s %4d workspace rows; err / bound %s' % (_ids(case), knob, path, used, '  '.join('%s %.3f' % kv for kv in worst.items())))


# ---- DW-G  the _bn forms ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('case', [(2, 19, 37, 136, 1, 1), (2, 10, 34, 136, 2, 1), (2, 11, 19, 136, 1, 2)], ids=_ids)
def test_dwg_bn_forms_equal_apply_plus_plain(dev, case, relu):
    L = _L()
    d = D.Desc(*case)
    lib, dd = L.lib, _desc(L, d)
    assert D.bn_ok(d) and lib.pylc_dwconv3x3_bn_ok(C.byref(dd)) == 1 and D.make_tiles(d).chunks == 2
    m, c = d.B * d.H * d.W, d.C
    what = 'DW-G %s relu %d' % (_ids(case), relu)
    r = np.random.RandomState(11)
    yin = D.to_half((r.standard_normal((m, c)) * 2.0 + np.linspace(-3, 3, c)).astype(np.float32), P.bits_of(16.0))
    scale, shift = (1 + 0.3 * r.standard_normal(c)).astype(np.float32), (0.5 * r.standard_normal(c)).astype(np.float32)
    x_bits = P.bits_of(np.abs(yin.v * scale + shift).max() * 1.01)
    w, wa = D.filt(3, c)
    dyh = D.wide_half(2, (d.B, d.OH, d.OW, c), 2.0 ** -8)
    yt, xt = _ht(dev, m, c, yin.h), _ht(dev, m, c)
    yb, xb, sc, sh = _scalar(dev, yin.bits), _scalar(dev, x_bits), torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)
    ex = L.BnExtra()
    ex.nplanes = 1
    ex.y_half_bound = L.ptr(yb)
    ex.out_planes, ex.out_plane_stride, ex.out_bound = L.ptr(xt.v), m * c, L.ptr(xb)
    L.check(lib.pylc_bn_apply_ex(L.ptr(yt.v), c, L.ptr(sc), L.ptr(sh), None, 0, None, c, m, c, relu, None, C.byref(ex), L.stream()))
    torch.cuda.synchronize()
    xh = D.to_half(np.zeros(1, np.float32), x_bits)._replace(h=xt.get(what + ' x', (d.B, d.H, d.W, c)))
    assert not np.isnan(xh.h).any() and (not relu or (xh.h >= 0).all())
    # forward
    wab, wt = _scalar(dev, wa), _wt(dev, w)
    y1, b1, st1, rows = _fwd_h(L, dev, d, xh, w, wa, what=what + ' plain')
    y2t, b2, st2 = _ht(dev, d.B * d.OH * d.OW, c), _Out(dev), _T(dev, rows, 2 * c)
    L.check(lib.pylc_dwconv3x3_fwd_h_bn(C.byref(dd), L.ptr(yt.v), L.ptr(yb), L.ptr(sc), L.ptr(sh), relu, L.ptr(xb), L.ptr(wt), L.ptr(wab), L.ptr(y2t.v),
                                        L.ptr(b2.p), L.ptr(st2.v), L.stream()))
    torch.cuda.synchronize()
    assert b2.bits(what) == b1
    assert np.array_equal(y2t.get(what + ' y', y1.shape).view(np.uint16), y1.view(np.uint16)), what + ': y of the _bn form differs'
    assert np.array_equal(st2.get(what + ' statistics').view(np.uint32), st1.get(what + ' statistics').view(np.uint32)), what + ': statistics rows differ'
    # filter gradient
    dw1, _ = _wgrad_h(L, dev, d, xh, dyh, what + ' plain')
    dw2, _ = _wgrad_h(L, dev, d, xh._replace(h=yin.h), dyh, what + ' bn', bn=(yb, sc, sh, relu))
    assert np.array_equal(dw1.view(np.uint32), dw2.view(np.uint32)), what + ': dw of the _bn form differs'
    yt.get(what + ' y_in')
    print('%s: y, y_bound_out, %d statistics rows and dw identical to pylc_bn_apply_ex + the plain forms' % (what, rows))


# ---- DW-H  predicates ---------------------------------------------------------------------------------------------------------------------------------
PRED = [D.Desc(*c) for c in D.F32_CASES + D.HALF_CASES + [D.HALF_BIG]] + [
    D.Desc(2, 9, 17, 8, 1, 1, 12, 8), D.Desc(2, 9, 17, 8, 1, 1, 8, 16), D.Desc(1, 8, 32, 8, 2, 1, 12, 12),          # pitched
    D.Desc(1, 5, 6, 12), D.Desc(1, 8, 16, 12, 2, 1), D.Desc(1, 8, 16, 12, 1, 2),                                  # C = 12
    D.Desc(1, 7, 16, 8, 2, 1), D.Desc(1, 8, 15, 8, 2, 1), D.Desc(1, 7, 15, 8, 2, 1),                               # stride 2, odd sizes
    D.Desc(1, 9, 16, 8, 1, 3), D.Desc(1, 9, 1, 8), D.Desc(1, 1, 9, 8), D.Desc(1, 9, 1, 12), D.Desc(1, 8, 16, 8, 2, 2)]


@pytest.mark.parametrize('knob', [3, 0, 1, 2])
def test_dwh_predicates(dev, knob):
    L = _L()
    lib = L.lib
    with _Knob(L, knob):
        for d in PRED:
            dd = _desc(L, d)
            got = (lib.pylc_dwconv3x3_half_ok(C.byref(dd)), lib.pylc_dwconv3x3_bn_ok(C.byref(dd)), lib.pylc_dwconv3x3_dgrad_h_add_ok(C.byref(dd)),
                   lib.pylc_dwconv3x3_fwd_stats_rows(C.byref(dd)), lib.pylc_dwconv3x3_fwd_h_stats_rows(C.byref(dd)))
            want = (int(D.half_ok(d, knob)), int(D.bn_ok(d, knob)), int(D.add_ok(d, knob)), D.f32_stats_rows(d), D.half_stats_rows(d, knob))
            assert got == want, 'DW-H knob %d %s: (half_ok, bn_ok, add_ok, fwd_stats_rows, fwd_h_stats_rows) = %s, the statement says %s' % (knob, d, got, want)
    print('DW-H knob %d: %d descriptors agree with the statement' % (knob, len(PRED)))


def test_dwh_ineligible_shape_is_refused(dev):
    L = _L()
    lib = L.lib
    for d, knob in ((D.Desc(1, 7, 15, 8, 2, 1), 3), (D.Desc(1, 8, 16, 8, 1, 2), 0), (D.Desc(1, 9, 1, 8), 0), (D.Desc(1, 9, 17, 8, 1, 1, 12, 8), 3)):
        with _Knob(L, knob):
            dd = _desc(L, d)
            assert not D.half_ok(d, knob) and lib.pylc_dwconv3x3_half_ok(C.byref(dd)) == 0
            xh = D.wide_half(1, (d.B, d.H, d.W, d.C))
            w, wa = D.filt(3, d.C)
            xt, yt, yb = _T(dev, d.B * d.H * d.W, d.C, d.x_pitch, xh.h, dtype=torch.float16), _T(dev, d.B * d.OH * d.OW, d.C, d.y_pitch, dtype=torch.float16), _Out(dev)
            xb, wab, wt = _scalar(dev, xh.bits), _scalar(dev, wa), _wt(dev, w)
            st = _T(dev, 4, 2 * d.C)
            rc = lib.pylc_dwconv3x3_fwd_h(C.byref(dd), L.ptr(xt.v), L.ptr(xb), L.ptr(wt), L.ptr(wab), L.ptr(yt.v), L.ptr(yb.p), L.ptr(st.v), L.stream())
            torch.cuda.synchronize()
            assert rc == ERR_ARG and yt.untouched() and st.untouched() and yb.untouched(), 'DW-H %s knob %d: an ineligible shape' % (d, knob)
            yt.get('DW-H y')
    print('DW-H: fwd_h refuses the four ineligible descriptors and writes nothing')
