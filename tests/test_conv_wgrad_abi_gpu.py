"""The dense convolution's filter gradient at the C ABI against the float64 model of tests/_conv_wgrad.py (-m gpu): pylc_conv2d_wgrad on
fp16-plane operands in precision modes 2 (f16x3, two planes) and 3 (one plane) and on fp32 tensors in modes 0 / 1 / 2, pylc_conv2d_wgrad_slabs
followed by pylc_splitk_reduce_batch, and the batch sum alone on synthetic slabs.  Operands are built on the host as planes (no GPU producer
in the loop); every device buffer lies between sentinel regions (fp32: NaN, halves: 0x7e00) that must be intact after the call, inputs and
range scalars must be bit for bit what was uploaded, dw starts as NaN and EVERY element of it is compared:
    |dw - dw64| <= TOL_W dwa        dw64 / dwa: the gather-form float64 sum of the values the operands hold and its absolute-value twin
    taps no pixel reaches           exact zeros
The workspace is a buffer of EXACTLY pylc_conv2d_wgrad_workspace(d) bytes between guards, prefilled with NaN: a kernel that leaves part of
a slab unwritten, or relies on a zeroed workspace, shows up as NaN in dw.  Every case asserts its split plan before it launches --
workspace / (4 * slab) == the table's split count, and for the _slabs entry pending.splits / n4 / slab_stride -- which is the "which form
ran" assertion of the filter gradient: tile configuration and geometry path follow from the geometry by the rules tests/_conv_wgrad.py
records.  Every case runs twice, the bits must be equal (deterministic slabs, reduced in a fixed order).

The precision mode is set through the set_mode fixture and every pylc_debug_wgrad_* knob through the knobs fixture alone, which restores
m16 = 2, dma = 1, sets = 1, acc1 = 0, flags = 0, max_steps = 256 when the test ends, passed or failed.

Each check prints one line `CW <entry> cfg<k> fast<f> splits<s> mode <m> <geometry> <option>: worst error / (TOL mag)`;
profiles/conv_wgrad_abi.txt keeps those of the implementing run on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _conv_wgrad as W
from tests import _eval_conv as E
from tests.test_eval_conv_abi_gpu import _Buf, _f32, _L, _Scalars, _u16, set_mode      # noqa: F401  (set_mode: a fixture)

pytestmark = pytest.mark.gpu

GUARD = E.GUARD
NAN = float('nan')
WGRAD, SLABS, BATCH = 'pylc_conv2d_wgrad', 'pylc_conv2d_wgrad_slabs', 'pylc_splitk_reduce_batch'


@pytest.fixture
def knobs(dev):
    """The one place the process-wide pylc_debug_wgrad_* knobs are set; the defaults come back when the test ends."""
    L = _L()

    def go(**kw):
        for name, value in kw.items():
            assert name in W.KNOB_DEFAULTS
            L.check(getattr(L.lib, 'pylc_debug_wgrad_' + name)(int(value)))
    yield go
    for name, value in W.KNOB_DEFAULTS.items():
        L.check(getattr(L.lib, 'pylc_debug_wgrad_' + name)(value))


def _report(entry, row, mode, g, option, ratio):
    print('CW %s cfg%d fast%d splits%d mode %d %r %s: worst error / (TOL mag) %.3f' % (entry, row[0], row[1], row[2], mode, g, option, ratio))


def _upload(dev, raw):
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)


# ---- one case on the host: operands as the kernel reads them and the float64 sums, once per (table, case, mode) ----------------------------------
_HOST = {}


def _host(kind, idx, mode, geo=None):
    key = (kind, idx, mode, geo)
    if key not in _HOST:
        if geo is not None:                                            # a geometry outside the tables (refusals): no plan recorded
            row, y_pitch, max_steps = None, None, None
        elif kind == 'planes':
            geo, max_steps = W.PLANE_CASES[idx][:2]
            row, y_pitch = W.PLANE_CASES[idx][2:6], None
        else:
            geo, y_pitch, max_steps = W.F32_CASES[idx][:3]
            row = W.F32_CASES[idx][3:7]
        g = E.Geom(*geo)
        d = W.make_wgrad_data(g, 21 + (idx or 0))
        x2, dy2 = d['x'].reshape(-1, g.cin), d['dy'].reshape(-1, g.cout)
        h = dict(g=g, row=row, max_steps=max_steps, x2=x2, dy2=dy2, y_pitch=y_pitch, img={})
        if kind == 'planes':
            npl = h['npl'] = 2 if mode == 2 else 1
            mult = 2.0 if (idx or 0) % 2 else 1.0                      # odd cases: both operands split under twice their true maximum
            h['x'] = E.Operand(x2, E.times_pow2(E.amax_bits(x2), mult), npl)
            h['dy'] = E.Operand(dy2, E.times_pow2(E.amax_bits(dy2), mult), npl)
            h['bits'] = dict(x=h['x'].bits, dy=h['dy'].bits)
            h['dw'], h['dwa'] = W.wgrad64(h['dy'].seen, h['x'].seen, g)
        else:
            h['bits'] = dict(x=E.amax_bits(x2), dy=E.amax_bits(dy2))
            h['dw'], h['dwa'] = W.wgrad64(dy2, x2, g)
        _HOST.clear()                                                  # one case at a time
        _HOST[key] = h
    return _HOST[key]


class _WCase:
    def __init__(self, dev, kind, idx, mode, knobs, geo=None, extra=W.PITCH_EXTRA):
        self.L, self.dev, self.kind, self.mode, self.extra = _L(), dev, kind, mode, extra
        h = self.h = _host(kind, idx, mode, geo)
        self.g, self.row = h['g'], h['row']
        self.slab = self.g.cout * self.g.k * self.g.k * self.g.cin
        if h['max_steps']:
            knobs(max_steps=h['max_steps'])
        self._ops = {}

    def operands(self, pitched, pad=None):
        """(x buffer, x offset, x pitch, dy buffer, dy offset, dy pitch), uploaded once per layout.  pad: what channels [Cout, roundup4(Cout))
        of an fp32 dy hold instead of the zeros pylc_conv2d_fwd writes there."""
        if pad is not None:
            g, yp = self.g, self.h['y_pitch']
            yi = W.f32_image(self.h['dy2'], yp, zero_to=min(yp, (g.cout + 3) & ~3))
            yi[:, g.cout:min(yp, (g.cout + 3) & ~3)] = pad
            return self.operands(False)[:3] + (_f32(self.dev, yi), 0, yp)
        if pitched not in self._ops:
            h, g = self.h, self.g
            if self.kind == 'planes':
                xi, x0 = W.plane_image(h['x2'], h['x'].s, h['npl'], pitched, self.extra)
                yi, y0 = W.plane_image(h['dy2'], h['dy'].s, h['npl'], pitched, self.extra)
                xp, yp = (g.cin + self.extra, g.cout + self.extra) if pitched else (g.cin, g.cout)
                self._ops[pitched] = (_u16(self.dev, xi), x0, xp, _u16(self.dev, yi), y0, yp)
            else:
                assert not pitched
                yp = h['y_pitch']
                yi = W.f32_image(h['dy2'], yp, zero_to=min(yp, (g.cout + 3) & ~3))
                self._ops[pitched] = (_f32(self.dev, h['x2']), 0, g.cin, _f32(self.dev, yi), 0, yp)
        return self._ops[pitched]

    def call(self, entry=WGRAD, *, pitched=False, refused=False, breakit=None, ws='exact', dbias=False, pending='given', pad=None):
        """One pylc_conv2d_wgrad / pylc_conv2d_wgrad_slabs (+ the batch sum of its slabs).  Returns the host copy of the dw buffer."""
        L, g, h = self.L, self.g, self.h
        xb, x0, xp, yb, y0, yp = self.operands(pitched, pad)
        sc = _Scalars(self.dev, **h['bits'])
        d = L.ConvDesc(g.b, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.dil, g.oh, g.ow, xp, yp)
        d.x_amax, d.dy_amax = sc.ptr('x'), sc.ptr('dy')
        d.x_fmt = d.dy_fmt = int(self.kind == 'planes')
        if breakit:
            breakit(d)
        nbytes = L.lib.pylc_conv2d_wgrad_workspace(C.byref(d))
        if self.row is not None and not breakit:                       # the plan, before the launch
            splits = self.row[2]
            assert nbytes % (4 * self.slab) == 0 and nbytes // (4 * self.slab) == (splits if splits > 1 else 0), \
                'the workspace of %d bytes is %.3f slabs, the table says %d splits' % (nbytes, nbytes / (4.0 * self.slab), splits)
        # single split: the entry needs no workspace; it still gets one (of NaN) and must not touch it
        wsb = _f32(self.dev, np.full(nbytes // 4 if nbytes else 256, NAN, dtype=np.float32))
        give_ptr, give_bytes = (wsb.ptr(), nbytes) if nbytes else (wsb.ptr(), 1024)
        if ws == 'short':
            assert nbytes
            give_bytes = nbytes - 1
        elif ws == 'null':
            assert nbytes
            give_ptr = None
        dw = _f32(self.dev, np.full(self.slab, NAN, dtype=np.float32))
        db = _f32(self.dev, np.full(g.cout, NAN, dtype=np.float32)) if dbias else None
        before = sc.t.clone()
        pend = L.SlabSum()
        if entry == WGRAD:
            rc = L.lib.pylc_conv2d_wgrad(C.byref(d), xb.ptr(x0), yb.ptr(y0), dw.ptr(), db.ptr() if db else None, give_ptr, give_bytes, L.stream())
        else:
            rc = L.lib.pylc_conv2d_wgrad_slabs(C.byref(d), xb.ptr(x0), yb.ptr(y0), dw.ptr(), give_ptr, give_bytes,
                                               C.byref(pend) if pending == 'given' else None, L.stream())
        torch.cuda.synchronize()
        if refused:
            assert rc != 0, 'the call was accepted'
            assert dw.same() and wsb.same() and torch.equal(sc.t, before) and (db is None or db.same()), 'a refused call wrote to dw, the workspace or a scalar'
        else:
            assert rc == 0, L.lib.pylc_last_error().decode()
            n = wsb.buf.numel()
            assert torch.equal(wsb.buf[:GUARD], wsb.was[:GUARD]) and torch.equal(wsb.buf[n - GUARD:], wsb.was[n - GUARD:]), 'a guard around the workspace was written'
            if not nbytes:
                assert wsb.same(), 'a single-split filter gradient wrote to its workspace'
        assert xb.same() and yb.same(), 'an input buffer or its guards changed'
        assert sc.read() == h['bits'], 'an input scalar changed'
        if entry == SLABS and not refused:
            splits = self.row[2]
            if splits == 1:
                assert pend.splits == 0, 'one split, but pending.splits = %d' % pend.splits
            else:
                assert (pend.splits, pend.n4, pend.slab_stride) == (splits, self.slab // 4, self.slab), \
                    'pending = (splits %d, n4 %d, stride %d)' % (pend.splits, pend.n4, pend.slab_stride)
                assert pend.slabs == wsb.ptr() and pend.dw == dw.ptr()
                table = _upload(self.dev, bytes(pend))
                tiles = -(-pend.n4 // 32)
                prefix = torch.tensor([0, tiles], dtype=torch.int64, device=self.dev)
                L.check(L.lib.pylc_splitk_reduce_batch(table.data_ptr(), prefix.data_ptr(), 1, tiles, L.stream()))
                torch.cuda.synchronize()
                assert torch.equal(wsb.buf[:GUARD], wsb.was[:GUARD]) and torch.equal(wsb.buf[n - GUARD:], wsb.was[n - GUARD:])
        return dw.host()

    def run(self, entry=WGRAD, option='dense', **kw):
        """One call against the model: (worst error / (TOL mag), dw [Cout][k k][Cin] fp32)."""
        what = 'CW %s cfg%d fast%d splits%d mode %d %r %s' % ((entry,) + tuple(self.row[:3]) + (self.mode, self.g, option))
        r, dw = W.check_dw(self.call(entry, **kw), self.g, self.h['dw'], self.h['dwa'], what)
        _report(entry, self.row, self.mode, self.g, option, r)
        return r, dw


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    if not np.array_equal(a, b):
        i = E._first(a != b)
        raise AssertionError('%s: element %s differs: %#010x vs %#010x (%d of %d)' % (what, i, a[i], b[i], int((a != b).sum()), a.size))


# ---- plane operands -----------------------------------------------------------------------------------------------------------------------------
PLANE_IDS = ['cfg%d-fast%d-splits%d-%r' % (c[2], c[3], c[4], E.Geom(*c[0])) for c in W.PLANE_CASES]


@pytest.mark.parametrize('mode', [2, 3], ids=['f16x3', 'mode3'])
@pytest.mark.parametrize('idx', range(len(W.PLANE_CASES)), ids=PLANE_IDS)
def test_wgrad_on_planes_against_float64(dev, set_mode, knobs, idx, mode):
    set_mode(mode)
    case = _WCase(dev, 'planes', idx, mode, knobs)
    _, first = case.run(option='dense')
    _, again = case.run(option='dense, second run')
    _same_bits(first, again, 'two runs of the same call')
    _, wide = case.run(option='pitched operands', pitched=True)
    # the slabs entry and the batch sum of its slabs: the bits of pylc_conv2d_wgrad; a single split: dw complete, nothing pending
    _, later = case.run(SLABS, option='dense, slabs + batch sum' if case.row[2] > 1 else 'dense, nothing pending')
    _same_bits(first, later, 'pylc_conv2d_wgrad_slabs + pylc_splitk_reduce_batch against pylc_conv2d_wgrad')


FORMS = [('m16 0: 32x32x16', dict(m16=0)), ('dma 0: 16x16x32 register-staged', dict(dma=0)), ('sets 0', dict(sets=0)), ('sets 2', dict(sets=2)),
         ('m16 0 sets 0', dict(m16=0, sets=0)), ('m16 0 sets 2', dict(m16=0, sets=2)), ('acc1 1', dict(acc1=1))]


@pytest.mark.parametrize('mode', [2, 3], ids=['f16x3', 'mode3'])
@pytest.mark.parametrize('idx', W.SPLIT_PLANE_CASES, ids=[PLANE_IDS[i] for i in W.SPLIT_PLANE_CASES])
def test_every_dispatched_form_against_float64(dev, set_mode, knobs, idx, mode):
    """The 128 x 128 tile's forms: 32x32x16 (m16 0) with one or two staging sets, 16x16x32 register-staged (dma 0) or fed by LDS-DMA (the
    default), one accumulator (acc1, f16x3 only) -- each against float64 within the same tolerance.  The header calls the LDS-DMA form
    bit-identical to the register-staged one."""
    set_mode(mode)
    case = _WCase(dev, 'planes', idx, mode, knobs)
    _, default = case.run(option='default form')
    for label, kw in FORMS:
        if 'acc1' in kw and mode != 2:
            continue
        knobs(**dict(W.KNOB_DEFAULTS, max_steps=case.h['max_steps'] or 256))
        knobs(**kw)
        _, dw = case.run(option=label)
        if kw == dict(dma=0):
            _same_bits(default, dw, 'the register-staged 16x16x32 form against the LDS-DMA one')


@pytest.mark.parametrize('mode', [2, 3], ids=['f16x3', 'mode3'])
@pytest.mark.parametrize('idx', [0, 3], ids=['multi-tap', 'single-tap-Cin>Cout'])
def test_rasterisation_flags_change_no_element(dev, set_mode, knobs, idx, mode):
    """pylc_debug_wgrad_flags 1 / 2 / 4 / 8 renumber the blocks: every element is still written, and -- a block's arithmetic does not depend
    on its number, the slabs are summed in a fixed order -- with the bits of the default order."""
    set_mode(mode)
    case = _WCase(dev, 'planes', idx, mode, knobs)
    _, default = case.run(option='flags 0')
    for flags in (1, 2, 4, 8):
        knobs(flags=flags)
        _, dw = case.run(option='flags %d' % flags)
        _same_bits(default, dw, 'pylc_debug_wgrad_flags(%d) against the default order' % flags)


# ---- fp32 operands ------------------------------------------------------------------------------------------------------------------------------
F32 = [(i, m) for i in range(len(W.F32_CASES)) for m in (0, 1, 2)]


@pytest.mark.parametrize('idx,mode', F32, ids=['cfg%d-fast%d-splits%d-%r-mode%d' % (W.F32_CASES[i][3:6] + (E.Geom(*W.F32_CASES[i][0]), m)) for i, m in F32])
def test_wgrad_on_fp32_tensors_against_float64(dev, set_mode, knobs, idx, mode):
    """x_fmt = dy_fmt = 0: the operands are the fp32 values themselves (mode 0: the fp32 MFMA chain, 1: bf16x6, 2: f16x3 split in the kernel);
    same reference, same tolerance.  dy channels [Cout, roundup4(Cout)) hold zeros, as pylc_conv2d_fwd writes them; the 9-class head then
    runs again with 1e30 and with NaN there."""
    set_mode(mode)
    case = _WCase(dev, 'fp32', idx, mode, knobs)
    _, first = case.run(option='fp32 operands')
    _, again = case.run(option='fp32 operands, second run')
    _same_bits(first, again, 'two runs of the same call')
    _, later = case.run(SLABS, option='fp32 operands, slabs + batch sum' if case.row[2] > 1 else 'fp32 operands, nothing pending')
    _same_bits(first, later, 'pylc_conv2d_wgrad_slabs + pylc_splitk_reduce_batch against pylc_conv2d_wgrad')
    if case.g.cout % 4:
        # the header: those channels are read and reach no row of dw -- whatever they hold, 1e30 or NaN, dw keeps its bits
        for name, pad in (('1e30', 1e30), ('NaN', NAN)):
            _, other = case.run(option='fp32 operands, dy channels [Cout, roundup4(Cout)) = ' + name, pad=pad)
            _same_bits(first, other, 'dy channels [Cout, roundup4(Cout)) = %s against zeros' % name)


# ---- the batch sum on synthetic slabs -------------------------------------------------------------------------------------------------------------
def test_splitk_reduce_batch_on_synthetic_slabs(dev):
    """Four entries in ONE launch: splits 9 / 2 / 256 / 33, n4 33 / 1 / 4097 / 100 (none a multiple of 32; one tile beside 129 tiles),
    slab_stride > 4 n4 with NaN in the padding, values over 12 binades, slab 1 of the first entry all -0.0; every dw between guards."""
    L = _L()
    table = (L.SlabSum * len(W.SLAB_ENTRIES))()
    prefix, held = [0], []
    for e, (splits, n4, pad) in enumerate(W.SLAB_ENTRIES):
        buf, slabs = W.synthetic_slabs(40 + e, splits, n4, pad)
        if e == 0:
            buf[1, :4 * n4] = slabs[1] = -0.0
        sb, dw = _f32(dev, buf), _f32(dev, np.full(4 * n4, NAN, dtype=np.float32))
        table[e] = L.SlabSum(sb.ptr(), dw.ptr(), n4, 4 * n4 + pad, splits, 0)
        prefix.append(prefix[-1] + -(-n4 // 32))
        held.append((sb, dw, slabs))
    assert [b - a for a, b in zip(prefix, prefix[1:])] == [2, 1, 129, 4]
    tab, pre = _upload(dev, bytes(table)), torch.tensor(prefix, dtype=torch.int64, device=dev)
    L.check(L.lib.pylc_splitk_reduce_batch(tab.data_ptr(), pre.data_ptr(), len(held), prefix[-1], L.stream()))
    torch.cuda.synchronize()
    for e, (sb, dw, slabs) in enumerate(held):
        splits, n4, pad = W.SLAB_ENTRIES[e]
        assert sb.same(), 'entry %d: the slabs changed' % e
        r = W.check_slab_sum(dw.host(), slabs, 'CW %s entry %d (splits %d, n4 %d, stride %d)' % (BATCH, e, splits, n4, 4 * n4 + pad))
        print('CW %s synthetic entry %d splits%d n4 %d stride %d: worst error / sum_bound %.3f' % (BATCH, e, splits, n4, 4 * n4 + pad, r))
    for n, t in ((0, tab.data_ptr()), (len(held), None)):               # n = 0, a NULL table: refused, nothing written
        before = [dw.host() for _, dw, _ in held]
        assert L.lib.pylc_splitk_reduce_batch(t, pre.data_ptr(), n, prefix[-1], L.stream()) != 0
        torch.cuda.synchronize()
        for (_, dw, _), b in zip(held, before):
            assert np.array_equal(dw.host().view(np.uint32), b.view(np.uint32))


# ---- argument errors: refused, and dw, the workspace and the scalars bit for bit ---------------------------------------------------------------------
ONE, SPLIT = 7, 0                       # (64, 64, 3x3 valid) 20 x 24: one split;  (256, 256, 3x3) 48 x 32: three splits


def _set(**kw):
    def go(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return go


def test_wgrad_refuses_bad_arguments(dev, set_mode, knobs):
    set_mode(2)
    one = _WCase(dev, 'planes', ONE, 2, knobs)
    g = one.g
    one.call(dbias=True, refused=True)                                          # non-NULL dbias
    one.call(breakit=_set(dy_fmt=0), refused=True)                              # x_fmt != dy_fmt
    one.call(breakit=_set(x_fmt=0), refused=True)
    one.call(pitched=True, breakit=_set(x_pitch=g.cin + 28), refused=True)      # a pitch % 8 != 0 (inside the buffer of pitch Cin + 32)
    one.call(pitched=True, breakit=_set(y_pitch=g.cout + 28), refused=True)
    one.call(breakit=_set(dy_amax=None), refused=True)                          # mode 2 without a range
    one.call(breakit=_set(x_amax=None), refused=True)
    one.call(breakit=_set(y_pitch=g.cout - 8), refused=True)                    # y_pitch < roundup4(Cout)
    one.call(SLABS, pending='null', refused=True)
    for mode in (0, 1):                                                         # plane operands need precision mode 2 or 3
        set_mode(mode)
        one.call(refused=True)
        one.call(SLABS, refused=True)
    set_mode(2)
    split = _WCase(dev, 'planes', SPLIT, 2, knobs)
    split.call(ws='short', refused=True)                                        # a workspace one byte short
    split.call(ws='null', refused=True)                                         # NULL where bytes are needed
    split.call(SLABS, ws='short', refused=True)
    small = _WCase(dev, 'planes', None, 2, knobs, geo=(64, 64, 3, 1, 1, 1, 1, 12, 12))
    small.call(refused=True)                                                    # plane operands with OW < 16
    odd = _WCase(dev, 'planes', None, 2, knobs, geo=(64, 12, 1, 1, 0, 1, 1, 16, 16), extra=36)
    assert (odd.g.cout + 36) % 8 == 0 and (odd.g.cin + 36) % 8 != 0
    odd.call(pitched=True, breakit=_set(x_pitch=odd.g.cin + 32), refused=True)  # plane operands with Cout % 8 != 0 (both pitches % 8 == 0)
    fp32 = _WCase(dev, 'fp32', 3, 2, knobs)
    fp32.call(breakit=_set(dy_amax=None), refused=True)                         # fp32 operands in mode 2 need the ranges too
    fp32.call(breakit=_set(y_pitch=36), refused=True)                           # Cout 40: a pitch below it
