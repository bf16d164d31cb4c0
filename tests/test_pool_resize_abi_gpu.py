"""The fp32 kernels of pylc_amd/csrc/pool_resize.hip at the C ABI against the statements and bounds of tests/_resize.py (-m gpu; DESIGN.md
section 5.18).  Every tensor lies in a NaN-filled buffer with two guard rows before and after and, where the entry point takes a pitch,
pitch = C + 4 (or more): unused lanes and guards must stay NaN and the outputs must hold no NaN.  Errors are judged per element against the
derived bound, or bit for bit; no tolerance is tuned to the device's output.

Sections print their worst figure as error / bound (1.0 = at the bound):
  PR-A  pylc_bilinear_fwd, the rows form: within the bound of fp64 and bit-equal to the float32 model, nine size pairs
  PR-B  pylc_bilinear_fwd, the flat form (B = 65536): bit-equal to the same model
  PR-C  pylc_bilinear_bwd / pylc_bilinear_bwd_separable: the fp64 transpose, amax_bits, the adjoint identity against the GPU forward
  PR-D  pylc_maxpool_fwd / _bwd / _bwd_add: y and idx exact, dx within the gather bound (exact for 2 x 2), windows of the added gradient,
        the general backward kernel on a 2 x 2 pool (B = 65536)
  PR-E  pylc_gap_fwd / pylc_gap_bwd_acc
  PR-F  pylc_crop_copy, pylc_nhwc_to_nchw, pylc_nchw_to_nhwc: exact
The implementing run on an MI355X, worst over the cases of each section:
  PR-A  0.622 ((20, 20) -> (10, 30)); bit-equal to the float32 model at all nine pairs      PR-B  0.250, bit-equal
  PR-C  direct 0.440, separable 0.484, adjoint identity 0.007 of its slack; amax_bits exact, NULL accepted, same dx either way
  PR-D  y and idx exact in all seven cases; dx 0.999 of the gather bound for 3 x 3 / 2, exact for 2 x 2; with add 0.987 / 0.998 over seven
        windows each; B = 65536: the general kernel bit-equal to the specialised one, with and without add
  PR-E  forward 0.190 (C 2048); backward 1.000: the bound 2u |dy| / HW + u |result| is attained to three digits (C 2048, accumulate 1).
        A first version of that bound, 2u on both magnitudes, missed the third rounding of the accumulate form (reciprocal, product, sum)
        and was exceeded by 1.5 % on 16 elements of HW 15, C 2048; the derivation was wrong, not the kernel.
  PR-F  exact
"""
import numpy as np
import pytest
import torch

from tests import _resize as R

pytestmark = pytest.mark.gpu

NAN = float('nan')
GR = 2                          # guard rows


def _L():
    from pylc_amd import lib as L
    L.init()
    return L


class _T:
    """rows x c values at `pitch` inside a filled buffer with GR guard rows on either side."""

    def __init__(self, dev, rows, c, pitch=None, a=None, dtype=torch.float32, fill=NAN):
        self.rows, self.c, self.pitch, self.fill = rows, c, pitch or c, fill
        self.buf = torch.full((rows + 2 * GR, self.pitch), fill, dtype=dtype, device=dev)
        self.v = self.buf[GR:GR + rows, :c]
        if a is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(rows, c)))
        assert self.v.data_ptr() % ((4 if c % 4 == 0 else 1) * self.buf.element_size()) == 0          # a four-element vector's alignment

    def _is_fill(self, t):
        return torch.isnan(t).all() if self.fill != self.fill else (t == self.fill).all()

    def get(self, what, shape=None):
        assert self._is_fill(self.buf[:GR]) and self._is_fill(self.buf[GR + self.rows:]), '%s: a guard row was written' % what
        assert self._is_fill(self.buf[:, self.c:]), '%s: a lane beyond C was written' % what
        a = self.v.contiguous().cpu().numpy()
        return a.reshape(shape) if shape else a


def _ratio(got, ref, bound, what):
    assert not np.isnan(got).any(), '%s: NaN in the output' % what
    with np.errstate(invalid='ignore'):
        err = np.where(got == ref, 0.0, np.abs(got.astype(np.float64) - ref))        # equal infinities: no error
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError('%s: element %s is %.9g, fp64 says %.9g: err %.4g > bound %.4g; %d over the bound' %
                             (what, i, got[i], ref[i], err[i], bound[i], int(bad.sum())))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    if not np.array_equal(g, w):
        i = tuple(int(k[0]) for k in np.nonzero(g != w))
        raise AssertionError('%s: element %s is %#010x, the model says %#010x; %d differ' % (what, i, g[i], w[i], int((g != w).sum())))


# ---- PR-A / PR-B  pylc_bilinear_fwd ----------------------------------------------------------------------------------------------------------
def _bilinear_fwd(L, dev, x, OH, OW, what):
    B, H, W, C = x.shape
    xt = _T(dev, B * H * W, C, C + 4, x)
    yt = _T(dev, B * OH * OW, C, C + 8)
    L.check(L.lib.pylc_bilinear_fwd(L.ptr(xt.v), xt.pitch, L.ptr(yt.v), yt.pitch, B, H, W, C, OH, OW, L.stream()))
    xt.get(what + ': x')
    return yt.get(what, (B, OH, OW, C))


@pytest.mark.parametrize('size,out', R.RESIZE_PAIRS)
def test_pra_bilinear_fwd_rows(dev, size, out):
    L = _L()
    (H, W), (OH, OW) = size, out
    x = R.wide(H * 100 + OW, 2, H, W, 12)
    what = 'PR-A %s -> %s' % (size, out)
    y = _bilinear_fwd(L, dev, x, OH, OW, what)
    r = _ratio(y, R.bilinear64(x, OH, OW), R.bilinear_fwd_bound(x, OH, OW), what)
    _same_bits(y, R.bilinear_f32(x, OH, OW), what)
    print('PR-A %-8s -> %-8s err / bound %.3f, bit-equal to the float32 model' % (size, out, r))


def test_prb_bilinear_fwd_flat_form(dev):
    """B > 65535 takes bilinear_fwd_kernel (a flat index with 64-bit divisions) instead of the rows form."""
    L = _L()
    B, (H, W), (OH, OW) = 65536, (1, 2), (2, 3)
    x = R.wide(5, B, H, W, 4)
    y = _bilinear_fwd(L, dev, x, OH, OW, 'PR-B')
    _same_bits(y, R.bilinear_f32(x, OH, OW), 'PR-B')
    r = _ratio(y, R.bilinear64(x, OH, OW), R.bilinear_fwd_bound(x, OH, OW), 'PR-B')
    print('PR-B B 65536 (1, 2) -> (2, 3): err / bound %.3f, bit-equal to the float32 model' % r)


# ---- PR-C  the two bilinear backward kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,out', R.RESIZE_PAIRS_BWD)
def test_prc_bilinear_bwd(dev, size, out):
    L = _L()
    (H, W), (OH, OW) = size, out
    B, worst = 2, {'direct': 0.0, 'separable': 0.0, 'adjoint': 0.0}
    for C in (4, 12, 68):
        what = 'PR-C %s -> %s C %d' % (size, out, C)
        dy, x = R.wide(H + OW + C, B, OH, OW, C), R.wide(H + OW + C + 1, B, H, W, C)
        ref = R.bilinear_bwd64(dy, H, W)
        dyt = _T(dev, B * OH * OW, C, C + 4, dy)
        got = {}
        dxt = _T(dev, B * H * W, C, C + 8)
        L.check(L.lib.pylc_bilinear_bwd(L.ptr(dyt.v), dyt.pitch, L.ptr(dxt.v), dxt.pitch, B, H, W, C, OH, OW, L.stream()))
        got['direct'] = dxt.get(what + ' direct', (B, H, W, C))
        ws_n = L.lib.pylc_bilinear_bwd_workspace(B, W, C, OH) // 4
        assert ws_n == B * OH * W * C
        for with_amax in (True, False):
            dxt = _T(dev, B * H * W, C, C + 8)
            ws = _T(dev, 1, ws_n)
            amax = torch.full((3,), -1, dtype=torch.int32, device=dev)
            L.check(L.lib.pylc_bilinear_bwd_separable(L.ptr(dyt.v), dyt.pitch, L.ptr(dxt.v), dxt.pitch, B, H, W, C, OH, OW, L.ptr(ws.v),
                                                      L.ptr(amax[1:]) if with_amax else None, L.stream()))
            ws.get(what + ' workspace')
            dx = dxt.get(what + ' separable', (B, H, W, C))
            a = amax.cpu().numpy()
            assert a[0] == -1 and a[2] == -1
            if with_amax:
                got['separable'] = dx
                assert a[1:2].view(np.uint32)[0] == np.float32(np.abs(dx).max()).view(np.uint32), what + ': amax_bits'
            else:
                assert a[1] == -1
                _same_bits(dx, got['separable'], what + ': with and without amax_bits')
        dyt.get(what + ': dy')
        for name in ('direct', 'separable'):
            worst[name] = max(worst[name], _ratio(got[name], ref, R.bilinear_bwd_bound(dy, H, W, name == 'separable'), what + ' ' + name))
        # <dy, A x> = <A^T dy, x> with the GPU's forward: each side is off by at most sum |other factor| x its bound
        y = _bilinear_fwd(L, dev, x, OH, OW, what + ' forward').astype(np.float64)
        d64, x64 = dy.astype(np.float64), np.abs(x.astype(np.float64))
        lhs = (d64 * y).sum()
        slack_l = (np.abs(d64) * R.bilinear_fwd_bound(x, OH, OW)).sum()
        for name in ('direct', 'separable'):
            rhs = (got[name].astype(np.float64) * x.astype(np.float64)).sum()
            slack = slack_l + (R.bilinear_bwd_bound(dy, H, W, name == 'separable') * x64).sum()
            assert abs(lhs - rhs) <= slack, what + ': adjoint identity, %s' % name
            worst['adjoint'] = max(worst['adjoint'], abs(lhs - rhs) / slack)
    print('PR-C %-8s -> %-8s err / bound  %s' % (size, out, '  '.join('%s %.3f' % kv for kv in worst.items())))


# ---- PR-D  max pool ----------------------------------------------------------------------------------------------------------------------------
def _pool_fwd(L, dev, x, k, s, pad, what):
    B, H, W, C = x.shape
    OH, OW = R.pool_out(H, k, s, pad), R.pool_out(W, k, s, pad)
    xt = _T(dev, B * H * W, C, a=x)
    yt = _T(dev, B * OH * OW, C)
    it = _T(dev, B * OH * OW, C, dtype=torch.uint8, fill=0xA5)
    L.check(L.lib.pylc_maxpool_fwd(L.ptr(xt.v), L.ptr(yt.v), L.ptr(it.v), B, H, W, C, k, s, pad, OH, OW, L.stream()))
    xt.get(what + ': x')
    return yt.get(what + ': y', (B, OH, OW, C)), it, it.get(what + ': idx', (B, OH, OW, C))


def _pool_bwd(L, dev, dy, it, H, W, k, s, pad, what, add=None, window=None):
    B, OH, OW, C = dy.shape
    dyt = _T(dev, B * OH * OW, C, a=dy)
    dxt = _T(dev, B * H * W, C)
    if add is None:
        L.check(L.lib.pylc_maxpool_bwd(L.ptr(dyt.v), L.ptr(it.v), L.ptr(dxt.v), B, H, W, C, k, s, pad, OH, OW, L.stream()))
    else:
        h0, w0, AH, AW = window
        at = _T(dev, B * AH * AW, C, C + 8, add)
        L.check(L.lib.pylc_maxpool_bwd_add(L.ptr(dyt.v), L.ptr(it.v), L.ptr(dxt.v), B, H, W, C, k, s, pad, OH, OW, L.ptr(at.v), at.pitch, h0, w0, AH, AW,
                                           L.stream()))
        at.get(what + ': add')
    dyt.get(what + ': dy')
    return dxt.get(what + ': dx', (B, H, W, C))


POOLS = [(3, 2, 1, 16, 16), (3, 2, 1, 15, 9), (3, 2, 1, 1, 7), (3, 2, 1, 2, 2), (2, 2, 0, 12, 12), (2, 2, 0, 21, 13), (2, 2, 0, 2, 3)]


@pytest.mark.parametrize('k,s,pad,H,W', POOLS)
def test_prd_maxpool_fwd_and_bwd(dev, k, s, pad, H, W):
    L = _L()
    what = 'PR-D k %d s %d pad %d %dx%d' % (k, s, pad, H, W)
    x = R.pool_input(H + W, 2, H, W, 8)
    y, it, idx = _pool_fwd(L, dev, x, k, s, pad, what)
    yr, ir = R.maxpool_fwd(x, k, s, pad)
    _same_bits(y, yr, what + ': y')
    assert np.array_equal(idx, ir), what + ': idx'
    dy = R.wide(H * W, *y.shape)
    ref, mag, cnt = R.maxpool_bwd64(dy, ir, H, W, k, s, pad)
    dx = _pool_bwd(L, dev, dy, it, H, W, k, s, pad, what)
    bound = R.maxpool_bwd_bound(mag, cnt)
    r = _ratio(dx, ref, bound, what + ': dx')
    if k == 2:
        assert not bound.any()                                        # exact
        assert not dx[:, 2 * (H // 2):].any() and not dx[:, :, 2 * (W // 2):].any(), what + ': the odd last row / column is not zero'
    print('PR-D k %d s %d pad %d %2dx%-2d: y, idx exact; dx err / bound %.3f%s' % (k, s, pad, H, W, r, ' (exact)' if k == 2 else ''))


@pytest.mark.parametrize('k,s,pad,H,W', [(3, 2, 1, 15, 9), (2, 2, 0, 21, 13)])
def test_prd_maxpool_bwd_add_windows(dev, k, s, pad, H, W):
    L = _L()
    x = R.pool_input(H + W, 2, H, W, 8)
    worst = 0.0
    windows = {'interior': (3, 2, 5, 4), 'top-left': (0, 0, 2, 2), 'top-right': (0, W - 2, 2, 2), 'bottom-left': (H - 2, 0, 2, 2),
               'bottom-right': (H - 2, W - 2, 2, 2), 'last row': (H - 1, 0, 1, W), 'whole': (0, 0, H, W)}
    for name, win in windows.items():
        what = 'PR-D add k %d %s' % (k, name)
        y, it, idx = _pool_fwd(L, dev, x, k, s, pad, what)
        dy = R.wide(7, *y.shape)
        add = R.wide(9, 2, win[2], win[3], 8)
        ref, mag, cnt = R.maxpool_bwd64(dy, idx, H, W, k, s, pad, add, win)
        dx = _pool_bwd(L, dev, dy, it, H, W, k, s, pad, what, add, win)
        worst = max(worst, _ratio(dx, ref, R.maxpool_bwd_bound(mag, cnt), what))
    print('PR-D add, k %d, %d windows (add_pitch C + 8): dx err / bound %.3f' % (k, len(windows), worst))


def test_prd_general_backward_kernel_on_a_2x2_pool(dev):
    """B > 65535 does not fit the specialised kernel's grid: the general gather kernel runs a 2 x 2 / 2 pool.  Equal to the specialised
    kernel's result on the same data at B = 2, replicated."""
    L = _L()
    B, reps = 65536, 32768
    x2 = R.pool_input(4, 2, 2, 2, 4)
    x2[..., 2] = x2[..., 0][..., ::-1]                                  # (finite: the comparison is on dx)
    dy2 = R.wide(6, 2, 1, 1, 4)
    y, it, idx = _pool_fwd(L, dev, x2, 2, 2, 0, 'PR-D B 2')
    small = _pool_bwd(L, dev, dy2, it, 2, 2, 2, 2, 0, 'PR-D B 2')
    ref, mag, cnt = R.maxpool_bwd64(dy2, idx, 2, 2, 2, 2, 0)
    assert np.array_equal(small.astype(np.float64), ref)
    xb, dyb = np.tile(x2, (reps, 1, 1, 1)), np.tile(dy2, (reps, 1, 1, 1))
    yb, itb, idxb = _pool_fwd(L, dev, xb, 2, 2, 0, 'PR-D B 65536')
    assert np.array_equal(idxb, np.tile(idx, (reps, 1, 1, 1)))
    big = _pool_bwd(L, dev, dyb, itb, 2, 2, 2, 2, 0, 'PR-D B 65536')
    _same_bits(big, np.tile(small, (reps, 1, 1, 1)), 'PR-D B 65536 against B 2 replicated')
    win = (1, 0, 1, 2)
    add2 = R.wide(8, 2, 1, 2, 4)
    small = _pool_bwd(L, dev, dy2, it, 2, 2, 2, 2, 0, 'PR-D B 2 add', add2, win)
    big = _pool_bwd(L, dev, dyb, itb, 2, 2, 2, 2, 0, 'PR-D B 65536 add', np.tile(add2, (reps, 1, 1, 1)), win)
    _same_bits(big, np.tile(small, (reps, 1, 1, 1)), 'PR-D B 65536 with add against B 2 replicated')
    print('PR-D B 65536, 2x2 input, 2x2 pool: the general kernel equals the specialised one bit for bit, with and without add')


# ---- PR-E  global average pool -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 68, 2048])
def test_pre_gap_fwd_and_bwd(dev, C):
    L = _L()
    B, wf, wb = 3, 0.0, 0.0
    for hw in (1, 15, 16, 17, 127, 128, 129, 1000):
        what = 'PR-E HW %d C %d' % (hw, C)
        x = R.wide(hw + C, B, hw, C)
        xt, yt = _T(dev, B * hw, C, a=x), _T(dev, B, C)
        L.check(L.lib.pylc_gap_fwd(L.ptr(xt.v), L.ptr(yt.v), B, hw, C, L.stream()))
        xt.get(what + ': x')
        wf = max(wf, _ratio(yt.get(what + ': y'), x.astype(np.float64).mean(1), R.gap_fwd_bound(x), what + ': forward'))
        dy, dx0 = R.wide(hw + C + 1, B, C), R.wide(hw + C + 2, B, hw, C)
        dyt = _T(dev, B, C, a=dy)
        for acc in (0, 1):
            dxt = _T(dev, B * hw, C, a=dx0 if acc else None)                # accumulate 0: dx is NaN-filled and must be overwritten
            L.check(L.lib.pylc_gap_bwd_acc(L.ptr(dyt.v), L.ptr(dxt.v), B, hw, C, acc, L.stream()))
            ref = np.broadcast_to(dy.astype(np.float64)[:, None, :] / hw, (B, hw, C)) + (dx0.astype(np.float64) if acc else 0.0)
            bound = np.broadcast_to(R.gap_bwd_bound(dy, hw, dx0 if acc else None), (B, hw, C))
            wb = max(wb, _ratio(dxt.get(what + ': dx', (B, hw, C)), ref, bound, what + ': backward, accumulate %d' % acc))
        dyt.get(what + ': dy')
    print('PR-E C %4d, HW 1 .. 1000: forward err / bound %.3f, backward %.3f' % (C, wf, wb))


# ---- PR-F  crop and layout ---------------------------------------------------------------------------------------------------------------------
def test_prf_crop_copy(dev):
    L = _L()
    B, H, W, C = 2, 7, 9, 12
    x = R.wide(1, B, H, W, C)
    xt = _T(dev, B * H * W, C, C + 4, x)
    wins = [(0, 0, 3, 4), (0, W - 4, 3, 4), (H - 3, 0, 3, 4), (H - 3, W - 4, 3, 4), (3, 5, 1, 1), (0, 0, H, W), (2, 3, 4, 2)]
    for h0, w0, th, tw in wins:
        what = 'PR-F crop %s' % ((h0, w0, th, tw),)
        dt = _T(dev, B * th * tw, C, C + 8)
        L.check(L.lib.pylc_crop_copy(L.ptr(xt.v), xt.pitch, H, W, h0, w0, L.ptr(dt.v), dt.pitch, B, th, tw, C, L.stream()))
        _same_bits(dt.get(what, (B, th, tw, C)), x[:, h0:h0 + th, w0:w0 + tw], what)
    xt.get('PR-F crop: src')
    print('PR-F crop_copy: %d windows exact (pitches %d -> %d)' % (len(wins), C + 4, C + 8))


@pytest.mark.parametrize('C,pitch', [(3, 4), (9, 12), (3, 12), (9, 9)])
def test_prf_layout_transposes(dev, C, pitch):
    L = _L()
    B, H, W = 3, 5, 7
    x = R.wide(C, B, H, W, C)
    xt = _T(dev, B * H * W, C, pitch, x)
    ct = _T(dev, B * C, H * W)
    L.check(L.lib.pylc_nhwc_to_nchw(L.ptr(xt.v), pitch, L.ptr(ct.v), B, H, W, C, L.stream()))
    xt.get('PR-F: x')
    nchw = ct.get('PR-F nhwc_to_nchw', (B, C, H, W))
    _same_bits(nchw, x.transpose(0, 3, 1, 2), 'PR-F nhwc_to_nchw')
    bt = _T(dev, B * H * W, C, pitch)
    L.check(L.lib.pylc_nchw_to_nhwc(L.ptr(ct.v), L.ptr(bt.v), pitch, B, H, W, C, L.stream()))
    _same_bits(bt.get('PR-F nchw_to_nhwc', (B, H, W, C)), x, 'PR-F round trip')
    print('PR-F C %d pitch %2d: both transposes exact, round trip exact, pad lanes untouched' % (C, pitch))
