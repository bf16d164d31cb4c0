"""The filter-gradient model of tests/_conv_wgrad.py, without a GPU: wgrad64 against torch.autograd.grad of a float64 F.conv2d on every
geometry class of the case tables (small twins of the large cases: same kernel size, stride, padding, dilation and raggedness, fewer
channels and pixels) and against the weight gradient of F.conv_transpose2d for the role-swapped up-conv; the host-only plan of every table
row against the workspace the library asks for; and the comparison helpers' teeth: each corruption of a perfect dw that a wrong kernel would
produce must be reported, with the offending element."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import _conv_wgrad as W
from tests import _eval_conv as E
from tests import _planes as P

NAN = float('nan')


def _twin(geo):
    """The geometry with at most 12 / 10 channels, one or two images and at most 21 pixels a side beyond what padding and dilation need."""
    cin, cout, k, stride, pad, dil, b, h, w = geo
    need = dil * (k - 1) + 1
    return (min(cin, 12), min(cout, 10), k, stride, pad, dil, min(b, 2), min(h, max(need - 2 * pad, 0) + 13), min(w, max(need - 2 * pad, 0) + 12))


CLASSES = sorted({_twin(c[0]) for c in W.PLANE_CASES} | {_twin(c[0]) for c in W.F32_CASES})


def _torch_wgrad(d, g):
    x = torch.from_numpy(d['x'].astype(np.float64)).permute(0, 3, 1, 2)
    dy = torch.from_numpy(d['dy'].astype(np.float64)).permute(0, 3, 1, 2)
    w = torch.zeros(g.cout, g.cin, g.k, g.k, dtype=torch.float64, requires_grad=True)
    y = Fn.conv2d(x, w, None, g.stride, g.pad, g.dil)
    assert tuple(y.shape) == (g.b, g.cout, g.oh, g.ow)
    dw, = torch.autograd.grad(y, w, dy)
    return dw.permute(0, 2, 3, 1).reshape(g.cout, g.k * g.k, g.cin).numpy()


@pytest.mark.parametrize('geo', CLASSES, ids=[repr(E.Geom(*c)) for c in CLASSES])
def test_wgrad64_is_the_autograd_weight_gradient(geo):
    g = E.Geom(*geo)
    d = W.make_wgrad_data(g, 5)
    dw, dwa = W.wgrad64(d['dy'], d['x'], g)
    want = _torch_wgrad(d, g)
    assert (np.abs(dw - want) <= 1e-12 * dwa).all()
    wa = _torch_wgrad(dict(x=np.abs(d['x']), dy=np.abs(d['dy'])), g)
    assert (np.abs(dwa - wa) <= 1e-12 * dwa).all()
    reached = W.tap_reached(g)
    assert ((dwa > 0).any(axis=(0, 2)) == reached).all()              # a tap is reached exactly when its scale is not zero
    assert (dw[:, ~reached, :] == 0).all()


def test_the_role_swapped_case_is_the_transposed_convs_weight_gradient():
    """ops/conv.py hands the 2x2 stride-2 up-conv's filter gradient to pylc_conv2d_wgrad with x = the up-conv's dy [B, 2h, 2w, Cout_t] and
    dy = its input [B, h, w, Cin_t]: dw [Cin_t][2][2][Cout_t] is then the gradient of the [Cin_t, Cout_t, 2, 2] filter."""
    cout_t, cin_t = 8, 12
    g = E.Geom(cout_t, cin_t, 2, 2, 0, 1, 2, 10, 12)
    d = W.make_wgrad_data(g, 6)
    dw, dwa = W.wgrad64(d['dy'], d['x'], g)
    xin = torch.from_numpy(d['dy'].astype(np.float64)).permute(0, 3, 1, 2)      # the up-conv's input
    gout = torch.from_numpy(d['x'].astype(np.float64)).permute(0, 3, 1, 2)      # the gradient of its output
    w = torch.zeros(cin_t, cout_t, 2, 2, dtype=torch.float64, requires_grad=True)
    y = Fn.conv_transpose2d(xin, w, None, 2)
    want, = torch.autograd.grad(y, w, gout)
    assert (np.abs(dw - want.permute(0, 2, 3, 1).reshape(cin_t, 4, cout_t).numpy()) <= 1e-12 * dwa).all()


def test_slab_sum64_and_its_bound():
    buf, slabs = W.synthetic_slabs(1, 33, 25, 8)
    assert np.isnan(buf[:, 100:]).all() and np.array_equal(buf[:, :100], slabs)
    want, bound = W.slab_sum64(slabs)
    assert np.array_equal(want, slabs.astype(np.float64).sum(0))
    assert np.allclose(bound, 33 * 2.0 ** -24 * np.abs(slabs.astype(np.float64)).sum(0), rtol=1e-15)
    acc = np.zeros(100, dtype=np.float32)
    for k in range(33):                                               # a plain fp32 chain stays inside
        acc = acc + slabs[k]
    assert (np.abs(acc.astype(np.float64) - want) <= bound).all()


# ---- the host-only plan ---------------------------------------------------------------------------------------------------------------------------
ROWS = [('planes', c[0], c[0][1], c[1], c[2:6]) for c in W.PLANE_CASES] + [('fp32', c[0], c[1], c[2], c[3:7]) for c in W.F32_CASES]


@pytest.mark.parametrize('kind,geo,y_pitch,max_steps,want', ROWS, ids=['%s-%r' % (r[0], E.Geom(*r[1])) for r in ROWS])
def test_the_workspace_follows_the_recorded_plan(kind, geo, y_pitch, max_steps, want):
    """The table's literal == plan() == what pylc_conv2d_wgrad_workspace returns (a host-only function: no GPU needed)."""
    from pylc_amd.lib import lib, ConvDesc
    g = E.Geom(*geo)
    cfg, fast, splits, mps = want
    assert W.plan(g, max_steps or 256) == want
    assert (splits - 1) * mps < g.m <= splits * mps
    slab = g.cout * g.k * g.k * g.cin
    d = ConvDesc(g.b, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.dil, g.oh, g.ow, g.cin, y_pitch)
    d.x_fmt = d.dy_fmt = int(kind == 'planes')
    try:
        if max_steps:
            assert lib.pylc_debug_wgrad_max_steps(max_steps) == 0
        got = lib.pylc_conv2d_wgrad_workspace(C.byref(d))
    finally:
        lib.pylc_debug_wgrad_max_steps(W.KNOB_DEFAULTS['max_steps'])
    assert got == (splits * slab * 4 if splits > 1 else 0)


def test_pitched_and_dense_plane_images_hold_the_same_pieces():
    r = np.random.RandomState(2)
    t = (r.standard_normal((37, 64)) * 2.0 ** r.uniform(-12, 0, (37, 64))).astype(np.float32)
    s = P.scale_for(E.amax_bits(t))
    for npl in (1, 2):
        dense, off = W.plane_image(t, s, npl, False)
        assert off == 0 and dense.size == npl * 37 * 64
        h0, h1, back = E.decode_planes(dense, 37, 64, npl, s)
        wide, off = W.plane_image(t, s, npl, True)
        pitch = 64 + W.PITCH_EXTRA
        assert off == W.PITCH_C0 and wide.size == npl * 37 * pitch
        img = wide.reshape(npl, 37, pitch)
        assert np.array_equal(img[0, :, 16:80], h0.view(np.uint16))
        if npl == 2:
            assert np.array_equal(img[1, :, 16:80], h1.view(np.uint16))
        assert (img[:, :, :16] == P.FILL16).all() and (img[:, :, 80:] == P.FILL16).all()


# ---- teeth ----------------------------------------------------------------------------------------------------------------------------------------
TG = E.Geom(40, 12, 3, 1, 1, 1, 2, 9, 20)                              # 3x3, M = 360; "splits" of 96 pixels: the last one holds 72
TMPS = 96


@pytest.fixture(scope='module')
def perfect():
    d = W.make_wgrad_data(TG, 11)
    dw, dwa = W.wgrad64(d['dy'], d['x'], TG)
    return d, dw, dwa


def _buf(dw, g=TG):
    b = np.full(dw.size + 2 * W.GUARD, NAN, dtype=np.float32)
    b[W.GUARD:W.GUARD + dw.size] = dw.astype(np.float32).ravel()
    return b


def _body(b, g=TG):
    return b[W.GUARD:W.GUARD + g.cout * g.k * g.k * g.cin].reshape(g.cout, g.k * g.k, g.cin)


def test_a_perfect_dw_passes(perfect):
    d, dw, dwa = perfect
    r, got = W.check_dw(_buf(dw), TG, dw, dwa, 'perfect')
    assert r < 0.1 and got.shape == dw.shape                           # (one fp32 rounding of the float64 value: 2^-24 |dw| <= 0.06 TOL dwa)


def test_a_tap_with_its_neighbours_values_is_reported(perfect):
    d, dw, dwa = perfect
    b = _buf(dw)
    _body(b)[:, 4, :] = _body(b)[:, 5, :].copy()
    with pytest.raises(AssertionError, match=r'row 0 tap 4 channel \d+ is off'):
        W.check_dw(b, TG, dw, dwa, 'neighbour tap')


def test_a_tap_shifted_by_one_input_column_is_reported(perfect):
    d, dw, dwa = perfect
    shifted = np.zeros_like(d['x'])
    shifted[:, :, 1:] = d['x'][:, :, :-1]                              # the kernel read x[.., wi - 1, ..]: dw0 off by one
    other, _ = W.wgrad64(d['dy'], shifted, TG)
    b = _buf(dw)
    _body(b)[:, 7, :] = other[:, 7, :]
    with pytest.raises(AssertionError, match=r'row 0 tap 7 channel \d+ is off'):
        W.check_dw(b, TG, dw, dwa, 'shifted tap')


def test_a_missing_last_pixel_row_is_reported(perfect):
    d, dw, dwa = perfect
    pixels = np.ones(TG.m, dtype=bool)
    pixels[-TG.ow:] = False
    short, _ = W.wgrad64(d['dy'], d['x'], TG, pixels=pixels)
    with pytest.raises(AssertionError, match=r'row 0 tap \d channel \d+ is off'):
        W.check_dw(_buf(short), TG, dw, dwa, 'last row left out')


def test_a_missing_last_split_is_reported(perfect):
    d, dw, dwa = perfect
    split = W.split_of_pixel(TG, TMPS)
    assert split.max() == 3 and (split == 3).sum() == 72
    short, _ = W.wgrad64(d['dy'], d['x'], TG, pixels=split < 3)
    with pytest.raises(AssertionError, match=r'row 0 tap 0 channel \d+ is off'):
        W.check_dw(_buf(short), TG, dw, dwa, 'last split left out')


def test_a_zeroed_last_channel_group_is_reported(perfect):
    d, dw, dwa = perfect
    b = _buf(dw)
    _body(b)[:, :, TG.cin - 8:] = 0.0
    with pytest.raises(AssertionError, match=r'row 0 tap 0 channel 3[2-9] is off'):
        W.check_dw(b, TG, dw, dwa, 'ragged channel group zeroed')


def test_a_row_holding_the_row_four_below_is_reported(perfect):
    d, dw, dwa = perfect
    b = _buf(dw)
    _body(b)[3] = _body(b)[7].copy()
    with pytest.raises(AssertionError, match=r'row 3 tap 0 channel \d+ is off'):
        W.check_dw(b, TG, dw, dwa, 'row n holds row n + 4')


def test_a_value_in_an_unreached_tap_is_reported():
    g = E.Geom(8, 8, 3, 1, 18, 18, 1, 16, 16)
    assert W.tap_reached(g).tolist() == [False] * 4 + [True] + [False] * 4
    d = W.make_wgrad_data(g, 12)
    dw, dwa = W.wgrad64(d['dy'], d['x'], g)
    W.check_dw(_buf(dw, g), g, dw, dwa, 'dilation 18')
    b = _buf(dw, g)
    _body(b, g)[5, 8, 2] = 2.0 ** -140                                 # any nonzero bits: the scale there is 0
    with pytest.raises(AssertionError, match='row 5 tap 8 channel 2, a tap no pixel reaches, holds'):
        W.check_dw(b, g, dw, dwa, 'dilation 18')
    b = _buf(dw, g)
    _body(b, g)[5, 8, 2] = -0.0                                        # (the sign of a zero is not asserted)
    W.check_dw(b, g, dw, dwa, 'dilation 18')


def test_a_dropped_plane_1_cross_term_is_reported(perfect):
    d, dw, dwa = perfect
    i = np.unravel_index(np.argmax(np.abs(dw) / dwa), dw.shape)
    assert abs(dw[i]) * 2.0 ** -11 > 4 * W.TOL_W * dwa[i]              # the element least cancelled: the dropped term is well outside
    b = _buf(dw)
    _body(b)[i] = np.float32(dw[i] * (1.0 - 2.0 ** -11))
    with pytest.raises(AssertionError, match='row %d tap %d channel %d is off' % i):
        W.check_dw(b, TG, dw, dwa, 'cross term')


def test_a_store_past_the_end_is_reported(perfect):
    d, dw, dwa = perfect
    b = _buf(dw)
    b[W.GUARD + dw.size] = 0.0
    with pytest.raises(AssertionError, match='the guard behind dw was written'):
        W.check_dw(b, TG, dw, dwa, 'store past the end')
    b = _buf(dw)
    b[W.GUARD - 1] = 1.0
    with pytest.raises(AssertionError, match='the guard in front of dw was written'):
        W.check_dw(b, TG, dw, dwa, 'store in front')


def test_an_unwritten_element_is_reported(perfect):
    d, dw, dwa = perfect
    b = _buf(dw)
    _body(b)[11, 8, 39] = NAN
    with pytest.raises(AssertionError, match='row 11 tap 8 channel 39 was not written'):
        W.check_dw(b, TG, dw, dwa, 'unwritten')


def test_slab_sum_teeth():
    buf, slabs = W.synthetic_slabs(3, 40, 7, 4)
    want, bound = W.slab_sum64(slabs)
    n = slabs.shape[1]

    def image(v):
        b = np.full(n + 2 * W.GUARD, NAN, dtype=np.float32)
        b[W.GUARD:W.GUARD + n] = v
        return b
    assert W.check_slab_sum(image(want.astype(np.float32)), slabs, 'perfect') < 0.05
    j = int(np.argmax(np.abs(slabs[24])))
    assert abs(slabs[24, j]) > 4 * bound[j]
    with pytest.raises(AssertionError, match='element %d is off' % j):  # slab 24 skipped: its largest term is far outside 40 2^-24 sum|.|
        v = want.copy()
        v[j] -= slabs[24, j]
        W.check_slab_sum(image(v.astype(np.float32)), slabs, 'slab skipped')
    with pytest.raises(AssertionError, match='element 27 is NaN'):
        v = want.astype(np.float32)
        v[27] = NAN
        W.check_slab_sum(image(v), slabs, 'padding reached dw')
    with pytest.raises(AssertionError, match='a guard around dw was written'):
        b = image(want.astype(np.float32))
        b[-1] = 0.0
        W.check_slab_sum(b, slabs, 'past the end')
