"""The float64 model of the dense convolution's training entries (tests/_conv_train.py) against torch, and the teeth of its comparison
helpers: every way the data gradient's parity classes, its accumulate / masked-add epilogues, the pitched store and the forward's statistics
can go wrong that the GPU tests rely on them to catch, applied to an otherwise perfect synthetic output, must be reported.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _bn
from tests import _conv_train as T
from tests import _eval_conv as E
from tests import _planes as P


def _reduced(geo):
    """The geometry class at a small batch / size; the stride-2 cases stay as listed (they are tiny)."""
    cin, cout, k, stride, pad, dil, b, h, w = geo
    if stride == 2:
        return geo
    return (cin, cout, k, stride, pad, dil, 1, min(h, 19), min(w, 17))


ALL_GEOMS = sorted({_reduced(c[2]) for c in T.CASES})


def _torch_dgrad(dy, w, g):
    x = torch.zeros(g.b, g.cin, g.h, g.w, dtype=torch.float64, requires_grad=True)
    wt = torch.from_numpy(np.asarray(w, dtype=np.float64)).view(g.cout, g.k, g.k, g.cin).permute(0, 3, 1, 2)
    y = F.conv2d(x, wt, None, g.stride, g.pad, g.dil)
    gy = torch.from_numpy(np.asarray(dy, dtype=np.float64)).permute(0, 3, 1, 2)
    return torch.autograd.grad(y, x, gy)[0].permute(0, 2, 3, 1).reshape(-1, g.cin).numpy()


@pytest.mark.parametrize('geo', ALL_GEOMS, ids=[repr(E.Geom(*g)) for g in ALL_GEOMS])
def test_dgrad64_equals_torch_autograd(geo):
    g = E.Geom(*geo)
    d = T.make_train_data(g, 11)
    dx, dxa = T.dgrad64(d['dy'], d['w'], g)
    want = _torch_dgrad(d['dy'], d['w'], g)
    assert dx.shape == want.shape == (g.b * g.h * g.w, g.cin)
    err = np.abs(dx - want)
    assert (err <= 1e-12 * dxa).all(), (g, float(err.max()))
    assert (dxa >= np.abs(dx)).all()
    # the pixels no tap reaches are those whose scale is zero whatever the data
    dead = ~T.reached(g)
    assert (dxa[dead] == 0).all() and (dxa[~dead] > 0).all()
    # ... and the forward the statistics cases use is _eval_conv's conv64, the adjoint of this: <conv(x), dy> == <x, dgrad(dy)>
    x = np.random.RandomState(5).standard_normal((g.b, g.h, g.w, g.cin))
    z, za = E.conv64(x, d['w'], g)
    lhs, rhs = float((z * d['dy'].reshape(g.m, g.cout)).sum()), float((x.reshape(-1, g.cin) * dx).sum())
    assert abs(lhs - rhs) <= 1e-10 * float((za * np.abs(d['dy'].reshape(g.m, g.cout))).sum())


def test_mask_model_equals_unpack_relu_bits():
    r = np.random.RandomState(2)
    for m, c in ((1, 8), (7, 72), (33, 256)):
        raw = r.randint(0, 256, m * c // 8).astype(np.uint8)
        want = _bn.unpack_relu_bits(torch.from_numpy(raw), m, c).numpy()
        got = T.mask_bits(raw, m, c)
        assert got.dtype == np.bool_ and np.array_equal(got, want)
        assert np.array_equal(T.pack_mask(got), raw)
    bits = T.mask_bits(T.make_train_data(E.Geom(64, 8, 1, 1, 0, 1, 4, 32, 32), 3)['mask'], 4096, 64)
    assert abs(bits.mean() - 0.55) < 0.01


def test_transposed_filter_and_bound():
    w = np.arange(9 * 2 * 4, dtype=np.float32).reshape(9, 2, 4)
    t = T.w_crsk(w)
    assert t.shape == (4, 2, 12) and (t[:, :, 9:] == 0).all() and t[3, 1, 8] == w[8, 1, 3]
    a, b = P.bits_of(np.float32(0.7)), P.bits_of(np.float32(1.3))
    assert T.product_bound(288, a, b) == {P.bits_of(np.float32(np.float32(np.float32(288.0) * np.float32(0.7)) * np.float32(1.3)))}
    assert T.tile_height(2046, 16) == 128 and T.tile_height(2046, 8) == 256 and T.tile_height(100, 1) == 128
    with pytest.raises(AssertionError):
        T.tile_height(2046, 15)


def test_case_forms_are_known():
    from pylc_amd import lib as L
    assert {c[1] for c in T.CASES} <= set(L.CONV_FORMS)
    assert {c[0] for c in T.CASES} == {'pylc_conv2d_dgrad_add', 'pylc_conv2d_dgrad', 'pylc_conv2d_fwd', 'pylc_conv2d_fwd_stats'}
    assert {'plhn', 'plh', 'pl256', 'plp', 'pl128', 'pl128-narrow'} <= {c[0] for c in T.DGRAD_CASES}


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------------
class _PerfectDgrad:
    """A synthetic perfect data gradient: the float64 reference of each epilogue rounded to fp32, in the buffers the GPU test hands to the helpers."""

    def __init__(self, geo):
        self.g = g = E.Geom(*geo)
        self.mi = g.b * g.h * g.w
        d = self.d = T.make_train_data(g, 21)
        self.dy = E.Operand(d['dy'], E.amax_bits(d['dy']), 2)
        self.w = E.Operand(d['w'], E.amax_bits(d['w']), 2)
        self.dx, self.dxa = T.dgrad64(self.dy.seen, self.w.seen, g)

    def ref(self, kind, mask=None):
        d = self.d
        if kind == 'acc':
            return T.dgrad_epilogue64(self.dx, self.dxa, old=d['old'])
        if kind == 'add':
            return T.dgrad_epilogue64(self.dx, self.dxa, add=d['add'])
        if kind == 'addmask':
            return T.dgrad_epilogue64(self.dx, self.dxa, add=d['add'], mask=d['mask'] if mask is None else mask)
        return T.dgrad_epilogue64(self.dx, self.dxa)

    def buf(self, y, pitch=None, c0=0):
        g = self.g
        pitch = pitch or g.cin
        buf = np.full(self.mi * pitch + 2 * T.GUARD, np.nan, dtype=np.float32)
        buf[T.GUARD:T.GUARD + self.mi * pitch].reshape(self.mi, pitch)[:, c0:c0 + g.cin] = np.asarray(y).reshape(self.mi, g.cin)
        return buf

    def check(self, kind, buf, pitch=None, c0=0):
        v, mag = self.ref(kind)
        return E.check_f32(buf, self.mi, self.g.cin, pitch or self.g.cin, c0, v, mag, 'synthetic ' + kind, tol=T.TOL_C)


S2_LIVE = (8, 8, 3, 2, 1, 1, 1, 9, 8)           # stride 2, 3x3: all four classes live, odd and even size
S2_DEAD = (8, 8, 1, 2, 0, 1, 1, 9, 8)           # stride-2 1x1: three empty classes
S1 = (16, 8, 3, 1, 1, 1, 1, 9, 7)               # stride 1, M = 63: ragged against every tile height


@pytest.fixture(scope='module')
def live():
    return _PerfectDgrad(S2_LIVE)


@pytest.fixture(scope='module')
def dead():
    return _PerfectDgrad(S2_DEAD)


@pytest.fixture(scope='module')
def s1():
    return _PerfectDgrad(S1)


def _fails(match, fn, *a, **k):
    with pytest.raises(AssertionError, match=match):
        fn(*a, **k)


ELEMENT = r'element \(\d+, \d+\) is off by'


def test_perfect_outputs_pass(live, dead, s1):
    for p in (live, dead, s1):
        for kind in ('fresh', 'acc', 'add', 'addmask'):
            v, _ = p.ref(kind)
            r, y = p.check(kind, p.buf(v.astype(np.float32)))
            assert r <= 2.0 ** -24 / T.TOL_C + 1e-9                             # one rounding of the reference
            r, _ = p.check(kind, p.buf(v.astype(np.float32), p.g.cin + 32, 16), p.g.cin + 32, 16)
            assert r <= 0.06
    assert T.check_classes(dead.ref('fresh')[0].astype(np.float32), dead.d['old'], dead.g, 0, 'synthetic') == 72 - 20
    assert T.check_classes(dead.ref('acc')[0].astype(np.float32), dead.d['old'], dead.g, 1, 'synthetic') == 52
    assert T.check_classes(live.ref('fresh')[0].astype(np.float32), live.d['old'], live.g, 0, 'synthetic') == 0


def test_a_parity_class_shifted_by_one_pixel_is_caught(live):
    p, g = live, live.g
    for kind in ('fresh', 'acc'):
        for ph, pw in ((0, 0), (1, 0), (0, 1), (1, 1)):
            y = p.ref(kind)[0].astype(np.float32).reshape(g.b, g.h, g.w, g.cin).copy()
            y[:, ph::2, pw::2] = np.roll(y[:, ph::2, pw::2], 1, axis=2)
            _fails(ELEMENT, p.check, kind, p.buf(y))


def test_wrong_empty_classes_are_caught(dead):
    p, g = dead, dead.g
    dead_px = ~T.reached(g)
    old = p.d['old']
    # accumulate = 0: the empty classes still hold what dx held before the call
    y = p.ref('fresh')[0].astype(np.float32)
    y[dead_px] = old[dead_px]
    _fails(ELEMENT, p.check, 'fresh', p.buf(y))
    _fails('no tap reaches, is not zero', T.check_classes, y, old, g, 0, 'synthetic')
    # accumulate = 1: the empty classes were zeroed
    y = p.ref('acc')[0].astype(np.float32)
    y[dead_px] = 0.0
    _fails(ELEMENT, p.check, 'acc', p.buf(y))
    _fails('does not hold the old value', T.check_classes, y, old, g, 1, 'synthetic')
    # ... or hold the old value up to a rounding only (check_f32 allows that; the bit comparison does not)
    y = p.ref('acc')[0].astype(np.float32)
    first = int(np.nonzero(dead_px)[0][0])
    y[first, 3] = np.nextafter(y[first, 3], np.float32(np.inf))
    p.check('acc', p.buf(y))
    _fails('pixel %d channel 3' % first, T.check_classes, y, old, g, 1, 'synthetic')


def test_a_wrong_mask_is_caught(s1):
    p = s1
    bits = T.mask_bits(p.d['mask'], p.mi, p.g.cin)
    # add_src applied where the bit is clear: in one element
    m, c = (int(k[0]) for k in np.nonzero(~bits))
    y = p.ref('addmask')[0].astype(np.float32)
    y[m, c] = np.float32(p.dx[m, c] + p.d['add'][m, c])
    _fails(r'element \(%d, %d\)' % (m, c), p.check, 'addmask', p.buf(y))
    # the unmasked sum everywhere / the mask ignored altogether
    _fails(ELEMENT, p.check, 'addmask', p.buf(p.ref('add')[0].astype(np.float32)))
    _fails(ELEMENT, p.check, 'addmask', p.buf(p.ref('fresh')[0].astype(np.float32)))
    # the two nibbles of one mask byte swapped
    raw = p.d['mask'].copy()
    i = int(np.nonzero((raw & 15) != (raw >> 4))[0][5])
    raw[i] = ((raw[i] & 15) << 4) | (raw[i] >> 4)
    y = p.ref('addmask', mask=raw)[0].astype(np.float32)
    row, q = divmod(i, p.g.cin // 8)
    with pytest.raises(AssertionError, match=r'element \(%d, (\d+)\)' % row) as e:
        p.check('addmask', p.buf(y))
    assert 8 * q <= int(e.value.args[0].split('element (%d, ' % row)[1].split(')')[0]) < 8 * q + 8
    # the mask read one vector (quad of rows' worth of bytes) late
    late = np.roll(p.d['mask'], -4)
    _fails(ELEMENT, p.check, 'addmask', p.buf(p.ref('addmask', mask=late)[0].astype(np.float32)))


def test_old_added_without_accumulate_is_caught(s1, live):
    for p in (s1, live):
        _fails(ELEMENT, p.check, 'fresh', p.buf(p.ref('acc')[0].astype(np.float32)))
        _fails(ELEMENT, p.check, 'acc', p.buf(p.ref('fresh')[0].astype(np.float32)))


def test_an_unwritten_last_row_is_caught(s1):
    p = s1
    y = p.ref('fresh')[0].astype(np.float32)
    y[-1] = np.nan
    _fails(r'element \(%d, 0\)' % (p.mi - 1), p.check, 'fresh', p.buf(y))


def test_a_store_past_a_pitched_row_is_caught(s1):
    p = s1
    pitch = p.g.cin + 32
    y = p.ref('acc')[0].astype(np.float32)
    buf = p.buf(y, pitch, 16)
    buf[T.GUARD + 5 * pitch + 16 + p.g.cin] = 0.0                                # one element past the slice of row 5, inside the pitch
    _fails('outside the output slice', p.check, 'acc', buf, pitch, 16)
    buf = p.buf(y, pitch, 16)
    buf[T.GUARD + 5 * pitch + 15] = 0.0
    _fails('outside the output slice', p.check, 'acc', buf, pitch, 16)
    buf = p.buf(y)
    buf[T.GUARD + p.mi * p.g.cin] = 0.0
    _fails('guard', p.check, 'acc', buf)


class _PerfectStats:
    def __init__(self):
        self.g = g = E.Geom(24, 40, 1, 1, 0, 1, 1, 23, 13)                       # M = 299: three tiles of 128, the last ragged; two of 256
        d = E.make_data(g, 22)
        x, w = E.Operand(d['x'], E.amax_bits(d['x']), 2), E.Operand(d['w'], E.amax_bits(d['w']), 2)
        self.z, self.za = E.conv64(x.seen, w.seen, g)
        self.bias = T.big_bias(self.z, g.cout, 1)
        self.floats = -(-g.m // 128) * 2 * g.cout

    def buf(self, z, bm, extra_rows=0):
        s, q = T.stats64(z, T.linear_tiles(self.g.m, bm))
        body = np.full(self.floats, np.nan, dtype=np.float32)
        rows = s.shape[0]
        body[:rows * 2 * self.g.cout] = np.stack((s, q), axis=1).astype(np.float32).ravel()
        buf = np.full(self.floats + 2 * T.GUARD, np.nan, dtype=np.float32)
        buf[T.GUARD:T.GUARD + self.floats] = body
        return buf, rows

    def check(self, buf, rows, halo=False):
        return T.check_stats(buf, self.floats, rows, self.g.cout, self.z, self.za, 'synthetic statistics', halo=halo)


@pytest.fixture(scope='module')
def stats():
    return _PerfectStats()


def test_perfect_statistics_pass(stats):
    p = stats
    for bm in (128, 256):
        buf, rows = p.buf(p.z, bm)
        assert rows == -(-p.g.m // bm)
        assert p.check(buf, rows) <= 0.2
        assert p.check(buf, rows, halo=True) <= 0.2


def test_statistics_after_the_bias_are_caught(stats):
    p = stats
    buf, rows = p.buf(p.z + p.bias.astype(np.float64), 128)
    _fails(r'sum of statistics row 0 channel 0', p.check, buf, rows)
    _fails(r'sum of statistics row 0 channel 0', p.check, buf, rows, halo=True)


def test_a_row_with_its_neighbours_sums_is_caught(stats):
    p = stats
    buf, rows = p.buf(p.z, 128)
    body = buf[T.GUARD:T.GUARD + rows * 2 * p.g.cout].reshape(rows, 2, p.g.cout)
    body[1] = body[0]
    _fails(r'statistics row 1 channel', p.check, buf, rows)
    buf, rows = p.buf(p.z, 128)
    body = buf[T.GUARD:T.GUARD + rows * 2 * p.g.cout].reshape(rows, 2, p.g.cout)
    body[[0, 1]] = body[[1, 0]]                                                   # two rows exchanged: the totals cannot see it, the rows do
    p.check(buf, rows, halo=True)
    _fails(r'statistics row 0 channel', p.check, buf, rows)


def test_statistics_rows_and_guards(stats):
    p = stats
    buf, rows = p.buf(p.z, 256)
    buf[T.GUARD + rows * 2 * p.g.cout] = 0.0                                      # a float past the rows reported
    _fails('past the 2 rows reported', p.check, buf, rows)
    buf, rows = p.buf(p.z, 128)
    buf[T.GUARD + 2 * 2 * p.g.cout + 7] = np.nan                                  # a hole in the last row
    _fails('row 2 .sum. channel 7 was not written', p.check, buf, rows)
    buf, rows = p.buf(p.z, 128)
    buf[T.GUARD + p.floats] = 0.0
    _fails('guard', p.check, buf, rows)
    buf, rows = p.buf(p.z, 128)
    _fails('do not fit', p.check, buf, rows + 1)                                  # more rows than the buffer holds
    _fails('past the 2 rows reported', p.check, buf, rows - 1)                    # three rows written, two reported


def test_a_low_out_bound_is_caught(s1):
    p = s1
    kp = T.roundup4(p.g.cout)
    cand = T.product_bound(kp * p.g.k * p.g.k, p.dy.bits, p.w.bits)
    (bits,) = cand
    true_max = np.abs(p.dx).max()
    E.check_bound(bits, cand, true_max, 'synthetic')
    assert float(P.float_of(bits)) >= float(p.dxa.max())                        # the product of the bounds covers every sum of products
    _fails('none of the model', E.check_bound, bits - 1, cand, true_max, 'one ulp low')
    _fails('none of the model', E.check_bound, bits + 1, cand, true_max, 'one ulp high')
    _fails('none of the model', E.check_bound, next(iter(T.product_bound(p.g.cout * 9 - 1, p.dy.bits, p.w.bits))), cand, true_max, 'another reduction length')
    _fails('below the true maximum', E.check_bound, bits, cand, 2.0 * float(P.float_of(bits)), 'a bound below the maximum')
    # a one-plane output under that bound goes through check_planes
    s = P.scale_for(bits)
    v, mag = p.ref('fresh')
    buf = np.full(2 * p.mi * p.g.cin + 2 * T.GUARD, P.FILL16, dtype=np.uint16)
    E.encode_planes(v.astype(np.float32), s, 1, out=buf, base=T.GUARD)
    assert E.check_planes(buf, p.mi, p.g.cin, 1, bits, v, mag, 'synthetic one-plane dx', tol=T.TOL_C) <= 0.06
    low = np.full_like(buf, P.FILL16)
    E.encode_planes(v.astype(np.float32), P.scale_for(bits - (1 << 23)), 1, out=low, base=T.GUARD)      # encoded under the scale of half the bound
    _fails(ELEMENT, E.check_planes, low, p.mi, p.g.cin, 1, bits, v, mag, 'synthetic one-plane dx', tol=T.TOL_C)
